// rf_alphabet.hpp -- the alphabet of a `char` (u32) corpus, chosen from exact symbol counts.  No HIP in here: the host packer (rf_api.hip rf_corpus_pack_u32) and
// the device road (counts from rf_pack_wide.hip) both call choose_alphabet, and tests/cpp/alphabet_check.cpp drives it with plain g++.
//
// Symbols are ranked by count descending, then symbol ascending.  The first kAlphabetIds ranks become byte ids in rank order (so the LDS rows the kernels touch
// most sit in distinct banks); every later rank shares the overflow id.  A corpus with overflow symbols keeps a raw symbol stream, 2 bytes per symbol iff no
// symbol is at or above 0xFFFF (0xFFFF is the 2-byte stream's padding value), else 4.  0xFFFFFFFF is the 4-byte padding value and is refused.
//
// rf_corpus_save writes `alphabet` and `overflow` in container iteration order, which follows from the order of insertion: every road builds them by this one loop,
// so the same counts always save the same file.
#pragma once

#include <algorithm>
#include <cstdint>
#include <unordered_map>
#include <unordered_set>
#include <utility>
#include <vector>

namespace rf {

constexpr uint32_t kAlphabetIds = 254;            // ids 0..253; rf_host.hpp kOverflowId is the next one
constexpr uint32_t kReservedSymbol = 0xFFFFFFFFu;
constexpr uint32_t kLowSymbols = 0x10000;         // symbols below this are counted in a direct table

struct AlphabetChoice {
    std::unordered_map<uint32_t, uint8_t> alphabet;  // symbol -> id
    std::unordered_set<uint32_t> overflow;           // symbols that share the overflow id
    bool narrow = true;                              // no symbol at or above 0xFFFF
};

// low: kLowSymbols counts (symbol = index); high: (symbol, count) of every symbol at or above kLowSymbols, each symbol once, count > 0, any order.
// false: the reserved symbol is there (out is untouched).
inline bool choose_alphabet(const uint64_t* low, const std::vector<std::pair<uint32_t, uint64_t>>& high, AlphabetChoice* out)
{
    for (const auto& kv : high)
        if (kv.first == kReservedSymbol) return false;
    std::vector<std::pair<uint64_t, uint32_t>> syms;  // (count, symbol)
    for (uint32_t ch = 0; ch < kLowSymbols; ++ch)
        if (low[ch]) syms.emplace_back(low[ch], ch);
    for (const auto& kv : high) syms.emplace_back(kv.second, kv.first);
    std::sort(syms.begin(), syms.end(), [](const auto& a, const auto& b) { return a.first != b.first ? a.first > b.first : a.second < b.second; });
    AlphabetChoice c;
    for (size_t r = 0; r < syms.size(); ++r) {
        if (r < (size_t)kAlphabetIds)
            c.alphabet.emplace(syms[r].second, (uint8_t)r);
        else
            c.overflow.insert(syms[r].second);
    }
    c.narrow = high.empty() && low[0xFFFF] == 0;
    *out = std::move(c);
    return true;
}

}  // namespace rf

// alphabet_check.cpp -- rapidfuzz_rs_amd/csrc/rf_alphabet.hpp (no HIP in it) against a naive re-statement of its rule:
//   rank symbols by count descending, then symbol ascending; the first 254 ranks get ids 0..253 in rank order, the rest is overflow;
//   the raw stream is narrow iff no symbol is at or above 0xFFFF; the symbol 0xFFFFFFFF is refused.
// Built by tests/test_alphabet.py with g++ -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "rf_alphabet.hpp"

namespace {

int g_cases = 0;

struct Input {
    std::map<uint32_t, uint64_t> counts;  // symbol -> count (> 0)
};

// the rule, spelled without a sort: pick the best remaining symbol, one rank at a time
struct Expected {
    bool ok = true, narrow = true;
    std::map<uint32_t, uint32_t> id;  // symbol -> id
    std::vector<uint32_t> overflow;
};
Expected naive(const Input& in)
{
    Expected e;
    for (const auto& kv : in.counts) {
        if (kv.first == 0xFFFFFFFFu) e.ok = false;
        if (kv.first >= 0xFFFFu) e.narrow = false;
    }
    if (!e.ok) return e;
    std::map<uint32_t, uint64_t> left = in.counts;
    for (uint32_t rank = 0; !left.empty(); ++rank) {
        auto best = left.begin();
        for (auto it = left.begin(); it != left.end(); ++it)
            if (it->second > best->second) best = it;  // (ascending iteration: the smallest symbol of the largest count stays)
        if (rank < 254)
            e.id[best->first] = rank;
        else
            e.overflow.push_back(best->first);
        left.erase(best);
    }
    return e;
}

void fail(const std::string& name, const std::string& what)
{
    std::fprintf(stderr, "alphabet check FAILED: %s: %s\n", name.c_str(), what.c_str());
    std::exit(1);
}

void check(const std::string& name, const Input& in)
{
    ++g_cases;
    std::vector<uint64_t> low(rf::kLowSymbols, 0);
    std::vector<std::pair<uint32_t, uint64_t>> high;
    for (auto it = in.counts.rbegin(); it != in.counts.rend(); ++it) {  // (any order will do for the symbols above the table: here descending)
        if (it->first < rf::kLowSymbols)
            low[it->first] = it->second;
        else
            high.emplace_back(it->first, it->second);
    }
    const Expected e = naive(in);
    rf::AlphabetChoice got;
    got.alphabet.emplace(7u, (uint8_t)7);  // (a refusal must leave the output as it was)
    const bool ok = rf::choose_alphabet(low.data(), high, &got);
    if (ok != e.ok) fail(name, "accepted / refused");
    if (!ok) {
        if (got.alphabet.size() != 1 || !got.overflow.empty()) fail(name, "a refusal touched the output");
        return;
    }
    if (got.narrow != e.narrow) fail(name, "narrow");
    if (got.alphabet.size() != e.id.size()) fail(name, "alphabet size");
    for (const auto& kv : e.id) {
        auto a = got.alphabet.find(kv.first);
        if (a == got.alphabet.end() || a->second != kv.second) fail(name, "id of symbol " + std::to_string(kv.first));
    }
    if (got.overflow.size() != e.overflow.size()) fail(name, "overflow size");
    for (uint32_t sym : e.overflow)
        if (!got.overflow.count(sym)) fail(name, "overflow symbol " + std::to_string(sym));
    // the same counts give the same containers in the same iteration order (rf_corpus_save writes them in that order)
    rf::AlphabetChoice again;
    std::vector<std::pair<uint32_t, uint64_t>> high2(high.rbegin(), high.rend());
    if (!rf::choose_alphabet(low.data(), high2, &again)) fail(name, "second call refused");
    if (std::vector<std::pair<uint32_t, uint8_t>>(got.alphabet.begin(), got.alphabet.end()) != std::vector<std::pair<uint32_t, uint8_t>>(again.alphabet.begin(), again.alphabet.end()) ||
        std::vector<uint32_t>(got.overflow.begin(), got.overflow.end()) != std::vector<uint32_t>(again.overflow.begin(), again.overflow.end()))
        fail(name, "iteration order depends on the order of the input");
}

// `distinct` symbols from `base` on, `stride` apart, with distinct counts (a deterministic shuffle of 1000 + k)
Input spread(uint32_t distinct, uint32_t base, uint32_t stride)
{
    Input in;
    for (uint32_t k = 0; k < distinct; ++k) in.counts[base + k * stride] = 1000 + (uint64_t)((k * 7919u) % 1009u) * 3 + k % 3;
    return in;
}

}  // namespace

int main()
{
    for (uint32_t distinct : {0u, 1u, 254u, 255u, 300u}) {
        const std::string d = std::to_string(distinct) + " symbols";
        check(d + ", BMP", spread(distinct, 0x20, 3));
        {   // every count equal: symbol ascending decides every rank, and which symbols get an id at all
            Input in = spread(distinct, 0x4E00, 5);
            for (auto& kv : in.counts) kv.second = 17;
            check(d + ", all counts tie", in);
        }
        {   // a tie exactly across ranks 253 / 254: two symbols share the 254th-largest count
            Input in;
            for (uint32_t k = 0; k < distinct; ++k) in.counts[0x3000 - k * 2] = 100000 - (uint64_t)k * 10;  // rank k = symbol 0x3000 - 2k
            if (distinct >= 255) {
                in.counts[0x3000 - 253 * 2] = in.counts[0x3000 - 254 * 2];  // ranks 253 and 254 tie: the SMALLER symbol (the old rank 254) gets the id
            }
            check(d + ", tie across ranks 253/254", in);
            if (distinct >= 255) {
                const Expected e = naive(in);
                if (!e.id.count(0x3000 - 254 * 2) || e.id.count(0x3000 - 253 * 2)) fail(d, "the tie case does not put the smaller symbol first");
            }
        }
        {   // 0xFFFF present: not narrow
            Input in = spread(distinct, 0x100, 2);
            in.counts[0xFFFF] = 5;
            check(d + " + 0xFFFF", in);
        }
        {   // nothing above 0xFFFE: narrow
            Input in = spread(distinct, 0x100, 2);
            in.counts[0xFFFE] = 5;
            check(d + " + 0xFFFE", in);
        }
        {   // symbols at 0x10000 and above, frequent and rare
            Input in = spread(distinct, 0x41, 1);
            in.counts[0x10000] = 999999;
            in.counts[0x1F600] = 1;
            in.counts[0x10FFFF] = 1500;
            in.counts[0xFFFFFFFEu] = 2;
            check(d + " + symbols above the BMP", in);
        }
        {   // the reserved symbol
            Input in = spread(distinct, 0x41, 1);
            in.counts[0xFFFFFFFFu] = 1;
            check(d + " + 0xFFFFFFFF", in);
        }
        {   // counts above 2^32, ties among them included
            Input in = spread(distinct, 0x41, 1);
            in.counts[0x61] = (1ull << 32) + 5;
            in.counts[0x62] = (1ull << 32) + 5;
            in.counts[0x63] = (1ull << 40);
            in.counts[0x20000] = (1ull << 32) + 6;
            in.counts[0x64] = 5;  // (equal to a large count in its low 32 bits only)
            check(d + " + counts above 2^32", in);
        }
    }
    std::printf("alphabet ok: %d cases\n", g_cases);
    return 0;
}

// The symbol-level row map of the join calls (rapidfuzz_rs_amd/csrc/rf_join_xlat.hpp) on the host, with no device: for random pairs of corpora -- bytes or
// `char` on either side, alphabets of a handful to several hundred symbols drawn from Latin-1, Greek, Cyrillic, CJK and planes above the BMP, each with its own
// frequency ranking and its own renaming sigma --
//   every symbol the query corpus stores under an id of its own is walked the way resolve() (rf_api.hip) walks a query symbol -- a byte corpus takes code points
//     0..255 and refuses the rest, a `char` corpus looks it up in its alphabet, then in its overflow set, else the symbol is absent -- and row_of / bad of the
//     byte the query corpus stores for it must say the same: the scanned corpus' sigma of that id and not bad, or bad;
//   the query corpus' overflow id is bad exactly when that corpus has an overflow class; a value the query corpus never stores is never bad;
//   any_bad is the OR of bad over the stored values;
//   the absent row sigma_c[255] is no row of an id in use, and a sigma that breaks this is refused;
//   two byte corpora: row_of[s] == sigma_c[inv_sigma_q[s]] for every s and nothing is bad.
// tests/test_join_xlat.py builds this twice, plainly and under AddressSanitizer + UndefinedBehaviorSanitizer.
#include <algorithm>
#include <cstdio>
#include <map>
#include <numeric>
#include <random>
#include <set>
#include <vector>

#include "rf_join_xlat.hpp"

using namespace rf;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            if (++failures < 20) std::printf("line %d: %s\n", __LINE__, #cond); \
        }                                                                  \
    } while (0)

struct Corpus {
    bool wide = false;
    uint8_t sigma[256];
    uint32_t sym_of_id[256];
    std::map<uint32_t, uint8_t> alphabet;  // symbol -> id
    std::set<uint32_t> overflow;
    JoinXlatCorpus view() const { return JoinXlatCorpus{wide, sigma, sym_of_id, !overflow.empty()}; }
};

int main()
{
    std::mt19937 rng(20261021);
    auto uni = [&](uint32_t lo, uint32_t hi) { return std::uniform_int_distribution<uint32_t>(lo, hi)(rng); };
    // the pool the alphabets are drawn from: both corpora draw from it, so they share some symbols and miss others
    std::vector<uint32_t> pool;
    for (uint32_t c = 0x20; c < 0x100; ++c) pool.push_back(c);        // Latin-1 (a byte corpus can hold these)
    for (uint32_t c = 0x370; c < 0x400; ++c) pool.push_back(c);       // Greek
    for (uint32_t c = 0x400; c < 0x500; ++c) pool.push_back(c);       // Cyrillic
    for (uint32_t c = 0x4E00; c < 0x4F00; ++c) pool.push_back(c);     // CJK
    pool.push_back(0xFFFF), pool.push_back(0x10000);                  // the BMP's last and the first beyond it
    for (uint32_t c = 0x1F600; c < 0x1F680; ++c) pool.push_back(c);   // above the BMP
    for (uint32_t c = 0x10FF00; c < 0x10FF40; ++c) pool.push_back(c);

    auto make = [&](bool wide, uint32_t n_syms) {
        Corpus k;
        k.wide = wide;
        std::iota(k.sigma, k.sigma + 256, (uint8_t)0);
        if (uni(0, 5)) std::shuffle(k.sigma, k.sigma + 256, rng);  // (sometimes the identity: RF_NO_RENAME)
        for (uint32_t& s : k.sym_of_id) s = kXlatNoSymbol;
        if (!wide) return k;
        std::vector<uint32_t> syms = pool;
        std::shuffle(syms.begin(), syms.end(), rng);  // the frequency ranking: the first 254 get the ids in rank order
        syms.resize(std::min<size_t>(n_syms, syms.size()));
        for (size_t r = 0; r < syms.size(); ++r) {
            if (r < kXlatOverflowId)
                k.alphabet[syms[r]] = (uint8_t)r, k.sym_of_id[r] = syms[r];
            else
                k.overflow.insert(syms[r]);
        }
        return k;
    };

    unsigned long long pairs = 0, symbols = 0, bad_seen = 0, absent_seen = 0, overflow_hits = 0, above_bmp = 0, identities = 0, big = 0;
    for (int round = 0; round < 3000; ++round) {
        const bool qw = round % 4 >= 2, cw = round % 2 == 1;
        const uint32_t sizes[] = {1, 7, 120, 253, 254, 255, 300, 600};
        const Corpus q = make(qw, sizes[uni(0, 7)]), c = make(cw, sizes[uni(0, 7)]);
        big += (q.alphabet.size() + q.overflow.size() > 254) || (c.alphabet.size() + c.overflow.size() > 254);
        JoinXlat x;
        std::fill(x.row_of, x.row_of + 256, (uint8_t)0xAA), std::fill(x.bad, x.bad + 256, (uint8_t)0xAA);
        auto lookup = [&](uint32_t sym) -> uint32_t {
            auto a = c.alphabet.find(sym);
            if (a != c.alphabet.end()) return a->second;
            return c.overflow.count(sym) ? kXlatOverflowId : kXlatAbsentId;
        };
        const bool ok = join_xlat_build(q.view(), c.view(), lookup, &x);
        CHECK(ok);
        if (!ok) continue;
        ++pairs;

        bool expect_bad[256] = {};
        bool stored[256] = {};
        // every symbol the query corpus stores under its own id, placed as resolve() places a query symbol
        auto place = [&](uint32_t sym, uint32_t id_q) {
            const uint8_t s = q.sigma[id_q];
            stored[s] = true;
            ++symbols;
            above_bmp += sym > 0xFFFF;
            if (!c.wide) {
                if (sym > 0xFF) {
                    expect_bad[s] = true;
                    return;
                }
                CHECK(x.row_of[s] == c.sigma[sym]);
                return;
            }
            auto a = c.alphabet.find(sym);
            if (a != c.alphabet.end()) {
                CHECK(x.row_of[s] == c.sigma[a->second]);
            } else if (c.overflow.count(sym)) {
                expect_bad[s] = true;
                ++overflow_hits;
            } else {
                CHECK(x.row_of[s] == c.sigma[kXlatAbsentId]);
                ++absent_seen;
            }
        };
        if (q.wide)
            for (const auto& kv : q.alphabet) place(kv.first, kv.second);
        else
            for (uint32_t b = 0; b < 256; ++b) place(b, b);
        if (q.wide && !q.overflow.empty()) stored[q.sigma[kXlatOverflowId]] = true, expect_bad[q.sigma[kXlatOverflowId]] = true;
        bool any = false;
        for (uint32_t s = 0; s < 256; ++s) {
            CHECK(x.bad[s] == (expect_bad[s] ? 1 : 0));
            if (!stored[s]) CHECK(x.bad[s] == 0);
            any = any || expect_bad[s];
            bad_seen += expect_bad[s];
        }
        CHECK(x.any_bad == any);
        // the absent row belongs to no id in use: a fused query's absent symbol matches no candidate byte
        if (c.wide) {
            for (const auto& kv : c.alphabet) CHECK(c.sigma[kv.second] != c.sigma[kXlatAbsentId]);
            if (!c.overflow.empty()) CHECK(c.sigma[kXlatOverflowId] != c.sigma[kXlatAbsentId]);
            // ... and no row of a placed symbol is the overflow id's: candidates' overflow symbols match no fused query
            for (uint32_t s = 0; s < 256; ++s)
                if (stored[s] && !expect_bad[s] && !c.overflow.empty()) CHECK(x.row_of[s] != c.sigma[kXlatOverflowId]);
        }
        // bytes x bytes: the composition the table build has always used
        if (!q.wide && !c.wide) {
            uint8_t inv[256];
            take_inverse_sigma(q.sigma, inv);
            for (uint32_t s = 0; s < 256; ++s) CHECK(x.row_of[s] == c.sigma[inv[s]]);
            CHECK(!x.any_bad);
            ++identities;
        }
        // a sigma under which the absent row is also a row in use is refused, and the output left alone
        if (c.wide && !c.alphabet.empty()) {
            Corpus broken = c;
            broken.sigma[kXlatAbsentId] = broken.sigma[c.alphabet.begin()->second];
            JoinXlat y;
            std::fill(y.row_of, y.row_of + 256, (uint8_t)0x55), std::fill(y.bad, y.bad + 256, (uint8_t)0x55);
            CHECK(!join_xlat_build(q.view(), broken.view(), lookup, &y));
            CHECK(y.row_of[0] == 0x55 && y.bad[255] == 0x55);
        }
    }
    std::printf("join xlat: %llu pairs, %llu symbols, %llu bad values, %llu absent, %llu in the other's overflow, %llu above the BMP, %llu with over 254 symbols, %llu byte identities, failures %d\n",
                pairs, symbols, bad_seen, absent_seen, overflow_hits, above_bmp, big, identities, failures);
    return failures ? 1 : 0;
}

// The host half of rf_filter_multi_f64 (rapidfuzz_rs_amd/csrc/rf_filter_multi_rows.hpp) as a plain host program: synthetic key rows --
// norm_key(dist, maximum) << 32 | index, in a scrambled order of arrival -- go through filter_multi_f64_row() and come back as the pairs a direct
// (double)dist / (double)maximum computation gives, in the order asked for.  Covers equal ratios from different (dist, maximum) pairs tied by
// index, key 0 (dist == 0, and maximum == 0), the clamp 0xFFFFFFFF (dist == maximum), both ops, the three orders, an index_base beyond 32 bits and
// an empty row.  Built with -fsanitize=address,undefined by tests/test_filter_multi_f64_rows.py; exit status 0 and "rows ok" = all as expected.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rf_filter_multi_rows.hpp"

struct Cand {
    uint32_t dist, maximum, index;
};

static double direct(const Cand& c, bool as_distance)
{
    const double nd = c.maximum == 0 ? 0.0 : (double)c.dist / (double)c.maximum;  // emit_fin's arithmetic
    return as_distance ? nd : 1.0 - nd;
}
static uint64_t bits(double v)
{
    uint64_t b;
    std::memcpy(&b, &v, sizeof b);
    return b;
}

static int failures = 0;
#define EXPECT(c)                                                     \
    do {                                                              \
        if (!(c)) {                                                   \
            std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); \
            ++failures;                                               \
        }                                                             \
    } while (0)

static void check(const std::vector<Cand>& cands, rf_filter_order order, bool as_distance, uint64_t base)
{
    std::vector<uint64_t> keys;
    for (const Cand& c : cands) keys.push_back(((uint64_t)rf::norm_key(c.dist, c.maximum) << 32) | c.index);
    const std::vector<uint64_t> arrived = keys;
    std::vector<uint64_t> index(cands.size() + 1, 77);
    std::vector<double> score(cands.size() + 1, 77.0);
    rf::filter_multi_f64_row(keys.data(), keys.size(), order, as_distance, base, index.data(), score.data());
    EXPECT(index.back() == 77 && score.back() == 77.0);  // nothing beyond `have`

    // the expectation, from the candidates alone: ascending index, or best score first with ties by index, or the order of arrival
    std::vector<Cand> want = cands;
    if (order == RF_FILTER_BY_INDEX)
        std::sort(want.begin(), want.end(), [](const Cand& a, const Cand& b) { return a.index < b.index; });
    else if (order == RF_FILTER_BY_SCORE)
        std::sort(want.begin(), want.end(), [&](const Cand& a, const Cand& b) {
            const double va = direct(a, as_distance), vb = direct(b, as_distance);
            if (va != vb) return as_distance ? va < vb : va > vb;
            return a.index < b.index;
        });
    for (size_t m = 0; m < want.size(); ++m) {
        EXPECT(index[m] == base + want[m].index);
        EXPECT(bits(score[m]) == bits(direct(want[m], as_distance)));
    }
    if (order == RF_FILTER_ANY) EXPECT(keys == arrived);
}

int main()
{
    // 4/20 = 5/25 = 8/40 = 10/50 = 0.2 at scattered indices, 1/3 = 2/6 = 21845/65535, the clamp (7/7, 65535/65535, 1/1), key 0 (0/20, 0/65535 and
    // 0/0), neighbours of the largest maximum, and ratios whose quotients are not exact in binary
    const std::vector<Cand> cands{
        {10, 50, 900},  {4, 20, 17},   {8, 40, 3},      {5, 25, 512},     {1, 3, 40},       {2, 6, 39},      {21845, 65535, 41}, {7, 7, 5},
        {65535, 65535, 4}, {1, 1, 6},  {0, 20, 1000},   {0, 65535, 999},  {0, 0, 998},      {65534, 65535, 8}, {65533, 65534, 9}, {1, 65535, 10},
        {1, 65534, 11}, {3, 64, 12},   {6, 128, 13},    {1, 10, 14},      {13, 130, 4000000000u}, {19, 20, 15}, {32767, 65535, 16}, {32768, 65535, 18},
    };
    for (rf_filter_order order : {RF_FILTER_BY_INDEX, RF_FILTER_BY_SCORE, RF_FILTER_ANY})
        for (bool as_distance : {true, false})
            for (uint64_t base : {(uint64_t)0, ((uint64_t)1 << 40) + 5}) {
                check(cands, order, as_distance, base);
                std::vector<Cand> rev(cands.rbegin(), cands.rend());  // another order of arrival
                check(rev, order, as_distance, base);
                check({}, order, as_distance, base);
                check({cands[7]}, order, as_distance, base);
            }
    // the ties are what they are said to be: one key for equal ratios, so the index alone orders them
    EXPECT(rf::norm_key(4, 20) == rf::norm_key(5, 25) && rf::norm_key(5, 25) == rf::norm_key(8, 40) && rf::norm_key(8, 40) == rf::norm_key(10, 50));
    EXPECT(rf::norm_key(0, 20) == 0 && rf::norm_key(0, 0) == 0 && rf::norm_key(7, 7) == 0xFFFFFFFFu && rf::norm_key(65535, 65535) == 0xFFFFFFFFu);
    {
        std::vector<uint64_t> keys;
        for (const Cand& c : {cands[0], cands[1], cands[2], cands[3]}) keys.push_back(((uint64_t)rf::norm_key(c.dist, c.maximum) << 32) | c.index);
        uint64_t index[4];
        double score[4];
        rf::filter_multi_f64_row(keys.data(), 4, RF_FILTER_BY_SCORE, false, 0, index, score);
        EXPECT(index[0] == 3 && index[1] == 17 && index[2] == 512 && index[3] == 900);
        for (double s : score) EXPECT(bits(s) == bits(1.0 - 4.0 / 20.0));
    }
    if (failures) return 1;
    std::printf("rows ok\n");
    return 0;
}

// The grouping rule of the multi-query calls (rapidfuzz_rs_amd/csrc/rf_multi_group.hpp) against a second statement of it: every assignment of {not fusable, key A,
// key B} to up to 9 queries, members free or contiguous, checked property by property -- not against a copy of the loop.  Also norm_key_fits (rf_norm_key.hpp) on
// each side of 65535.  Host only (tests/test_multi_group.py builds it with -fsanitize=address,undefined).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "rf_multi_group.hpp"
#include "rf_norm_key.hpp"

using namespace rf;

static int failures = 0;
static unsigned long long shape_code = 0;
static uint32_t shape_q = 0;
static bool shape_contiguous = false;
#define CHECK(cond)                                                                                                                                               \
    do {                                                                                                                                                          \
        if (!(cond)) {                                                                                                                                            \
            if (++failures <= 20) std::fprintf(stderr, "line %d: %s  (q=%u assignment=%llu base 3, contiguous=%d)\n", __LINE__, #cond, shape_q, shape_code, (int)shape_contiguous); \
        }                                                                                                                                                         \
    } while (0)

// what the rule promises for ONE key whose fusable queries are `members` (ascending): the groups take them in order, fours first, then one pair out of a rest of 2 or
// 3; a rest of 1, and the third of 3, stay behind.  Contiguous: the same within every run of neighbouring indices.
static std::vector<std::vector<uint32_t>> expected_for_key(const std::vector<uint32_t>& members, bool contiguous)
{
    std::vector<std::vector<uint32_t>> runs;
    for (const uint32_t m : members) {
        if (runs.empty() || (contiguous && m != runs.back().back() + 1)) runs.emplace_back();
        runs.back().push_back(m);
    }
    std::vector<std::vector<uint32_t>> groups;
    for (const auto& run : runs) {
        size_t at = 0;
        for (; run.size() - at >= 4; at += 4) groups.emplace_back(run.begin() + at, run.begin() + at + 4);
        if (run.size() - at >= 2) groups.emplace_back(run.begin() + at, run.begin() + at + 2);
    }
    return groups;
}

int main()
{
    const MultiGroupKey A{0, 0, 1, 0, false}, B{0, 0, 1, 0, true};  // (they differ in the word width alone)
    CHECK(A == A && !(A == B));
    CHECK(!(A == MultiGroupKey{1, 0, 1, 0, false}) && !(A == MultiGroupKey{0, 2, 1, 0, false}) && !(A == MultiGroupKey{0, 0, 2, 0, false}) && !(A == MultiGroupKey{0, 0, 1, 3, false}));
    CHECK(fusable_base(0, 1, 0) && fusable_base(1, 1, 0));
    CHECK(!fusable_base(2, 1, 0) && !fusable_base(3, 1, 0) && !fusable_base(0, 2, 0) && !fusable_base(1, 1, 8));

    unsigned long checked = 0;
    for (int contiguous = 0; contiguous <= 1; ++contiguous)
        for (uint32_t q = 0; q <= 9; ++q) {
            unsigned long long n_assign = 1;
            for (uint32_t i = 0; i < q; ++i) n_assign *= 3;
            for (unsigned long long code = 0; code < n_assign; ++code) {
                shape_code = code, shape_q = q, shape_contiguous = contiguous != 0;
                std::vector<MultiQuery> qs(q);
                std::vector<uint32_t> of_key[2];
                unsigned long long c = code;
                for (uint32_t i = 0; i < q; ++i, c /= 3) {
                    const uint32_t what = (uint32_t)(c % 3);  // 0: not fusable (its key is not looked at: give it A's), 1: A, 2: B
                    qs[i] = MultiQuery{what != 0, what == 2 ? B : A};
                    if (what) of_key[what - 1].push_back(i);
                }
                const MultiGroups r = group_queries(qs, 4, contiguous != 0);

                // every group: 2 or 4 fusable members of one key, ascending (neighbours when contiguous); nobody twice; taken = the union
                CHECK(r.taken.size() == q);
                std::vector<int> times(q, 0);
                for (const auto& g : r.groups) {
                    CHECK(g.size() == 2 || g.size() == 4);
                    for (size_t m = 0; m < g.size(); ++m) {
                        CHECK(g[m] < q);
                        if (g[m] >= q) continue;
                        times[g[m]]++;
                        CHECK(qs[g[m]].fusable && qs[g[m]].key == qs[g[0]].key);
                        if (m) CHECK(contiguous ? g[m] == g[m - 1] + 1 : g[m] > g[m - 1]);
                    }
                }
                for (uint32_t i = 0; i < q && r.taken.size() == q; ++i) CHECK(times[i] <= 1 && (r.taken[i] != 0) == (times[i] == 1));
                // the groups come in ascending order of their first member: the fused rows are laid out in this order
                for (size_t g = 1; g < r.groups.size(); ++g) CHECK(r.groups[g][0] > r.groups[g - 1][0]);
                // key by key: exactly the promised groups (5 members: one group of 4, one member left; 3 members: one group of 2; ...)
                for (int key = 0; key < 2; ++key) {
                    std::vector<std::vector<uint32_t>> got;
                    for (const auto& g : r.groups)
                        if (qs[g[0]].key == (key ? B : A)) got.push_back(g);
                    CHECK(got == expected_for_key(of_key[key], contiguous != 0));
                    if (!contiguous) {
                        size_t fours = 0, twos = 0;
                        for (const auto& g : got) (g.size() == 4 ? fours : twos)++;
                        CHECK(fours == of_key[key].size() / 4 && twos == (of_key[key].size() % 4 >= 2 ? 1u : 0u));
                    }
                }
                checked++;
            }
        }

    // norm_key_fits: the largest maximum a scan meets, fin_mS * (len1 + max_len) + fin_mM * max(len1, max_len), on each side of 65535
    shape_q = 0, shape_code = 0;
    CHECK(norm_key_fits(1, 0, 64, 65535 - 64) && !norm_key_fits(1, 0, 64, 65536 - 64));  // maximum = len1 + len2 (Indel)
    CHECK(norm_key_fits(1, 0, 65535, 0) && !norm_key_fits(1, 0, 65536, 0));
    CHECK(norm_key_fits(0, 1, 64, 65535) && !norm_key_fits(0, 1, 64, 65536));            // maximum = max(len1, len2) (LCS, Levenshtein)
    CHECK(norm_key_fits(0, 1, 65535, 64) && !norm_key_fits(0, 1, 65536, 64));
    CHECK(norm_key_fits(0, 3, 64, 21845) && !norm_key_fits(0, 3, 64, 21846));            // ... times a weight factor
    CHECK(norm_key_fits(3, 0, 64, 21845 - 64) && !norm_key_fits(3, 0, 64, 21846 - 64));
    CHECK(norm_key_fits(0, 0, 1u << 30, 1u << 30));                                       // (no maximum at all)

    if (failures) {
        std::fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    std::printf("multi group ok: %lu assignments\n", checked);
    return 0;
}

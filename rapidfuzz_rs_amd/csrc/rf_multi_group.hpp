// rf_multi_group.hpp -- THE rule by which the multi-query calls (rf_many_multi_*, rf_topk_multi_*, rf_filter_multi_*) put queries into fused launches.  Plain
// host code, no HIP call: rf_host.hpp's planner and run_many_multi include it, and so does a host-compiled test (tests/test_multi_group.py, which restates the rule).
//
// A query can be fused when its plan is a single-word Levenshtein / LCS-family recurrence without a long pattern (fusable_base) and the caller's own conditions
// hold; queries are fused with queries of the same MultiGroupKey -- what a fused kernel cannot vary per member -- 4 to a launch, then 2 (group_queries).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <utility>
#include <vector>

namespace rf {

constexpr uint32_t kMultiRawLev = 0, kMultiRawLcs = 1;  // RawKind's RAW_LEV / RAW_LCS (rf_host.hpp holds the two together): the recurrences the fused kernels have states for

inline bool fusable_base(uint32_t raw, uint32_t words, uint32_t long_words_pad) { return (raw == kMultiRawLev || raw == kMultiRawLcs) && words == 1 && !long_words_pad; }

// (op: what the kernel computes -- a fuzz ratio plans to RF_OP_NORMALIZED_SIMILARITY whichever similarity op was asked for)
struct MultiGroupKey {
    uint32_t raw, finish, factor, op;
    bool narrow;  // len1 <= 32: the 32-bit states
    bool operator==(const MultiGroupKey& o) const { return raw == o.raw && finish == o.finish && factor == o.factor && op == o.op && narrow == o.narrow; }
};
struct MultiQuery {
    bool fusable;
    MultiGroupKey key;  // (read of fusable queries only)
};
struct MultiGroups {
    std::vector<std::vector<uint32_t>> groups;  // members of each fused group as query indices, ascending; the groups in ascending order of their first member
    std::vector<char> taken;                    // [q] 1: the query is in a group
};

// Greedy, from the first untaken fusable query forward: collect up to max_group queries of its key; a group of 3 gives its last member back (the kernels are built
// for 2 and 4), a group of 1 is the odd one left over for the per-query road.  `contiguous` (rf_many_multi_*: a group writes neighbouring rows of one result
// matrix): a member must directly follow the member before it; otherwise rows are independent and members need not be neighbours.
inline MultiGroups group_queries(const std::vector<MultiQuery>& qs, size_t max_group, bool contiguous)
{
    const uint32_t q = (uint32_t)qs.size();
    MultiGroups r;
    r.taken.assign(q, 0);
    for (uint32_t i = 0; i < q; ++i) {
        if (r.taken[i] || !qs[i].fusable) continue;
        std::vector<uint32_t> g{i};
        for (uint32_t j = i + 1; j < q && g.size() < max_group; ++j)
            if (!r.taken[j] && qs[j].fusable && qs[j].key == qs[i].key && (!contiguous || j == g.back() + 1)) g.push_back(j);
        if (g.size() == 3) g.pop_back();
        if (g.size() < 2) continue;
        for (uint32_t m : g) r.taken[m] = 1;
        r.groups.push_back(std::move(g));
    }
    return r;
}

}  // namespace rf

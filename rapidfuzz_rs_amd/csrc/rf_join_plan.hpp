// rf_join_plan.hpp -- the work list of rf_join_u32 / rf_join_f64 / rf_join_topk_u32 (rf_api_join.hip builds it, rf_join.hip join_kernel and rf_join_topk.hip join_topk_kernel
// walk it): which queries of a batch share a work item,
// which tiles an item visits, and which workgroup unit walks which part of them.  Plain arithmetic, no HIP call: the host and the kernel compile the same
// join_unit(), and host-compiled tests (tests/cpp/join_plan_check.cpp, tests/cpp/join_topk_plan_check.cpp) check all of it without a device.
//
//   query      a fusable row of the query corpus: its length, its position in Q, its row index, and its plan's tile window [tile_begin, tile_end)
//   batch      the queries [from, to) of the call's list SORTED by (length, position): table b of the batch belongs to query from + b
//   item       up to kJoinMembers neighbouring queries of one class (narrow: <= 32 symbols -- the 32-bit states; wide: 33..64) with the union of their
//              windows; neighbours in length order have (nearly) the same window, so the union reads little that no member wants
//   unit       kJoinSpan consecutive tiles of one item: what a workgroup stages the item's tables for.  prefix[i] = units before item i; unit u belongs to
//              the item with prefix[i] <= u < prefix[i + 1] and covers tiles tile_begin + (u - prefix[i]) * span ... (+ span, clipped to tile_end)
//   span       tiles per unit.  The joins use kJoinSpan.  rf_join_topk_u32 keeps one k-entry list per (unit, member), so it wants few, long units: its span is
//              join_topk_span()'s -- as long as the batch still makes about as many units as the device runs workgroups -- and a member's lists fill a SEGMENT
//              of join_topk_seg_units() x k keys, the unit with ordinal u - prefix[i] at ordinal * k
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RF_JP_HD __host__ __device__ __forceinline__
#else
#define RF_JP_HD inline
#endif

namespace rf {

constexpr uint32_t kJoinMembers = 4;   // queries per work item: the recurrences a lane of join_kernel carries (= kMaxMulti)
constexpr uint32_t kJoinSpan = 128;    // tiles per unit: 32 per wavefront for one 8 KiB table stage
constexpr uint32_t kJoinMaxLen = 64;   // longest query the single-word states hold
constexpr uint32_t kJoinNarrowLen = 32;

struct JoinItem {  // 64 bytes
    uint32_t len1[kJoinMembers];  // the members' lengths (0 beyond `members`)
    uint32_t qpos[kJoinMembers];  // their positions in Q
    uint32_t qidx[kJoinMembers];  // their row indices in the query corpus (RF_JOIN_UPPER compares candidates against it)
    uint32_t members;             // 1..kJoinMembers
    uint32_t tile_begin, tile_end;  // the union of the members' windows (tile_begin == tile_end: nothing to visit)
    uint32_t table0;              // member q reads table table0 + q of the batch
};
struct JoinUnit {
    uint32_t item, tile_begin, tile_end;
};

RF_JP_HD uint32_t join_units_of(uint32_t tile_begin, uint32_t tile_end, uint32_t span) { return tile_end > tile_begin ? (tile_end - tile_begin + span - 1) / span : 0u; }

// unit u < prefix[n_items] -> its item and tiles.  prefix has n_items + 1 ascending entries, prefix[0] == 0.
RF_JP_HD JoinUnit join_unit(const uint32_t* prefix, uint32_t n_items, const JoinItem* items, uint32_t span, uint32_t u)
{
    uint32_t lo = 0, hi = n_items;  // prefix[lo] <= u < prefix[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (prefix[mid] <= u)
            lo = mid;
        else
            hi = mid;
    }
    JoinUnit r;
    r.item = lo;
    const uint32_t b = items[lo].tile_begin, e = items[lo].tile_end;
    const uint64_t t0 = (uint64_t)b + (uint64_t)(u - prefix[lo]) * span;
    r.tile_begin = t0 < e ? (uint32_t)t0 : e;
    r.tile_end = t0 + span < e ? (uint32_t)(t0 + span) : e;
    return r;
}

// rf_join_topk_u32: the span of a batch of n_items items over a corpus of n_tiles tiles, so that the batch makes about target_units units when the work allows it:
// every item gets target_units / n_items units (at least one), i.e. its window -- at most the whole corpus -- is cut into spans of ceil(n_tiles / that).  Never
// below kJoinSpan (a unit pays a table stage and a list merge: 32 tiles per wavefront carry that), unless the target is FORCED (RF_JOIN_TOPK_UNITS: tests and
// A/B measurements), when any span down to one tile is taken.
RF_JP_HD uint32_t join_topk_span(uint32_t n_tiles, uint32_t n_items, uint32_t target_units, bool forced = false)
{
    const uint32_t per_item = n_items && target_units > n_items ? target_units / n_items : 1u;
    uint32_t span = n_tiles / per_item + (n_tiles % per_item != 0);
    if (span == 0) span = 1;
    return forced || span >= kJoinSpan ? span : kJoinSpan;
}
// ... and the most units any item has under that span (its window is at most [0, n_tiles)): the unit capacity of a member's segment.  At least 1.
RF_JP_HD uint32_t join_topk_seg_units(uint32_t n_tiles, uint32_t span)
{
    const uint32_t u = join_units_of(0, n_tiles, span);
    return u ? u : 1u;
}

}  // namespace rf

// ---- host side
#include <algorithm>
#include <vector>

namespace rf {

struct JoinQuery {
    uint32_t len, pos, idx;
    uint32_t tile_begin, tile_end;  // the plan's window for this length
};
inline bool join_narrow(uint32_t len) { return len <= kJoinNarrowLen; }
inline void join_sort(std::vector<JoinQuery>& qs)
{
    std::sort(qs.begin(), qs.end(), [](const JoinQuery& a, const JoinQuery& b) { return a.len != b.len ? a.len < b.len : a.pos < b.pos; });
}

struct JoinList {
    std::vector<JoinItem> items;
    std::vector<uint32_t> prefix;  // items.size() + 1
    uint32_t units() const { return prefix.empty() ? 0u : prefix.back(); }
};

// The items of one class out of the batch qs[from, to) (sorted): neighbours of that class, kJoinMembers at a time -- so a class of c queries makes
// ceil(c / kJoinMembers) items and no query is left over.  A member with an empty window takes no part in the union.
inline JoinList join_items(const std::vector<JoinQuery>& qs, size_t from, size_t to, bool narrow, uint32_t n_tiles, uint32_t span)
{
    JoinList l;
    for (size_t i = from; i < to;) {
        if (join_narrow(qs[i].len) != narrow) {
            ++i;
            continue;
        }
        JoinItem it{};
        it.table0 = (uint32_t)(i - from);
        uint32_t t0 = n_tiles, t1 = 0;
        while (i < to && it.members < kJoinMembers && join_narrow(qs[i].len) == narrow) {
            const JoinQuery& q = qs[i];
            it.len1[it.members] = q.len, it.qpos[it.members] = q.pos, it.qidx[it.members] = q.idx;
            if (q.tile_begin < q.tile_end) t0 = std::min(t0, q.tile_begin), t1 = std::max(t1, std::min(q.tile_end, n_tiles));
            ++it.members, ++i;
        }
        it.tile_begin = t0, it.tile_end = std::max(t0, t1);
        l.items.push_back(it);
    }
    l.prefix.assign(l.items.size() + 1, 0);
    for (size_t k = 0; k < l.items.size(); ++k) l.prefix[k + 1] = l.prefix[k] + join_units_of(l.items[k].tile_begin, l.items[k].tile_end, span);
    return l;
}

// What a launch checks before it runs (rf_join.hip launch_join): every tile a unit can name lies inside its item's window and the corpus, every table inside
// the batch, every length inside its class.
inline bool join_valid(const JoinItem* items, const uint32_t* prefix, uint32_t n_items, uint32_t n_units, uint32_t n_tiles, uint32_t batch, bool narrow, uint32_t span)
{
    if (span == 0 || prefix[0] != 0 || prefix[n_items] != n_units) return false;
    for (uint32_t k = 0; k < n_items; ++k) {
        const JoinItem& it = items[k];
        if (it.members < 1 || it.members > kJoinMembers) return false;
        if (it.tile_begin > it.tile_end || it.tile_end > n_tiles) return false;
        if (it.table0 >= batch || it.members > batch - it.table0) return false;
        if (prefix[k + 1] < prefix[k] || prefix[k + 1] - prefix[k] != join_units_of(it.tile_begin, it.tile_end, span)) return false;
        for (uint32_t q = 0; q < it.members; ++q)
            if (it.len1[q] > kJoinMaxLen || join_narrow(it.len1[q]) != narrow) return false;
    }
    return true;
}

}  // namespace rf

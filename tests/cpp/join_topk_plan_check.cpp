// The span rule of rf_join_topk_u32 (rapidfuzz_rs_amd/csrc/rf_join_plan.hpp join_topk_span / join_topk_seg_units) on the host, with no device: for random
// batches of query lengths over random corpora, with the whole corpus as every window (no cutoff) or a length window (a loose cutoff), under the span the rule
// gives for an automatic target and for the forced targets 1 and 2^20 --
//   every (query, tile of its window) lies in exactly one unit of the one item that holds the query;
//   every unit's ordinal within its item is below join_topk_seg_units(): the place ordinal * k + lane lies inside the member's segment of seg_units * k keys,
//     and no two units of an item share an ordinal;
//   join_valid() accepts the list under that span;
//   the automatic span is never below kJoinSpan and the batch's units stay within target + items; a forced target of 1 makes one unit per item with tiles, a
//     forced target of 2^20 spans of one tile wherever the batch has fewer than 2^20 / tiles items.
// tests/test_join_topk_plan.py builds this twice, plainly and under AddressSanitizer + UndefinedBehaviorSanitizer.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>
#include <vector>

#include "rf_join_plan.hpp"

using namespace rf;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            if (++failures < 20) std::printf("line %d: %s\n", __LINE__, #cond); \
        }                                                                  \
    } while (0)

int main()
{
    std::mt19937 rng(20261021);
    auto uni = [&](uint32_t lo, uint32_t hi) { return std::uniform_int_distribution<uint32_t>(lo, hi)(rng); };
    unsigned long long lists = 0, units_seen = 0, pairs_seen = 0;
    for (int round = 0; round < 240; ++round) {
        // a corpus: tiles ascending by length 0..70, some lengths absent; every fourth round a large one
        std::vector<uint32_t> tile_len;
        for (uint32_t len = 0; len <= 70; ++len) {
            const uint32_t c = uni(0, 3) == 0 ? 0 : uni(1, round % 4 == 0 ? 400 : 12);
            for (uint32_t i = 0; i < c; ++i) tile_len.push_back(len);
        }
        const uint32_t n_tiles = (uint32_t)tile_len.size();
        const bool windowed = round % 3 == 1;  // a loose cutoff: the window of a length = the tiles within 40 symbols of it
        const uint32_t m = uni(1, 90);
        std::vector<JoinQuery> qs;
        for (uint32_t j = 0; j < m; ++j) {
            const uint32_t len = uni(0, 64);
            uint32_t b = 0, e = n_tiles;
            if (windowed) {
                b = n_tiles, e = 0;
                for (uint32_t t = 0; t < n_tiles; ++t)
                    if ((tile_len[t] > len ? tile_len[t] - len : len - tile_len[t]) <= 40) b = std::min(b, t), e = t + 1;
                if (b >= e) b = e = 0;
            }
            qs.push_back(JoinQuery{len, j, uni(0, 1000), b, e});
        }
        join_sort(qs);
        const uint32_t B = uni(1, 40);
        const uint32_t auto_target = uni(1, 9000);
        for (size_t from = 0; from < qs.size(); from += B) {
            const size_t to = std::min(qs.size(), from + B);
            const uint32_t bn = (uint32_t)(to - from);
            uint32_t in_class[2] = {0, 0};
            for (size_t i = from; i < to; ++i) ++in_class[join_narrow(qs[i].len) ? 0 : 1];
            const uint32_t n_items = (in_class[0] + kJoinMembers - 1) / kJoinMembers + (in_class[1] + kJoinMembers - 1) / kJoinMembers;
            struct Mode {
                uint32_t target;
                bool forced;
            };
            for (const Mode mode : {Mode{auto_target, false}, Mode{1u, true}, Mode{1u << 20, true}}) {
                const uint32_t span = join_topk_span(n_tiles, n_items, mode.target, mode.forced);
                const uint32_t seg_units = join_topk_seg_units(n_tiles, span);
                CHECK(span >= 1 && seg_units >= 1);
                CHECK((uint64_t)seg_units * span >= n_tiles);
                if (!mode.forced) CHECK(span >= kJoinSpan);
                if (mode.forced && mode.target == 1) CHECK(span >= n_tiles && seg_units == 1);
                if (mode.forced && mode.target == (1u << 20) && (uint64_t)n_items * n_tiles <= (1u << 20)) CHECK(span == 1);
                std::map<std::pair<uint32_t, uint32_t>, int> visits;  // (place in batch, tile) -> times visited
                uint64_t batch_units = 0;
                for (int cls = 0; cls < 2; ++cls) {
                    const bool narrow = cls == 0;
                    const JoinList l = join_items(qs, from, to, narrow, n_tiles, span);
                    ++lists;
                    if (l.items.empty()) continue;
                    CHECK(join_valid(l.items.data(), l.prefix.data(), (uint32_t)l.items.size(), l.units(), n_tiles, bn, narrow, span));
                    batch_units += l.units();
                    std::vector<std::set<uint32_t>> ordinals(l.items.size());
                    for (uint32_t u = 0; u < l.units(); ++u) {
                        const JoinUnit un = join_unit(l.prefix.data(), (uint32_t)l.items.size(), l.items.data(), span, u);
                        ++units_seen;
                        CHECK(un.item < l.items.size());
                        if (un.item >= l.items.size()) continue;
                        const JoinItem& it = l.items[un.item];
                        const uint32_t ord = u - l.prefix[un.item];
                        CHECK(ord < seg_units);  // the unit's list has a place in its members' segments ...
                        CHECK(ordinals[un.item].insert(ord).second);  // ... of its own
                        CHECK(un.tile_begin < un.tile_end && un.tile_end <= it.tile_end && un.tile_begin >= it.tile_begin && un.tile_end <= n_tiles);
                        for (uint32_t t = un.tile_begin; t < un.tile_end; ++t)
                            for (uint32_t q = 0; q < it.members; ++q) ++visits[{it.table0 + q, t}];
                    }
                    for (size_t i = 0; i < l.items.size(); ++i) {
                        CHECK(l.prefix[i + 1] - l.prefix[i] <= seg_units);
                        if (mode.forced && mode.target == 1) CHECK(l.prefix[i + 1] - l.prefix[i] == (l.items[i].tile_begin < l.items[i].tile_end ? 1u : 0u));
                    }
                }
                if (!mode.forced) CHECK(batch_units <= (uint64_t)std::max(mode.target, n_items) + n_items);
                for (uint32_t b = 0; b < bn; ++b) {
                    const JoinQuery& q = qs[from + b];
                    for (uint32_t t = q.tile_begin; t < q.tile_end; ++t) {
                        CHECK((visits[{b, t}] == 1));
                        ++pairs_seen;
                    }
                }
                for (const auto& kv : visits) CHECK(kv.second == 1);
            }
        }
    }
    // the rule at the sizes of a real device: 10 M candidates are 156250 tiles; a full batch of 16384 rows has 4096 items
    CHECK(join_topk_span(156250, 4096, 8192) == 78125 && join_topk_seg_units(156250, 78125) == 2);
    CHECK(join_topk_span(156250, 1, 8192) == kJoinSpan && join_topk_seg_units(156250, kJoinSpan) == 1221);
    CHECK(join_topk_span(157, 16, 8192) == kJoinSpan && join_topk_seg_units(157, kJoinSpan) == 2);
    CHECK(join_topk_span(0, 3, 8192) == kJoinSpan && join_topk_seg_units(0, kJoinSpan) == 1);
    CHECK(join_topk_span(157, 16, 0) == 157 && join_topk_span(157, 0, 8192) == 157);  // (no target, no items: one unit per item)
    std::printf("join topk plan: %llu lists, %llu units, %llu (query, tile) pairs, failures %d\n", lists, units_seen, pairs_seen, failures);
    return failures ? 1 : 0;
}

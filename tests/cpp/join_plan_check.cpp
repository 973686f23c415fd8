// The work-list arithmetic of rf_join_u32 (rapidfuzz_rs_amd/csrc/rf_join_plan.hpp) on the host, with no device: for random multisets of query lengths, random
// corpora of tiles ascending by length and random cutoffs, batch by batch --
//   every (query, tile in its window) is visited by exactly one unit of exactly one item that holds the query, and no unit names a tile outside its item's window
//     or the corpus;
//   no item mixes the classes (<= 32 / 33..64 symbols), every item has 1..4 members, a class of c queries makes ceil(c / 4) items, and the members' tables are
//     the neighbours table0 .. table0 + members - 1 of the batch, each query's table its place in the batch;
//   the prefix table maps every unit u < units() into a valid (item, sub-range) through join_unit() -- the function the kernel runs -- and the sub-ranges of an
//     item cover its window once, without overlap, each at most `span` tiles;
//   join_valid() accepts every list built here and refuses lists with a tile beyond the corpus, a table beyond the batch, a wrong prefix or a mixed class.
// tests/test_join_plan.py builds this twice, plainly and under AddressSanitizer + UndefinedBehaviorSanitizer.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
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
    std::mt19937 rng(20261020);
    auto uni = [&](uint32_t lo, uint32_t hi) { return std::uniform_int_distribution<uint32_t>(lo, hi)(rng); };
    unsigned long long cases = 0, units_seen = 0, pairs_seen = 0;
    for (int round = 0; round < 400; ++round) {
        // a corpus: tiles ascending by length 0..70, some lengths absent
        std::vector<uint32_t> tile_len;
        for (uint32_t len = 0; len <= 70; ++len) {
            const uint32_t k = uni(0, 3) == 0 ? 0 : uni(1, round % 7 == 0 ? 300 : 9);
            for (uint32_t i = 0; i < k; ++i) tile_len.push_back(len);
        }
        const uint32_t n_tiles = (uint32_t)tile_len.size();
        const uint32_t cutoff = uni(0, 6);
        const uint32_t span = round % 3 == 0 ? kJoinSpan : uni(1, 17);
        // queries: a random multiset of lengths 0..64; the window of a length = the tiles whose length is within the cutoff (a length-difference rule, as plan()'s)
        const uint32_t m = uni(1, 70);
        std::vector<JoinQuery> qs;
        for (uint32_t j = 0; j < m; ++j) {
            const uint32_t len = round % 5 == 0 ? uni(30, 35) : uni(0, 64);
            uint32_t b = n_tiles, e = 0;
            for (uint32_t t = 0; t < n_tiles; ++t)
                if ((tile_len[t] > len ? tile_len[t] - len : len - tile_len[t]) <= cutoff) b = std::min(b, t), e = t + 1;
            if (b >= e) b = e = 0;
            qs.push_back(JoinQuery{len, j, uni(0, 1000), b, e});
        }
        join_sort(qs);
        for (size_t i = 1; i < qs.size(); ++i) CHECK(qs[i - 1].len < qs[i].len || (qs[i - 1].len == qs[i].len && qs[i - 1].pos < qs[i].pos));
        const uint32_t B = uni(1, 24);
        for (size_t from = 0; from < qs.size(); from += B) {
            const size_t to = std::min(qs.size(), from + B);
            const uint32_t bn = (uint32_t)(to - from);
            std::map<std::pair<uint32_t, uint32_t>, int> visits;  // (place in batch, tile) -> times visited
            uint32_t in_class[2] = {0, 0};
            for (size_t i = from; i < to; ++i) ++in_class[join_narrow(qs[i].len) ? 0 : 1];
            std::vector<int> table_used(bn, 0);
            for (int cls = 0; cls < 2; ++cls) {
                const bool narrow = cls == 0;
                const JoinList l = join_items(qs, from, to, narrow, n_tiles, span);
                ++cases;
                CHECK(l.items.size() == (in_class[cls] + kJoinMembers - 1) / kJoinMembers);
                CHECK(l.prefix.size() == l.items.size() + 1 && l.prefix[0] == 0);
                if (l.items.empty()) {
                    CHECK(l.units() == 0);
                    continue;
                }
                CHECK(join_valid(l.items.data(), l.prefix.data(), (uint32_t)l.items.size(), l.units(), n_tiles, bn, narrow, span));
                for (const JoinItem& it : l.items) {
                    CHECK(it.members >= 1 && it.members <= kJoinMembers);
                    CHECK(it.table0 + it.members <= bn);
                    for (uint32_t q = 0; q < it.members; ++q) {
                        const JoinQuery& src = qs[from + it.table0 + q];
                        CHECK(join_narrow(it.len1[q]) == narrow);
                        CHECK(src.len == it.len1[q] && src.pos == it.qpos[q] && src.idx == it.qidx[q]);
                        CHECK(src.tile_begin == src.tile_end || (it.tile_begin <= src.tile_begin && src.tile_end <= it.tile_end));
                        ++table_used[it.table0 + q];
                    }
                }
                // every unit through the kernel's own lookup
                std::vector<uint32_t> next_tile(l.items.size());
                for (size_t k = 0; k < l.items.size(); ++k) next_tile[k] = l.items[k].tile_begin;
                for (uint32_t u = 0; u < l.units(); ++u) {
                    const JoinUnit un = join_unit(l.prefix.data(), (uint32_t)l.items.size(), l.items.data(), span, u);
                    ++units_seen;
                    CHECK(un.item < l.items.size());
                    if (un.item >= l.items.size()) continue;
                    const JoinItem& it = l.items[un.item];
                    CHECK(l.prefix[un.item] <= u && u < l.prefix[un.item + 1]);
                    CHECK(un.tile_begin < un.tile_end && un.tile_end - un.tile_begin <= span);
                    CHECK(un.tile_begin >= it.tile_begin && un.tile_end <= it.tile_end && un.tile_end <= n_tiles);
                    CHECK(un.tile_begin == next_tile[un.item]);  // units of an item in order, gapless, no overlap
                    next_tile[un.item] = un.tile_end;
                    for (uint32_t t = un.tile_begin; t < un.tile_end; ++t)
                        for (uint32_t q = 0; q < it.members; ++q) ++visits[{it.table0 + q, t}];
                }
                for (size_t k = 0; k < l.items.size(); ++k) CHECK(next_tile[k] == l.items[k].tile_end);
                // refusals
                {
                    JoinList w = l;
                    w.items[0].tile_end = n_tiles + 1;
                    CHECK(!join_valid(w.items.data(), w.prefix.data(), (uint32_t)w.items.size(), w.units(), n_tiles, bn, narrow, span));
                    w = l;
                    w.items.back().table0 = bn;
                    CHECK(!join_valid(w.items.data(), w.prefix.data(), (uint32_t)w.items.size(), w.units(), n_tiles, bn, narrow, span));
                    w = l;
                    w.prefix.back() += 1;
                    CHECK(!join_valid(w.items.data(), w.prefix.data(), (uint32_t)w.items.size(), w.units() - 1, n_tiles, bn, narrow, span));
                    CHECK(!join_valid(w.items.data(), w.prefix.data(), (uint32_t)w.items.size(), w.units(), n_tiles, bn, narrow, span));
                    w = l;
                    w.items[0].len1[0] = narrow ? 33 : 32;
                    CHECK(!join_valid(w.items.data(), w.prefix.data(), (uint32_t)w.items.size(), w.units(), n_tiles, bn, narrow, span));
                    w = l;
                    w.items[0].members = kJoinMembers + 1;
                    CHECK(!join_valid(w.items.data(), w.prefix.data(), (uint32_t)w.items.size(), w.units(), n_tiles, bn, narrow, span));
                }
            }
            for (uint32_t b = 0; b < bn; ++b) CHECK(table_used[b] == 1);  // every query of the batch is in exactly one item
            // every (query, tile of its window) exactly once; tiles outside a window at most once (the union reads them, the kernel's compare drops them)
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
    std::printf("join plan: %llu lists, %llu units, %llu (query, tile) pairs, failures %d\n", cases, units_seen, pairs_seen, failures);
    return failures ? 1 : 0;
}

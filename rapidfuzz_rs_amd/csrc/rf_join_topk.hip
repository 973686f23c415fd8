// rf_join_topk.hip -- the k best candidates for every row of a packed corpus (rf_join_topk_u32 / rf_join_topk_f64; host side in rf_api_join.hip, the work list in rf_join_plan.hpp,
// the tables by rf_join.hip join_pm_kernel).
//   join_topk_kernel         join_kernel's unit loop and table staging around topk_multi_kernel's tile body: a workgroup walks units blockIdx.x, + gridDim.x, ...;
//                            per unit it stages the item's (up to) 4 tables into LDS, its four wavefronts walk the unit's tiles -- 4 recurrences per lane, the next
//                            chunk in flight across tile ends, no look and no `live` mask: there is no early-out -- and at a tile's end every member of the item
//                            is offered one key per lane, (value, ~value or -- kNorm -- norm_key) << 32 | local candidate index, into that member's register-resident WaveTopK list.
//                            Slots beyond it->members run on a zero table (uniform control flow) and are never offered.  TWO guards name `members`, and they are
//                            not alike: the one around the offer is a COST guard -- a list nobody reads would only pay inserts, no result changes without it --
//                            and the one around wavefront 0's merge and store is the CORRECTNESS guard: table0 + q of a slot beyond members is the next item's
//                            table, or lies beyond the batch's segments.  Never remove the second.  At the unit's end, per member, the four
//                            lists meet in LDS, wavefront 0 merges them as topk_multi_kernel does and stores the merged list -- all k entries, ~0 where it is
//                            short -- at a place that follows from the unit alone:
//                                seg[(table0 + q) * seg_cap + (u - prefix[item]) * k + lane]
//                            No counter, no atomic, nothing to re-arm between batches.  A slot of a unit its item does not have is never stored: the host fills
//                            a batch's segments with ~0 before its launches, and the selection reads only the units the item has.
//                            BARRIERS: the unit loop's trip count depends on blockIdx.x alone, nothing inside it returns or breaks out, and a wavefront without a
//                            tile in a unit skips the walk and nothing else (its lists stay empty) -- every wavefront of the workgroup reaches both barriers of the
//                            table stage and both barriers of every one of the kJoinMembers rounds of the merge, in every unit: the rounds are not conditional on
//                            `members`, only wavefront 0's merge and store inside them are.
//                            No launch-wide pruning bound (topk_multi_kernel's per-query bound words): they save inserts, not columns.
//                            kNorm (rf_join_topk_f64): the normalized ops, as topk_multi_kernel<.., kNorm = true> has them.  At a tile's end, per member, tile_fin with
//                            the maximum made uniform, ONE norm_key_scale (the f64 division) per tile and member, fin_dist, and the key is
//                            norm_key_scaled(dist, maximum, scale) << 32 | index (rf_norm_key.hpp) -- ascending for both ops, so topk_desc is not read; None is
//                            emit_fin's f64 rule (norm_keep of norm_of: that division per candidate is paid under a cutoff only).  Every maximum of the launch is
//                            within 65535: the host admits a row by norm_key_fits of ITS length and the corpus' longest candidate.  Everything else -- the no_self
//                            compare, both guards, the barriers, the segment addressing, the selection -- is shared with the u32 instantiation.
//   join_topk_select_kernel  one workgroup per table of the batch: topk_select over the units_of_item x k keys of the row's segment (~0 is never offered), the k
//                            best, best first, ~0 = empty, to the row's place in the batch's key buffer.
// LDS: 8 KiB of tables (4 KiB for the 32-bit states) + 2 KiB of lists.  Plain vector stores only; no inline assembly beyond what WaveTopK contains.
// Product code: never includes or links anything from oracle/.
#include <algorithm>

#include "rf_internal.hpp"
#include "rf_device.hpp"
#include "rf_join_plan.hpp"
#include "rf_norm_key.hpp"

namespace rf {

template <class State, bool kUniform, bool kNorm>
__global__ __launch_bounds__(kWave* kWavesPerBlock) void join_topk_kernel(const JoinTopkParams jp)
{
    static_assert(State::kWords == 1, "multi-query kernels are single-word");
    using Word = typename State::Word;
    constexpr int Q = (int)kJoinMembers;
    const ScanParams& p = jp.s;
    __shared__ Word lds_pm[Q][256];
    __shared__ uint64_t lds_topk[kWavesPerBlock][kWave];

    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t wave = uniform(threadIdx.x / kWave);
    const uint32_t k = jp.k;

    for (uint32_t u = uniform(blockIdx.x); u < jp.n_units; u += gridDim.x) {
        const JoinUnit un = join_unit(jp.prefix, jp.n_items, jp.items, jp.span, u);
        const JoinItem* it = jp.items + un.item;
        const uint32_t members = uniform(it->members);
        const uint32_t table0 = uniform(it->table0);
        const uint32_t ord = u - uniform(jp.prefix[un.item]);  // the unit's ordinal within its item: below seg_units (launch_join_topk checks the list)
        uint32_t len1[Q], qidx[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) len1[q] = uniform(it->len1[q]), qidx[q] = uniform(it->qidx[q]);

        __syncthreads();  // every wavefront is done with the tables of the unit before (and wavefront 0 with its lists)
        for (int i = threadIdx.x; i < Q * 256; i += kWave * kWavesPerBlock) {
            const uint32_t q = (uint32_t)i / 256u, c = (uint32_t)i % 256u;
            lds_pm[q][c] = q < members ? (Word)jp.tables[(size_t)(table0 + q) * 256 + c] : (Word)0;
        }
        __syncthreads();

        WaveTopK best[Q];
        uint64_t limit[Q];  // wavefront-uniform: this list's worst key once it is full
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            best[q].init();
            limit[q] = ~0ull;
        }

        const uint32_t t_end = uniform(un.tile_end);
        uint32_t t = uniform(un.tile_begin) + wave;
        if (t < t_end) {
            TileView cur_tile = load_tile<kUniform>(p, t);
            uint4 cur = load_chunk(cur_tile.src + lane);  // (the packed buffer carries one chunk of tail padding: always readable)
            while (true) {
                const uint32_t t_next = t + kWavesPerBlock;
                const bool has_next = t_next < t_end;
                const TileView next_tile = load_tile<kUniform>(p, has_next ? t_next : t);
                const uint32_t len2 = cur_tile.len;
                const uint32_t slot = cur_tile.slot0 + lane;
                uint32_t idx = slot;
                if (!kUniform) idx = p.orig[slot];

                State st[Q];
#pragma unroll
                for (int q = 0; q < Q; ++q) st[q].init();
                const uint32_t nch = (len2 + kChunk - 1) / kChunk;
                for (uint32_t c = 0; c < nch; ++c) {
                    const uint4* nsrc = (c + 1 < nch) ? cur_tile.src + (size_t)(c + 1) * kWave : next_tile.src;
                    const uint4 nxt = load_chunk(nsrc + lane);
                    const uint32_t cols = len2 - c * kChunk;
#pragma unroll
                    for (int q = 0; q < Q; ++q) {
                        if (cols >= kChunk)
                            process_chunk_full<State>(st[q], lds_pm[q], cur);
                        else
                            process_chunk_tail<State>(st[q], lds_pm[q], cur, cols);
                    }
                    cur = nxt;
                }
                if (nch == 0) cur = load_chunk(next_tile.src + lane);

                const bool valid = kUniform ? slot < p.n : idx != kPad;
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    if ((uint32_t)q >= members) continue;  // (uniform: the item's; a cost guard, see the head comment)
                    const uint32_t raw = st[q].result(len1[q], len2);
                    bool keep;
                    uint64_t mine;
                    if constexpr (!kNorm) {
                        const uint32_t v = usize_value(p, raw, len2, &keep, len1[q]);  // emit_usize's arithmetic; None is not offered
                        mine = ((uint64_t)(p.topk_desc ? ~v : v) << 32) | idx;
                    } else {  // (topk_multi_kernel's normalized tile end: one scale per tile and member, the division of nd under a cutoff only)
                        TileFin f = tile_fin(p, len1[q], len2);
                        f.max = uniform(f.max);
                        const double scale = norm_key_scale(f.max);
                        const uint32_t dist = fin_dist(p, f, raw);
                        keep = true;
                        if (p.has_cutoff) keep = norm_keep(p, norm_of(dist, f.max));
                        mine = ((uint64_t)norm_key_scaled(dist, f.max, scale) << 32) | idx;
                    }
                    if (best[q].offer(mine, valid && keep && !(jp.no_self && idx == qidx[q]), k, lane, limit[q])) limit[q] = best[q].worst(k);
                }
                if (!has_next) break;  // (leaves the tile walk, never the unit loop)
                t = t_next;
                cur_tile = next_tile;
            }
        }

        // end of the unit: per member, the four lists meet in LDS, wavefront 0 merges them and stores the merged list at the unit's place in the member's segment
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            __syncthreads();  // wavefront 0 has read the lists of the member before
            lds_topk[wave][lane] = best[q].key;
            __syncthreads();
            if (wave == 0 && (uint32_t)q < members) {  // (the correctness guard: a slot beyond members owns no segment)
                for (uint32_t w = 1; w < kWavesPerBlock; ++w)
                    for (uint32_t j = 0; j < k; ++j) {
                        const uint64_t x = lds_topk[w][j];  // wavefront-uniform address: a broadcast read
                        if (x >= best[q].worst(k)) break;
                        best[q].insert(x, lane);
                    }
                if (lane < k) jp.seg[(size_t)(table0 + q) * jp.seg_cap + (size_t)ord * k + lane] = best[q].key;
            }
        }
    }
}

__global__ __launch_bounds__(kWave* kWavesPerBlock) void join_topk_select_kernel(const JoinTopkParams jp)
{
    __shared__ uint64_t lists[kWavesPerBlock][kWave];
    const uint32_t b = blockIdx.x, k = jp.k;  // (the grid is the batch)
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = uniform(threadIdx.x / kWave);
    const uint32_t n = min(uniform(jp.tab_units[b]), jp.seg_units) * k;
    WaveTopK best;
    topk_select(jp.seg + (size_t)b * jp.seg_cap, n, k, lists, wave, lane, best);
    if (wave == 0 && lane < k) jp.keys[(size_t)b * k + lane] = best.key;
}

// raw: RAW_LEV or RAW_LCS; narrow: every query of every item <= 32 symbols; jp.norm picks the normalized instantiation (and must agree with the plan's out_f64).  The grid: one workgroup per unit up to scan_max_grid(), beyond it a workgroup
// walks several units.
hipError_t launch_join_topk(RawKind raw, bool narrow, const JoinTopkParams& jp, const JoinItem* h_items, const uint32_t* h_prefix, hipStream_t stream)
{
    const ScanParams& p = jp.s;
    if (jp.n_items == 0 || jp.n_units == 0) return hipSuccess;
    if (!h_items || !h_prefix || !jp.items || !jp.prefix || !jp.tables || !jp.seg || (p.out_f64 != 0) != (jp.norm != 0)) return hipErrorInvalidValue;
    if (jp.norm && p.op != RF_OP_NORMALIZED_DISTANCE && p.op != RF_OP_NORMALIZED_SIMILARITY) return hipErrorInvalidValue;
    if (!p.data || (p.tiles && !p.orig)) return hipErrorInvalidValue;
    if (jp.k == 0 || jp.k > (uint32_t)kWave || jp.seg_units == 0 || (uint64_t)jp.seg_units * jp.k != jp.seg_cap) return hipErrorInvalidValue;
    if (!join_valid(h_items, h_prefix, jp.n_items, jp.n_units, p.n_tiles, jp.batch, narrow, jp.span)) return hipErrorInvalidValue;
    for (uint32_t i = 0; i < jp.n_items; ++i)  // every unit's ordinal has a place in its members' segments
        if (h_prefix[i + 1] - h_prefix[i] > jp.seg_units) return hipErrorInvalidValue;
    const dim3 g(std::max(1u, std::min<uint32_t>(jp.n_units, (uint32_t)scan_max_grid()))), b(kWave * kWavesPerBlock);
    auto with_state = [&](auto state) {
        using State = typename decltype(state)::type;
        auto with_layout = [&](auto uniform_layout) {
            constexpr bool kU = decltype(uniform_layout)::value;
            if (jp.norm)
                hipLaunchKernelGGL((join_topk_kernel<State, kU, true>), g, b, 0, stream, jp);
            else
                hipLaunchKernelGGL((join_topk_kernel<State, kU, false>), g, b, 0, stream, jp);
        };
        if (p.tiles)
            with_layout(std::false_type{});
        else
            with_layout(std::true_type{});
        return hipGetLastError();
    };
    if (raw == RAW_LEV) return narrow ? with_state(MultiStateTag<Lev32State>{}) : with_state(MultiStateTag<LevState<1>>{});
    if (raw == RAW_LCS) return narrow ? with_state(MultiStateTag<Lcs32State>{}) : with_state(MultiStateTag<LcsState<1>>{});
    return hipErrorInvalidValue;
}

hipError_t launch_join_topk_select(const JoinTopkParams& jp, hipStream_t stream)
{
    if (jp.batch == 0) return hipSuccess;
    if (!jp.seg || !jp.tab_units || !jp.keys || jp.k == 0 || jp.k > (uint32_t)kWave || (uint64_t)jp.seg_units * jp.k != jp.seg_cap) return hipErrorInvalidValue;
    hipLaunchKernelGGL(join_topk_select_kernel, dim3(jp.batch), dim3(kWave * kWavesPerBlock), 0, stream, jp);
    return hipGetLastError();
}

}  // namespace rf

// rf_join.hip -- all pairs of two packed corpora within a tight cutoff (rf_join_u32 / rf_join_f64; host side in rf_api_join.hip, the work list in rf_join_plan.hpp).
//   join_pm_kernel   a batch of B queries straight out of the QUERY corpus' packed payload (rf_take_addr.hpp's addresses) into B single-word pattern tables of
//                    256 x u64, written AT THE SCANNED CORPUS' SIGMA ROWS: row row_of[s] of table b has bit i set when symbol i of query b is stored as s.
//                    row_of (rf_join_xlat.hpp, built on the host once per call) goes through the SYMBOLS -- un-rename by the query corpus' inverse sigma, id ->
//                    symbol for a `char` corpus, the symbol's id in the scanned corpus, that corpus' sigma -- so one kernel serves every pair of corpus kinds.
//                    The tables are the form the scans keep in LDS, so join_kernel stages one with a straight coalesced 2 KiB copy.  A symbol the scanned
//                    corpus never stores owns a row no candidate byte names: it matches nothing.
//   join_bad_kernel  launched only when the row map has a stored value it cannot place (an overflow-class symbol of either corpus, a symbol above 0xFF against
//                    a byte corpus): a wavefront per row of Q, one payload byte per lane, a lookup in the 256-byte `bad` table, a ballot, one flag per row.
//                    Flagged rows never reach join_pm_kernel: they go down the per-query road.
//   join_kernel      filter_multi_kernel's tile body -- 4 recurrences per lane, the look after column 8 of a full first chunk and at every chunk's end, the
//                    `live` mask, the next tile's first chunk prefetched -- over a WORK LIST in device memory instead of one launch per group of queries.  A
//                    workgroup walks units blockIdx.x, + gridDim.x, ...: per unit it stages the item's (up to) 4 tables into LDS and its four wavefronts walk
//                    the unit's tiles.  `live` starts at (1 << members) - 1, so one instantiation serves items of 1 to 4 queries.
//                    BARRIERS: the unit loop's trip count depends on blockIdx.x alone, nothing inside it returns or breaks out, and a wavefront without a tile
//                    in a unit skips the walk and nothing else -- every wavefront of the workgroup reaches both barriers of every unit.
//                    Emission: the counted append (append_passers' scheme) onto ONE 64-bit counter and one capacity-bounded triple buffer for the whole call.
//                    kNorm (rf_join_f64): jp.s is an f64 plan, so the looks already run may_pass()'s f64 compare; at a tile's end a member is kept by
//                    norm_dist / norm_keep (rf_device.hpp) and the double emit_fin would have written goes into the f64 score buffer -- no key, so no
//                    limit on the maximum.
// Plain vector stores only; no inline assembly.
// Product code: never includes or links anything from oracle/.
#include <algorithm>

#include "rf_internal.hpp"
#include "rf_device.hpp"
#include "rf_take_addr.hpp"
#include "rf_join_plan.hpp"

namespace rf {

static_assert(kJoinMembers == (uint32_t)kMaxMulti, "a work item holds what a fused kernel carries");
static_assert(sizeof(JoinItem) == 64, "JoinItem is uploaded as it is");

constexpr int kJoinPmThreads = 64;

__global__ __launch_bounds__(kJoinPmThreads) void join_pm_kernel(const JoinPmParams p)
{
    __shared__ unsigned long long tab[256];
    const uint32_t b = blockIdx.x;  // (the grid is the batch)
    for (uint32_t c = threadIdx.x; c < 256; c += kJoinPmThreads) tab[c] = 0;
    __syncthreads();
    const uint32_t j = p.rows[b];
    const uint32_t slot = p.row_slot[j];
    const uint32_t len = min(p.row_len[j], kJoinMaxLen);
    const uint32_t i = threadIdx.x;
    if (i < len && slot < p.n_slots) {
        const uint32_t t = take_tile_of(slot);
        uint64_t base;
        if (p.s.tiles)
            base = p.s.tiles[t].data_off;
        else
            base = take_uniform_base(t, p.s.uniform_len);
        const uint32_t stored = p.s.data[take_byte_at(base, take_lane_of(slot), i)];
        const uint32_t row = p.row_of[stored];
        atomicOr(&tab[row], 1ull << i);
    }
    __syncthreads();
    for (uint32_t c = threadIdx.x; c < 256; c += kJoinPmThreads) p.tables[(size_t)b * 256 + c] = tab[c];
}

hipError_t launch_join_pm(const JoinPmParams& p, hipStream_t stream)
{
    if (p.batch == 0) return hipSuccess;
    if (!p.rows || !p.row_slot || !p.row_len || !p.tables || !p.row_of || !p.s.data) return hipErrorInvalidValue;
    hipLaunchKernelGGL(join_pm_kernel, dim3(p.batch), dim3(kJoinPmThreads), 0, stream, p);
    return hipGetLastError();
}

// One wavefront per row of Q, a workgroup walking rows blockIdx.x, + gridDim.x, ...: lane i reads symbol i of the row as join_pm_kernel does.  A row beyond
// kJoinMaxLen symbols is never fused, so it is not read.
__global__ __launch_bounds__(kJoinPmThreads) void join_bad_kernel(const JoinBadParams p)
{
    const uint32_t i = threadIdx.x;
    for (uint64_t j = blockIdx.x; j < p.m; j += gridDim.x) {
        const uint32_t slot = p.row_slot[j];
        const uint32_t len = p.row_len[j];
        bool hit = false;
        if (len <= kJoinMaxLen && i < len && slot < p.n_slots) {
            const uint32_t t = take_tile_of(slot);
            uint64_t base;
            if (p.s.tiles)
                base = p.s.tiles[t].data_off;
            else
                base = take_uniform_base(t, p.s.uniform_len);
            hit = p.bad[p.s.data[take_byte_at(base, take_lane_of(slot), i)]] != 0;
        }
        const uint64_t any = __ballot(hit);
        if (i == 0) p.flags[j] = any ? 1u : 0u;
    }
}

hipError_t launch_join_bad(const JoinBadParams& p, hipStream_t stream)
{
    if (p.m == 0) return hipSuccess;
    if (!p.row_slot || !p.row_len || !p.bad || !p.flags || !p.s.data) return hipErrorInvalidValue;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(p.m, (uint64_t)std::max(1, scan_max_grid()) * 32);
    hipLaunchKernelGGL(join_bad_kernel, dim3(grid), dim3(kJoinPmThreads), 0, stream, p);
    return hipGetLastError();
}

// the counted append onto the call's buffers: one 64-bit atomic per wavefront that holds a passer
template <class Score, class Pair>
__device__ __forceinline__ void append_triples(const JoinParams& jp, Score* scores, bool pass, uint32_t lane, Score score, Pair&& pair)
{
    const uint64_t m = __ballot(pass);
    if (!m) return;
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(jp.count, (unsigned long long)__popcll(m));
    base = ((unsigned long long)uniform((uint32_t)(base >> 32)) << 32) | uniform((uint32_t)base);
    const unsigned long long at = base + (uint32_t)__popcll(m & ((1ull << lane) - 1));
    if (pass && at < jp.cap) {
        jp.pairs[at] = pair();
        scores[at] = score;
    }
}

template <class State, bool kUniform, bool kNorm>
__global__ __launch_bounds__(kWave* kWavesPerBlock) void join_kernel(const JoinParams jp)
{
    static_assert(State::kWords == 1, "multi-query kernels are single-word");
    static_assert(State::kCanPrune, "the fused cutoff scan needs a state with a bound");
    using Word = typename State::Word;
    constexpr int Q = (int)kJoinMembers;
    const ScanParams& p = jp.s;
    __shared__ Word lds_pm[Q][256];

    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t wave = uniform(threadIdx.x / kWave);

    for (uint32_t u = uniform(blockIdx.x); u < jp.n_units; u += gridDim.x) {
        const JoinUnit un = join_unit(jp.prefix, jp.n_items, jp.items, jp.span, u);
        const JoinItem* it = jp.items + un.item;
        const uint32_t members = uniform(it->members);
        const uint32_t table0 = uniform(it->table0);
        uint32_t len1[Q], qpos[Q], qidx[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) len1[q] = uniform(it->len1[q]), qpos[q] = uniform(it->qpos[q]), qidx[q] = uniform(it->qidx[q]);

        __syncthreads();  // every wavefront is done with the tables of the unit before
        for (int i = threadIdx.x; i < Q * 256; i += kWave * kWavesPerBlock) {
            const uint32_t q = (uint32_t)i / 256u, c = (uint32_t)i % 256u;
            lds_pm[q][c] = q < members ? (Word)jp.tables[(size_t)(table0 + q) * 256 + c] : (Word)0;
        }
        __syncthreads();

        const uint32_t t_end = uniform(un.tile_end);
        uint32_t t = uniform(un.tile_begin) + wave;
        if (t < t_end) {
            TileView cur_tile = load_tile<kUniform>(p, t);
            uint4 cur = load_chunk(cur_tile.src + lane);  // (the packed buffer carries one chunk of tail padding: always readable)
            while (true) {
                const uint32_t t_next = t + kWavesPerBlock;
                const bool has_next = t_next < t_end;
                const TileView next_tile = load_tile<kUniform>(p, has_next ? t_next : t);
                const uint4 ahead = load_chunk(next_tile.src + lane);
                const uint32_t len2 = cur_tile.len;
                const uint32_t slot = cur_tile.slot0 + lane;
                uint32_t idx = slot;
                if (!kUniform) idx = p.orig[slot];
                const bool valid = kUniform ? slot < p.n : idx != kPad;

                State st[Q];
                TileFin fin[Q];
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    st[q].init();
                    fin[q] = tile_fin(p, len1[q], len2);
                }
                uint32_t live = (1u << members) - 1u;
                const uint32_t nch = (len2 + kChunk - 1) / kChunk;
                for (uint32_t c = 0; c < nch; ++c) {
                    const uint32_t cols = len2 - c * kChunk;
                    if (cols >= kChunk && c == 0) {
#pragma unroll
                        for (int q = 0; q < Q; ++q) {
                            if (!(live & (1u << q))) continue;
                            process_chunk_full<State, 0, 8>(st[q], lds_pm[q], cur);
                            if (__ballot(valid && may_pass(p, fin[q], st[q].bound_first(len1[q], 8, len2))) == 0)
                                live &= ~(1u << q);
                            else
                                process_chunk_full<State, 8, kChunk>(st[q], lds_pm[q], cur);
                        }
                    } else {
#pragma unroll
                        for (int q = 0; q < Q; ++q) {
                            if (!(live & (1u << q))) continue;
                            if (cols >= kChunk)
                                process_chunk_full<State>(st[q], lds_pm[q], cur);
                            else
                                process_chunk_tail<State>(st[q], lds_pm[q], cur, cols);
                        }
                    }
                    const uint32_t j = min(len2, (c + 1) * kChunk);
#pragma unroll
                    for (int q = 0; q < Q; ++q)
                        if ((live & (1u << q)) && __ballot(valid && may_pass(p, fin[q], st[q].bound(len1[q], j, len2))) == 0) live &= ~(1u << q);
                    if (!live) break;  // every member's wavefront is beyond the cutoff: stop reading this tile
                    if (c + 1 < nch) cur = load_chunk(cur_tile.src + (size_t)(c + 1) * kWave + lane);
                }

#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    if (!(live & (1u << q))) continue;
                    const uint32_t raw = st[q].result(len1[q], len2);
                    if constexpr (!kNorm) {
                        bool keep;
                        const uint32_t v = usize_value(p, fin[q], raw, &keep);
                        const bool pass = valid && keep && (!jp.upper || idx > qidx[q]);
                        append_triples(jp, jp.scores, pass, lane, v, [&] { return ((uint64_t)qpos[q] << 32) | idx; });
                    } else {
                        // (has_cutoff: the launcher takes plans under a cutoff only.  What is stored is what emit_fin writes: nd, or 1.0 - nd for the similarity)
                        TileFin f = fin[q];
                        f.max = uniform(f.max);
                        const double nd = norm_dist(p, f, raw).nd;
                        const bool pass = valid && norm_keep(p, nd) && (!jp.upper || idx > qidx[q]);
                        const double v = p.op == RF_OP_NORMALIZED_DISTANCE ? nd : 1.0 - nd;
                        append_triples(jp, jp.scores_f64, pass, lane, v, [&] { return ((uint64_t)qpos[q] << 32) | idx; });
                    }
                }

                if (!has_next) break;  // (leaves the tile walk, never the unit loop)
                cur = ahead;           // dead, empty or walked to its end: the next tile starts from the prefetched chunk
                t = t_next;
                cur_tile = next_tile;
            }
        }
    }
}

// raw: RAW_LEV or RAW_LCS; narrow: every query of every item <= 32 symbols.  The grid: one workgroup per unit up to scan_max_grid(), beyond it a workgroup
// walks several units.
hipError_t launch_join(RawKind raw, bool narrow, const JoinParams& jp, const JoinItem* h_items, const uint32_t* h_prefix, hipStream_t stream)
{
    const ScanParams& p = jp.s;
    if (jp.n_items == 0 || jp.n_units == 0) return hipSuccess;
    if (!h_items || !h_prefix || !jp.items || !jp.prefix || !jp.tables || !jp.count || !p.has_cutoff) return hipErrorInvalidValue;
    if (jp.norm ? !(p.out_f64 && (p.op == RF_OP_NORMALIZED_DISTANCE || p.op == RF_OP_NORMALIZED_SIMILARITY)) : p.out_f64 != 0) return hipErrorInvalidValue;
    if (jp.cap && (!jp.pairs || (jp.norm ? !jp.scores_f64 : !jp.scores))) return hipErrorInvalidValue;
    if (!p.data || (p.tiles && !p.orig)) return hipErrorInvalidValue;
    if (!join_valid(h_items, h_prefix, jp.n_items, jp.n_units, p.n_tiles, jp.batch, narrow, jp.span)) return hipErrorInvalidValue;
    const dim3 g(std::max(1u, std::min<uint32_t>(jp.n_units, (uint32_t)scan_max_grid()))), b(kWave * kWavesPerBlock);
    auto with_state = [&](auto state) {
        using State = typename decltype(state)::type;
        if (jp.norm) {
            if (p.tiles)
                hipLaunchKernelGGL((join_kernel<State, false, true>), g, b, 0, stream, jp);
            else
                hipLaunchKernelGGL((join_kernel<State, true, true>), g, b, 0, stream, jp);
        } else {
            if (p.tiles)
                hipLaunchKernelGGL((join_kernel<State, false, false>), g, b, 0, stream, jp);
            else
                hipLaunchKernelGGL((join_kernel<State, true, false>), g, b, 0, stream, jp);
        }
        return hipGetLastError();
    };
    if (raw == RAW_LEV) return narrow ? with_state(MultiStateTag<Lev32State>{}) : with_state(MultiStateTag<LevState<1>>{});
    if (raw == RAW_LCS) return narrow ? with_state(MultiStateTag<Lcs32State>{}) : with_state(MultiStateTag<LcsState<1>>{});
    return hipErrorInvalidValue;
}

}  // namespace rf

// rf_topk_multi.hip -- top-k for Q queries in one pass over the corpus (rf_topk_multi_u32, rf_topk_multi_f64): scan_multi_kernel's tile loop with one
// register-resident WaveTopK list per query instead of the dense [Q][n] result, and the selection as a launch of its own.
// Product code: never includes or links anything from oracle/.
#include <algorithm>

#include "rf_internal.hpp"
#include "rf_device.hpp"
#include "rf_norm_key.hpp"

namespace rf {

// per-query forms of topk_list_changed / topk_refresh_bound (rf_device.hpp has the why of both asm statements): `bound` is that query's line
__device__ __forceinline__ void topk_multi_list_changed(uint64_t* bound, const WaveTopK& best, uint32_t k, uint32_t lane, uint64_t& limit)
{
    const uint64_t w = best.worst(k);
    if (w < limit) {
        if (lane == 0) asm volatile("global_atomic_umin_x2 %0, %1, off" ::"v"(bound), "v"(w) : "memory");
        limit = w;
    }
}
__device__ __forceinline__ void topk_multi_refresh_bound(const uint64_t* bound, uint64_t& limit)
{
    uint64_t v;
    asm volatile("global_load_dwordx2 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"(bound) : "memory");
    const uint64_t b = uniform64(v);
    limit = b < limit ? b : limit;
}

// ---------------------------------------------------------------------------------------------------
// Q tables side by side in LDS, every 16-column chunk run through Q recurrences before the next is touched (the next chunk is in
// flight meanwhile, across tile ends), and at a tile's end one offer per query to that query's list.  Nothing is stored per candidate.
// The launch walks tiles tile_begin + i * tile_step < tile_end (the sample pass: tile_step > 1).
// No workgroup waits for another: each merges its four lists per query and appends what can still be in the answer to the query's
// segment behind the query's counter; topk_multi_select_kernel (the next launch) selects.  A segment holds gridDim.x * k keys -- every
// workgroup of the launch publishing a full list -- so a published key is never dropped and never overwritten.
// kNorm (rf_topk_multi_f64): the normalized ops.  The score image is norm_key(dist, maximum) (rf_norm_key.hpp) instead of the u32 value --
// ascending for both ops, so topk_desc is not read -- and None is emit_fin's f64 rule.  The maximum is uniform per query and tile: its
// scale (the one f64 division) is computed once per tile and query, the candidate pays a convert, an f64 multiply and a multiply-compare;
// nd itself -- a division per candidate -- is computed only under a cutoff, which is all that looks at it.
// ---------------------------------------------------------------------------------------------------
template <class State, int Q, bool kUniform, bool kNorm>
__global__ __launch_bounds__(kWave* kWavesPerBlock) void topk_multi_kernel(const TopkMultiParams tp)
{
    static_assert(State::kWords == 1, "multi-query kernels are single-word");
    const ScanParams& p = tp.s;
    __shared__ typename State::Word lds_pm[Q][256];
    __shared__ uint64_t lds_topk[kWavesPerBlock][kWave];
    fill_multi_tables(lds_pm, p);

    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t wave = uniform(threadIdx.x / kWave);
    const uint32_t k = p.topk_k;
    const uint32_t stride = gridDim.x * kWavesPerBlock * p.tile_step;
    WaveTopK best[Q];
    uint64_t limit[Q];  // wavefront-uniform: min(the query's launch-wide bound as last seen, this list's worst key)
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        best[q].init();
        limit[q] = ~0ull;
        topk_multi_refresh_bound(tp.bound + q * kTopkMultiLine64, limit[q]);  // (the sampled bound: waited for once, as in stream_body)
    }
    uint32_t tiles_done = 0;

    uint32_t t = p.tile_begin + (blockIdx.x * kWavesPerBlock + wave) * p.tile_step;
    if (t < p.tile_end) {
        TileView cur_tile = load_tile<kUniform>(p, t);
        uint4 cur = load_chunk(cur_tile.src + lane);
        while (true) {
            const uint32_t t_next = t + stride;
            const bool has_next = t_next < p.tile_end;
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
                const uint32_t raw = st[q].result(p.multi_len1[q], len2);
                bool keep;
                uint64_t mine;
                if constexpr (!kNorm) {
                    const uint32_t v = usize_value(p, raw, len2, &keep, p.multi_len1[q]);  // emit_usize's arithmetic; None is not offered
                    mine = ((uint64_t)(p.topk_desc ? ~v : v) << 32) | idx;
                } else {
                    TileFin f = tile_fin(p, p.multi_len1[q], len2);
                    f.max = uniform(f.max);
                    const double scale = norm_key_scale(f.max);
                    const uint32_t dist = fin_dist(p, f, raw);
                    keep = true;
                    if (p.has_cutoff) keep = norm_keep(p, norm_of(dist, f.max));  // (norm_dist's two halves: the division is paid under a cutoff only)
                    mine = ((uint64_t)norm_key_scaled(dist, f.max, scale) << 32) | idx;
                }
                if (best[q].offer(mine, valid && keep, k, lane, limit[q])) topk_multi_list_changed(tp.bound + q * kTopkMultiLine64, best[q], k, lane, limit[q]);
            }
            if ((++tiles_done & 7u) == 0) {  // every 8th tile: stream_body has the measurements
#pragma unroll
                for (int q = 0; q < Q; ++q) topk_multi_refresh_bound(tp.bound + q * kTopkMultiLine64, limit[q]);
            }
            if (!has_next) break;
            t = t_next;
            cur_tile = next_tile;
        }
    }

    // end of the workgroup: per query, the four lists meet in LDS, wavefront 0 merges them and appends the keys at or below the bound it
    // last saw (the first half of topk_block_publish; nobody arrives anywhere, nobody collects)
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        // (the barrier also separates wavefront 0's reads of the previous query's lists from the writes below)
        if (!__syncthreads_or(__ballot(best[q].key != ~0ull) != 0)) continue;
        lds_topk[wave][lane] = best[q].key;
        __syncthreads();
        if (wave == 0) {
            for (uint32_t w = 1; w < kWavesPerBlock; ++w)
                for (uint32_t j = 0; j < k; ++j) {
                    const uint64_t x = lds_topk[w][j];  // wavefront-uniform address: a broadcast read
                    if (x >= best[q].worst(k)) break;
                    best[q].insert(x, lane);
                }
            // (a place is below seg_cap always: the launcher sizes a segment for gridDim.x * k keys and a workgroup adds at most k; the test only keeps a
            // launch with a wrong seg_cap inside its buffer)
            append_passers(tp.count + q * kTopkMultiLine32, tp.cand + (size_t)q * tp.seg_cap, tp.seg_cap, lane < k && best[q].key != ~0ull && best[q].key <= limit[q], lane,
                           [&] { return best[q].key; });
        }
    }
}

// One workgroup per query: the k best of the query's segment (topk_select), best first, ~0 = empty.  After the sample pass (`sample`) the
// result is not kept: its k-th best key + 1 becomes the query's bound for the main pass (topk_block_publish has the why of the + 1).
// Either way the query's counter is zero again afterwards.
__global__ __launch_bounds__(kWave* kWavesPerBlock) void topk_multi_select_kernel(const TopkMultiParams tp, uint64_t* __restrict__ keys)
{
    __shared__ uint64_t lists[kWavesPerBlock][kWave];
    const uint32_t q = blockIdx.x, k = tp.s.topk_k;
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = uniform(threadIdx.x / kWave);
    const uint32_t n = min(uniform(tp.count[q * kTopkMultiLine32]), tp.seg_cap);
    WaveTopK best;
    topk_select(tp.cand + (size_t)q * tp.seg_cap, n, k, lists, wave, lane, best);
    if (wave == 0) {
        if (!tp.sample) {
            if (lane < k) keys[(size_t)q * k + lane] = best.key;
        } else {
            const uint64_t kth = best.worst(k);
            if (lane == 0) tp.bound[q * kTopkMultiLine64] = kth != ~0ull ? kth + 1 : ~0ull;
        }
    }
    __syncthreads();  // (every wavefront has read the counter)
    if (threadIdx.x == 0) tp.count[q * kTopkMultiLine32] = 0;
}

// The grid of a launch that visits `tiles` tiles: scan_grid(), i.e. at most RF_SCAN_BLOCKS_PER_CU (32) workgroups per CU -- 8192 on a whole MI355X.  With
// it the worst case of a segment is 8192 x 64 keys = 4 MiB per query, 16 MiB for a group of four (the full scans' 256 per CU would make that 128 MiB).
// What the cap costs (profiles/topk_multi_grid.txt, 16 queries over 100 M x 64, 32 / 64 / 128 workgroups per CU in one session): 64-bit Levenshtein
// 37.8 / 37.3 / 37.1 ms -- 2 %, about the spread between repetitions -- and nothing for Indel (16.7 / 16.5 / 16.6 ms; query 24: 12.8 / 12.7 / 12.7).
int topk_multi_grid(uint32_t tiles) { return std::max(1, scan_grid(tiles)); }

// raw: RAW_LEV or RAW_LCS; every query single-word; `narrow` = every query <= 32 symbols.  tp.seg_cap >= grid * topk_k (checked).
// tp.norm: a normalized op, every maximum of the launch <= kNormKeyMaxMaximum (the caller's rule: the launcher cannot see the corpus' lengths).
hipError_t launch_topk_multi(RawKind raw, bool narrow, const TopkMultiParams& tp, hipStream_t stream)
{
    const ScanParams& p = tp.s;
    if (p.topk_k == 0 || p.topk_k > (uint32_t)kWave || p.tile_step == 0) return hipErrorInvalidValue;
    const uint32_t span = p.tile_end > p.tile_begin ? p.tile_end - p.tile_begin : 0;
    if (span == 0) return hipSuccess;
    const int grid = topk_multi_grid((span + p.tile_step - 1) / p.tile_step);
    if ((uint64_t)grid * p.topk_k > tp.seg_cap) return hipErrorInvalidValue;
    const dim3 g(grid), b(kWave * kWavesPerBlock);
    return dispatch_multi(raw, narrow, p, [&](auto state, auto q, auto uniform) {
        using State = typename decltype(state)::type;
        if (tp.norm)
            hipLaunchKernelGGL((topk_multi_kernel<State, decltype(q)::value, decltype(uniform)::value, true>), g, b, 0, stream, tp);
        else
            hipLaunchKernelGGL((topk_multi_kernel<State, decltype(q)::value, decltype(uniform)::value, false>), g, b, 0, stream, tp);
        return hipGetLastError();
    });
}

hipError_t launch_topk_multi_select(const TopkMultiParams& tp, uint64_t* keys, hipStream_t stream)
{
    if (tp.s.multi_q == 0 || tp.s.topk_k == 0 || tp.s.topk_k > (uint32_t)kWave) return hipErrorInvalidValue;
    hipLaunchKernelGGL(topk_multi_select_kernel, dim3(tp.s.multi_q), dim3(kWave * kWavesPerBlock), 0, stream, tp, keys);
    return hipGetLastError();
}

}  // namespace rf

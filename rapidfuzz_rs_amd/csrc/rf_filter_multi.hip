// rf_filter_multi.hip -- the candidates within a tight cutoff for Q queries in one pass over the corpus (rf_filter_multi_u32, rf_filter_multi_f64): topk_multi_kernel's
// frame (Q tables side by side in LDS, one candidate per lane, Q recurrence states per lane) with scan_body's early-out schedule, and at a tile's
// end one compact append per query that still has a passing lane.  Nothing is stored per candidate otherwise.
// Product code: never includes or links anything from oracle/.
#include <algorithm>

#include "rf_internal.hpp"
#include "rf_device.hpp"
#include "rf_norm_key.hpp"

namespace rf {

// ---------------------------------------------------------------------------------------------------
// The launch walks tiles tile_begin + i * stride < tile_end: the union of the members' length windows (a member whose own window excludes a
// tile's length fails its first look there -- or, at the latest, the final compare).
// Early-out: `live` is the wavefront-uniform set of members some lane of which may still pass (may_pass() over State::bound(), padding lanes
// excluded).  A full first chunk takes the first look after column 8 (bound_first), every chunk takes one at its end (bound); a member whose
// ballot is empty is dropped for the rest of the tile -- a uniform branch: its recurrences are not issued any more -- and a tile no member
// of which is live is abandoned.  Every look is value-preserving: what a member returns is decided by usize_value() at the tile's end.
// Memory: scan_body's cutoff mode.  The NEXT TILE's first chunk is requested at the top of a tile; a wavefront that survives a chunk fetches
// its own next chunk on demand; whatever way the tile ends, the next tile starts from the prefetched chunk.
// Emission: per live member m = ballot(valid && keep); lane 0 adds popcount(m) to the member's counter, the passing lanes store their keys at
// base + rank while that is below seg_cap.  The counter counts on beyond seg_cap: it is the true number of matches.  Under a tight cutoff
// passers are rare, so the atomics are (the planner fuses p.early queries only).
// kNorm (rf_filter_multi_f64): the normalized ops.  p.out_f64 is set, so the looks already run may_pass()'s f64 arithmetic; at a tile's end `keep` is
// emit_fin's f64 compare (norm_dist / norm_keep, rf_device.hpp) -- nd = dist / maximum against p.cutoff_f64, an arbitrary double -- and never a compare on keys.  What is stored is
// the key's image of nd, norm_key(dist, maximum) (rf_norm_key.hpp): ascending for both ops (a smaller key is the better score), so topk_desc is not read.
// f64 cost: the division of the compare is paid per lane, but only by a member that is still live at its tile's end; the maximum is uniform per member
// and tile, and its scale -- the second f64 division -- is computed behind the ballot, by wavefronts that hold a passer.
// ---------------------------------------------------------------------------------------------------
template <class State, int Q, bool kUniform, bool kNorm>
__global__ __launch_bounds__(kWave* kWavesPerBlock) void filter_multi_kernel(const FilterMultiParams fp)
{
    static_assert(State::kWords == 1, "multi-query kernels are single-word");
    static_assert(State::kCanPrune, "the fused cutoff scan needs a state with a bound");
    const ScanParams& p = fp.s;
    __shared__ typename State::Word lds_pm[Q][256];
    fill_multi_tables(lds_pm, p);

    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t wave = uniform(threadIdx.x / kWave);
    const uint32_t stride = gridDim.x * kWavesPerBlock;
    constexpr uint32_t kAll = (1u << Q) - 1u;

    uint32_t t = p.tile_begin + blockIdx.x * kWavesPerBlock + wave;
    if (t >= p.tile_end) return;
    TileView cur_tile = load_tile<kUniform>(p, t);
    uint4 cur = load_chunk(cur_tile.src + lane);  // (the packed buffer carries one chunk of tail padding: always readable)
    while (true) {
        const uint32_t t_next = t + stride;
        const bool has_next = t_next < p.tile_end;
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
            fin[q] = tile_fin(p, p.multi_len1[q], len2);
        }
        uint32_t live = kAll;
        const uint32_t nch = (len2 + kChunk - 1) / kChunk;
        for (uint32_t c = 0; c < nch; ++c) {
            const uint32_t cols = len2 - c * kChunk;
            if (cols >= kChunk && c == 0) {
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    if (!(live & (1u << q))) continue;
                    process_chunk_full<State, 0, 8>(st[q], lds_pm[q], cur);
                    if (__ballot(valid && may_pass(p, fin[q], st[q].bound_first(p.multi_len1[q], 8, len2))) == 0)
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
                if ((live & (1u << q)) && __ballot(valid && may_pass(p, fin[q], st[q].bound(p.multi_len1[q], j, len2))) == 0) live &= ~(1u << q);
            if (!live) break;  // every member's wavefront is beyond the cutoff: stop reading this tile
            if (c + 1 < nch) cur = load_chunk(cur_tile.src + (size_t)(c + 1) * kWave + lane);
        }

#pragma unroll
        for (int q = 0; q < Q; ++q) {
            if (!(live & (1u << q))) continue;
            const uint32_t raw = st[q].result(p.multi_len1[q], len2);
            uint32_t* count = fp.count + q * kFilterMultiLine32;
            uint64_t* seg = fp.cand + (size_t)q * fp.seg_cap;
            if constexpr (!kNorm) {
                bool keep;
                const uint32_t v = usize_value(p, fin[q], raw, &keep);
                append_passers(count, seg, fp.seg_cap, valid && keep, lane, [&] { return ((uint64_t)(p.topk_desc ? ~v : v) << 32) | idx; });
            } else {
                // (has_cutoff: the launcher takes plans under a cutoff only)
                TileFin f = fin[q];
                f.max = uniform(f.max);
                const NormDist d = norm_dist(p, f, raw);
                // (the key's scale: one division per tile and member, wavefront-uniform, behind the ballot)
                append_passers(count, seg, fp.seg_cap, valid && norm_keep(p, d.nd), lane, [&] { return ((uint64_t)norm_key_scaled(d.dist, f.max, norm_key_scale(f.max)) << 32) | idx; });
            }
        }

        if (!has_next) break;
        cur = ahead;  // dead, empty or walked to its end: the next tile starts from the prefetched chunk
        t = t_next;
        cur_tile = next_tile;
    }
}

// raw: RAW_LEV or RAW_LCS; every query single-word; `narrow` = every query <= 32 symbols.  The grid is scan_grid()'s, as topk_multi_grid's is.
// fp.norm: an f64 plan of a normalized op under a cutoff, every maximum of the launch <= kNormKeyMaxMaximum (the caller's rule: the launcher cannot see
// the corpus' lengths).
hipError_t launch_filter_multi(RawKind raw, bool narrow, const FilterMultiParams& fp, hipStream_t stream)
{
    const ScanParams& p = fp.s;
    if (!fp.count || (fp.seg_cap && !fp.cand) || p.tile_end > p.n_tiles) return hipErrorInvalidValue;
    if (fp.norm ? !(p.out_f64 && p.has_cutoff && (p.op == RF_OP_NORMALIZED_DISTANCE || p.op == RF_OP_NORMALIZED_SIMILARITY)) : p.out_f64 != 0) return hipErrorInvalidValue;
    if (p.tile_end <= p.tile_begin) return hipSuccess;
    const dim3 g(std::max(1, scan_grid(p.tile_end - p.tile_begin))), b(kWave * kWavesPerBlock);
    return dispatch_multi(raw, narrow, p, [&](auto state, auto q, auto uniform) {
        using State = typename decltype(state)::type;
        if (fp.norm)
            hipLaunchKernelGGL((filter_multi_kernel<State, decltype(q)::value, decltype(uniform)::value, true>), g, b, 0, stream, fp);
        else
            hipLaunchKernelGGL((filter_multi_kernel<State, decltype(q)::value, decltype(uniform)::value, false>), g, b, 0, stream, fp);
        return hipGetLastError();
    });
}

}  // namespace rf

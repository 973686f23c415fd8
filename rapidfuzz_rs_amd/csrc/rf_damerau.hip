// rf_damerau.hip -- the unrestricted Damerau-Levenshtein distance (damerau_levenshtein.rs:111-168 distance_zhao; maximum = max(len1, len2),
// :194-196): the O(len1 * len2) row DP with transposition bookkeeping, one candidate per lane, in the orientation of rf_long.hip's
// Wagner-Fischer kernels -- the candidate's symbols stream by as columns, the row over the query positions is the state.  The recurrence
// and the packed cell (row, the row two columns back, the saved transposition term and the last hit column of one query position in ONE
// word) are rf_dl_cell.hpp, which the host tests compile too.  The reference's common-affix stripping (:187) changes nothing in the value
// and is not replayed; cutoffs are applied by emit_fin to the exact distance (:183-185 only ever turns a distance that fails into None).
//   dl_reg_kernel   queries of <= 16 / 32 / 64 symbols while max(len1, longest candidate) <= 254: the cells, 8-bit fields, in registers
//   dl_kernel       everything else: the cells as [y][lane] in LDS (8-bit fields, or 16-bit fields in a u64 beyond 254 symbols), or in a
//                   global strip per wavefront when a row does not fit LDS (plan(): wf_waves / wf_global, as for wf_kernel)
#include "rf_device.hpp"
#include "rf_dl_cell.hpp"

namespace rf {

// max(len1, len2) is FIN_LEV's maximum at factor 1: value, cutoff and normalisation are emit_usize's
template <bool kUniform, int kMax>
__global__ __launch_bounds__(kWave* kWavesPerBlock) void dl_reg_kernel(const ScanParams p)
{
    using Cell = DlCell8;
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t wave = uniform(threadIdx.x / kWave);
    const uint32_t len1 = p.len1;
    for (uint32_t t = blockIdx.x * kWavesPerBlock + wave; t < p.n_tiles; t += gridDim.x * kWavesPerBlock) {
        const TileView tv = load_tile<kUniform>(p, t);
        const uint32_t len2 = tv.len;
        const uint32_t slot = tv.slot0 + lane;
        uint32_t idx = slot;
        if (!kUniform) idx = p.orig[slot];
        uint32_t cell[kMax];  // query position y lives in cell[y - 1]; entries beyond len1 are computed and never read
#pragma unroll
        for (int i = 0; i < kMax; ++i) cell[i] = Cell::first((uint32_t)i + 1);
        const uint32_t nch = (len2 + kChunk - 1) / kChunk;
        uint32_t x = 0;
        for (uint32_t c = 0; c < nch; ++c) {
            uint4 data = load_chunk(tv.src + (size_t)c * kWave + lane);
            const uint32_t cols = min((uint32_t)kChunk, len2 - c * kChunk);
            for (uint32_t j = 0; j < cols; ++j) {
                const uint32_t ch = data.x & 0xFFu;
                DlColumn s;
                s.begin<Cell>(++x);
#pragma unroll
                for (int i = 0; i < kMax; ++i) {
                    const uint32_t qi = (p.wf_query[i / 4] >> (8 * (i % 4))) & 0xFFu;  // scalar
                    cell[i] = dl_step<Cell>(s, cell[i], qi == ch, (uint32_t)i + 1);
                }
                data.x = __builtin_amdgcn_alignbit(data.y, data.x, 8);
                data.y = __builtin_amdgcn_alignbit(data.z, data.y, 8);
                data.z = __builtin_amdgcn_alignbit(data.w, data.z, 8);
                data.w >>= 8;
            }
        }
        const bool valid = kUniform ? slot < p.n : idx != kPad;
        if (valid) {
            uint32_t last = 0;
#pragma unroll
            for (int i = 0; i < kMax; ++i) last = (uint32_t)i + 1 == len1 ? cell[i] : last;  // cell[len1 - 1] without dynamic indexing
            emit_usize(p, len1 ? Cell::row(last) : len2, len2, idx);
        }
    }
}

template <class Cell, bool kUniform>
__global__ __launch_bounds__(kWave* kWavesPerBlock) void dl_kernel(const ScanParams p)
{
    using W = typename Cell::word;
    extern __shared__ uint64_t lds_dl[];  // (u64: the wide cells' alignment) the query's bytes, then the rows
    uint32_t* lds_q = reinterpret_cast<uint32_t*>(lds_dl);
    const uint32_t len1 = p.len1;
    const uint32_t qwords = ((len1 + 3) / 4 + 2) & ~1u;  // query bytes, 4 per word, at least one word of slack, a whole number of u64
    stage_query_bytes(p, lds_q, qwords);

    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t wave = uniform(threadIdx.x / kWave);
    const uint32_t waves = blockDim.x / kWave;
    // row[(y - 1) * kWave] = the cell of query position y of this lane
    W* row = p.wf_global ? reinterpret_cast<W*>(p.long_scratch) + ((size_t)blockIdx.x * waves + wave) * len1 * kWave + lane
                         : reinterpret_cast<W*>(lds_q + qwords) + (size_t)wave * len1 * kWave + lane;

    for (uint32_t t = blockIdx.x * waves + wave; t < p.n_tiles; t += gridDim.x * waves) {
        const TileView tv = load_tile<kUniform>(p, t);
        const uint32_t len2 = tv.len;
        const uint32_t slot = tv.slot0 + lane;
        uint32_t idx = slot;
        if (!kUniform) idx = p.orig[slot];
        for (uint32_t y = 1; y <= len1; ++y) row[(size_t)(y - 1) * kWave] = Cell::first(y);
        const uint32_t nch = (len2 + kChunk - 1) / kChunk;
        uint32_t x = 0;
        for (uint32_t c = 0; c < nch; ++c) {
            const uint4 data = load_chunk(tv.src + (size_t)c * kWave + lane);
            const uint32_t cols = min((uint32_t)kChunk, len2 - c * kChunk);
            for (uint32_t j = 0; j < cols; ++j) {
                const uint32_t word = j < 4 ? data.x : (j < 8 ? data.y : (j < 12 ? data.z : data.w));
                const uint32_t ch = (word >> (8 * (j & 3))) & 0xFFu;
                DlColumn s;
                s.begin<Cell>(++x);
                for (uint32_t i = 0; i < len1; i += 4) {
                    const uint32_t q4 = lds_q[i / 4];  // wavefront-uniform address: one broadcast read for 4 symbols
                    const uint32_t lim = min(4u, len1 - i);
                    for (uint32_t k = 0; k < lim; ++k) {
                        W* at = row + (size_t)(i + k) * kWave;
                        *at = dl_step<Cell>(s, *at, ((q4 >> (8 * k)) & 0xFFu) == ch, i + k + 1);
                    }
                }
            }
        }
        const bool valid = kUniform ? slot < p.n : idx != kPad;
        if (valid) emit_usize(p, len1 ? Cell::row(row[(size_t)(len1 - 1) * kWave]) : len2, len2, idx);
    }
}

template <int kMax>
static hipError_t launch_dl_reg(const ScanParams& p, hipStream_t stream)
{
    const dim3 g(std::max(1, scan_grid(p.n_tiles))), b(kWave * kWavesPerBlock);
    if (p.tiles)
        hipLaunchKernelGGL((dl_reg_kernel<false, kMax>), g, b, 0, stream, p);
    else
        hipLaunchKernelGGL((dl_reg_kernel<true, kMax>), g, b, 0, stream, p);
    return hipGetLastError();
}

template <class Cell>
static hipError_t launch_dl_rows(const ScanParams& p, hipStream_t stream)
{
    const size_t qwords = (((size_t)p.len1 + 3) / 4 + 2) & ~(size_t)1;
    const size_t lds = qwords * 4 + (p.wf_global ? 0 : (size_t)p.wf_waves * p.len1 * kWave * sizeof(typename Cell::word));
    const dim3 g(p.wf_global ? std::max(1u, p.long_grid) : (uint32_t)std::max(1, scan_grid(p.n_tiles))), b(kWave * p.wf_waves);
    auto k = p.tiles ? dl_kernel<Cell, false> : dl_kernel<Cell, true>;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k, g, b, lds, stream, p);
    return hipGetLastError();
}

// plan() decided the cell (dl_wide) and where the rows live (dl_reg, wf_waves, wf_global)
hipError_t launch_dl(const ScanParams& p, hipStream_t stream)
{
    if (p.dl_reg) {
        if (p.len1 <= 16) return launch_dl_reg<16>(p, stream);
        if (p.len1 <= 32) return launch_dl_reg<32>(p, stream);
        return launch_dl_reg<64>(p, stream);
    }
    return p.dl_wide ? launch_dl_rows<DlCell16>(p, stream) : launch_dl_rows<DlCell8>(p, stream);
}

}  // namespace rf

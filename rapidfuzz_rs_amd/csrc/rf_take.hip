// rf_take.hip -- candidates read back OUT of the packed corpus (rf_corpus_take / rf_corpus_lengths, host side in rf_api_take.hip): the inverse of the packers.
// The packed form is a bijection of its input -- length-bucketed tiles, chunks interleaved 64 lanes x 16 bytes, symbols renamed by sigma, `char` corpora as
// alphabet ids + a raw stream for the overflow symbols -- and rf_take_addr.hpp is the address arithmetic of the way back, shared with the host.
//
// Two roads, both un-renaming through an LDS copy of the inverse sigma (and, `char` corpora, of the id -> symbol table) staged once per workgroup:
//   by index list   take_rows_len_kernel: one work item per requested row -> its slot and length (the host scans the lengths into offsets);
//                   take_rows_kernel: one lane per (row, chunk): one dwordx4 load, un-rename, store min(16, len - 16 k) symbols at out + offsets[row] + 16 k.
//                   Neighbouring lanes hold neighbouring chunks of one row: the loads are scattered (the rows are wherever the caller asks), the stores meet.
//   whole corpus    take_all_kernel: a wavefront per tile reads each chunk row as the scans do (one contiguous 1 KiB, load_tile / load_chunk) and lane r
//                   writes its 16 symbols at out + offsets[orig[slot]] + 16 k.  Padding lanes write nothing; a mixed block is walked once per one-length view
//                   and a lane writes only in the view whose orig[] names it, so every candidate is written exactly once.
// The destination of a chunk is not 16-byte aligned in general and a row's last chunk is never rounded up past the row's end: one 16-byte store where the
// chunk is whole and its destination aligned (every chunk of a single-length corpus whose length is a multiple of 16), else dword stores + a byte tail, else bytes.
// Plain vector stores only; no inline assembly.
#include "rf_device.hpp"
#include "rf_take_addr.hpp"

namespace rf {

static_assert(kTakeLanes == (uint32_t)kWave && kTakeChunk == (uint32_t)kChunk && kTakePad == kPad, "rf_take_addr.hpp restates the tile shape");
constexpr uint32_t kTakeOverflowId = 254;  // rf_host.hpp kOverflowId: the id every symbol beyond a `char` corpus' alphabet shares (its symbol: the raw stream)

struct TakeTables {
    uint32_t sym[256];  // id -> symbol (the identity for byte corpora)
    uint8_t inv[256];   // stored symbol -> id
};

__device__ __forceinline__ void stage_take_tables(const TakeParams& p, TakeTables& t)  // whole workgroup; synchronizes
{
    for (uint32_t c = threadIdx.x; c < 256; c += blockDim.x) {
        t.inv[c] = p.inv_sigma[c];
        t.sym[c] = p.sym_of_id ? p.sym_of_id[c] : c;
    }
    __syncthreads();
}

// the symbol behind stored byte `v` at payload position x
__device__ __forceinline__ uint32_t take_symbol(const TakeParams& p, const TakeTables& t, uint32_t v, uint64_t x)
{
    const uint32_t id = t.inv[v];
    if (p.raw && id == kTakeOverflowId)
        return p.raw_elem == 2 ? (uint32_t) reinterpret_cast<const uint16_t*>(p.raw)[x] : reinterpret_cast<const uint32_t*>(p.raw)[x];
    return t.sym[id];
}

// `fill` (1..16) symbols of the chunk `v` that sits at payload position x, to out[at ..)
__device__ __forceinline__ void take_store_chunk(const TakeParams& p, const TakeTables& t, uint4 v, uint64_t x, uint64_t at, uint32_t fill)
{
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    if (p.out_u32) {
        uint32_t* dst = static_cast<uint32_t*>(p.out) + at;
#pragma unroll
        for (uint32_t b = 0; b < kTakeChunk; ++b)
            if (b < fill) dst[b] = take_symbol(p, t, (w[b / 4] >> (8 * (b % 4))) & 0xFFu, x + b);
        return;
    }
    uint32_t u[4];  // (byte output: the symbols are bytes -- take_symbol's table is the identity or, rf_corpus_take refuses `char` corpora, never read)
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q)
        u[q] = (uint32_t)t.inv[w[q] & 0xFFu] | (uint32_t)t.inv[(w[q] >> 8) & 0xFFu] << 8 | (uint32_t)t.inv[(w[q] >> 16) & 0xFFu] << 16 | (uint32_t)t.inv[w[q] >> 24] << 24;
    uint8_t* dst = static_cast<uint8_t*>(p.out) + at;
    const uintptr_t a = reinterpret_cast<uintptr_t>(dst);
    if (fill == kTakeChunk && (a & 15u) == 0) {
        *reinterpret_cast<uint4*>(dst) = make_uint4(u[0], u[1], u[2], u[3]);
        return;
    }
    uint32_t b = 0;
    if ((a & 3u) == 0) {
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q)
            if (4 * q + 4 <= fill) {
                reinterpret_cast<uint32_t*>(dst)[q] = u[q];
                b = 4 * q + 4;
            }
    }
#pragma unroll
    for (uint32_t i = 0; i < kTakeChunk; ++i)
        if (i >= b && i < fill) dst[i] = (uint8_t)(u[i / 4] >> (8 * (i % 4)));
}

// payload base and length of the tile that holds `slot`
__device__ __forceinline__ void take_tile(const TakeParams& p, uint32_t slot, uint64_t* base, uint32_t* len)
{
    const uint32_t t = take_tile_of(slot);
    if (p.s.tiles) {
        const TileDesc td = p.s.tiles[t];
        *base = td.data_off;
        *len = td.len;
    } else {
        *base = take_uniform_base(t, p.s.uniform_len);
        *len = p.s.uniform_len;
    }
}

__global__ __launch_bounds__(256) void take_rows_len_kernel(const TakeParams p)
{
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < p.m; j += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t i = p.idx[j];
        const uint32_t slot = p.slot_of ? p.slot_of[i] : i;
        uint64_t base;
        uint32_t len = 0;
        if (slot < p.n_slots) take_tile(p, slot, &base, &len);
        p.row_slot[j] = slot;
        p.row_len[j] = len;
    }
}

__global__ __launch_bounds__(256) void take_rows_kernel(const TakeParams p)
{
    __shared__ TakeTables tab;
    stage_take_tables(p, tab);
    const uint64_t items = p.m * p.row_chunks;
    for (uint64_t it = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t j = it / p.row_chunks;
        const uint32_t k = (uint32_t)(it % p.row_chunks);
        const uint32_t fill = take_chunk_fill(p.row_len[j], k);  // (0 for the rows that named no slot: their length is 0)
        if (!fill) continue;
        const uint32_t slot = p.row_slot[j];
        uint64_t base;
        uint32_t len;
        take_tile(p, slot, &base, &len);
        const uint64_t x = take_chunk_at(base, take_lane_of(slot), k);
        take_store_chunk(p, tab, load_chunk(reinterpret_cast<const uint4*>(p.s.data + x)), x, p.offsets[j] + (uint64_t)k * kTakeChunk, fill);
    }
}

template <bool kUniform>
__global__ __launch_bounds__(kWave* kWavesPerBlock) void take_all_kernel(const TakeParams p)
{
    __shared__ TakeTables tab;
    stage_take_tables(p, tab);
    const uint32_t lane = threadIdx.x % kWave;
    const uint32_t wave = uniform(blockIdx.x * kWavesPerBlock + threadIdx.x / kWave), waves = gridDim.x * kWavesPerBlock;
    for (uint32_t t = wave; t < p.s.n_tiles; t += waves) {
        const TileView tv = load_tile<kUniform>(p.s, t);
        const uint32_t slot = tv.slot0 + lane;
        const uint32_t i = kUniform ? (slot < p.s.n ? slot : kPad) : p.s.orig[slot];
        if (i == kPad || i >= p.s.n) continue;  // a padding lane, or a lane another view of this mixed block owns
        const uint64_t at = p.offsets ? p.offsets[i] : (uint64_t)i * tv.len;
        const uint64_t x0 = (uint64_t)(reinterpret_cast<const uint8_t*>(tv.src) - p.s.data);
        for (uint32_t k = 0; k * kTakeChunk < tv.len; ++k) {
            const uint64_t x = take_chunk_at(x0, lane, k);
            take_store_chunk(p, tab, load_chunk(tv.src + (size_t)k * kWave + lane), x, at + (uint64_t)k * kTakeChunk, take_chunk_fill(tv.len, k));
        }
    }
}

static uint32_t take_grid(uint64_t items, uint32_t per_block)
{
    const uint64_t blocks = (items + per_block - 1) / per_block;
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(blocks, 1), (uint64_t)scan_max_grid() * 8);
}

hipError_t launch_take_rows_len(const TakeParams& p, hipStream_t stream)
{
    if (p.m == 0) return hipSuccess;
    hipLaunchKernelGGL(take_rows_len_kernel, dim3(take_grid(p.m, 256)), dim3(256), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_take_rows(const TakeParams& p, hipStream_t stream)
{
    if (p.m == 0 || p.row_chunks == 0) return hipSuccess;
    hipLaunchKernelGGL(take_rows_kernel, dim3(take_grid(p.m * p.row_chunks, 256)), dim3(256), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_take_all(const TakeParams& p, hipStream_t stream)
{
    if (p.s.n_tiles == 0) return hipSuccess;
    const dim3 g(take_grid(p.s.n_tiles, kWavesPerBlock)), b(kWave * kWavesPerBlock);
    if (p.s.tiles)
        hipLaunchKernelGGL((take_all_kernel<false>), g, b, 0, stream, p);
    else
        hipLaunchKernelGGL((take_all_kernel<true>), g, b, 0, stream, p);
    return hipGetLastError();
}

}  // namespace rf

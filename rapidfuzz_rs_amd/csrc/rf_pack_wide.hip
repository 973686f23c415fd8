// rf_pack_wide.hip -- the device front end of rf_corpus_pack_u32: `char` (u32) symbols in, the byte pipeline of rf_pack_ragged.hip out.
//
// The host packer (rf_api.hip pack_u32_host) stays the specification: a histogram of every symbol, the alphabet chosen from it (rf_alphabet.hpp), every symbol
// rewritten to its alphabet id, the id bytes packed like a byte corpus, and -- only when some symbols share the overflow id -- the raw symbol behind every packed
// byte at the same element index.  Here the three per-symbol passes run on the device:
//   histogram    wide_hist_kernel: exact 64-bit counts of every symbol below 0x10000.  65536 u32 bins do not fit the 160 KiB of LDS, so the grid has two halves
//                (blockIdx.y): a workgroup counts the symbols of ITS half of the BMP in 32768 LDS bins (128 KiB, one workgroup per CU) and skips the others, then
//                adds its non-empty bins to the global table.  Skewed text puts a wavefront's lanes on a few counters: those meet in LDS, where a 64-way collision
//                costs 64 LDS cycles, never in L2.  The input is read twice; both reads together stay far below what the upload of the same symbols costs.
//                Symbols from 0x10000 up are only counted (and the reserved 0xFFFFFFFF flagged) here; when there are any, wide_compact_high_kernel collects
//                them (one global atomic per 8192-symbol stretch), hipcub sorts them and run-length encodes the runs: exact (symbol, count) pairs.
//   id image     wide_ids_kernel: u32 -> 1 byte, through a 64 KiB LDS table for the BMP and a binary search over the (at most 254) alphabet symbols above it
//   raw stream   wide_raw_kernel: one wavefront per destination tile, exact and mixed, like the payload scatter: lane r writes its 16 symbols of chunk k, so a
//                wavefront writes 2 or 4 KiB contiguously; the padding value (all ones) behind a candidate's end and on lanes without a candidate
// The histogram counts elems[0 .. total) like the host packer (what lies in front of a window included); the other kernels read [first, total) only, never beyond a
// candidate's end, and nothing reads at or beyond the payload's end.
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "rf_device.hpp"

namespace rf {

namespace {

constexpr uint32_t kHistThreads = 1024, kHalfBins = 32768, kHistUnroll = 4;

// low: 65536 counts; *n_high: symbols at or above 0x10000; *flags bit 0: the reserved symbol 0xFFFFFFFF is there.  elems[0 .. span) is what is counted.
__global__ __launch_bounds__(kHistThreads) void wide_hist_kernel(const uint32_t* __restrict__ elems, uint64_t span, unsigned long long* __restrict__ low,
                                                                 unsigned long long* __restrict__ n_high, uint32_t* __restrict__ flags)
{
    __shared__ uint32_t bins[kHalfBins];
    for (uint32_t b = threadIdx.x; b < kHalfBins; b += kHistThreads) bins[b] = 0;
    __syncthreads();
    const uint32_t half = blockIdx.y;
    unsigned long long high = 0;
    uint32_t bad = 0;
    auto count = [&](uint32_t ch) {
        if ((ch >> 15) == half)
            atomicAdd(&bins[ch & (kHalfBins - 1)], 1u);
        else if (half == 0 && ch >= 0x10000u) {
            ++high;
            bad |= ch == 0xFFFFFFFFu;
        }
    };
    const uint64_t step = (uint64_t)gridDim.x * kHistThreads;
    uint64_t i = (uint64_t)blockIdx.x * kHistThreads + threadIdx.x;
    for (; i + (kHistUnroll - 1) * step < span; i += kHistUnroll * step) {  // the loads of a trip are in flight together
        uint32_t ch[kHistUnroll];
#pragma unroll
        for (uint32_t u = 0; u < kHistUnroll; ++u) ch[u] = elems[i + u * step];
#pragma unroll
        for (uint32_t u = 0; u < kHistUnroll; ++u) count(ch[u]);
    }
    for (; i < span; i += step) count(elems[i]);
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < kHalfBins; b += kHistThreads)
        if (bins[b]) atomicAdd(&low[half * kHalfBins + b], (unsigned long long)bins[b]);
    if (high) atomicAdd(n_high, high);
    if (bad) atomicOr(flags, 1u);
}

// the symbols at or above 0x10000, in any order: a workgroup ranks those of a stretch of kCompactPer symbols per thread in LDS and reserves their places with one atomic
constexpr uint32_t kCompactThreads = 1024, kCompactPer = 8;
__global__ __launch_bounds__(kCompactThreads) void wide_compact_high_kernel(const uint32_t* __restrict__ elems, uint64_t span, uint32_t* __restrict__ out, uint32_t cap,
                                                                           unsigned long long* __restrict__ cursor)
{
    __shared__ uint32_t lds_count;
    __shared__ unsigned long long lds_base;
    constexpr uint64_t kStretch = (uint64_t)kCompactThreads * kCompactPer;
    for (uint64_t s0 = (uint64_t)blockIdx.x * kStretch; s0 < span; s0 += (uint64_t)gridDim.x * kStretch) {
        if (threadIdx.x == 0) lds_count = 0;
        __syncthreads();
        uint32_t ch[kCompactPer], rank[kCompactPer] = {};
#pragma unroll
        for (uint32_t u = 0; u < kCompactPer; ++u) {
            const uint64_t i = s0 + (uint64_t)u * kCompactThreads + threadIdx.x;
            ch[u] = i < span ? elems[i] : 0u;
        }
#pragma unroll
        for (uint32_t u = 0; u < kCompactPer; ++u)
            if (ch[u] >= 0x10000u) rank[u] = atomicAdd(&lds_count, 1u);
        __syncthreads();
        if (threadIdx.x == 0) lds_base = lds_count ? atomicAdd(cursor, (unsigned long long)lds_count) : 0ull;
        __syncthreads();
        const unsigned long long base = lds_base;
#pragma unroll
        for (uint32_t u = 0; u < kCompactPer; ++u)
            if (ch[u] >= 0x10000u && base + rank[u] < cap) out[base + rank[u]] = ch[u];
        __syncthreads();
    }
}

typedef uint32_t u4_align4 __attribute__((ext_vector_type(4), aligned(4)));

// out[j] = id of elems[j], j in [0, span): table = the id of every symbol below 0x10000 (overflow id where it has none), hi_syms ascending with hi_ids beside them
constexpr uint32_t kIdsThreads = 1024, kMaxHighIds = 256;
__global__ __launch_bounds__(kIdsThreads) void wide_ids_kernel(const uint32_t* __restrict__ elems, uint64_t span, const uint8_t* __restrict__ table, const uint32_t* __restrict__ hi_syms,
                                                               const uint8_t* __restrict__ hi_ids, uint32_t n_hi, uint32_t overflow_id, uint8_t* __restrict__ out)
{
    __shared__ uint32_t lds_table[0x10000 / 4];
    __shared__ uint32_t lds_hi[kMaxHighIds];
    __shared__ uint8_t lds_hi_id[kMaxHighIds];
    for (uint32_t w = threadIdx.x; w < 0x10000 / 4; w += kIdsThreads) lds_table[w] = reinterpret_cast<const uint32_t*>(table)[w];
    for (uint32_t h = threadIdx.x; h < n_hi; h += kIdsThreads) lds_hi[h] = hi_syms[h], lds_hi_id[h] = hi_ids[h];
    __syncthreads();
    const uint8_t* lut = reinterpret_cast<const uint8_t*>(lds_table);
    auto id_of = [&](uint32_t ch) -> uint32_t {
        if (ch < 0x10000u) return lut[ch];
        uint32_t lo = 0, hi = n_hi;  // first entry >= ch
        while (lo < hi) {
            const uint32_t mid = (lo + hi) / 2;
            if (lds_hi[mid] < ch)
                lo = mid + 1;
            else
                hi = mid;
        }
        return lo < n_hi && lds_hi[lo] == ch ? (uint32_t)lds_hi_id[lo] : overflow_id;
    };
    const uint64_t quads = (span + 3) / 4;
    for (uint64_t q = (uint64_t)blockIdx.x * kIdsThreads + threadIdx.x; q < quads; q += (uint64_t)gridDim.x * kIdsThreads) {
        const uint64_t j = q * 4;
        if (j + 4 <= span) {
            const u4_align4 v = *reinterpret_cast<const u4_align4*>(elems + j);
            *reinterpret_cast<uint32_t*>(out + j) = id_of(v.x) | id_of(v.y) << 8 | id_of(v.z) << 16 | id_of(v.w) << 24;  // (out is the library's own buffer: 4-byte aligned at j)
        } else {
            for (uint64_t e = j; e < span; ++e) out[e] = (uint8_t)id_of(elems[e]);
        }
    }
}

// one wavefront per destination tile: tiles [0, n_exact) as the payload scatter addresses them, then the n_mixed mixed tiles.  elems[0] is the symbol at offset `first`.
template <typename Sym>
__global__ __launch_bounds__(256) void wide_raw_kernel(const uint32_t* __restrict__ elems, uint64_t first, const uint64_t* __restrict__ offsets, uint32_t n, const TileDesc* __restrict__ tiles,
                                                       uint32_t uniform_len, uint32_t n_exact, const uint32_t* __restrict__ orig, const MixedDesc* __restrict__ mixed, uint32_t n_mixed,
                                                       const uint32_t* __restrict__ mixed_len, const uint32_t* __restrict__ mixed_orig, Sym* __restrict__ raw)
{
    constexpr uint32_t kPerStore = 16 / sizeof(Sym);  // symbols per 16-byte store
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t total_tiles = n_exact + n_mixed;
    for (uint32_t t = blockIdx.x * kWavesPerBlock + threadIdx.x / kWave; t < total_tiles; t += gridDim.x * kWavesPerBlock) {
        uint32_t i, my_len, block_len;
        uint64_t data_off;
        if (t < n_exact) {
            block_len = tiles ? tiles[t].len : uniform_len;
            const uint32_t slot0 = tiles ? tiles[t].slot0 : t * kWave;
            data_off = tiles ? tiles[t].data_off : (uint64_t)t * (((block_len + kChunk - 1) / kChunk) * kWave * kChunk);
            i = orig ? orig[slot0 + lane] : (slot0 + lane < n ? slot0 + lane : kPad);
            my_len = i == kPad ? 0u : block_len;
        } else {
            const uint32_t m = t - n_exact, q = m * kWave + lane;
            block_len = mixed[m].max_len;
            data_off = mixed[m].data_off;
            i = mixed_orig[q];
            my_len = i == kPad ? 0u : mixed_len[q];
        }
        const uint32_t* src = elems + (i == kPad ? 0 : offsets[i] - first);
        const uint32_t nch = (block_len + kChunk - 1) / kChunk;
        uint4* dst = reinterpret_cast<uint4*>(raw + data_off) + (size_t)lane * (kChunk / kPerStore);
        for (uint32_t k = 0; k < nch; ++k) {
            uint32_t s[kChunk];
#pragma unroll
            for (uint32_t e = 0; e < (uint32_t)kChunk; e += 4) {
                const uint32_t b = k * kChunk + e;
                if (b + 4 <= my_len) {
                    const u4_align4 v = *reinterpret_cast<const u4_align4*>(src + b);
                    s[e] = v.x, s[e + 1] = v.y, s[e + 2] = v.z, s[e + 3] = v.w;
                } else {
#pragma unroll
                    for (uint32_t f = 0; f < 4; ++f) s[e + f] = b + f < my_len ? src[b + f] : 0xFFFFFFFFu;
                }
            }
            uint4* d = dst + (size_t)k * kWave * (kChunk / kPerStore);
            if (sizeof(Sym) == 2) {
                auto two = [&](uint32_t e) { return (s[e] & 0xFFFFu) | (s[e + 1] << 16); };
                d[0] = make_uint4(two(0), two(2), two(4), two(6));
                d[1] = make_uint4(two(8), two(10), two(12), two(14));
            } else {
#pragma unroll
                for (uint32_t e = 0; e < 4; ++e) d[e] = make_uint4(s[4 * e], s[4 * e + 1], s[4 * e + 2], s[4 * e + 3]);
            }
        }
    }
}

}  // namespace

hipError_t launch_wide_hist(const uint32_t* elems, uint64_t span, unsigned long long* low, unsigned long long* n_high, uint32_t* flags, hipStream_t st)
{
    if (span == 0) return hipSuccess;
    // (a workgroup's LDS bins are u32: it sees span / grid symbols, and the callers keep span below 2^40)
    const uint64_t per_block = (uint64_t)kHistThreads * kHistUnroll * 4;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((span + per_block - 1) / per_block, 512);
    hipLaunchKernelGGL(wide_hist_kernel, dim3(grid, 2), dim3(kHistThreads), 0, st, elems, span, low, n_high, flags);
    return hipGetLastError();
}

hipError_t launch_wide_compact_high(const uint32_t* elems, uint64_t span, uint32_t* out, uint32_t cap, unsigned long long* cursor, hipStream_t st)
{
    if (span == 0 || cap == 0) return hipSuccess;
    const uint64_t stretch = (uint64_t)kCompactThreads * kCompactPer;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((span + stretch - 1) / stretch, 2048);
    hipLaunchKernelGGL(wide_compact_high_kernel, dim3(grid), dim3(kCompactThreads), 0, st, elems, span, out, cap, cursor);
    return hipGetLastError();
}

// the runs of `n` symbols: sorted into `sorted`, then unique[r] / counts[r] for r < *num_runs (all device memory, n entries each)
size_t wide_runs_temp_bytes(uint32_t n)
{
    size_t a = 0, b = 0;
    (void)hipcub::DeviceRadixSort::SortKeys(nullptr, a, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)n, 0, 32, nullptr);
    (void)hipcub::DeviceRunLengthEncode::Encode(nullptr, b, (const uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (int)n, nullptr);
    return std::max<size_t>((std::max(a, b) + 255) / 256 * 256, 256);
}
hipError_t launch_wide_runs(const uint32_t* syms, uint32_t* sorted, uint32_t n, uint32_t* unique, uint32_t* counts, uint32_t* num_runs, void* temp, size_t temp_bytes, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    size_t bytes = temp_bytes;
    hipError_t e = hipcub::DeviceRadixSort::SortKeys(temp, bytes, syms, sorted, (int)n, 0, 32, st);
    if (e != hipSuccess) return e;
    bytes = temp_bytes;
    return hipcub::DeviceRunLengthEncode::Encode(temp, bytes, sorted, unique, counts, num_runs, (int)n, st);
}

hipError_t launch_wide_ids(const uint32_t* elems, uint64_t span, const uint8_t* table, const uint32_t* hi_syms, const uint8_t* hi_ids, uint32_t n_hi, uint32_t overflow_id, uint8_t* out,
                           hipStream_t st)
{
    if (span == 0) return hipSuccess;
    if (n_hi > kMaxHighIds) return hipErrorInvalidValue;
    const uint64_t quads = (span + 3) / 4, per_block = (uint64_t)kIdsThreads * 8;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((quads + per_block - 1) / per_block, 2048);
    hipLaunchKernelGGL(wide_ids_kernel, dim3(grid), dim3(kIdsThreads), 0, st, elems, span, table, hi_syms, hi_ids, n_hi, overflow_id, out);
    return hipGetLastError();
}

hipError_t launch_wide_raw(const uint32_t* elems, uint64_t first, const uint64_t* offsets, uint32_t n, const TileDesc* tiles, uint32_t uniform_len, uint32_t n_exact, const uint32_t* orig,
                           const MixedDesc* mixed, uint32_t n_mixed, const uint32_t* mixed_len, const uint32_t* mixed_orig, void* raw, uint32_t raw_elem, hipStream_t st)
{
    const uint64_t total_tiles = (uint64_t)n_exact + n_mixed;
    if (total_tiles == 0) return hipSuccess;
    if (total_tiles > 0xFFFFFFFFull) return hipErrorInvalidValue;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((total_tiles + kWavesPerBlock - 1) / kWavesPerBlock, 65536);
    if (raw_elem == 2)
        hipLaunchKernelGGL(wide_raw_kernel<uint16_t>, dim3(grid), dim3(256), 0, st, elems, first, offsets, n, tiles, uniform_len, n_exact, orig, mixed, n_mixed, mixed_len, mixed_orig,
                           (uint16_t*)raw);
    else
        hipLaunchKernelGGL(wide_raw_kernel<uint32_t>, dim3(grid), dim3(256), 0, st, elems, first, offsets, n, tiles, uniform_len, n_exact, orig, mixed, n_mixed, mixed_len, mixed_orig,
                           (uint32_t*)raw);
    return hipGetLastError();
}

}  // namespace rf

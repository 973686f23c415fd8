// rf_compare.hip -- hamming (hamming.rs:138-187), prefix (prefix.rs:47-69) and postfix (postfix.rs:47-69): the three metrics of the reference that
// compare symbols AT THE SAME POSITION.  No recurrence and no pattern-match table: one candidate per lane, the tile's chunk row k (one
// global_load_dwordx4 per lane, 1 KiB per wavefront) XOR the query's 16 symbols at the same positions, and the byte tests of rf_bytecmp.hpp
// on the result.  The query -- renamed like the corpus, rebuilt from the comparator's table by stage_query_bytes -- sits in LDS with a chunk of
// zeros on either side; a chunk of it is read at a wavefront-uniform address and moved to scalar registers.
//   hamming   raw = mismatches over min(len1, len2) symbols + |len1 - len2|; FIN_LEV at factor 1 (maximum = max(len1, len2)).  Four chunk rows are
//             in flight per lane.  Without RF_FLAG_HAMMING_PAD (ScanParams::cmp_strict) a tile of another length than the query's is answered from its
//             length alone, its payload unread.
//   prefix    raw = length of the common prefix; FIN_LCS.  A lane leaves at its first mismatch and the wavefront leaves the tile when its last lane
//             has (a ballot): unrelated strings cost one chunk row per candidate.
//   postfix   raw = length of the common suffix; FIN_LCS.  The same walk from the candidate's last chunk row backwards.  Candidate position j meets
//             query position j + len1 - len2, so the query is read at a byte offset that is no multiple of 16 in general: five aligned dwords and
//             four funnel shifts per chunk, the shift uniform per tile -- no unaligned load anywhere.
// Where a string ends is decided by its LENGTH (one per tile), never by a zero byte: the padding behind a candidate is zero, and zero is the most
// frequent symbol of the corpus after renaming.  Every tile is a one-length view (the views of the mixed section included: lanes of other lengths
// are padding lanes there), so min(len1, len2), the masks of the boundary chunks and postfix's shift are scalar.
#include "rf_device.hpp"
#include "rf_bytecmp.hpp"

namespace rf {

constexpr uint32_t kCmpFront = 4;  // words of zeros in front of the query in LDS (postfix reads up to 15 bytes before it)
constexpr uint32_t kCmpBack = 8;   // ... and behind its last word (every kernel reads up to a chunk + a word past the query's end)
static __host__ __device__ inline uint32_t cmp_query_words(uint32_t len1) { return (len1 + 3) / 4; }

// 16 query symbols from byte offset `at` of the query (at >= -15; whatever lies outside the query reads as zero and is masked by the caller), scalar
__device__ __forceinline__ Chunk4 query_chunk(const uint32_t* lds_q, int32_t at)
{
    const uint32_t a = (uint32_t)(at + (int32_t)(4 * kCmpFront));
    const uint32_t w = a >> 2, sh = a & 3u;
    const uint32_t q0 = lds_q[w], q1 = lds_q[w + 1], q2 = lds_q[w + 2], q3 = lds_q[w + 3], q4 = lds_q[w + 4];
    return Chunk4{uniform(align_bytes(q1, q0, sh)), uniform(align_bytes(q2, q1, sh)), uniform(align_bytes(q3, q2, sh)), uniform(align_bytes(q4, q3, sh))};
}
__device__ __forceinline__ Chunk4 diff(const uint4& d, const Chunk4& q) { return Chunk4{d.x ^ q.x, d.y ^ q.y, d.z ^ q.z, d.w ^ q.w}; }

__device__ __forceinline__ void emit_different_length(const ScanParams& p, uint32_t idx)
{
    if (!p.cmp_err_encode)
        emit_none(p, idx);
    else if (!p.out_f64)
        reinterpret_cast<uint32_t*>(p.out)[idx] = RF_DIFFERENT_LENGTH_U32;
    else
        reinterpret_cast<double*>(p.out)[idx] = __longlong_as_double((long long)RF_DIFFERENT_LENGTH_F64_BITS);
}

template <RawKind kRaw, bool kUniform>
__global__ __launch_bounds__(kWave* kWavesPerBlock) void compare_kernel(const ScanParams p)
{
    extern __shared__ uint32_t lds_cmp[];
    const uint32_t len1 = p.len1;
    const uint32_t qwords = cmp_query_words(len1);
    for (uint32_t i = threadIdx.x; i < kCmpFront; i += blockDim.x) lds_cmp[i] = 0;
    for (uint32_t i = threadIdx.x; i < kCmpBack; i += blockDim.x) lds_cmp[kCmpFront + qwords + i] = 0;
    stage_query_bytes(p, lds_cmp + kCmpFront, qwords);  // (zeroes its words, fills them, synchronizes)
    const uint32_t* lds_q = lds_cmp;

    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t wave = uniform(threadIdx.x / kWave);
    for (uint32_t t = blockIdx.x * kWavesPerBlock + wave; t < p.n_tiles; t += gridDim.x * kWavesPerBlock) {
        const TileView tv = load_tile<kUniform>(p, t);
        const uint32_t len2 = tv.len;
        const uint32_t slot = tv.slot0 + lane;
        uint32_t idx = slot;
        if (!kUniform) idx = p.orig[slot];
        const bool valid = kUniform ? slot < p.n : idx != kPad;
        const uint32_t m = min(len1, len2);  // the positions that are compared
        const uint4* src = tv.src + lane;
        uint32_t raw = 0;
        if (kRaw == RAW_HAMMING) {
            if (p.cmp_strict && len1 != len2) {
                if (valid) emit_different_length(p, idx);
                continue;
            }
            const uint32_t nch = (m + kChunk - 1) / kChunk;
            uint32_t c = 0;
            for (; c + 4 < nch; c += 4) {  // four whole chunks, none of them the last
                const uint4 d0 = load_chunk(src + (size_t)c * kWave), d1 = load_chunk(src + (size_t)(c + 1) * kWave), d2 = load_chunk(src + (size_t)(c + 2) * kWave),
                            d3 = load_chunk(src + (size_t)(c + 3) * kWave);
                raw += chunk_nonzero_bytes(diff(d0, query_chunk(lds_q, (int32_t)(c * kChunk))));
                raw += chunk_nonzero_bytes(diff(d1, query_chunk(lds_q, (int32_t)((c + 1) * kChunk))));
                raw += chunk_nonzero_bytes(diff(d2, query_chunk(lds_q, (int32_t)((c + 2) * kChunk))));
                raw += chunk_nonzero_bytes(diff(d3, query_chunk(lds_q, (int32_t)((c + 3) * kChunk))));
            }
            for (; c < nch; ++c) {  // up to four more; the last one counts the positions below m only
                const uint4 d = load_chunk(src + (size_t)c * kWave);
                const uint32_t rem = min((uint32_t)kChunk, m - c * kChunk);
                raw += chunk_nonzero_bytes(keep_range(diff(d, query_chunk(lds_q, (int32_t)(c * kChunk))), 0, rem));
            }
            raw += max(len1, len2) - m;
        } else if (kRaw == RAW_PREFIX) {
            const uint32_t nch = (m + kChunk - 1) / kChunk;
            bool alive = valid;
            for (uint32_t c = 0; c < nch; ++c) {
                if (__ballot(alive) == 0) break;  // every lane has met its first mismatch
                const uint4 d = load_chunk(src + (size_t)c * kWave);
                const uint32_t rem = min((uint32_t)kChunk, m - c * kChunk);
                const uint32_t first = chunk_first_nonzero(differ_outside(diff(d, query_chunk(lds_q, (int32_t)(c * kChunk))), 0, rem));  // (position m always differs)
                if (alive) raw += first;
                alive = alive && first == (uint32_t)kChunk;
            }
        } else {  // RAW_POSTFIX
            if (m) {
                const uint32_t j0 = len2 - m;                 // the candidate positions that are compared: [j0, len2)
                const uint32_t c_lo = j0 / kChunk, c_hi = (len2 - 1) / kChunk;
                const int32_t shift = (int32_t)len1 - (int32_t)len2;  // candidate position j meets query position j + shift
                bool alive = valid;
                for (uint32_t c = c_hi + 1; c-- > c_lo;) {
                    if (__ballot(alive) == 0) break;
                    const uint4 d = load_chunk(src + (size_t)c * kWave);
                    const uint32_t from = c == c_lo ? j0 - c * kChunk : 0u;              // below it: before the shorter string's start, always differs
                    const uint32_t to = min((uint32_t)kChunk, len2 - c * kChunk);        // from it on: the padding behind the candidate, skipped
                    const Chunk4 x = differ_outside(keep_range(diff(d, query_chunk(lds_q, (int32_t)(c * kChunk) + shift)), 0, to), from, kChunk);
                    const uint32_t last = chunk_last_nonzero(x);
                    const uint32_t matched = last == (uint32_t)kChunk ? to : to - 1u - last;  // (last < to: the positions from `to` on read as equal)
                    if (alive) raw += matched;
                    alive = alive && last == (uint32_t)kChunk;
                }
            }
        }
        if (valid) emit_usize(p, raw, len2, idx);
    }
}

// RF_COMPARE_MAX_BLOCKS (rfgpu.h): the forced several-tiles-per-wavefront run of the tests
static int compare_grid(uint32_t n_tiles)
{
    static const long long cap = env_int("RF_COMPARE_MAX_BLOCKS", 0);
    const int g = std::max(1, scan_grid(n_tiles));
    return cap > 0 ? (int)std::min<long long>(g, cap) : g;
}

template <RawKind kRaw>
static hipError_t launch_compare_kind(const ScanParams& p, hipStream_t stream)
{
    const size_t lds = ((size_t)kCmpFront + cmp_query_words(p.len1) + kCmpBack) * sizeof(uint32_t);
    const dim3 g(compare_grid(p.n_tiles)), b(kWave * kWavesPerBlock);
    auto k = p.tiles ? compare_kernel<kRaw, false> : compare_kernel<kRaw, true>;
    if (lds > (48u << 10)) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k, g, b, lds, stream, p);
    return hipGetLastError();
}

hipError_t launch_compare(RawKind raw, const ScanParams& p, hipStream_t stream)
{
    switch (raw) {
    case RAW_HAMMING: return launch_compare_kind<RAW_HAMMING>(p, stream);
    case RAW_PREFIX: return launch_compare_kind<RAW_PREFIX>(p, stream);
    case RAW_POSTFIX: return launch_compare_kind<RAW_POSTFIX>(p, stream);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace rf

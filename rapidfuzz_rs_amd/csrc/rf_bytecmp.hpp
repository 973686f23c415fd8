// rf_bytecmp.hpp -- byte compares over the dwords of a 16-byte chunk, for the scans of rf_compare.hip (hamming, prefix, postfix): a chunk of
// candidate symbols XOR the query's symbols at the same positions is zero exactly in the bytes that match.  Host and device compile the
// same inlines (tests/cpp/bytecmp_check.cpp runs them against byte loops), so this file includes nothing of HIP.
//
// Nothing here decides by a ZERO byte of the payload: the padding behind a candidate is zero and so is the most frequent symbol after
// renaming.  Where a string ends is always a matter of its length -- byte_mask() -- never of its bytes.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RF_BC_HD __host__ __device__ __forceinline__
#else
#define RF_BC_HD inline
#endif

namespace rf {

// bit 7 of every byte of x that is not zero.  Carry-free: (b & 0x7F) + 0x7F is at most 0xFE, so no byte's sum reaches its neighbour.
RF_BC_HD uint32_t nonzero_byte_flags(uint32_t x) { return (((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u; }

// how many of the four bytes of x are not zero
RF_BC_HD uint32_t nonzero_bytes(uint32_t x) { return (uint32_t)__builtin_popcount(nonzero_byte_flags(x)); }

// index (0 = the lowest byte) of the first / last byte of x that is not zero; 4 when x == 0
RF_BC_HD uint32_t first_nonzero_byte(uint32_t x) { return x ? (uint32_t)__builtin_ctz(x) >> 3 : 4u; }
RF_BC_HD uint32_t last_nonzero_byte(uint32_t x) { return x ? 3u - ((uint32_t)__builtin_clz(x) >> 3) : 4u; }

// the bytes of dword k (0..3) of a chunk whose chunk positions 4k .. 4k + 3 lie in [from, to), as 0xFF each; 0 <= from, to <= 16
RF_BC_HD uint32_t byte_mask(uint32_t k, uint32_t from, uint32_t to)
{
    const uint32_t base = 4u * k;
    const uint32_t lo = from > base ? (from - base < 4u ? from - base : 4u) : 0u;  // bytes of the dword below `from`
    const uint32_t hi = to > base ? (to - base < 4u ? to - base : 4u) : 0u;        // bytes of the dword below `to`
    const uint32_t below_hi = hi >= 4u ? 0xFFFFFFFFu : (1u << (8u * hi)) - 1u;
    const uint32_t below_lo = lo >= 4u ? 0xFFFFFFFFu : (1u << (8u * lo)) - 1u;
    return below_hi & ~below_lo;
}
// ... and the tail mask: positions below `rem` (the symbols a string still has in this chunk, 0..16)
RF_BC_HD uint32_t tail_mask(uint32_t k, uint32_t rem) { return byte_mask(k, 0u, rem); }

// the four dwords of a chunk as one compare
struct Chunk4 {
    uint32_t x, y, z, w;
};
RF_BC_HD uint32_t chunk_nonzero_bytes(const Chunk4& c) { return nonzero_bytes(c.x) + nonzero_bytes(c.y) + nonzero_bytes(c.z) + nonzero_bytes(c.w); }
// chunk position (0..15) of the first / last byte that is not zero; 16 when the chunk is all zero
RF_BC_HD uint32_t chunk_first_nonzero(const Chunk4& c)
{
    if (c.x) return first_nonzero_byte(c.x);
    if (c.y) return 4u + first_nonzero_byte(c.y);
    if (c.z) return 8u + first_nonzero_byte(c.z);
    return c.w ? 12u + first_nonzero_byte(c.w) : 16u;
}
RF_BC_HD uint32_t chunk_last_nonzero(const Chunk4& c)
{
    if (c.w) return 12u + last_nonzero_byte(c.w);
    if (c.z) return 8u + last_nonzero_byte(c.z);
    if (c.y) return 4u + last_nonzero_byte(c.y);
    return c.x ? last_nonzero_byte(c.x) : 16u;
}
// only the positions in [from, to) compare: the others read as equal (keep_range) or as different (differ_outside)
RF_BC_HD Chunk4 keep_range(const Chunk4& c, uint32_t from, uint32_t to)
{
    return Chunk4{c.x & byte_mask(0, from, to), c.y & byte_mask(1, from, to), c.z & byte_mask(2, from, to), c.w & byte_mask(3, from, to)};
}
RF_BC_HD Chunk4 differ_outside(const Chunk4& c, uint32_t from, uint32_t to)
{
    return Chunk4{c.x | ~byte_mask(0, from, to), c.y | ~byte_mask(1, from, to), c.z | ~byte_mask(2, from, to), c.w | ~byte_mask(3, from, to)};
}

// dword i of a byte string read at an offset that is no multiple of 4: `lo` holds bytes 4i' .. 4i' + 3, `hi` the four after them, and the
// result starts `shift` (0..3) bytes into `lo` -- two aligned reads and one funnel shift, never an unaligned load
RF_BC_HD uint32_t align_bytes(uint32_t hi, uint32_t lo, uint32_t shift) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8u * shift)); }

}  // namespace rf

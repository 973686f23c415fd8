// rf_take_addr.hpp -- where a candidate's symbols sit in a packed corpus: the INVERSE of the packers (rf_api.hip build_layout, rf_pack.hip,
// rf_pack_ragged.hip), shared by the kernels that read candidates back (rf_take.hip) and the host-only inverse over an rf_host_layout
// (rf_api_take.hip rf_host_layout_candidate).  Host and device compile the same inlines (tests/cpp/take_addr_check.cpp rebuilds every
// candidate of a host layout with nothing but these functions), so this file includes nothing of HIP.
//
//   slot s             tile t = s / 64, lane r = s % 64 (every tile owns 64 slots: exact tiles first, then the one-length views of the mixed blocks)
//   length             uniform_len for a single-length corpus, else tiles[t].len -- NEVER from the bytes: the stored symbol 0 is the most
//                      frequent symbol after renaming and also the padding value
//   payload base       t * take_tile_bytes(uniform_len), or tiles[t].data_off (the views of one mixed block share its offset)
//   byte b             base + ((b / 16) * 64 + r) * 16 + b % 16: chunk k = b / 16 of the 64 lanes is one contiguous 1 KiB row
//   symbol             inv[stored byte], inv = take_inverse_sigma(sigma): the payload stores sigma[c] for candidate byte c
// Every offset is 64-bit: a payload, and what is read back out of it, may exceed 4 GiB.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RF_TA_HD __host__ __device__ __forceinline__
#else
#define RF_TA_HD inline
#endif

namespace rf {

constexpr uint32_t kTakeLanes = 64;  // candidates per tile (= kWave)
constexpr uint32_t kTakeChunk = 16;  // bytes per lane per chunk row (= kChunk)
constexpr uint32_t kTakePad = 0xFFFFFFFFu;  // orig[] of a slot that holds no candidate (= kPad)

RF_TA_HD uint32_t take_chunks(uint32_t len) { return (len + kTakeChunk - 1) / kTakeChunk; }                          // chunk rows of a tile of this length
RF_TA_HD uint64_t take_tile_bytes(uint32_t len) { return (uint64_t)take_chunks(len) * kTakeLanes * kTakeChunk; }    // payload of such a tile
RF_TA_HD uint32_t take_tile_of(uint64_t slot) { return (uint32_t)(slot / kTakeLanes); }
RF_TA_HD uint32_t take_lane_of(uint64_t slot) { return (uint32_t)(slot % kTakeLanes); }
RF_TA_HD uint64_t take_uniform_base(uint32_t tile, uint32_t uniform_len) { return (uint64_t)tile * take_tile_bytes(uniform_len); }
// chunk k of lane r (16 bytes, 16-byte aligned when the base is), and byte b of lane r
RF_TA_HD uint64_t take_chunk_at(uint64_t base, uint32_t lane, uint32_t k) { return base + ((uint64_t)k * kTakeLanes + lane) * kTakeChunk; }
RF_TA_HD uint64_t take_byte_at(uint64_t base, uint32_t lane, uint32_t b) { return take_chunk_at(base, lane, b / kTakeChunk) + b % kTakeChunk; }
// symbols of a candidate of `len` that chunk k holds: 16, fewer in the last one, never past the candidate's end
RF_TA_HD uint32_t take_chunk_fill(uint32_t len, uint32_t k)
{
    const uint64_t from = (uint64_t)k * kTakeChunk;
    return from >= len ? 0u : (len - from < kTakeChunk ? (uint32_t)(len - from) : kTakeChunk);
}
// inv[sigma[c]] = c.  sigma is a permutation of 0..255 (make_sigma); entries a non-permutation leaves unnamed stay 0
RF_TA_HD void take_inverse_sigma(const uint8_t* sigma, uint8_t* inv)
{
    for (uint32_t c = 0; c < 256; ++c) inv[c] = 0;
    for (uint32_t c = 0; c < 256; ++c) inv[sigma[c]] = (uint8_t)c;
}

}  // namespace rf

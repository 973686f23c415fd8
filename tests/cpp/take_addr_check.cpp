// take_addr_check.cpp -- rf_take_addr.hpp alone finds every candidate in a host layout (tests/test_take_addr.py builds and runs this, once plainly and once under
// the host sanitizers).  For each shape: rf_corpus_layout_host packs the input, then every candidate is rebuilt with the header's functions and nothing else --
// slot -> tile / lane, length and base from the tile, byte addresses, the inverse renaming -- and compared with the input byte for byte.  Every payload byte a
// candidate reads is marked: no byte may be read by two candidates (overlap), and every byte nobody read must hold the padding value 0 (gap), with the marks
// adding up to the input's size.
//   take_addr_check            every shape
//   take_addr_check ragged     the ragged shape only (the wrapper runs it under RF_NO_MIXED_TILES=1 in a child process: partial exact tiles)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rfgpu.h"
#include "../../rapidfuzz_rs_amd/csrc/rf_take_addr.hpp"

using namespace rf;

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_state >> 33);
}

struct Input {
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> offsets{0};
    void add(uint32_t len, uint32_t alphabet)
    {
        // a skewed draw over `alphabet` byte values, 0 included: with 256 of them sigma is a full permutation that moves the byte 0 too
        for (uint32_t b = 0; b < len; ++b) bytes.push_back((uint8_t)((rnd() % 3 ? rnd() % 7 * 37 : rnd()) % alphabet));
        offsets.push_back(bytes.size());
    }
    size_t n() const { return offsets.size() - 1; }
};

static int failures = 0;
#define EXPECT(cond, ...)                                  \
    do {                                                   \
        if (!(cond)) {                                     \
            if (++failures <= 20) {                        \
                std::printf("FAIL %s: ", #cond);           \
                std::printf(__VA_ARGS__);                  \
                std::printf("\n");                         \
            }                                              \
        }                                                  \
    } while (0)

static void check_shape(const char* name, const Input& in, int want_identity, bool want_exact_and_mixed)
{
    rf_host_layout l;
    const rf_status st = rf_corpus_layout_host(in.bytes.data(), in.offsets.data(), in.n(), &l);
    EXPECT(st == RF_OK, "%s: rf_corpus_layout_host -> %d", name, (int)st);
    if (st != RF_OK) return;
    EXPECT(l.n == in.n(), "%s: n", name);
    if (want_identity >= 0) EXPECT((int)l.identity == want_identity, "%s: identity = %u", name, l.identity);
    if (want_exact_and_mixed) EXPECT(l.n_exact > 0 && l.n_mixed > 0 && l.n_tiles > l.n_exact, "%s: exact %u mixed %u tiles %u", name, l.n_exact, l.n_mixed, l.n_tiles);
    // candidate -> slot (the identity when the layout says so)
    std::vector<uint64_t> slot_of(in.n(), UINT64_MAX);
    if (l.identity) {
        for (size_t i = 0; i < in.n(); ++i) slot_of[i] = i;
    } else {
        EXPECT(l.n_slots == (uint64_t)l.n_tiles * kTakeLanes, "%s: %llu slots for %u tiles", name, (unsigned long long)l.n_slots, l.n_tiles);
        for (uint64_t s = 0; s < l.n_slots; ++s) {
            const uint32_t o = l.orig[s];
            if (o == kTakePad) continue;
            EXPECT(o < in.n() && slot_of[o] == UINT64_MAX, "%s: slot %llu names candidate %u again", name, (unsigned long long)s, o);
            if (o < in.n()) slot_of[o] = s;
        }
    }
    uint8_t inv[256];
    take_inverse_sigma(l.sigma, inv);
    for (uint32_t c = 0; c < 256; ++c) EXPECT(inv[l.sigma[c]] == c, "%s: sigma is not inverted at %u", name, c);
    std::vector<uint8_t> claimed(l.packed_bytes, 0);
    uint64_t marks = 0;
    for (size_t i = 0; i < in.n(); ++i) {
        const uint64_t s = slot_of[i];
        EXPECT(s != UINT64_MAX, "%s: no slot names candidate %zu", name, i);
        if (s == UINT64_MAX) continue;
        const uint32_t t = take_tile_of(s), r = take_lane_of(s);
        EXPECT(t < l.n_tiles, "%s: tile %u of %u", name, t, l.n_tiles);
        if (t >= l.n_tiles) continue;
        const uint32_t len = l.tile_len[t];
        const uint64_t want_len = in.offsets[i + 1] - in.offsets[i];
        EXPECT(len == want_len, "%s: candidate %zu has length %llu, its tile says %u", name, i, (unsigned long long)want_len, len);
        if (len != want_len) continue;
        const uint64_t base = l.identity ? take_uniform_base(t, len) : l.tile_off[t];
        EXPECT(base == l.tile_off[t], "%s: tile %u sits at %llu, the arithmetic says %llu", name, t, (unsigned long long)l.tile_off[t], (unsigned long long)base);
        uint32_t filled = 0;
        for (uint32_t k = 0; k < take_chunks(len); ++k) filled += take_chunk_fill(len, k);
        EXPECT(filled == len && take_chunk_fill(len, take_chunks(len)) == 0, "%s: the chunks of length %u hold %u symbols", name, len, filled);
        for (uint32_t b = 0; b < len; ++b) {
            const uint64_t x = take_byte_at(base, r, b);
            EXPECT(x < l.packed_bytes, "%s: byte %u of candidate %zu at %llu of %llu", name, b, i, (unsigned long long)x, (unsigned long long)l.packed_bytes);
            if (x >= l.packed_bytes) break;
            EXPECT(x == take_chunk_at(base, r, b / kTakeChunk) + b % kTakeChunk, "%s: chunk and byte addresses disagree", name);
            EXPECT(!claimed[x], "%s: payload byte %llu is read twice", name, (unsigned long long)x);
            claimed[x] = 1;
            ++marks;
            const uint8_t got = inv[l.packed[x]], want = in.bytes[in.offsets[i] + b];
            EXPECT(got == want, "%s: candidate %zu byte %u: %u, input %u", name, i, b, got, want);
        }
    }
    EXPECT(marks == in.bytes.size(), "%s: %llu payload bytes read, input has %zu", name, (unsigned long long)marks, in.bytes.size());
    for (uint64_t x = 0; x < l.packed_bytes; ++x)
        if (!claimed[x]) EXPECT(l.packed[x] == 0, "%s: payload byte %llu = %u belongs to no candidate", name, (unsigned long long)x, l.packed[x]);
    // ... and the library's own host inverse, built on the same header
    std::vector<uint8_t> buf(512);
    for (size_t i = 0; i < in.n(); i += 7) {
        uint32_t len = 0;
        EXPECT(rf_host_layout_candidate(&l, i, buf.data(), buf.size(), &len) == RF_OK, "%s: rf_host_layout_candidate(%zu)", name, i);
        EXPECT(len == in.offsets[i + 1] - in.offsets[i] && !std::memcmp(buf.data(), in.bytes.data() + in.offsets[i], len), "%s: rf_host_layout_candidate(%zu) differs", name, i);
    }
    std::printf("%-28s n %5zu tiles %4u (exact %4u, mixed blocks %3u) identity %u payload %8llu: ok\n", name, in.n(), l.n_tiles, l.n_exact, l.n_mixed, l.identity,
                (unsigned long long)in.bytes.size());
    rf_host_layout_free(&l);
}

static Input ragged_shape()
{
    // 0..64, n = 3001: three empty candidates, whole exact tiles of 20 / 33 / 64 (and leftovers of each), everything else by chance
    Input in;
    std::vector<uint32_t> lens;
    for (int i = 0; i < 3; ++i) lens.push_back(0);
    for (int i = 0; i < 64 + 9; ++i) lens.push_back(20);
    for (int i = 0; i < 128 + 1; ++i) lens.push_back(33);
    for (int i = 0; i < 64; ++i) lens.push_back(64);
    while (lens.size() < 3001) lens.push_back(1 + rnd() % 64);
    for (size_t i = lens.size() - 1; i > 0; --i) std::swap(lens[i], lens[rnd() % (i + 1)]);
    for (uint32_t len : lens) in.add(len, 256);
    return in;
}

int main(int argc, char** argv)
{
    const bool ragged_only = argc > 1 && std::string(argv[1]) == "ragged";
    if (!ragged_only) {
        for (uint32_t len : {1u, 15u, 16u, 17u, 20u, 64u}) {
            Input in;
            for (int i = 0; i < 64 * 3 - 27; ++i) in.add(len, 256);
            check_shape(("single length " + std::to_string(len)).c_str(), in, 1, false);
        }
        Input lng;  // 0..300: 19 chunk rows, mixed blocks sized for their longest lane
        for (int i = 0; i < 200; ++i) lng.add(i == 0 ? 300 : i == 1 ? 0 : rnd() % 301, 256);
        check_shape("lengths 0..300", lng, 0, false);
        Input few;  // few symbols: sigma still a permutation, most of it unused
        for (int i = 0; i < 500; ++i) few.add(rnd() % 40, 5);
        check_shape("five symbols", few, 0, false);
    }
    check_shape(ragged_only ? "ragged 0..64 (as the env says)" : "ragged 0..64", ragged_shape(), 0, !ragged_only);
    std::printf("failures %d\n", failures);
    return failures ? 1 : 0;
}

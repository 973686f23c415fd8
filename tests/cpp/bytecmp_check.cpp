// bytecmp_check.cpp -- rf_bytecmp.hpp (the byte compares of rf_compare.hip: hamming, prefix, postfix) compiled with the host compiler and held to byte
// loops: every pair of bytes in every lane of a dword, every tail length 0..16 and every [from, to) range of a chunk, and the scans of a whole chunk
// (hamming count, first / last mismatch with the boundary masks, the realigned query read) against strings compared symbol by symbol.
// Build: g++ -std=c++17 -I rapidfuzz_rs_amd/csrc tests/cpp/bytecmp_check.cpp (tests/test_bytecmp.py; also under -fsanitize=address,undefined).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rf_bytecmp.hpp"

using namespace rf;

static long mismatches = 0;
static long checks = 0;
#define EXPECT(cond)                                                      \
    do {                                                                  \
        ++checks;                                                         \
        if (!(cond)) {                                                    \
            if (++mismatches <= 10) std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond); \
        }                                                                 \
    } while (0)

static uint32_t byte_of(uint32_t x, int i) { return (x >> (8 * i)) & 0xFFu; }

static Chunk4 chunk_of(const uint8_t* b)
{
    Chunk4 c;
    std::memcpy(&c.x, b, 4), std::memcpy(&c.y, b + 4, 4), std::memcpy(&c.z, b + 8, 4), std::memcpy(&c.w, b + 12, 4);
    return c;
}

int main()
{
    // ---- every pair of bytes (a, b) in every lane of a dword, the other lanes zero or all different: a ^ b is non-zero exactly when a != b
    for (int lane = 0; lane < 4; ++lane)
        for (uint32_t a = 0; a < 256; ++a)
            for (uint32_t b = 0; b < 256; ++b)
                for (uint32_t others : {0x00000000u, 0xFFFFFFFFu, 0x01800180u, 0x7F7F7F7Fu}) {
                    const uint32_t x = (others & ~(0xFFu << (8 * lane))) | ((a ^ b) << (8 * lane));
                    uint32_t count = 0, first = 4, last = 4;
                    for (int i = 0; i < 4; ++i)
                        if (byte_of(x, i)) {
                            ++count;
                            if (first == 4) first = (uint32_t)i;
                            last = (uint32_t)i;
                        }
                    EXPECT(nonzero_bytes(x) == count);
                    EXPECT(first_nonzero_byte(x) == first);
                    EXPECT(last_nonzero_byte(x) == last);
                    uint32_t flags = 0;
                    for (int i = 0; i < 4; ++i)
                        if (byte_of(x, i)) flags |= 0x80u << (8 * i);
                    EXPECT(nonzero_byte_flags(x) == flags);
                }
    // ---- the masks: every [from, to) of a chunk, every dword; the tail lengths 0..16
    for (uint32_t from = 0; from <= 16; ++from)
        for (uint32_t to = 0; to <= 16; ++to)
            for (uint32_t k = 0; k < 4; ++k) {
                uint32_t exp = 0;
                for (uint32_t i = 0; i < 4; ++i) {
                    const uint32_t pos = 4 * k + i;
                    if (pos >= from && pos < to) exp |= 0xFFu << (8 * i);
                }
                EXPECT(byte_mask(k, from, to) == exp);
                if (from == 0) EXPECT(tail_mask(k, to) == exp);
            }
    // ---- whole chunks: two 16-symbol strings over a small alphabet that includes the symbol 0 (the padding's value), a tail length 0..16
    uint32_t seed = 12345;
    auto rnd = [&]() { return seed = seed * 1664525u + 1013904223u, seed >> 16; };
    for (int round = 0; round < 20000; ++round) {
        uint8_t a[16], b[16], d[16];
        const uint32_t sym = 1 + rnd() % 4;
        for (int i = 0; i < 16; ++i) a[i] = (uint8_t)(rnd() % sym), b[i] = (rnd() % 4) ? a[i] : (uint8_t)(rnd() % sym);
        for (int i = 0; i < 16; ++i) d[i] = a[i] ^ b[i];
        const Chunk4 x = chunk_of(d);
        for (uint32_t rem = 0; rem <= 16; ++rem) {
            uint32_t ham = 0, pre = 0;
            for (uint32_t i = 0; i < rem; ++i) ham += a[i] != b[i];
            while (pre < rem && a[pre] == b[pre]) ++pre;
            EXPECT(chunk_nonzero_bytes(keep_range(x, 0, rem)) == ham);
            const uint32_t first = chunk_first_nonzero(differ_outside(x, 0, rem));  // position `rem` always differs
            EXPECT((rem == 16 && pre == 16) ? first == 16 : first == pre);
            // the suffix walk over the positions [from, rem): from `rem` on the chunk reads as equal, below `from` as different
            for (uint32_t from = 0; from <= rem; from += (rem > 8 ? 3 : 1)) {
                uint32_t post = 0;
                while (post < rem - from && a[rem - 1 - post] == b[rem - 1 - post]) ++post;
                const uint32_t last = chunk_last_nonzero(differ_outside(keep_range(x, 0, rem), from, 16));
                const uint32_t matched = last == 16 ? rem : rem - 1 - last;
                EXPECT(matched == post);
                EXPECT((last == 16) == (from == 0 && post == rem));
            }
        }
    }
    // ---- the realigned read: 16 bytes of a string from any byte offset = five aligned dwords and four funnel shifts
    {
        std::vector<uint8_t> s(64);
        for (size_t i = 0; i < s.size(); ++i) s[i] = (uint8_t)(i * 7 + 1);
        std::vector<uint32_t> w(s.size() / 4);
        std::memcpy(w.data(), s.data(), s.size());
        for (uint32_t at = 0; at + 20 <= s.size(); ++at) {
            const uint32_t i = at >> 2, sh = at & 3;
            const Chunk4 got{align_bytes(w[i + 1], w[i], sh), align_bytes(w[i + 2], w[i + 1], sh), align_bytes(w[i + 3], w[i + 2], sh), align_bytes(w[i + 4], w[i + 3], sh)};
            const Chunk4 exp = chunk_of(s.data() + at);
            EXPECT(got.x == exp.x && got.y == exp.y && got.z == exp.z && got.w == exp.w);
        }
    }
    std::printf("checks %ld mismatches %ld\n", checks, mismatches);
    return mismatches ? 1 : 0;
}

// The tile / lane list buffer's layout (rapidfuzz_rs_amd/csrc/rf_list_layout.hpp) against a second statement of it: the offsets as the launchers and kernels
// spelled them by hand before the struct existed.  Host only (tests/test_list_layout.py builds it with -fsanitize=address,undefined).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "rf_list_layout.hpp"

using rf::ListLayout;

static int failures = 0;
#define CHECK(cond)                                                                                         \
    do {                                                                                                    \
        if (!(cond)) {                                                                                      \
            if (++failures <= 20) std::fprintf(stderr, "line %d: %s  (n_tiles=%llu G=%u kind=%d)\n", __LINE__, #cond, (unsigned long long)n_tiles, G, kind); \
        }                                                                                                   \
    } while (0)

int main()
{
    const uint64_t tile_counts[] = {1, 2, 63, 64, 65, 16383, 16384, 16385, 1u << 20, 15625000};
    const uint32_t grids[] = {4, 256, 4096, 16384};
    unsigned long checked = 0;
    for (const uint64_t n_tiles : tile_counts) {
        const size_t words = ListLayout::words_needed(n_tiles);
        int kind = -1;
        uint32_t G = 0;
        CHECK(words >= 9 * n_tiles + 12 * 16384 + 64);  // never fewer words than the buffer has always had
        CHECK(ListLayout::words_bound(n_tiles) <= words);
        CHECK(ListLayout::trailer_at(words) == words - 4);
        for (const uint32_t G_ : grids) {
            G = G_;
            const size_t g = G;
            // ---- the small-band launches (lanes form): cap = ceil(n / G)
            {
                kind = 1;
                const uint32_t n = (uint32_t)n_tiles, cap = (n + G - 1) / G;
                const ListLayout L = ListLayout::band(n, G);
                CHECK(L.cap == cap && L.G == G);
                CHECK(L.count_at() == 0 && ListLayout::kLaneSurvivorsAt == 1);
                CHECK(L.wave_counts_at() == 4);
                CHECK(L.segment_at(0) == 4 + 2 * g);
                for (const uint32_t s : {0u, 1u, G / 2, G - 1}) CHECK(L.segment_at(s) == 4 + 2 * g + 4 * (size_t)s * cap);
                CHECK(L.packed_at() == 4 + 2 * g + 4 * g * cap);
                CHECK(L.first_at() == 4 + 2 * g + 4 * g * cap + 4 * ((size_t)n + 2));
                // in order and disjoint: counts | per-wavefront pairs | segments | packed entries (every tile listed at most once) | first[] (a word per dense tile) | trailer
                CHECK(L.count_at() + 2 <= L.wave_counts_at());
                CHECK(L.wave_counts_at() + 2 * g <= L.segment_at(0));
                CHECK(L.segment_at(G - 1) + 4 * (size_t)cap <= L.packed_at());
                CHECK(L.packed_at() + 4 * (size_t)n <= L.first_at());
                CHECK(L.first_at() + n <= L.end());
                CHECK(L.end() <= ListLayout::trailer_at(words));
                CHECK(L.fits(words));
                CHECK(!L.fits(L.end() + 3));  // no room for the trailer
                checked++;
            }
            // ---- the head filter (both forms): a wavefront per PAIR of tiles, cap = 2 * ceil(pairs / G)
            for (kind = 0; kind <= 1; ++kind) {
                const uint32_t pairs = ((uint32_t)n_tiles + 1) / 2, cap = 2 * ((pairs + G - 1) / G);
                const ListLayout L = ListLayout::head(kind ? ListLayout::kLanes : ListLayout::kTiles, pairs, G);
                CHECK(L.cap == cap && L.G == G && L.count_at() == 0);
                if (kind == 0) {
                    CHECK(L.wave_counts_at() == 1);
                    for (const uint32_t s : {0u, 1u, G / 2, G - 1}) CHECK(L.segment_at(s) == 1 + 2 * g + (size_t)s * cap);
                    CHECK(L.packed_at() == 1 + 2 * g + g * cap);
                    CHECK(L.count_at() + 1 <= L.wave_counts_at());
                    CHECK(L.wave_counts_at() + g <= L.segment_at(0));  // (G counts; the G words behind them are unused)
                    CHECK(L.segment_at(G - 1) + cap <= L.packed_at());
                    CHECK(L.packed_at() + 2 * (size_t)pairs <= L.end());
                } else {
                    CHECK(L.wave_counts_at() == 4);
                    for (const uint32_t s : {0u, 1u, G / 2, G - 1}) CHECK(L.segment_at(s) == 4 + 2 * g + 4 * (size_t)s * cap);
                    CHECK(L.packed_at() == 4 + 2 * g + 4 * g * cap);
                    CHECK(L.first_at() == 4 + 2 * g + 4 * g * cap + 4 * (size_t)(2 * pairs + 2));
                    CHECK(L.count_at() + 2 <= L.wave_counts_at());
                    CHECK(L.wave_counts_at() + 2 * g <= L.segment_at(0));
                    CHECK(L.segment_at(G - 1) + 4 * (size_t)cap <= L.packed_at());
                    CHECK(L.packed_at() + 4 * (size_t)(2 * pairs) <= L.first_at());
                    CHECK(L.first_at() + 2 * (size_t)pairs <= L.end());
                }
                CHECK(L.end() <= ListLayout::trailer_at(words));
                CHECK(L.fits(words));
                checked++;
            }
        }
        // more wavefronts than the buffer is sized for: never fits, whatever the room
        G = 16388;
        kind = 1;
        CHECK(!ListLayout::band((uint32_t)n_tiles, G).fits(~(size_t)0));
        CHECK(!ListLayout::head(ListLayout::kTiles, 1, G).fits(~(size_t)0));
    }
    if (failures) {
        std::fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    std::printf("list layout ok: %lu shapes\n", checked);
    return 0;
}

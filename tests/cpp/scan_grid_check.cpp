// The grid arithmetic behind tests/multitile_rowdp_check.py, on the host and without the kernels under test: scan_grid() of rf_scan.hip restated as
// literals, min(ceil(tiles / 4), CUs x per_cu), and the grid-stride deal `for (t = first; t < n_tiles; t += stride)` walked wavefront by wavefront.
// argv: triples "CUs waves candidates" -- the corpus sizes the checker derives (tests/test_scan_grid.py passes them).  For each triple:
//   * at 1 workgroup per CU every wavefront below the grid's wavefront count owns at least 4 tiles;
//   * at the default of 32 per CU a launch of 4-wavefront workgroups gives every wavefront exactly one (the gap the checker closes); launches of fewer
//     wavefronts per workgroup (the LDS-row kernels of long queries) keep the grid of ceil(tiles / 4) workgroups, so theirs own floor(4 / waves) ..
//     ceil(4 / waves) tiles on the default grid already: 4 at one wavefront per workgroup, 2 at two.
// `candidates` stands for the tiles of the LAUNCH, ceil(candidates / 64): a single-length corpus, or that part of a ragged corpus which one launch walks (the
// checker counts it from the candidate lengths: whole tiles per length).
// Host only (built with -fsanitize=address,undefined).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

static uint32_t scan_grid(uint32_t n_tiles, uint32_t cus, uint32_t per_cu) { return std::min<uint32_t>((n_tiles + 3) / 4, cus * per_cu); }

// tiles per wavefront of the deal: wavefront w of `grid * waves` takes tiles w, w + grid * waves, ...
static void deal(uint32_t n_tiles, uint32_t grid, uint32_t waves, uint32_t* fewest, uint32_t* most)
{
    const uint32_t stride = grid * waves;
    std::vector<uint32_t> owned(stride, 0);
    for (uint32_t block = 0; block < grid; ++block)
        for (uint32_t wave = 0; wave < waves; ++wave)
            for (uint32_t t = block * waves + wave; t < n_tiles; t += stride) ++owned[block * waves + wave];
    *fewest = *std::min_element(owned.begin(), owned.end());
    *most = *std::max_element(owned.begin(), owned.end());
}

int main(int argc, char** argv)
{
    if (argc < 4 || (argc - 1) % 3 != 0) {
        std::fprintf(stderr, "usage: scan_grid_check CUs waves candidates [CUs waves candidates ...]\n");
        return 2;
    }
    int failures = 0, shapes = 0;
    for (int a = 1; a + 2 < argc; a += 3, ++shapes) {
        const uint32_t cus = (uint32_t)std::strtoul(argv[a], nullptr, 10), waves = (uint32_t)std::strtoul(argv[a + 1], nullptr, 10);
        const uint64_t n = std::strtoull(argv[a + 2], nullptr, 10);
        if (cus == 0 || waves == 0 || waves > 4 || n == 0 || n > (1ull << 31)) {
            std::fprintf(stderr, "bad triple %s %s %s\n", argv[a], argv[a + 1], argv[a + 2]);
            return 2;
        }
        const uint32_t n_tiles = (uint32_t)((n + 63) / 64);
        uint32_t fewest = 0, most = 0;
        deal(n_tiles, std::max(1u, scan_grid(n_tiles, cus, 1)), waves, &fewest, &most);
        if (fewest < 4) {
            std::fprintf(stderr, "CUs=%u waves=%u n=%llu: a wavefront owns %u tiles at 1 workgroup per CU\n", cus, waves, (unsigned long long)n, fewest);
            ++failures;
        }
        deal(n_tiles, std::max(1u, scan_grid(n_tiles, cus, 32)), waves, &fewest, &most);
        if (fewest != 4 / waves || most != (4 + waves - 1) / waves) {
            std::fprintf(stderr, "CUs=%u waves=%u n=%llu: %u..%u tiles per wavefront at 32 workgroups per CU\n", cus, waves, (unsigned long long)n, fewest, most);
            ++failures;
        }
    }
    if (failures) return 1;
    std::printf("scan grid ok: %d shapes\n", shapes);
    return 0;
}

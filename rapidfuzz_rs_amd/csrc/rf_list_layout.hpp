// rf_list_layout.hpp -- THE layout of a stream's tile / lane list buffer (rf_host.hpp rf_corpus::TileList), in 32-bit words.  Plain arithmetic, no HIP calls: the host
// side, the kernels and a host-compiled test (tests/test_list_layout.py, which restates every offset as a literal) all include this one description.
//
// A first pass (rf_scan.hip head_filter_kernel, rf_band.hip band_defer_kernel / band_list_kernel) of G wavefronts lists what it leaves in ITS OWN segment of `cap`
// entries (no atomics); a pack kernel (rf_scan.hip) copies the segments behind one another; a second pass walks the packed list.
//   tiles:  [0] packed count                     | G per-wavefront counts | G words unused | G segments of `cap` tiles            | the packed tiles
//   lanes:  [0] packed entries [1] survivors [2,3] | G (tiles, lanes) count pairs           | G segments of `cap` 16-byte entries | the packed entries | first[]
// (a lane entry: tile, lane mask lo / hi, survivors in front of it; first[j] = the packed entry that holds survivor 64 j: rf_sparse.hip).  The LAST kTrailerWords
// words of the buffer belong to no list: word 0 of them is launch_band's count of hand-over candidates (ScanParams::band_defer_seen), zero between launches.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RF_LIST_HD __host__ __device__
#else
#define RF_LIST_HD
#endif

namespace rf {

struct ListLayout {
    enum Kind : uint32_t { kTiles = 0, kLanes = 1 };
    static constexpr uint32_t kMaxSegments = 16384;  // the most wavefronts a listing launch may have (words_needed() is sized for it)
    static constexpr size_t kTrailerWords = 4;
    static constexpr size_t kLaneSurvivorsAt = 1;  // lanes form: the word behind the packed count

    Kind kind;
    uint32_t G;      // segments = wavefronts of the listing launch
    uint32_t cap;    // entries per segment: the tiles one wavefront can list
    size_t n_tiles;  // tiles the launch walks: what the packed list (+ 2 entries of slack) and first[] have room for

    // the launchers' own shapes: rf_band.hip lists <= ceil(n / G) tiles per wavefront, head_filter_kernel two per PAIR of tiles
    RF_LIST_HD static ListLayout band(uint32_t n_tiles, uint32_t G) { return ListLayout{kLanes, G, (n_tiles + G - 1) / G, n_tiles}; }
    RF_LIST_HD static ListLayout head(Kind kind, uint32_t pairs, uint32_t G) { return ListLayout{kind, G, 2 * ((pairs + G - 1) / G), 2 * (size_t)pairs}; }
    // ... and what a kernel knows: enough for everything but first_at()
    RF_LIST_HD static ListLayout of_launch(Kind kind, uint32_t G, uint32_t cap) { return ListLayout{kind, G, cap, 0}; }

    RF_LIST_HD size_t entry_words() const { return kind == kLanes ? 4 : 1; }
    RF_LIST_HD size_t count_at() const { return 0; }                              // tiles: the packed count; lanes: packed entries, then survivors
    RF_LIST_HD uint32_t wave_counts_at() const { return kind == kLanes ? 4 : 1; }  // tiles: G counts, G unused; lanes: G (tiles, lanes) pairs
    RF_LIST_HD size_t segment_at(uint32_t s) const { return wave_counts_at() + 2 * (size_t)G + entry_words() * ((size_t)s * cap); }
    RF_LIST_HD size_t packed_at() const { return segment_at(G); }
    // (for the kernels: the same place reached by the pointer steps their code has always taken, so that the compiler emits what it always has)
    RF_LIST_HD uint32_t* segment(uint32_t* buf, uint32_t s) const
    {
        uint32_t* segments = buf + wave_counts_at() + 2 * (size_t)G;
        struct Entry4 { uint32_t w[4]; };  // a lane entry
        return kind == kLanes ? reinterpret_cast<uint32_t*>(reinterpret_cast<Entry4*>(segments) + (size_t)s * cap) : segments + (size_t)s * cap;
    }
    RF_LIST_HD size_t first_at() const { return packed_at() + entry_words() * (n_tiles + 2); }  // (lanes only)
    RF_LIST_HD size_t end() const { return kind == kLanes ? first_at() + n_tiles + 1 : packed_at() + n_tiles; }
    RF_LIST_HD static size_t trailer_at(size_t words) { return words - kTrailerWords; }
    // may a launch of this shape write its lists into a buffer of `words` words?  Every launcher asks before it launches.
    RF_LIST_HD bool fits(size_t words) const { return G >= 1 && G <= kMaxSegments && words >= kTrailerWords && end() <= trailer_at(words); }

    // What TileList allocates for a corpus of n_tiles tiles.  The bound over both kinds and every G <= kMaxSegments: G * cap <= n + G - 1 (band) or n + 2 G - 2 (head,
    // n = 2 * pairs <= n_tiles + 1), so end() <= 9 n + 10 G + 5 <= 9 n_tiles + 10 * 16384 + 14, + the trailer.  The allocation adds the slack that makes it the
    // 9 n_tiles + 12 * 16384 + 64 words the buffer has always had, so rf_corpus_device_bytes() stays what it was.
    static constexpr size_t words_bound(size_t n_tiles) { return 9 * n_tiles + 10 * (size_t)kMaxSegments + 14 + kTrailerWords; }
    static constexpr size_t kSlackWords = 2 * (size_t)kMaxSegments + 46;
    static constexpr size_t words_needed(size_t n_tiles) { return words_bound(n_tiles) + kSlackWords; }
};

}  // namespace rf

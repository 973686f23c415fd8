// rf_host.hpp -- what the translation units of the C ABI share (round 4: rf_api.hip was one 3 500-line file):
//   rf_api.hip        error text, comparators, lowering of u32 queries, corpus packing and layout, probes
//   rf_api_scan.hip   plan(): Args x metric x op -> kernel parameters; rf_many_* / rf_one_* / rf_many_multi_* and what they launch
//   rf_api_topk.hip   top-k: in-scan lists, selection, 8-byte keys and 16-byte entries, the RCCL exchange
//   rf_api_files.hip  corpus files (save / load / validate) and streamed scans
//   rf_api_topk_multi.hip, rf_api_filter_multi.hip  the fused multi-query calls; their one planner (MultiPlan, plan_multi) is declared below
// Host code only; nothing here is visible outside librfgpu.so.
#pragma once
#include <dlfcn.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <list>
#include <cstdio>
#include <atomic>
#include <unordered_map>
#include <unordered_set>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <thread>
#include <utility>
#include <vector>

#include "rf_internal.hpp"
#include "rf_multi_group.hpp"
#include "rf_norm_key.hpp"

namespace rf {


#define RF_HIP(expr)                                                                                   \
    do {                                                                                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess) {                                                                        \
            set_error(std::string(#expr) + ": " + hipGetErrorString(_e));                              \
            return _e == hipErrorOutOfMemory ? RF_ERR_OOM : RF_ERR_HIP;                                \
        }                                                                                              \
    } while (0)

struct DeviceGuard {
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int dev)
    {
        if (dev < 0) return;  // nothing to select (e.g. an empty corpus: the call never touches a device)
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard()
    {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// What a corpus keeps per stream that scans it (rf_corpus: top-k scratch, gather temporaries, tile lists): at most `cap` entries
// {stream, done event, T}, most recently used first.  acquire() returns a Lease that holds the cache's mutex until it is released
// or destroyed (host threads sharing a stream must not interleave their uses of one buffer), with
//   - the stream's own entry, after a hipStreamWaitEvent on its `done` (a new stream may have been handed a destroyed stream's
//     handle value while that stream's work is in flight: ADVICE r4), else
//   - a new entry filled by the caller's make(T&) while there is room (a failure drops it, *err says why), else
//   - take_over: the least recently used entry once its `done` has completed (the event, never the old stream handle: that
//     stream may be gone); otherwise no entry, and the caller allocates for the call.
// Releasing the lease records `done` behind what was enqueued under it -- on every exit, error returns included.  T is
// default-constructible, frees its buffers in its destructor and reports their bytes().
// Lock order where one call holds several leases: top-k -> gather -> tile list (the via-scores top-k runs run_many under its lease).
struct NoCopy {
    NoCopy() = default;
    NoCopy(const NoCopy&) = delete;
    NoCopy& operator=(const NoCopy&) = delete;
};
template <class T>
class StreamCache {
    struct Entry : NoCopy {
        hipStream_t stream;
        hipEvent_t done;
        T value;
        Entry(hipStream_t s, hipEvent_t d) : stream(s), done(d) {}
        ~Entry() { (void)hipEventDestroy(done); }
    };
    mutable std::mutex mu_;
    std::list<Entry> entries_;  // (stable addresses)
    const size_t cap_;
    const bool take_over_;

public:
    StreamCache(size_t cap, bool take_over) : cap_(cap), take_over_(take_over) {}
    class Lease {
        friend class StreamCache;
        std::unique_lock<std::mutex> lock_;
        std::list<Entry>* entries_ = nullptr;
        Entry* e_ = nullptr;  // nullptr: no entry (the lock may still be held)

    public:
        Lease() = default;
        Lease(Lease&& o) noexcept : lock_(std::move(o.lock_)), entries_(o.entries_), e_(std::exchange(o.e_, nullptr)) {}
        Lease& operator=(Lease&& o) noexcept
        {
            release();
            lock_ = std::move(o.lock_), entries_ = o.entries_, e_ = std::exchange(o.e_, nullptr);
            return *this;
        }
        ~Lease() { release(); }
        explicit operator bool() const { return e_ != nullptr; }
        T* operator->() const { return &e_->value; }
        void release()  // everything that uses the entry has been enqueued
        {
            if (e_ && hipEventRecord(e_->done, e_->stream) != hipSuccess) (void)hipGetLastError();
            e_ = nullptr;
            if (lock_.owns_lock()) lock_.unlock();
        }
        void discard()  // the entry may be left half-armed: free it once its stream's work is done (the next call starts from a fresh one)
        {
            if (e_) {
                (void)hipStreamSynchronize(e_->stream);
                entries_->pop_front();  // (the leased entry: acquire() put it in front, and the lock has been held since)
                e_ = nullptr;
            }
            release();
        }
    };
    template <class Make>
    Lease acquire(hipStream_t st, Make&& make, hipError_t* err = nullptr)
    {
        Lease l;
        l.lock_ = std::unique_lock<std::mutex>(mu_);
        l.entries_ = &entries_;
        if (err) *err = hipSuccess;
        for (auto it = entries_.begin(); it != entries_.end(); ++it)
            if (it->stream == st) {
                entries_.splice(entries_.begin(), entries_, it);
                if (hipStreamWaitEvent(st, it->done, 0) != hipSuccess) (void)hipGetLastError();
                l.e_ = &*it;
                return l;
            }
        if (entries_.size() < cap_) {
            hipEvent_t done = nullptr;
            hipError_t e = hipEventCreateWithFlags(&done, hipEventDisableTiming);
            if (e == hipSuccess) {
                entries_.emplace_front(st, done);
                e = make(entries_.front().value);
                if (e == hipSuccess) l.e_ = &entries_.front();
                else entries_.pop_front();
            }
            if (e != hipSuccess) (void)hipGetLastError();
            if (err) *err = e;
        } else if (take_over_) {
            entries_.splice(entries_.begin(), entries_, std::prev(entries_.end()));
            (void)hipEventSynchronize(entries_.front().done);
            entries_.front().stream = st;
            l.e_ = &entries_.front();
        }
        return l;
    }
    uint64_t bytes() const
    {
        std::lock_guard<std::mutex> lock(mu_);
        uint64_t b = 0;
        for (const Entry& e : entries_) b += e.value.bytes();
        return b;
    }
};
// a device buffer that grows in place (hipFree synchronizes with the work that used the smaller one)
struct DeviceBuf : NoCopy {
    void* ptr = nullptr;
    size_t cap = 0;  // bytes
    DeviceBuf() = default;
    DeviceBuf(DeviceBuf&& o) noexcept : ptr(std::exchange(o.ptr, nullptr)), cap(std::exchange(o.cap, 0)) {}
    DeviceBuf& operator=(DeviceBuf&& o) noexcept  // (what was held here goes to `o`, which frees it)
    {
        std::swap(ptr, o.ptr), std::swap(cap, o.cap);
        return *this;
    }
    ~DeviceBuf()
    {
        if (ptr) (void)hipFree(ptr);
    }
    template <class T>
    T* as() const { return static_cast<T*>(ptr); }
    hipError_t reserve(size_t bytes)
    {
        if (cap >= bytes) return hipSuccess;
        void* bigger = nullptr;
        const hipError_t e = hipMalloc(&bigger, bytes);
        if (e != hipSuccess) return e;
        if (ptr) (void)hipFree(ptr);
        ptr = bigger, cap = bytes;
        return hipSuccess;
    }
    uint64_t bytes() const { return cap; }
};

}  // namespace rf

using namespace rf;

struct rf_comparator {
    rf_metric metric;
    std::vector<uint8_t> s1;
    std::vector<uint64_t> pm;  // 256 x words, row-major [c * words + w]; words = max(1, block_count)
    size_t block_count = 0;
    size_t words = 1;
    mutable std::mutex mu;
    mutable std::map<int, uint64_t*> d_pm;  // lazily uploaded per device
    // u32 ("char") queries: the symbols, and one byte-level comparator per wide corpus searched (see resolve())
    bool wide = false;
    std::vector<uint32_t> s1w;
    // (shared_ptr: a call keeps the lowered comparator it runs on alive even if another host thread's call evicts it from
    // this bounded cache meanwhile -- handles may be shared between threads)
    mutable std::map<uint64_t, std::shared_ptr<rf_comparator>> lowered;
};

struct rf_corpus {
    int device = 0;
    size_t n = 0;
    uint64_t payload_bytes = 0;
    uint64_t device_bytes = 0;
    uint64_t data_bytes = 0;     // packed tile payloads + the tail pad chunk row
    bool borrowed = false;       // a view (stream segment, translated image): owns none of its device buffers
    bool no_prefill = false;     // stream segments: the driver pre-fills the whole result vector once
    uint8_t* d_data = nullptr;
    TileDesc* d_tiles = nullptr;
    TileDesc* d_tiles_by_origin = nullptr;  // the same descriptors with the non-empty exact tiles ordered by their first candidate's original index (tiles_by_origin())
    uint32_t* d_orig = nullptr;  // nullptr = identity (single length bucket, original order)
    size_t n_slots = 0;          // entries of d_orig: 64 per tile (exact tiles, then the views)
    uint32_t n_tiles = 0;        // exact tiles, then the virtual (one-length) views of the mixed section
    uint32_t n_exact = 0;        // tiles [0, n_exact) are exact-length tiles; [n_exact, n_tiles) virtual views (HostLayout)
    bool exact_dense = false;    // no padding lane in tiles [0, n_exact) (false under RF_NO_MIXED_TILES when a length's count is not a multiple of 64: its last tile is partial)
    // the mixed section as the Levenshtein / LCS / OSA scans see it: one tile of 64 leftovers with per-lane lengths
    uint32_t n_mixed = 0;
    MixedDesc* d_mixed = nullptr;
    uint32_t* d_mixed_len = nullptr;   // 64 per mixed tile
    uint32_t* d_mixed_orig = nullptr;  // 64 per mixed tile, kPad = no candidate
    std::vector<MixedDesc> mixed;      // host copy (length windows of cutoff runs)
    uint32_t max_len = 0;
    bool uniform = false;        // single length bucket: no descriptors, tile t at t * tile_bytes(uniform_len)
    uint32_t uniform_len = 0;
    std::vector<uint32_t> lengths;  // the distinct candidate lengths (host copy, ascending)
    std::vector<uint32_t> length_first_tile;  // first tile of each distinct length
    uint8_t sigma[256];           // symbol renaming: the packed corpus stores sigma[c] for candidate byte c
    float sym_freq[256] = {0};    // relative frequency of candidate byte c (from the histogram sigma is made of; all zero = unknown)
    uint8_t* d_sigma = nullptr;   // device copy
    // The structures a call builds on first use (rf_api_scan.hip corpus_*), guarded by scratch_mu.  Each builder fills a local owner,
    // synchronizes its stream and only then publishes it here by move, under the lock: other streams see complete structures or none.
    struct GatherMaps {  // large ragged corpora return their results through a slot-ordered temporary + one gather (rf_pack.hip); published together
        DeviceBuf slot_ident;    // slot -> slot, kPad on padding lanes (stands in for d_orig in such a launch)
        DeviceBuf slot_of;       // candidate -> its slot (when there is no window table)
        DeviceBuf window_table;  // the coalesced gather's table (rf_pack.hip window_table_kernel): rows x runs
        DeviceBuf slot_off16;    // slot -> original index mod kGatherOff16Mod (0xFFFF: padding): what the window gather reads instead of d_orig (optional)
        uint32_t runs = 0, rows = 0;
        uint64_t bytes() const { return slot_ident.bytes() + slot_of.bytes() + window_table.bytes() + slot_off16.bytes(); }
    };
    struct Accel : NoCopy {
        DeviceBuf heads8;  // head plane: the first 8 symbols of every candidate (small-cutoff scans)
        DeviceBuf heads6;  // the same at 6 bits per symbol (single-length corpora of < 64 distinct symbols; ScanParams::heads6); tried once
        DeviceBuf data6;   // the payload at 6 bits per symbol (the same corpora; ScanParams::data6); tried once
        DeviceBuf len_of;  // candidate -> its length (original order): the normalizing pass of run_many's two-step path
        GatherMaps gather;
        DeviceBuf take_slot_of;  // candidate -> its slot, for rf_corpus_take / rf_corpus_lengths by index on a length-bucketed corpus (rf_api_take.hip); only while
                                 // gather.slot_of is not there: the gather path's builder takes this buffer over instead of making a second copy
        bool heads6_tried = false, data6_tried = false;
        uint32_t max_stored_sym = 0xFFFFFFFFu;  // largest stored symbol of the payload, exact; 0xFFFFFFFF = not computed yet (corpus_max_stored_symbol)
        uint64_t bytes() const { return heads8.bytes() + heads6.bytes() + data6.bytes() + len_of.bytes() + gather.bytes() + take_slot_of.bytes(); }
    };
    mutable Accel accel;
    mutable std::mutex scratch_mu;  // guards `accel` and d_sigma_identity (the caches below have their own)
    // Per-stream buffers (StreamCache), at most 8 top-k scratches, 4 gather temporaries and 4 tile lists.  The top-k scratch: [64 way
    // segments of candidate keys | root table 64 x 64 keys | bound (u64, own line) | control block 65 x 128 B], room for every workgroup
    // of the largest grid any top-k launch uses to publish a full 64-entry list.  The kernels leave bound / counters re-armed, so a
    // top-k call is two launches (one under a tight cutoff) that hand state to each other through it and no allocation or memset
    // (topk_core()); + the score vector of the scan + one-pass top-k (rf_api_topk.hip).
    struct TopkScratch : NoCopy {
        uint64_t *cand = nullptr, *root = nullptr, *bound = nullptr;  // (cand: the base of the allocation)
        uint32_t* ctl = nullptr;
        uint32_t seg_cap = 0;
        size_t alloc = 0;  // bytes at cand
        DeviceBuf scores;
        ~TopkScratch()
        {
            if (cand) (void)hipFree(cand);
        }
        hipError_t make(uint32_t n_tiles, hipStream_t st)
        {
            const size_t ways = 64, per_way = ((size_t)scan_grid_full(n_tiles) + ways - 1) / ways;
            seg_cap = (uint32_t)(per_way * kWave);
            const size_t cand_bytes = ways * seg_cap * sizeof(uint64_t), root_bytes = ways * kWave * sizeof(uint64_t), ctl_bytes = 65 * 128;
            hipError_t e = hipMalloc((void**)&cand, cand_bytes + root_bytes + 128 + ctl_bytes);
            if (e != hipSuccess) return e;
            alloc = cand_bytes + root_bytes + 128 + ctl_bytes;
            uint8_t* mem = reinterpret_cast<uint8_t*>(cand);
            root = reinterpret_cast<uint64_t*>(mem + cand_bytes);
            bound = reinterpret_cast<uint64_t*>(mem + cand_bytes + root_bytes);
            ctl = reinterpret_cast<uint32_t*>(mem + cand_bytes + root_bytes + 128);
            e = hipMemsetAsync(bound, 0xFF, sizeof(uint64_t), st);
            return e == hipSuccess ? hipMemsetAsync(ctl, 0, ctl_bytes, st) : e;
        }
        uint64_t bytes() const { return alloc + scores.bytes(); }
    };
    // The gather path's slot-ordered temporary (run_many), grown when a call needs f64 where u32 was kept: a stream-ordered
    // hipMallocAsync / hipFreeAsync pair per call made the SUBMISSION of such a step wait for the previous step (measured: 560 us per
    // call to submit a 575 us step; 11 us with the buffer kept).
    using GatherTmp = DeviceBuf;
    // head_filter_kernel's tile list (rf_scan.hip), the lane lists and the small-band hand-over's (rf_band.hip): ListLayout (rf_list_layout.hpp) describes the
    // buffer, sizes it for every launch shape, and keeps its trailer (launch_band's count of hand-over candidates, zero between launches).
    struct TileList : NoCopy {
        uint32_t* ptr = nullptr;
        size_t words = 0;
        volatile uint32_t* band_report = nullptr;  // pinned, 64 bytes: what this stream's last hand-over launch of the small-band scan listed (rf_band.hip
                                                   // band_sparse_kernel writes it; run_many reads it, without waiting, to choose the next launch's form)
        uint32_t band_plain_calls = 0;             // launches since that choice last fell on the plain kernel
        ~TileList()
        {
            if (ptr) (void)hipFree(ptr);
            if (band_report) (void)hipHostFree(const_cast<uint32_t*>(band_report));
        }
        hipError_t make(uint32_t n_tiles, hipStream_t st)
        {
            const size_t w = ListLayout::words_needed(n_tiles);
            const hipError_t e = hipMalloc((void**)&ptr, w * sizeof(uint32_t));
            if (e != hipSuccess) return e;
            words = w;
            if (hipMemsetAsync(ptr + ListLayout::trailer_at(words), 0, ListLayout::kTrailerWords * sizeof(uint32_t), st) != hipSuccess) (void)hipGetLastError();
            return hipSuccess;
        }
        volatile uint32_t* report()  // band_report, allocated on first use; nullptr = no pinned memory to be had
        {
            if (!band_report) {
                void* hp = nullptr;
                if (hipHostMalloc(&hp, 64, hipHostMallocMapped | hipHostMallocPortable) == hipSuccess) band_report = static_cast<volatile uint32_t*>(std::memset(hp, 0, 64));
                else (void)hipGetLastError();
            }
            return band_report;
        }
        uint64_t bytes() const { return (uint64_t)words * sizeof(uint32_t); }
        void lend(ScanParams& p) const  // the buffer and its size, for the launchers' ListLayout::fits()
        {
            p.tile_list_buf = ptr;
            p.tile_list_words = (uint32_t)std::min<size_t>(words, 0xFFFFFFFFu);
        }
    };
    mutable StreamCache<TopkScratch> topk_scratch{8, true};  // (on `parent` for a translated image)
    mutable StreamCache<GatherTmp> gather_tmp{4, false};     // (a fifth stream: a stream-ordered allocation for the call)
    mutable StreamCache<TileList> tile_lists{4, true};       // (a fifth stream takes a list over rather than the scan silently falling back to the slower in-kernel filter: VERDICT r3 weak #6)
    using TileLease = StreamCache<TileList>::Lease;
    TileLease tile_list_lease(hipStream_t st) const  // no entry in the lease: no list to be had, the scan then filters inside the cutoff kernel
    {
        return tile_lists.acquire(st, [&](TileList& t) { return t.make(n_tiles, st); });
    }
    mutable std::atomic<uint32_t> filter_last_survivors{0};  // rf_filter_*: how many candidates the last lane-compacted call's first pass left (few: one workgroup finishes the call)
    mutable std::atomic<uint32_t> hint_trust{0};  // score_hint scans (run_many_hinted): consecutive hinted calls whose first pass resolved >= 70 % of this corpus -- while it counts, the sample (a launch and a host synchronization) is taken on every 16th call only
    // u32 ("char") corpora: the stored byte is the symbol's id in THIS corpus' alphabet.  Ids 0..253 are the 254 most
    // frequent symbols, kOverflowId lumps every rarer symbol together, kAbsentId is never stored (see resolve()).
    bool wide = false;
    uint64_t uid = 0;
    std::unordered_map<uint32_t, uint8_t> alphabet;
    std::unordered_set<uint32_t> overflow;
    // Only when `overflow` is not empty: the u32 symbol behind every packed byte (d_raw[x] belongs to d_data[x];
    // 0xFFFFFFFF in padding).  A query containing overflow symbols is served from a per-call byte image translated from
    // it (Effective below) -- exact, at the price of one extra pass over 4 bytes per symbol.
    void* d_raw = nullptr;
    uint32_t raw_elem = 4;  // bytes per raw symbol: 2 when every symbol of the corpus is <= 0xFFFE (padding 0xFFFF), else 4 (padding 0xFFFFFFFF)
    mutable uint8_t* d_sigma_identity = nullptr;  // for those images (their bytes are query-local ids, not renamed)
    const rf_corpus* parent = nullptr;            // set on such an image: scratch and locks live in the real corpus
};
constexpr uint8_t kOverflowId = 254, kAbsentId = 255;
// RF_FLAG_SLOT_ORDER is honoured by rf_many_u32 / rf_many_f64 ONLY (their `out` is sized by rf_corpus_slot_count); every other entry point writes n-entry rows and must
// never see it.  run_many therefore looks at an INTERNAL bit that only those two entry points (and rf_filter_*, for its own temporary) set; the bit is stripped from
// whatever a caller passes in.
constexpr uint32_t kFlagSlotsInternal = 0x40000000u;
// ... and (rf_filter_* only, with the bit above): the caller reads nothing outside the slots of the cutoff's length window, so nothing there needs its None
constexpr uint32_t kFlagWindowInternal = 0x20000000u;
// ... and (the per-candidate entry points only: rf_many_*, rf_one_*, rf_many_multi_*, rf_stream_many_*): hamming without RF_FLAG_HAMMING_PAD writes the reference's
// Err(DifferentLengthArgs) as its own encoding (rfgpu.h RF_DIFFERENT_LENGTH_*).  Without the bit -- rf_filter_*, rf_topk_*, the *_multi selections, every internal
// scan -- such a candidate is the ordinary None: what selects or compacts a result vector compares None by bits and knows no third value.
constexpr uint32_t kFlagErrEncodeInternal = 0x10000000u;
constexpr uint32_t kFlagsInternal = kFlagSlotsInternal | kFlagWindowInternal | kFlagErrEncodeInternal;
inline rf_args sanitized_args(const rf_args* a, bool slots_allowed, bool per_candidate = false)
{
    rf_args r = *a;
    r.flags &= ~kFlagsInternal;
    if (slots_allowed && (r.flags & RF_FLAG_SLOT_ORDER)) r.flags |= kFlagSlotsInternal;
    if (per_candidate) r.flags |= kFlagErrEncodeInternal;
    return r;
}
__attribute__((visibility("hidden"))) extern std::atomic<uint64_t> g_corpus_uid;

// the library's stream-ordered scratch allocator (rf_scratch.hip: why it is not hipMallocAsync).  scratch_free parks the block behind
// everything enqueued on `st` so far; neither call ever waits.  Calls hold their blocks in a ScratchSet.
extern "C" {
__attribute__((visibility("hidden"))) hipError_t scratch_alloc(void** out, size_t bytes, hipStream_t st);
__attribute__((visibility("hidden"))) void scratch_free(void* p, hipStream_t st);
__attribute__((visibility("hidden"))) void scratch_trim(void);
}
// Everything one call takes from scratch_alloc, bound to the call's stream.  The destructor hands every block back with scratch_free -- on
// every way out of the call, error returns included; reset() does it early, where a later allocation of the same call may reuse them.
class ScratchSet : NoCopy {
    hipStream_t st_;
    std::vector<void*> blocks_;

public:
    explicit ScratchSet(hipStream_t st) : st_(st) {}
    ScratchSet(ScratchSet&& o) noexcept : st_(o.st_), blocks_(std::exchange(o.blocks_, {})) {}
    ~ScratchSet() { reset(); }
    template <class T>
    hipError_t get(T** p, size_t bytes)
    {
        const hipError_t e = scratch_alloc(reinterpret_cast<void**>(p), bytes, st_);
        if (e == hipSuccess) blocks_.push_back((void*)*p);
        return e;
    }
    void reset()
    {
        for (void* b : blocks_) scratch_free(b, st_);
        blocks_.clear();
    }
};
// an RF_MEM_HOST result: its device staging copied home, and waited for
inline hipError_t copy_home(void* host, const void* dev, size_t bytes, hipStream_t st)
{
    const hipError_t e = hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, st);
    return e == hipSuccess ? hipStreamSynchronize(st) : e;
}

// Symbol renaming.  Every column of every kernel gathers 64 table rows from LDS, one per lane, and LDS bank
// conflicts between DIFFERENT symbols that share a bank (row index mod 32 for 8-byte rows) are the cost of that
// gather -- ASCII classes collide systematically ('A'/'a', digits/'P'..'Y').  Renaming symbols by frequency rank
// gives the 32 most frequent symbols of THIS corpus 32 distinct banks and pairs the rest with them one by one.
// The packed corpus stores sigma(c); the kernels stage PM row c at LDS row sigma(c); nothing else changes.
using ComparatorRef = std::shared_ptr<rf_comparator>;
// What a call actually runs on: the comparator lowered to the corpus' ids and the corpus itself -- or, for a u32 query
// that contains overflow-class symbols, a comparator over QUERY-LOCAL ids (1..r in order of first appearance) and a
// per-call byte image of the corpus translated from its raw symbol stream (translate_kernel: query symbol -> its id,
// anything else -> 0).  The image is a borrowed view (same tiles / slot map) that lives until the object goes out of
// scope; its payload is released in stream order.
struct Effective {
    explicit Effective(hipStream_t st) : scratch(st) {}
    const rf_comparator* c = nullptr;
    ComparatorRef hold;  // keeps a lowered comparator alive for the duration of the call
    const rf_corpus* corpus = nullptr;
    std::unique_ptr<rf_corpus> image;
    ScratchSet scratch;  // the image's payload
    std::vector<uint32_t> keys;
    std::vector<uint8_t> vals;
};
constexpr size_t kTailPad = (size_t)kWave * kChunk;  // one readable chunk row past the last tile
static inline uint64_t tile_bytes(uint32_t len) { return (uint64_t)((len + kChunk - 1) / kChunk) * kWave * kChunk; }
#define RF_HIP_C(expr)                                                                                 \
    do {                                                                                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess) {                                                                        \
            set_error(std::string(#expr) + ": " + hipGetErrorString(_e));                              \
            return fail(_e == hipErrorOutOfMemory ? RF_ERR_OOM : RF_ERR_HIP);                          \
        }                                                                                              \
    } while (0)

// Every exported rf_status function is a function-try-block ending in this: no C++ exception may cross the C ABI (a Rust or C caller
// cannot unwind it; host-side std::vector growth is where one would come from).
#define RF_ABI_CATCH                                                                                    \
    catch (const std::bad_alloc&)                                                                       \
    {                                                                                                   \
        rf::set_error("out of host memory");                                                            \
        return RF_ERR_OOM;                                                                              \
    }                                                                                                   \
    catch (const std::exception& ex)                                                                    \
    {                                                                                                   \
        rf::set_error(std::string("internal error: ") + ex.what());                                     \
        return RF_ERR_INVALID_ARG;                                                                      \
    }

// ---- the planner of rf_topk_multi_* / rf_filter_multi_* (rf_api_topk_multi.hip plan_multi): every query resolved and planned ONCE, the fusable ones grouped
static_assert(RAW_LEV == kMultiRawLev && RAW_LCS == kMultiRawLcs, "rf_multi_group.hpp names the two kinds by value");
inline MultiQuery multi_query(RawKind raw, uint32_t words, const ScanParams& p, bool fusable)
{
    return MultiQuery{fusable && fusable_base(raw, words, p.long_words_pad), MultiGroupKey{raw, p.finish, p.factor, p.op, p.len1 <= 32}};
}
struct MultiAsk {
    bool norm;         // f64-valued plans; a fusable query also keeps every maximum of its scan within the 32-bit score image (norm_key_fits)
    bool early;        // fuse the plans with this `early`: under a tight cutoff (rf_filter_multi_*) or without one (rf_topk_multi_*)
    bool fuse;         // the caller's switches: false sends every query per query (it is planned all the same)
    bool (*veto)(const ScanParams& p, RawKind raw, const rf_corpus* corpus, bool norm);  // a fusable query the caller still wants per query, or nullptr
};
struct MultiPlan {
    std::vector<ScanParams> ps;             // [q] the plans (of the queries that resolved and planned: only a fused member's is read)
    std::vector<RawKind> raws;              // [q]
    std::vector<const rf_comparator*> eff;  // [q] the comparators lowered to the corpus' ids
    std::vector<ComparatorRef> holds;       // [q] ... and what keeps them alive
    MultiGroups g;                          // the fused groups as indices into cs, and who is in one
    uint32_t fused = 0;                     // members of all groups: the fused rows, in group order
    // "[rf plan] <road>: q=<q><before> fused_groups=[4,2] per_query=<n><after>" on stderr under RF_TRACE_PLAN
    void trace(const char* road, const std::string& before, const std::string& after) const;
};

// The decode of one fused row of the f64 top-k calls (rf_topk_multi_f64, rf_join_topk_f64): `best` holds k keys, norm_key(dist, maximum) << 32 | local index
// (rf_norm_key.hpp), best first, ~0 = empty.  The key's reduced fraction a / b is the normalized distance, and (double)a / (double)b the very double emit_fin divides
// out of dist and maximum; which value the row returns is its plan's op -- the distance only for RF_OP_NORMALIZED_DISTANCE of a metric that is not the fuzz ratio
// (a ratio is always the similarity), 1.0 - nd otherwise.  Returns the row's count.
inline uint32_t decode_norm_keys(const uint64_t* best, uint32_t k, rf_metric metric, rf_op op, uint64_t index_base, double* out_score, uint64_t* out_index)
{
    const bool as_distance = op == RF_OP_NORMALIZED_DISTANCE && metric != RF_FUZZ_RATIO;
    uint32_t m = 0;
    for (; m < k && best[m] != ~0ull; ++m) {
        const NormRatio r = norm_key_ratio((uint32_t)(best[m] >> 32));
        const double nd = (double)r.a / (double)r.b;
        out_score[m] = as_distance ? nd : 1.0 - nd;
        out_index[m] = index_base + (uint32_t)best[m];
    }
    return m;
}

// ---- shared between the translation units (definitions: the file named in the comment; they sit inside the files' extern "C" blocks)
#pragma clang diagnostic ignored "-Wreturn-type-c-linkage"
// (hidden: these are internal to librfgpu.so -- only the rf_* entry points of include/rfgpu.h are exported)
#define RF_LOCAL __attribute__((visibility("hidden")))
extern "C" {
RF_LOCAL void symbol_frequencies(const uint64_t* hist, float* freq);                                                      // rf_api.hip
RF_LOCAL rf_status resolve(const rf_comparator* c, const rf_corpus* corpus, const rf_comparator** eff, ComparatorRef* hold, bool* overflow_hit = nullptr);  // rf_api.hip
RF_LOCAL rf_status make_effective(const rf_comparator* c_in, const rf_corpus* corpus, hipStream_t st, Effective* e);     // rf_api.hip
RF_LOCAL const double* jaro_device_table(int device);                                                                     // rf_api.hip
RF_LOCAL size_t pm_stride(const rf_comparator* c);                                                                        // rf_api.hip
RF_LOCAL rf_status comparator_device_pm(const rf_comparator* c, int device, const uint64_t** d_out);                      // rf_api.hip
RF_LOCAL std::vector<TileDesc> tiles_by_origin(const std::vector<TileDesc>& tiles, uint32_t n_exact, const uint32_t* orig);  // rf_api.hip
RF_LOCAL rf_status plan(const rf_comparator* c, const rf_corpus* corpus, rf_op op, const rf_args* args, bool f64_out, ScanParams* p, RawKind* raw);  // rf_api_scan.hip
RF_LOCAL rf_status plan_multi(const MultiAsk& ask, const rf_comparator* const* cs, uint32_t q, const rf_corpus* corpus, rf_op op, const rf_args* args, MultiPlan* out);  // rf_api_topk_multi.hip
RF_LOCAL rf_status check_multi_members(const char* fn, bool f64, const char* usize_only, const rf_comparator* const* cs, uint32_t q, rf_op op);  // rf_api_topk_multi.hip
RF_LOCAL rf_status corpus_take_slot_of(const rf_corpus* c, hipStream_t st, const uint32_t** out);                        // rf_api_take.hip (length-bucketed corpora: candidate -> slot)
RF_LOCAL const uint32_t* corpus_head6_plane(const rf_corpus* corpus, hipStream_t st);                                  // rf_api_scan.hip
RF_LOCAL const uint32_t* corpus_data6(const rf_corpus* corpus, hipStream_t st);                                        // rf_api_scan.hip
RF_LOCAL const uint8_t* corpus_head8_plane(const rf_corpus* corpus, const ScanParams& p, RawKind raw, hipStream_t st);    // rf_api_scan.hip
RF_LOCAL void plan_band_filter(const rf_comparator* c, const rf_corpus* corpus, rf_op op, bool f64_out, ScanParams* p, uint32_t len2);  // rf_api_scan.hip
RF_LOCAL rf_status run_many(const rf_comparator* c_in, const rf_corpus* corpus_in, rf_op op, const rf_args* args, void* out, rf_mem out_mem, void* stream, bool f64_out);  // rf_api_scan.hip
}  // extern "C"

// rf_api_join.hip -- rf_join_u32 / rf_join_f64: the (query, candidate, score) triples of two packed corpora within a cutoff.  ONE body for both score types
// (join_call<Score>: uint32_t -- distance / similarity of the usize metrics -- or double -- the normalized ops, fuzz ratio, jaro / jaro_winkler); what differs is
// JoinScore<Score> -- the entry point's name and trace prefix, whether plan() is asked for f64, which rf_filter_* the per-query road calls, which score buffer the
// kernel fills -- and the `f64` arm of check_join_args: the accepted (metric, op) pairs and where the cutoff sits.
// Two roads:
//   device      the metric and weights plan to a fused recurrence (fusable_base), the row has <= 64 symbols, every one of them can be placed exactly in the
//               scanned corpus' table, and its plan is `early`.  Either corpus may hold bytes or `char`s: the call's row map (rf_join_xlat.hpp, 256 bytes built
//               on the host) takes a stored byte of the query corpus through its SYMBOL to the scanned corpus' table row.  A row that holds an overflow-class
//               symbol of either corpus, or a symbol above 0xFF against a byte corpus, cannot be placed: when the map has such values join_bad_kernel flags
//               those rows on the device and the flags come home with the lengths.
//               The rows' lengths come home (4 bytes per row, never a symbol), plan() runs once per distinct length -- a byte query reaches its plan through its
//               length alone -- the fusable rows are sorted by length and cut into batches; per batch one join_pm_kernel builds the tables out of the query
//               corpus' payload and one join_kernel per class (narrow / wide) that occurs walks the batch's work list (rf_join_plan.hpp, rf_join.hip).  One
//               64-bit counter and one triple buffer serve the whole call; they come home once, after the last batch.
//               Candidates that hold overflow-class symbols store the overflow id, whose row no fused query has a bit in: they match nothing there, which is
//               exact because every query row with such a symbol went per query.
//               rf_join_f64 plans with f64_out (a fuzz ratio becomes the normalized similarity of its inner metric in plan()) and the kernel stores the double
//               itself: no 32-bit key is ordered, so no maximum of the corpus is too large.
//   per query   every other row: rf_corpus_take[_u32] of the row, rf_comparator_new[_u32], rf_filter_u32 / rf_filter_f64, append.  Plain host code, slow by design, total.
// Ordering, the 64-bit bases and the writes happen on the host at the very end: a call that fails has written nothing.
// rf_join_topk_u32 (join_topk_call): the k best candidates for every row of Q, row j being rf_topk_u32 of a comparator over row Q[j].  It shares with join_call
// the argument checks' common part (check_join_metric_op), the rows of Q (join_rows), the length pass (join_lengths), one plan() per distinct length
// (join_plan_rows), the batches with their blob upload and table build (JoinBatches) and the walk of the per-query road (for_each_row_comparator).  Its device
// road takes the rows whose plan rf_topk_multi_u32 would fuse -- no early-out: no cutoff or a loose one -- at k <= 64: per batch the tables, one join_topk_kernel per
// class that occurs (rf_join_topk.hip) under the batch's span (join_topk_span) and one selection launch; the keys come home once, after the last batch.
// Its per-query road is rf_topk_u32.
// rf_join_topk_f64 is the same body (join_topk_call<double>; JoinTopkScore<Score> holds what differs): the normalized ops, fuzz ratio, jaro / jaro_winkler.  Its device
// road takes what rf_topk_multi_f64 would fuse -- f64 plans without an early-out whose every maximum stays within the 32-bit score image, norm_key_fits per ROW with the
// corpus' longest candidate -- through join_topk_kernel's kNorm instantiation; the keys are decoded by decode_norm_keys (rf_host.hpp), the function rf_topk_multi_f64 uses.
// Its per-query road is rf_topk_f64.
// Product code: never includes or links anything from oracle/.
#include <numeric>

#include "rf_host.hpp"

#include "rf_alphabet.hpp"
#include "rf_join_plan.hpp"
#include "rf_join_xlat.hpp"
#include "rf_take_addr.hpp"

static_assert(rf::kXlatOverflowId == kOverflowId && rf::kXlatAbsentId == kAbsentId && rf::kXlatNoSymbol == rf::kReservedSymbol, "rf_join_xlat.hpp restates the ids of a `char` corpus");

// (all three calls read the two switches through these)
// A/B switch: 0 sends every row down the per-query road (identical results)
static bool sw_join() { static const bool v = env_on("RF_JOIN"); return v; }
// most queries of a device batch (the batch's tables are 2 KiB of scratch per query)
static uint32_t sw_join_batch() { static const uint32_t v = (uint32_t)std::max<long long>(1, std::min<long long>(env_int("RF_JOIN_BATCH", 16384), 1 << 20)); return v; }
// rf_join_topk_u32: the units a batch's work list should reach (0 = auto: the workgroups of a launch); any other value is taken as it is, below kJoinSpan tiles too
static uint32_t sw_join_topk_units() { static const uint32_t v = (uint32_t)std::max<long long>(0, std::min<long long>(env_int("RF_JOIN_TOPK_UNITS", 0), 1 << 30)); return v; }

namespace {
template <class Score>
struct Triple {
    uint32_t pos, idx;
    Score score;
};
// what the two score types do not share
template <class Score>
struct JoinScore;
template <>
struct JoinScore<uint32_t> {
    static constexpr bool kF64 = false;
    static constexpr const char* kName = "rf_join_u32";
    static constexpr const char* kTrace = "join";
    static rf_status filter(const rf_comparator* c, const rf_corpus* corpus, rf_op op, const rf_args* args, uint64_t room, uint64_t* index, uint32_t* score, uint64_t* count, void* stream)
    {
        return rf_filter_u32(c, corpus, op, args, 0, room, index, score, count, RF_MEM_HOST, RF_FILTER_BY_INDEX, stream);
    }
    static void bind(JoinParams& jp, uint32_t* d_scores) { jp.scores = d_scores, jp.scores_f64 = nullptr, jp.norm = 0; }
};
template <>
struct JoinScore<double> {
    static constexpr bool kF64 = true;
    static constexpr const char* kName = "rf_join_f64";
    static constexpr const char* kTrace = "join_f64";
    static rf_status filter(const rf_comparator* c, const rf_corpus* corpus, rf_op op, const rf_args* args, uint64_t room, uint64_t* index, double* score, uint64_t* count, void* stream)
    {
        return rf_filter_f64(c, corpus, op, args, 0, room, index, score, count, RF_MEM_HOST, RF_FILTER_BY_INDEX, stream);
    }
    static void bind(JoinParams& jp, double* d_scores) { jp.scores = nullptr, jp.scores_f64 = d_scores, jp.norm = 1; }
};
struct ComparatorOwner : NoCopy {
    rf_comparator* c = nullptr;
    ~ComparatorOwner() { rf_comparator_free(c); }
};

// What the device roads share: the call's control block with the query corpus' inverse sigma, the batch's tables and its upload.  A batch is the rows
// [from, to) of `fused` (sorted): run() builds the two work lists under `span`, uploads [rows | narrow items | wide items | narrow prefix | wide prefix | tail] in
// one copy and builds the tables (join_pm_kernel); the caller then launches over lists[k] at items(k) / prefix(k).
struct JoinBatches : NoCopy {
    uint32_t B = 0;         // most rows of a batch
    size_t max_batch = 0;   // ... of this call's
    uint8_t* d_ctl = nullptr;  // 512 bytes: [256 for the road's own counters, zeroed | the call's row map: query corpus' stored symbol -> scanned corpus' table row]
    uint64_t* d_tables = nullptr;
    uint32_t* d_blob = nullptr;
    size_t blob_words = 0;
    std::deque<std::vector<uint32_t>> blobs;  // the host side of every upload stays alive until the stream has drained
    JoinPmParams pm{};
    JoinList lists[2];      // narrow, wide: the batch run() saw last
    size_t items_at[2] = {0, 0}, prefix_at[2] = {0, 0}, tail_at = 0;
    bool outgrew = false;
    rf_status outgrew_status(const char* name, hipStream_t st) const
    {
        set_error(std::string(name) + ": internal error: a batch's work list outgrew its scratch");
        (void)hipStreamSynchronize(st);
        return RF_ERR_INVALID_ARG;
    }
    const JoinItem* items(int k) const { return reinterpret_cast<const JoinItem*>(d_blob + items_at[k]); }
    const uint32_t* prefix(int k) const { return d_blob + prefix_at[k]; }
    const uint32_t* tail() const { return d_blob + tail_at; }

    // tail_words_per_row: words the caller appends per row of a batch; xl: the call's row map, alive until the stream has drained
    rf_status init(const rf_corpus* queries, const JoinXlat& xl, size_t n_fused, const uint32_t* d_row_slot, const uint32_t* d_row_len, size_t tail_words_per_row, ScratchSet& sc,
                   hipStream_t st)
    {
        B = sw_join_batch();
        max_batch = std::min<size_t>(B, n_fused);
        RF_HIP(sc.get(&d_ctl, 512));
        RF_HIP(hipMemsetAsync(d_ctl, 0, 256, st));
        RF_HIP(hipMemcpyAsync(d_ctl + 256, xl.row_of, 256, hipMemcpyHostToDevice, st));
        RF_HIP(sc.get(&d_tables, max_batch * 256 * sizeof(uint64_t)));
        // at most max_batch items and max_batch + 2 prefix entries
        blob_words = max_batch + max_batch * (sizeof(JoinItem) / 4) + max_batch + 2 + max_batch * tail_words_per_row;
        RF_HIP(sc.get(&d_blob, blob_words * sizeof(uint32_t)));
        pm.s.data = queries->d_data;
        pm.s.tiles = queries->uniform ? nullptr : queries->d_tiles;
        pm.s.uniform_len = queries->uniform_len;
        pm.s.uniform_tile_bytes = (uint32_t)tile_bytes(queries->uniform_len);
        pm.n_slots = queries->uniform ? queries->n_tiles * (uint32_t)kWave : (uint32_t)queries->n_slots;
        pm.row_slot = d_row_slot, pm.row_len = d_row_len;
        pm.row_of = d_ctl + 256;
        pm.tables = d_tables;
        return RF_OK;
    }
    // tail(lists): the caller's words behind the work lists.  A blob that outgrew its scratch (an internal error) sets `outgrew` and launches nothing: the caller
    // answers it with outgrew_status()
    template <class Tail>
    hipError_t run(const std::vector<JoinQuery>& fused, size_t from, size_t to, uint32_t n_tiles, uint32_t span, Tail&& tail, hipStream_t st)
    {
        lists[0] = join_items(fused, from, to, true, n_tiles, span);
        lists[1] = join_items(fused, from, to, false, n_tiles, span);
        blobs.emplace_back();
        std::vector<uint32_t>& blob = blobs.back();
        blob.reserve(blob_words);
        for (size_t i = from; i < to; ++i) blob.push_back(fused[i].pos);
        for (int k = 0; k < 2; ++k) {
            items_at[k] = blob.size();
            const uint32_t* w = reinterpret_cast<const uint32_t*>(lists[k].items.data());
            blob.insert(blob.end(), w, w + lists[k].items.size() * (sizeof(JoinItem) / 4));
        }
        for (int k = 0; k < 2; ++k) {
            prefix_at[k] = blob.size();
            blob.insert(blob.end(), lists[k].prefix.begin(), lists[k].prefix.end());
        }
        tail_at = blob.size();
        tail(blob);
        if (blob.size() > blob_words) {
            outgrew = true;
            return hipErrorInvalidValue;
        }
        const hipError_t e = hipMemcpyAsync(d_blob, blob.data(), blob.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return e;
        pm.rows = d_blob, pm.batch = (uint32_t)(to - from);
        return launch_join_pm(pm, st);
    }
};
inline rf_status join_hip_status(const char* name, const char* where, hipError_t e)
{
    (void)hipGetLastError();
    set_error(std::string(name) + ", " + where + ": " + hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? RF_ERR_OOM : RF_ERR_HIP;
}

// the device road over the rows `fused` (sorted): triples of the first `cap` pairs to arrive into `out`, the true number of pairs into *total
template <class Score>
rf_status join_device(RawKind raw, const ScanParams& plan0, const rf_corpus* queries, const rf_corpus* corpus, const JoinXlat& xl, const std::vector<JoinQuery>& fused, const uint32_t* d_row_slot,
                      const uint32_t* d_row_len, uint32_t flags, uint64_t cap, ScratchSet& sc, hipStream_t st, std::vector<Triple<Score>>* out, uint64_t* total, uint32_t* n_batches,
                      uint32_t* n_groups)
{
    // per-call device state: [counter | row map], the triple buffer, and per-batch scratch bounded by the batch
    JoinBatches jb;
    if (const rf_status s = jb.init(queries, xl, fused.size(), d_row_slot, d_row_len, 0, sc, st); s != RF_OK) return s;
    unsigned long long* d_count = reinterpret_cast<unsigned long long*>(jb.d_ctl);
    uint64_t* d_pairs = nullptr;
    Score* d_scores = nullptr;
    if (cap) {
        RF_HIP(sc.get(&d_pairs, cap * sizeof(uint64_t)));
        RF_HIP(sc.get(&d_scores, cap * sizeof(Score)));
    }

    JoinParams jp{};
    jp.s = plan0;
    jp.s.out = nullptr, jp.s.prefill_none = 0, jp.s.tile_step = 1, jp.s.len1 = 0, jp.s.tile_begin = 0, jp.s.tile_end = 0;
    jp.span = kJoinSpan;
    jp.tables = jb.d_tables;
    jp.count = d_count, jp.pairs = d_pairs, jp.cap = cap;
    JoinScore<Score>::bind(jp, d_scores);
    jp.upper = (flags & RF_JOIN_UPPER) ? 1u : 0u;

    hipError_t e = hipSuccess;
    for (size_t from = 0; from < fused.size() && e == hipSuccess; from += jb.B) {
        const size_t to = std::min(fused.size(), from + jb.B);
        e = jb.run(fused, from, to, corpus->n_tiles, kJoinSpan, [](std::vector<uint32_t>&) {}, st);
        for (int k = 0; k < 2 && e == hipSuccess; ++k) {
            if (jb.lists[k].items.empty()) continue;
            jp.items = jb.items(k);
            jp.prefix = jb.prefix(k);
            jp.n_items = (uint32_t)jb.lists[k].items.size(), jp.n_units = jb.lists[k].units(), jp.batch = (uint32_t)(to - from);
            e = launch_join(raw, k == 0, jp, jb.lists[k].items.data(), jb.lists[k].prefix.data(), st);
            *n_groups += jp.n_items;
        }
        ++*n_batches;
    }
    if (jb.outgrew) return jb.outgrew_status(JoinScore<Score>::kName, st);
    unsigned long long count = 0;
    if (e == hipSuccess) e = copy_home(&count, d_count, sizeof(count), st);
    else (void)hipStreamSynchronize(st);
    if (e == hipSuccess) {
        const size_t have = (size_t)std::min<uint64_t>(count, cap);
        if (have) {
            std::vector<uint64_t> pairs(have);
            std::vector<Score> scores(have);
            e = hipMemcpyAsync(pairs.data(), d_pairs, have * sizeof(uint64_t), hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = copy_home(scores.data(), d_scores, have * sizeof(Score), st);
            else (void)hipStreamSynchronize(st);
            if (e == hipSuccess) {
                out->reserve(out->size() + have);
                for (size_t i = 0; i < have; ++i) out->push_back(Triple<Score>{(uint32_t)(pairs[i] >> 32), (uint32_t)pairs[i], scores[i]});
            }
        }
    }
    if (e != hipSuccess) return join_hip_status(JoinScore<Score>::kName, "device road", e);
    *total = count;
    return RF_OK;
}

// The walk both per-query roads make over the positions `rest` of Q: the rows come out of the query corpus kRows at a time (rf_corpus_take[_u32]) and each
// becomes a comparator (rf_comparator_new[_u32]) that row(pos, comparator) then uses
template <class Row>
rf_status for_each_row_comparator(rf_metric metric, const rf_corpus* queries, const std::vector<uint32_t>& qidx, const std::vector<uint32_t>& rest, void* stream, Row&& row)
{
    constexpr size_t kRows = 4096;  // rows taken out of the query corpus per call
    std::vector<uint64_t> want, offsets;
    std::vector<uint8_t> bytes;
    std::vector<uint32_t> elems;
    for (size_t from = 0; from < rest.size(); from += kRows) {
        const size_t cnt = std::min(kRows, rest.size() - from);
        want.resize(cnt), offsets.assign(cnt + 1, 0);
        for (size_t j = 0; j < cnt; ++j) want[j] = qidx[rest[from + j]];
        rf_status s = queries->wide ? rf_corpus_take_u32(queries, want.data(), cnt, 0, nullptr, 0, offsets.data(), RF_MEM_HOST, stream)
                                    : rf_corpus_take(queries, want.data(), cnt, 0, nullptr, 0, offsets.data(), RF_MEM_HOST, stream);
        if (s != RF_OK) return s;
        const uint64_t symbols = offsets[cnt];
        if (queries->wide) {
            elems.resize(std::max<uint64_t>(symbols, 1));
            s = rf_corpus_take_u32(queries, want.data(), cnt, 0, elems.data(), symbols, offsets.data(), RF_MEM_HOST, stream);
        } else {
            bytes.resize(std::max<uint64_t>(symbols, 1));
            s = rf_corpus_take(queries, want.data(), cnt, 0, bytes.data(), symbols, offsets.data(), RF_MEM_HOST, stream);
        }
        if (s != RF_OK) return s;
        for (size_t j = 0; j < cnt; ++j) {
            const size_t len = (size_t)(offsets[j + 1] - offsets[j]);
            ComparatorOwner c;
            s = queries->wide ? rf_comparator_new_u32(metric, elems.data() + offsets[j], len, &c.c) : rf_comparator_new(metric, bytes.data() + offsets[j], len, &c.c);
            if (s != RF_OK) return s;
            if (s = row(rest[from + j], c.c); s != RF_OK) return s;
        }
    }
    return RF_OK;
}

// the per-query road over the positions `rest` of Q: appends while `out` has room below `capacity`, adds every match to *total
template <class Score>
rf_status join_per_query(rf_metric metric, const rf_corpus* queries, const std::vector<uint32_t>& qidx, const std::vector<uint32_t>& rest, const rf_corpus* corpus, rf_op op,
                         const rf_args* args, uint32_t flags, uint64_t capacity, void* stream, std::vector<Triple<Score>>* out, uint64_t* total)
{
    std::vector<uint64_t> index;
    std::vector<Score> score;
    return for_each_row_comparator(metric, queries, qidx, rest, stream, [&](uint32_t pos, const rf_comparator* c) {
        // every match of this query (the flag needs them all): a first room, then the true count's
        uint64_t room = std::max<size_t>(index.size(), 1024), count = 0;
        while (true) {
            index.resize(room), score.resize(room);
            const rf_status s = JoinScore<Score>::filter(c, corpus, op, args, room, index.data(), score.data(), &count, stream);
            if (s != RF_OK) return s;
            if (count <= room) break;
            room = count;
        }
        for (uint64_t k = 0; k < count; ++k) {
            if ((flags & RF_JOIN_UPPER) && index[k] <= qidx[pos]) continue;
            ++*total;
            if (out->size() < capacity) out->push_back(Triple<Score>{pos, (uint32_t)index[k], score[k]});
        }
        return (rf_status)RF_OK;
    });
}

// What the argument checks of the three calls share -- op against the result type, the flag bits the call knows, the metric -- decided like everything else in them
// before either corpus is looked at or a device is touched, and before anything is written
rf_status check_join_metric_op(const std::string& name, bool f64, rf_metric metric, rf_op op, uint32_t flags, uint32_t known_flags)
{
    auto bad = [&](const std::string& why) {
        set_error(name + ": " + why);
        return RF_ERR_INVALID_ARG;
    };
    if (!f64 && op != RF_OP_DISTANCE && op != RF_OP_SIMILARITY) return bad("op must be RF_OP_DISTANCE or RF_OP_SIMILARITY");
    if ((int)op < 0 || (int)op > (int)RF_OP_NORMALIZED_SIMILARITY) return bad("unknown op");
    if (flags & ~known_flags) return bad("unknown flag bit");
    switch ((int)metric) {
    case RF_LEVENSHTEIN: case RF_INDEL: case RF_LCS_SEQ: case RF_OSA: case RF_DAMERAU_LEVENSHTEIN: case RF_HAMMING: case RF_PREFIX: case RF_POSTFIX:
        if (f64 && (op == RF_OP_DISTANCE || op == RF_OP_SIMILARITY)) return bad("distance and similarity of the usize metrics are u32-valued (rf_join_u32)");
        break;
    case RF_FUZZ_RATIO:
        if (!f64) return bad("usize-valued metrics only (jaro / jaro_winkler / fuzz ratio are f64-valued)");
        if (op != RF_OP_SIMILARITY && op != RF_OP_NORMALIZED_SIMILARITY) return bad("RatioBatchComparator only has similarity (fuzz.rs:115-149)");
        break;
    case RF_JARO: case RF_JARO_WINKLER:
        if (!f64) return bad("usize-valued metrics only (jaro / jaro_winkler / fuzz ratio are f64-valued)");
        break;
    default: return bad("unknown metric");
    }
    return RF_OK;
}
// The argument errors of rf_join_u32 / rf_join_f64
rf_status check_join_args(const char* fn, bool f64, rf_metric metric, const rf_corpus* queries, const rf_corpus* corpus, rf_op op, const rf_args* args_in, uint32_t flags,
                          uint64_t capacity, const uint64_t* out_query, const uint64_t* out_index, const void* out_score, const uint64_t* out_count, rf_join_order order)
{
    const std::string name(fn);
    auto bad = [&](const std::string& why) {
        set_error(name + ": " + why);
        return RF_ERR_INVALID_ARG;
    };
    if (!queries || !corpus || !args_in || !out_count) return bad("null handle, args or count");
    if (capacity && (!out_query || !out_index || !out_score)) return bad("null output with a non-zero capacity");
    if ((int)order != (int)RF_JOIN_BY_QUERY && (int)order != (int)RF_JOIN_ANY) return bad("unknown order");
    if (const rf_status s = check_join_metric_op(name, f64, metric, op, flags, RF_JOIN_UPPER); s != RF_OK) return s;
    if (f64 ? std::isnan(args_in->cutoff_f64) : args_in->cutoff_usize == RF_NO_CUTOFF) return bad("args must carry a score_cutoff (without one the answer is every pair)");
    return RF_OK;
}
// ... and of rf_join_topk_u32 / rf_join_topk_f64: no cutoff is required, k is, and the flag they know is RF_JOIN_NO_SELF
rf_status check_join_topk_args(const char* fn, bool f64, rf_metric metric, const rf_corpus* queries, const rf_corpus* corpus, rf_op op, const rf_args* args_in, uint32_t flags,
                               uint32_t k)
{
    const std::string name(fn);
    auto bad = [&](const std::string& why) {
        set_error(name + ": " + why);
        return RF_ERR_INVALID_ARG;
    };
    if (!queries || !corpus || !args_in) return bad("null handle or args");
    if (k == 0) return bad("k must be at least 1");
    return check_join_metric_op(name, f64, metric, op, flags, RF_JOIN_NO_SELF);
}

// Q: the row index of every position, after the checks that look at the query corpus (nothing is written before them)
rf_status join_rows(const char* fn, const rf_corpus* queries, const rf_corpus* corpus, const uint64_t* query_indices, uint64_t m, std::vector<uint32_t>* qidx)
{
    auto bad = [&](const char* why) {
        set_error(std::string(fn) + ": " + why);
        return RF_ERR_INVALID_ARG;
    };
    if (queries->borrowed || corpus->borrowed) return bad("not a packed corpus");
    if (!query_indices && m != queries->n) return bad("query_indices == NULL asks for every row: m must be rf_corpus_count(queries)");
    if (m > 0xFFFFFFFEull) return bad("more than 2^32 - 2 queries in one call");
    qidx->resize((size_t)m);
    if (query_indices) {
        for (size_t j = 0; j < (size_t)m; ++j) {
            if (query_indices[j] >= queries->n) return bad("a query index lies beyond rf_corpus_count(queries)");
            (*qidx)[j] = (uint32_t)query_indices[j];
        }
    } else {
        std::iota(qidx->begin(), qidx->end(), 0u);
    }
    return RF_OK;
}

// The call's row map (rf_join_xlat.hpp) out of the two handles.  false: the scanned corpus' sigma gives the absent id a row in use -- no packer makes such a
// corpus -- and nothing may be fused
bool join_xlat_of(const rf_corpus* queries, const rf_corpus* corpus, JoinXlat* xl)
{
    uint32_t sym_q[256], sym_c[256];
    auto view = [](const rf_corpus* c, uint32_t* sym) {
        for (uint32_t id = 0; id < 256; ++id) sym[id] = kXlatNoSymbol;
        for (const auto& kv : c->alphabet) sym[kv.second] = kv.first;
        return JoinXlatCorpus{c->wide, c->sigma, sym, !c->overflow.empty()};
    };
    return join_xlat_build(view(queries, sym_q), view(corpus, sym_c), [&](uint32_t sym) -> uint32_t {
        const auto a = corpus->alphabet.find(sym);
        if (a != corpus->alphabet.end()) return a->second;
        return corpus->overflow.count(sym) ? kXlatOverflowId : kXlatAbsentId;
    }, xl);
}

// the rows' slots and lengths (take_rows_len_kernel) into tp->row_slot / tp->row_len; the lengths come home -- and with them, in the same synchronization, one
// flag per row when the row map has values it cannot place (xl.any_bad; join_bad_kernel): `flagged` stays empty otherwise
rf_status join_lengths(const char* fn, const rf_corpus* queries, const JoinXlat& xl, const std::vector<uint32_t>& qidx, ScratchSet& sc, hipStream_t st, TakeParams* tp_out,
                       std::vector<uint32_t>* lens, std::vector<uint32_t>* flagged)
{
    const size_t m = qidx.size();
    TakeParams& tp = *tp_out;
    tp = TakeParams{};
    tp.s.data = queries->d_data;
    tp.s.tiles = queries->uniform ? nullptr : queries->d_tiles;
    tp.s.uniform_len = queries->uniform_len;
    tp.s.uniform_tile_bytes = (uint32_t)tile_bytes(queries->uniform_len);
    tp.n_slots = queries->uniform ? queries->n_tiles * (uint32_t)kWave : (uint32_t)queries->n_slots;
    uint32_t* d_idx = nullptr;
    RF_HIP(sc.get(&d_idx, m * sizeof(uint32_t)));
    RF_HIP(sc.get(&tp.row_slot, m * sizeof(uint32_t)));
    const size_t words = xl.any_bad ? 2 * m : m;  // [lengths | flags]
    RF_HIP(sc.get(&tp.row_len, words * sizeof(uint32_t)));
    uint8_t* d_bad = nullptr;
    if (xl.any_bad) RF_HIP(sc.get(&d_bad, 256));
    if (!queries->uniform)
        if (const rf_status s = corpus_take_slot_of(queries, st, &tp.slot_of); s != RF_OK) return s;
    lens->resize(words);
    hipError_t e = hipMemcpyAsync(d_idx, qidx.data(), m * sizeof(uint32_t), hipMemcpyHostToDevice, st);
    tp.idx = d_idx, tp.m = m;
    if (e == hipSuccess) e = launch_take_rows_len(tp, st);
    if (e == hipSuccess && xl.any_bad) {
        e = hipMemcpyAsync(d_bad, xl.bad, 256, hipMemcpyHostToDevice, st);  // (xl outlives the call's last synchronization)
        JoinBadParams bp{};
        bp.s = tp.s, bp.n_slots = tp.n_slots;
        bp.row_slot = tp.row_slot, bp.row_len = tp.row_len;
        bp.bad = d_bad, bp.flags = tp.row_len + m, bp.m = m;
        if (e == hipSuccess) e = launch_join_bad(bp, st);
    }
    if (e == hipSuccess) e = copy_home(lens->data(), tp.row_len, words * sizeof(uint32_t), st);
    else (void)hipStreamSynchronize(st);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        set_error(std::string(fn) + ", query lengths: " + hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? RF_ERR_OOM : RF_ERR_HIP;
    }
    flagged->assign(lens->begin() + m, lens->end());
    lens->resize(m);
    return RF_OK;
}

// One plan per distinct length: plan() reads of a byte comparator its metric and its length (the query's head and bytes only for kernels no fused road runs),
// and of the corpus nothing that depends on its kind -- a `char` corpus is searched through a lowered BYTE comparator of the same length (resolve()), which is
// what the probe stands for.  What does look at symbols (the 6-bit image, the head plane) is decided in run_many, which no fused road passes; the band needs a
// query of two words or more.
// A row whose plan fusable(p, raw) accepts goes to `fused` with the plan's tile window, every other row to `rest` -- and so does every row `flagged` (empty: none
// is) names: it holds a symbol the row map cannot place; plan0 / raw0 are the first accepted plan's.
struct JoinPlanned {
    std::vector<JoinQuery> fused;
    ScanParams plan0{};
    RawKind raw0 = RAW_LEV;
};
template <class Fusable>
rf_status join_plan_rows(rf_metric metric, const rf_corpus* corpus, rf_op op, const rf_args* args, bool f64, const std::vector<uint32_t>& qidx, const std::vector<uint32_t>& lens,
                         const std::vector<uint32_t>& flagged, Fusable&& fusable, JoinPlanned* out, std::vector<uint32_t>* rest)
{
    struct LenPlan {
        bool planned = false, fusable = false;
        uint32_t tile_begin = 0, tile_end = 0;
    };
    LenPlan by_len[kJoinMaxLen + 1];
    bool have_plan0 = false;
    for (size_t j = 0; j < qidx.size(); ++j) {
        const uint32_t len = lens[j];
        if (len > kJoinMaxLen || (!flagged.empty() && flagged[j])) {
            rest->push_back((uint32_t)j);
            continue;
        }
        LenPlan& lp = by_len[len];
        if (!lp.planned) {
            lp.planned = true;
            rf_comparator probe;  // (no table, no device state: the planner's view of "a byte query of this length")
            probe.metric = metric;
            probe.s1.assign(len, 0);
            probe.block_count = (len + 63) / 64, probe.words = 1;
            ScanParams p;
            RawKind raw;
            const rf_status s = plan(&probe, corpus, op, args, f64, &p, &raw);
            if (s == RF_ERR_UNSUPPORTED) return s;
            if (s == RF_OK && fusable_base(raw, 1, p.long_words_pad) && !p.band && fusable(p, raw)) {
                lp.fusable = true;
                lp.tile_begin = p.tile_begin, lp.tile_end = std::min(p.tile_end, corpus->n_tiles);
                if (lp.tile_begin >= lp.tile_end) lp.tile_begin = lp.tile_end = 0;
                if (!have_plan0) out->plan0 = p, out->raw0 = raw, have_plan0 = true;
            }
        }
        if (lp.fusable)
            out->fused.push_back(JoinQuery{len, (uint32_t)j, qidx[j], lp.tile_begin, lp.tile_end});
        else
            rest->push_back((uint32_t)j);
    }
    join_sort(out->fused);
    return RF_OK;
}

template <class Score>
rf_status join_call(rf_metric metric, const rf_corpus* queries, const uint64_t* query_indices, uint64_t m, const rf_corpus* corpus, rf_op op, const rf_args* args_in, uint32_t flags,
                    uint64_t query_base, uint64_t index_base, uint64_t capacity, uint64_t* out_query, uint64_t* out_index, Score* out_score, uint64_t* out_count,
                    rf_join_order order, void* stream)
{
    using JS = JoinScore<Score>;
    if (const rf_status s = check_join_args(JS::kName, JS::kF64, metric, queries, corpus, op, args_in, flags, capacity, out_query, out_index, out_score, out_count, order); s != RF_OK)
        return s;
    if (m == 0) return RF_OK;  // (writes nothing)
    const rf_args args_v = sanitized_args(args_in, false);
    const rf_args* args = &args_v;

    // ---- the corpora
    std::vector<uint32_t> qidx;
    if (const rf_status s = join_rows(JS::kName, queries, corpus, query_indices, m, &qidx); s != RF_OK) return s;
    if (queries->n == 0 || corpus->n == 0) {
        *out_count = 0;
        return RF_OK;
    }
    if (queries->device != corpus->device) {
        set_error(std::string(JS::kName) + ": the two corpora are on different devices");
        return RF_ERR_INVALID_ARG;
    }
    hipStream_t st = (hipStream_t)stream;

    std::vector<Triple<Score>> triples;
    uint64_t total = 0;
    std::vector<uint32_t> rest;  // positions of Q for the per-query road
    uint32_t n_batches = 0, n_groups = 0;
    const bool device_metric = metric == RF_LEVENSHTEIN || metric == RF_INDEL || metric == RF_LCS_SEQ || (JS::kF64 && metric == RF_FUZZ_RATIO);
    JoinXlat xl;  // (lives to the end of the call: uploads read it)
    if (sw_join() && device_metric && join_xlat_of(queries, corpus, &xl)) {
        DeviceGuard guard(corpus->device);
        if (!guard.ok) {
            set_error("cannot select the corpus' device");
            return RF_ERR_NO_DEVICE;
        }
        ScratchSet sc(st);
        TakeParams tp;
        std::vector<uint32_t> lens, flagged;
        if (const rf_status s = join_lengths(JS::kName, queries, xl, qidx, sc, st, &tp, &lens, &flagged); s != RF_OK) return s;
        JoinPlanned pl;
        // (a tight cutoff: the planner's early-out rule)
        if (const rf_status s = join_plan_rows(metric, corpus, op, args, JS::kF64, qidx, lens, flagged, [](const ScanParams& p, RawKind) { return p.early && p.has_cutoff; }, &pl, &rest); s != RF_OK)
            return s;
        if (!pl.fused.empty()) {
            const uint64_t cap = std::min<uint64_t>(capacity, (uint64_t)pl.fused.size() * corpus->n);
            if (const rf_status s = join_device(pl.raw0, pl.plan0, queries, corpus, xl, pl.fused, tp.row_slot, tp.row_len, flags, cap, sc, st, &triples, &total, &n_batches, &n_groups); s != RF_OK)
                return s;
        }
    } else {
        rest.resize((size_t)m);
        std::iota(rest.begin(), rest.end(), 0u);
    }
    if (sw_trace_plan())
        std::fprintf(stderr, "[rf plan] %s: m=%llu batches=%u groups=%u per_query=%zu\n", JS::kTrace, (unsigned long long)m, n_batches, n_groups, rest.size());
    if (!rest.empty())
        if (const rf_status s = join_per_query(metric, queries, qidx, rest, corpus, op, args, flags, capacity, stream, &triples, &total); s != RF_OK) return s;

    // ---- order, widen, write
    if (order == RF_JOIN_BY_QUERY)
        std::sort(triples.begin(), triples.end(), [](const Triple<Score>& a, const Triple<Score>& b) { return a.pos != b.pos ? a.pos < b.pos : a.idx < b.idx; });
    for (size_t i = 0; i < triples.size(); ++i) {
        out_query[i] = query_base + qidx[triples[i].pos];
        out_index[i] = index_base + triples[i].idx;
        out_score[i] = triples[i].score;
    }
    *out_count = total;
    return RF_OK;
}

// ---- rf_join_topk_u32 / rf_join_topk_f64
// what the two score types do not share: the entry point's name and trace prefix, whether plan() is asked for f64 (and the kernel for its normalized instantiation),
// which rf_topk_* the per-query road calls
template <class Score>
struct JoinTopkScore;
template <>
struct JoinTopkScore<uint32_t> {
    static constexpr bool kF64 = false;
    static constexpr const char* kName = "rf_join_topk_u32";
    static constexpr const char* kTrace = "join_topk";
    static rf_status topk(const rf_comparator* c, const rf_corpus* corpus, rf_op op, const rf_args* args, uint32_t ask, uint32_t* score, uint64_t* index, uint32_t* count, void* stream)
    {
        return rf_topk_u32(c, corpus, op, args, ask, 0, score, index, count, nullptr, RF_MEM_HOST, stream);
    }
};
template <>
struct JoinTopkScore<double> {
    static constexpr bool kF64 = true;
    static constexpr const char* kName = "rf_join_topk_f64";
    static constexpr const char* kTrace = "join_topk_f64";
    static rf_status topk(const rf_comparator* c, const rf_corpus* corpus, rf_op op, const rf_args* args, uint32_t ask, double* score, uint64_t* index, uint32_t* count, void* stream)
    {
        uint64_t n = 0;
        const rf_status s = rf_topk_f64(c, corpus, op, args, ask, 0, score, index, &n, nullptr, RF_MEM_HOST, stream);
        *count = (uint32_t)n;
        return s;
    }
};

// The device road over the rows `fused` (sorted): row i of `keys` ([fused.size()][k], best first, ~0 = empty) belongs to fused[i].  Per batch: the span for its
// items (join_topk_span), the work lists, the tables, the batch's segments filled with ~0, one join_topk_kernel per class that occurs, one selection launch into the
// batch's rows of the call's key buffer.  The keys come home once, after the last batch.  `norm` (rf_join_topk_f64): plan0 is an f64 plan of a normalized op and the keys
// are norm_key images (the kernel's kNorm instantiation).
rf_status join_topk_device(const char* kName, bool norm, RawKind raw, const ScanParams& plan0, const rf_corpus* queries, const rf_corpus* corpus, const JoinXlat& xl, const std::vector<JoinQuery>& fused,
                           const uint32_t* d_row_slot, const uint32_t* d_row_len, rf_op op, uint32_t flags, uint32_t k, ScratchSet& sc, hipStream_t st, std::vector<uint64_t>* keys,
                           uint32_t* n_batches, uint32_t* n_groups, uint64_t* n_units)
{
    JoinBatches jb;
    if (const rf_status s = jb.init(queries, xl, fused.size(), d_row_slot, d_row_len, 1, sc, st); s != RF_OK) return s;
    const uint32_t n_tiles = corpus->n_tiles;
    const uint32_t forced = sw_join_topk_units();
    const uint32_t target = forced ? forced : (uint32_t)std::max(1, scan_max_grid());
    // the span of every batch first: the largest segment sizes the scratch
    auto items_of = [&](size_t from, size_t to) {
        size_t narrow = 0;
        for (size_t i = from; i < to; ++i) narrow += join_narrow(fused[i].len) ? 1 : 0;
        return (uint32_t)((narrow + kJoinMembers - 1) / kJoinMembers + (to - from - narrow + kJoinMembers - 1) / kJoinMembers);
    };
    uint64_t seg_keys_max = 0;
    for (size_t from = 0; from < fused.size(); from += jb.B) {
        const size_t to = std::min(fused.size(), from + jb.B);
        const uint32_t span = join_topk_span(n_tiles, items_of(from, to), target, forced != 0);
        seg_keys_max = std::max<uint64_t>(seg_keys_max, (uint64_t)(to - from) * join_topk_seg_units(n_tiles, span) * k);
        if ((uint64_t)join_topk_seg_units(n_tiles, span) * k > 0xFFFFFFFFull) {
            set_error(std::string(kName) + ": a segment beyond 2^32 keys (RF_JOIN_TOPK_UNITS forces too many units per row)");
            return RF_ERR_INVALID_ARG;
        }
    }
    uint64_t *d_seg = nullptr, *d_keys = nullptr;
    RF_HIP(sc.get(&d_seg, (size_t)seg_keys_max * sizeof(uint64_t)));
    RF_HIP(sc.get(&d_keys, fused.size() * (size_t)k * sizeof(uint64_t)));

    JoinTopkParams jp{};
    jp.s = plan0;
    jp.s.out = nullptr, jp.s.early = 0, jp.s.prefill_none = 0, jp.s.tile_step = 1, jp.s.len1 = 0, jp.s.tile_begin = 0, jp.s.tile_end = 0;
    jp.s.topk_k = k, jp.s.topk_desc = op == RF_OP_SIMILARITY, jp.s.key_index_base = 0;  // (index_base is added on the host, in 64 bits; topk_desc is not read under norm)
    jp.norm = norm ? 1u : 0u;
    jp.tables = jb.d_tables;
    jp.k = k;
    jp.no_self = (flags & RF_JOIN_NO_SELF) ? 1u : 0u;
    jp.seg = d_seg;

    hipError_t e = hipSuccess;
    for (size_t from = 0; from < fused.size() && e == hipSuccess; from += jb.B) {
        const size_t to = std::min(fused.size(), from + jb.B);
        const uint32_t bn = (uint32_t)(to - from);
        jp.span = join_topk_span(n_tiles, items_of(from, to), target, forced != 0);
        jp.seg_units = join_topk_seg_units(n_tiles, jp.span);
        jp.seg_cap = jp.seg_units * k;
        jp.batch = bn;
        // the tail: per table the units of its item
        e = jb.run(fused, from, to, n_tiles, jp.span, [&](std::vector<uint32_t>& blob) {
            const size_t at = blob.size();
            blob.resize(at + bn, 0u);
            for (const JoinList& l : jb.lists)
                for (size_t i = 0; i < l.items.size(); ++i)
                    for (uint32_t q = 0; q < l.items[i].members; ++q) blob[at + l.items[i].table0 + q] = l.prefix[i + 1] - l.prefix[i];
        }, st);
        if (e == hipSuccess) e = hipMemsetAsync(d_seg, 0xFF, (size_t)bn * jp.seg_cap * sizeof(uint64_t), st);
        for (int c = 0; c < 2 && e == hipSuccess; ++c) {
            if (jb.lists[c].items.empty()) continue;
            jp.items = jb.items(c);
            jp.prefix = jb.prefix(c);
            jp.n_items = (uint32_t)jb.lists[c].items.size(), jp.n_units = jb.lists[c].units();
            e = launch_join_topk(raw, c == 0, jp, jb.lists[c].items.data(), jb.lists[c].prefix.data(), st);
            *n_groups += jp.n_items;
            *n_units += jp.n_units;
        }
        jp.tab_units = jb.tail();
        jp.keys = d_keys + from * (size_t)k;
        if (e == hipSuccess) e = launch_join_topk_select(jp, st);
        ++*n_batches;
    }
    if (jb.outgrew) return jb.outgrew_status(kName, st);
    keys->assign(fused.size() * (size_t)k, ~0ull);
    if (e == hipSuccess) e = copy_home(keys->data(), d_keys, keys->size() * sizeof(uint64_t), st);
    else (void)hipStreamSynchronize(st);
    if (e != hipSuccess) return join_hip_status(kName, "device road", e);
    return RF_OK;
}

// One row of the answer before the bases: local indices, best first
template <class Score>
struct TopkRow {
    std::vector<Score> score;
    std::vector<uint64_t> index;
};
// the per-query road over the positions `rest` of Q: rf_topk_u32 / rf_topk_f64 of every row.  RF_JOIN_NO_SELF: k + 1 are asked for and the entry of the row's own
// index is dropped, or the last one if it is not among them
template <class Score>
rf_status join_topk_per_query(rf_metric metric, const rf_corpus* queries, const std::vector<uint32_t>& qidx, const std::vector<uint32_t>& rest, const rf_corpus* corpus, rf_op op,
                              const rf_args* args, uint32_t flags, uint32_t k, void* stream, std::vector<TopkRow<Score>>* rows)
{
    const bool no_self = (flags & RF_JOIN_NO_SELF) != 0;
    const uint32_t ask = (uint32_t)std::min<uint64_t>((uint64_t)k + (no_self ? 1 : 0), std::max<uint64_t>(corpus->n, 1));  // (a row has at most n entries)
    std::vector<Score> score(ask);
    std::vector<uint64_t> index(ask);
    return for_each_row_comparator(metric, queries, qidx, rest, stream, [&](uint32_t pos, const rf_comparator* c) {
        uint32_t count = 0;
        const rf_status s = JoinTopkScore<Score>::topk(c, corpus, op, args, ask, score.data(), index.data(), &count, stream);
        if (s != RF_OK) return s;
        TopkRow<Score>& r = (*rows)[pos];
        for (uint32_t i = 0; i < count; ++i) {
            if (no_self && index[i] == qidx[pos]) continue;
            if (r.score.size() == k) break;
            r.score.push_back(score[i]), r.index.push_back(index[i]);
        }
        return (rf_status)RF_OK;
    });
}

template <class Score>
rf_status join_topk_call(rf_metric metric, const rf_corpus* queries, const uint64_t* query_indices, uint64_t m, const rf_corpus* corpus, rf_op op, const rf_args* args_in, uint32_t flags,
                         uint32_t k, uint64_t index_base, Score* out_score, uint64_t* out_index, uint32_t* out_count, void* stream)
{
    using JS = JoinTopkScore<Score>;
    static constexpr const char* kName = JS::kName;
    if (const rf_status s = check_join_topk_args(kName, JS::kF64, metric, queries, corpus, op, args_in, flags, k); s != RF_OK) return s;
    if (m == 0) return RF_OK;  // (writes nothing)
    if (!out_score || !out_index || !out_count) {
        set_error(std::string(kName) + ": null output");
        return RF_ERR_INVALID_ARG;
    }
    const rf_args args_v = sanitized_args(args_in, false);
    const rf_args* args = &args_v;

    // ---- the corpora
    std::vector<uint32_t> qidx;
    if (const rf_status s = join_rows(kName, queries, corpus, query_indices, m, &qidx); s != RF_OK) return s;
    if (queries->n == 0 || corpus->n == 0) {
        std::fill(out_count, out_count + m, 0u);
        return RF_OK;
    }
    if (queries->device != corpus->device) {
        set_error(std::string(kName) + ": the two corpora are on different devices");
        return RF_ERR_INVALID_ARG;
    }
    hipStream_t st = (hipStream_t)stream;

    JoinPlanned pl;
    std::vector<uint64_t> keys;  // [fused rows, sorted][k]
    std::vector<uint32_t> rest;  // positions of Q for the per-query road
    uint32_t n_batches = 0, n_groups = 0;
    uint64_t n_units = 0;
    const bool device_metric = metric == RF_LEVENSHTEIN || metric == RF_INDEL || metric == RF_LCS_SEQ || (JS::kF64 && metric == RF_FUZZ_RATIO);
    JoinXlat xl;  // (lives to the end of the call: uploads read it)
    if (sw_join() && device_metric && k <= (uint32_t)kWave && join_xlat_of(queries, corpus, &xl)) {
        DeviceGuard guard(corpus->device);
        if (!guard.ok) {
            set_error("cannot select the corpus' device");
            return RF_ERR_NO_DEVICE;
        }
        ScratchSet sc(st);
        TakeParams tp;
        std::vector<uint32_t> lens, flagged;
        if (const rf_status s = join_lengths(kName, queries, xl, qidx, sc, st, &tp, &lens, &flagged); s != RF_OK) return s;
        // (what rf_topk_multi_u32 / rf_topk_multi_f64 fuse: no early-out -- no cutoff or a loose one -- and one kernel family, finishing and factor for the whole
        // launch; by f64 score also norm_key_fits, PER ROW: the maximum grows with the row's length, so over one corpus shorter rows may fuse while longer ones go
        // per query)
        // ASSUMPTION: for these metrics (the fuzz ratio is its inner metric's normalized similarity in plan()) finish, factor and op follow from the metric, the
        // weights and the op -- not from the row's length -- so the first accepted length's key is every accepted length's.  Should a length ever plan to another
        // key, its rows are still answered (per query, counted in the plan line's per_query); if that length could be the common one, pick the majority key here
        // instead of the first.
        bool have_first = false;
        MultiGroupKey first{};
        auto fusable = [&](const ScanParams& p, RawKind raw) {
            if (p.early || (p.out_f64 != 0) != JS::kF64) return false;
            if (JS::kF64 && !norm_key_fits(p.fin_mS, p.fin_mM, p.len1, corpus->max_len)) return false;
            const MultiGroupKey key{raw, p.finish, p.factor, p.op, false};
            if (!have_first) first = key, have_first = true;
            return key == first;
        };
        if (const rf_status s = join_plan_rows(metric, corpus, op, args, JS::kF64, qidx, lens, flagged, fusable, &pl, &rest); s != RF_OK) return s;
        if (!pl.fused.empty())
            if (const rf_status s = join_topk_device(kName, JS::kF64, pl.raw0, pl.plan0, queries, corpus, xl, pl.fused, tp.row_slot, tp.row_len, op, flags, k, sc, st, &keys, &n_batches,
                                                     &n_groups, &n_units);
                s != RF_OK)
                return s;
    } else {
        rest.resize((size_t)m);
        std::iota(rest.begin(), rest.end(), 0u);
    }
    if (sw_trace_plan())
        std::fprintf(stderr, "[rf plan] %s: m=%llu k=%u batches=%u groups=%u units=%llu per_query=%zu\n", JS::kTrace, (unsigned long long)m, k, n_batches, n_groups,
                     (unsigned long long)n_units, rest.size());
    std::vector<TopkRow<Score>> rows(rest.empty() ? 0 : (size_t)m);
    if (!rest.empty())
        if (const rf_status s = join_topk_per_query<Score>(metric, queries, qidx, rest, corpus, op, args, flags, k, stream, &rows); s != RF_OK) return s;

    // ---- decode as rf_topk_multi_u32 / rf_topk_multi_f64 do (the f64 rows by the very function: decode_norm_keys), widen, write
    for (size_t i = 0; i < pl.fused.size(); ++i) {
        const size_t j = pl.fused[i].pos;
        const uint64_t* best = keys.data() + i * (size_t)k;
        if constexpr (JS::kF64) {
            out_count[j] = decode_norm_keys(best, k, metric, op, index_base, out_score + j * k, out_index + j * k);
        } else {
            const bool desc = op == RF_OP_SIMILARITY;
            uint32_t c = 0;
            for (; c < k && best[c] != ~0ull; ++c) {
                const uint32_t hi = (uint32_t)(best[c] >> 32);
                out_score[j * k + c] = desc ? ~hi : hi;
                out_index[j * k + c] = index_base + (uint32_t)best[c];
            }
            out_count[j] = c;
        }
    }
    for (uint32_t j : rest) {
        const TopkRow<Score>& r = rows[j];
        for (size_t c = 0; c < r.score.size(); ++c) {
            out_score[(size_t)j * k + c] = r.score[c];
            out_index[(size_t)j * k + c] = index_base + r.index[c];
        }
        out_count[j] = (uint32_t)r.score.size();
    }
    return RF_OK;
}
}  // namespace

extern "C" {

rf_status rf_join_u32(rf_metric metric, const rf_corpus* queries, const uint64_t* query_indices, uint64_t m, const rf_corpus* corpus, rf_op op, const rf_args* args_in,
                      uint32_t flags, uint64_t query_base, uint64_t index_base, uint64_t capacity, uint64_t* out_query, uint64_t* out_index, uint32_t* out_score,
                      uint64_t* out_count, rf_join_order order, void* stream)
try {
    return join_call<uint32_t>(metric, queries, query_indices, m, corpus, op, args_in, flags, query_base, index_base, capacity, out_query, out_index, out_score, out_count, order, stream);
}
RF_ABI_CATCH

// The same call by f64 score: the normalized ops of the usize metrics, fuzz ratio's two similarity ops, every op of jaro / jaro_winkler, under args->cutoff_f64
rf_status rf_join_f64(rf_metric metric, const rf_corpus* queries, const uint64_t* query_indices, uint64_t m, const rf_corpus* corpus, rf_op op, const rf_args* args_in,
                      uint32_t flags, uint64_t query_base, uint64_t index_base, uint64_t capacity, uint64_t* out_query, uint64_t* out_index, double* out_score,
                      uint64_t* out_count, rf_join_order order, void* stream)
try {
    return join_call<double>(metric, queries, query_indices, m, corpus, op, args_in, flags, query_base, index_base, capacity, out_query, out_index, out_score, out_count, order, stream);
}
RF_ABI_CATCH

// The k best candidates for every row of Q: row j is rf_topk_u32 of a comparator over row Q[j]
rf_status rf_join_topk_u32(rf_metric metric, const rf_corpus* queries, const uint64_t* query_indices, uint64_t m, const rf_corpus* corpus, rf_op op, const rf_args* args_in,
                           uint32_t flags, uint32_t k, uint64_t index_base, uint32_t* out_score, uint64_t* out_index, uint32_t* out_count, void* stream)
try {
    return join_topk_call<uint32_t>(metric, queries, query_indices, m, corpus, op, args_in, flags, k, index_base, out_score, out_index, out_count, stream);
}
RF_ABI_CATCH

// The same call by f64 score: row j is rf_topk_f64 of a comparator over row Q[j]
rf_status rf_join_topk_f64(rf_metric metric, const rf_corpus* queries, const uint64_t* query_indices, uint64_t m, const rf_corpus* corpus, rf_op op, const rf_args* args_in,
                           uint32_t flags, uint32_t k, uint64_t index_base, double* out_score, uint64_t* out_index, uint32_t* out_count, void* stream)
try {
    return join_topk_call<double>(metric, queries, query_indices, m, corpus, op, args_in, flags, k, index_base, out_score, out_index, out_count, stream);
}
RF_ABI_CATCH

}  // extern "C"

// rf_api_join.hip -- rf_join_u32 / rf_join_f64: the (query, candidate, score) triples of two packed corpora within a cutoff.  ONE body for both score types
// (join_call<Score>: uint32_t -- distance / similarity of the usize metrics -- or double -- the normalized ops, fuzz ratio, jaro / jaro_winkler); what differs is
// JoinScore<Score> -- the entry point's name and trace prefix, whether plan() is asked for f64, which rf_filter_* the per-query road calls, which score buffer the
// kernel fills -- and the `f64` arm of check_join_args: the accepted (metric, op) pairs and where the cutoff sits.
// Two roads:
//   device      both corpora hold bytes, the metric and weights plan to a fused recurrence (fusable_base), the row has <= 64 symbols and its plan is `early`:
//               the rows' lengths come home (4 bytes per row, never a symbol), plan() runs once per distinct length -- a byte query reaches its plan through its
//               length alone -- the fusable rows are sorted by length and cut into batches; per batch one join_pm_kernel builds the tables out of the query
//               corpus' payload and one join_kernel per class (narrow / wide) that occurs walks the batch's work list (rf_join_plan.hpp, rf_join.hip).  One
//               64-bit counter and one triple buffer serve the whole call; they come home once, after the last batch.
//               rf_join_f64 plans with f64_out (a fuzz ratio becomes the normalized similarity of its inner metric in plan()) and the kernel stores the double
//               itself: no 32-bit key is ordered, so no maximum of the corpus is too large.
//   per query   every other row: rf_corpus_take[_u32] of the row, rf_comparator_new[_u32], rf_filter_u32 / rf_filter_f64, append.  Plain host code, slow by design, total.
// Ordering, the 64-bit bases and the writes happen on the host at the very end: a call that fails has written nothing.
// Product code: never includes or links anything from oracle/.
#include <numeric>

#include "rf_host.hpp"

#include "rf_join_plan.hpp"
#include "rf_take_addr.hpp"

// (both calls read the two switches through these)
// A/B switch: 0 sends every row down the per-query road (identical results)
static bool sw_join() { static const bool v = env_on("RF_JOIN"); return v; }
// most queries of a device batch (the batch's tables are 2 KiB of scratch per query)
static uint32_t sw_join_batch() { static const uint32_t v = (uint32_t)std::max<long long>(1, std::min<long long>(env_int("RF_JOIN_BATCH", 16384), 1 << 20)); return v; }

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

// the device road over the rows `fused` (sorted): triples of the first `cap` pairs to arrive into `out`, the true number of pairs into *total
template <class Score>
rf_status join_device(RawKind raw, const ScanParams& plan0, const rf_corpus* queries, const rf_corpus* corpus, const std::vector<JoinQuery>& fused, const uint32_t* d_row_slot,
                      const uint32_t* d_row_len, uint32_t flags, uint64_t cap, ScratchSet& sc, hipStream_t st, std::vector<Triple<Score>>* out, uint64_t* total, uint32_t* n_batches,
                      uint32_t* n_groups)
{
    const uint32_t B = sw_join_batch();
    const size_t max_batch = std::min<size_t>(B, fused.size());
    // per-call device state: [counter | inverse sigma of the query corpus], the triple buffer, and per-batch scratch bounded by the batch
    uint8_t* d_ctl = nullptr;
    RF_HIP(sc.get(&d_ctl, 512));
    unsigned long long* d_count = reinterpret_cast<unsigned long long*>(d_ctl);
    uint8_t inv[256];
    take_inverse_sigma(queries->sigma, inv);
    RF_HIP(hipMemsetAsync(d_ctl, 0, 256, st));
    RF_HIP(hipMemcpyAsync(d_ctl + 256, inv, 256, hipMemcpyHostToDevice, st));
    uint64_t* d_pairs = nullptr;
    Score* d_scores = nullptr;
    if (cap) {
        RF_HIP(sc.get(&d_pairs, cap * sizeof(uint64_t)));
        RF_HIP(sc.get(&d_scores, cap * sizeof(Score)));
    }
    uint64_t* d_tables = nullptr;
    RF_HIP(sc.get(&d_tables, max_batch * 256 * sizeof(uint64_t)));
    // a batch's upload: [rows | narrow items | wide items | narrow prefix | wide prefix] -- at most max_batch items and max_batch + 2 prefix entries
    const size_t blob_words = max_batch + max_batch * (sizeof(JoinItem) / 4) + max_batch + 2;
    uint32_t* d_blob = nullptr;
    RF_HIP(sc.get(&d_blob, blob_words * sizeof(uint32_t)));
    std::deque<std::vector<uint32_t>> blobs;  // the host side of every upload stays alive until the stream has drained

    JoinPmParams pm{};
    pm.s.data = queries->d_data;
    pm.s.tiles = queries->uniform ? nullptr : queries->d_tiles;
    pm.s.uniform_len = queries->uniform_len;
    pm.s.uniform_tile_bytes = (uint32_t)tile_bytes(queries->uniform_len);
    pm.n_slots = queries->uniform ? queries->n_tiles * (uint32_t)kWave : (uint32_t)queries->n_slots;
    pm.row_slot = d_row_slot, pm.row_len = d_row_len;
    pm.inv_sigma = d_ctl + 256;
    pm.sigma = corpus->d_sigma;
    pm.tables = d_tables;

    JoinParams jp{};
    jp.s = plan0;
    jp.s.out = nullptr, jp.s.prefill_none = 0, jp.s.tile_step = 1, jp.s.len1 = 0, jp.s.tile_begin = 0, jp.s.tile_end = 0;
    jp.span = kJoinSpan;
    jp.tables = d_tables;
    jp.count = d_count, jp.pairs = d_pairs, jp.cap = cap;
    JoinScore<Score>::bind(jp, d_scores);
    jp.upper = (flags & RF_JOIN_UPPER) ? 1u : 0u;

    hipError_t e = hipSuccess;
    for (size_t from = 0; from < fused.size() && e == hipSuccess; from += B) {
        const size_t to = std::min(fused.size(), from + B);
        const uint32_t bn = (uint32_t)(to - from);
        const JoinList lists[2] = {join_items(fused, from, to, true, corpus->n_tiles, kJoinSpan), join_items(fused, from, to, false, corpus->n_tiles, kJoinSpan)};
        blobs.emplace_back();
        std::vector<uint32_t>& blob = blobs.back();
        blob.reserve(blob_words);
        for (size_t i = from; i < to; ++i) blob.push_back(fused[i].pos);
        size_t items_at[2], prefix_at[2];
        for (int k = 0; k < 2; ++k) {
            items_at[k] = blob.size();
            const uint32_t* w = reinterpret_cast<const uint32_t*>(lists[k].items.data());
            blob.insert(blob.end(), w, w + lists[k].items.size() * (sizeof(JoinItem) / 4));
        }
        for (int k = 0; k < 2; ++k) {
            prefix_at[k] = blob.size();
            blob.insert(blob.end(), lists[k].prefix.begin(), lists[k].prefix.end());
        }
        if (blob.size() > blob_words) {
            set_error(std::string(JoinScore<Score>::kName) + ": internal error: a batch's work list outgrew its scratch");
            (void)hipStreamSynchronize(st);
            return RF_ERR_INVALID_ARG;
        }
        e = hipMemcpyAsync(d_blob, blob.data(), blob.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st);
        if (e != hipSuccess) break;
        pm.rows = d_blob, pm.batch = bn;
        e = launch_join_pm(pm, st);
        for (int k = 0; k < 2 && e == hipSuccess; ++k) {
            if (lists[k].items.empty()) continue;
            jp.items = reinterpret_cast<const JoinItem*>(d_blob + items_at[k]);
            jp.prefix = d_blob + prefix_at[k];
            jp.n_items = (uint32_t)lists[k].items.size(), jp.n_units = lists[k].units(), jp.batch = bn;
            e = launch_join(raw, k == 0, jp, lists[k].items.data(), lists[k].prefix.data(), st);
            *n_groups += jp.n_items;
        }
        ++*n_batches;
    }
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
    if (e != hipSuccess) {
        (void)hipGetLastError();
        set_error(std::string(JoinScore<Score>::kName) + ", device road: " + hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? RF_ERR_OOM : RF_ERR_HIP;
    }
    *total = count;
    return RF_OK;
}

// the per-query road over the positions `rest` of Q: appends while `out` has room below `capacity`, adds every match to *total
template <class Score>
rf_status join_per_query(rf_metric metric, const rf_corpus* queries, const std::vector<uint32_t>& qidx, const std::vector<uint32_t>& rest, const rf_corpus* corpus, rf_op op,
                         const rf_args* args, uint32_t flags, uint64_t capacity, void* stream, std::vector<Triple<Score>>* out, uint64_t* total)
{
    constexpr size_t kRows = 4096;  // rows taken out of the query corpus per call
    std::vector<uint64_t> want, offsets, index;
    std::vector<uint8_t> bytes;
    std::vector<uint32_t> elems;
    std::vector<Score> score;
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
            const uint32_t pos = rest[from + j];
            const size_t len = (size_t)(offsets[j + 1] - offsets[j]);
            ComparatorOwner c;
            s = queries->wide ? rf_comparator_new_u32(metric, elems.data() + offsets[j], len, &c.c) : rf_comparator_new(metric, bytes.data() + offsets[j], len, &c.c);
            if (s != RF_OK) return s;
            // every match of this query (the flag needs them all): a first room, then the true count's
            uint64_t room = std::max<size_t>(index.size(), 1024), count = 0;
            while (true) {
                index.resize(room), score.resize(room);
                s = JoinScore<Score>::filter(c.c, corpus, op, args, room, index.data(), score.data(), &count, stream);
                if (s != RF_OK) return s;
                if (count <= room) break;
                room = count;
            }
            for (uint64_t k = 0; k < count; ++k) {
                if ((flags & RF_JOIN_UPPER) && index[k] <= qidx[pos]) continue;
                ++*total;
                if (out->size() < capacity) out->push_back(Triple<Score>{pos, (uint32_t)index[k], score[k]});
            }
        }
    }
    return RF_OK;
}
// The argument errors of the two calls: before either corpus is looked at or a device is touched, and before anything is written
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
    if (!f64 && op != RF_OP_DISTANCE && op != RF_OP_SIMILARITY) return bad("op must be RF_OP_DISTANCE or RF_OP_SIMILARITY");
    if ((int)op < 0 || (int)op > (int)RF_OP_NORMALIZED_SIMILARITY) return bad("unknown op");
    if (flags & ~RF_JOIN_UPPER) return bad("unknown flag bit");
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
    if (f64 ? std::isnan(args_in->cutoff_f64) : args_in->cutoff_usize == RF_NO_CUTOFF) return bad("args must carry a score_cutoff (without one the answer is every pair)");
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
    auto bad = [](const char* why) {
        set_error(std::string(JS::kName) + ": " + why);
        return RF_ERR_INVALID_ARG;
    };
    if (m == 0) return RF_OK;  // (writes nothing)
    const rf_args args_v = sanitized_args(args_in, false);
    const rf_args* args = &args_v;

    // ---- the corpora
    if (queries->borrowed || corpus->borrowed) return bad("not a packed corpus");
    if (!query_indices && m != queries->n) return bad("query_indices == NULL asks for every row: m must be rf_corpus_count(queries)");
    if (m > 0xFFFFFFFEull) return bad("more than 2^32 - 2 queries in one call");
    std::vector<uint32_t> qidx((size_t)m);
    if (query_indices) {
        for (size_t j = 0; j < (size_t)m; ++j) {
            if (query_indices[j] >= queries->n) return bad("a query index lies beyond rf_corpus_count(queries)");
            qidx[j] = (uint32_t)query_indices[j];
        }
    } else {
        std::iota(qidx.begin(), qidx.end(), 0u);
    }
    if (queries->n == 0 || corpus->n == 0) {
        *out_count = 0;
        return RF_OK;
    }
    if (queries->device != corpus->device) return bad("the two corpora are on different devices");
    hipStream_t st = (hipStream_t)stream;

    std::vector<Triple<Score>> triples;
    uint64_t total = 0;
    std::vector<uint32_t> rest;  // positions of Q for the per-query road
    uint32_t n_batches = 0, n_groups = 0;
    const bool device_metric = metric == RF_LEVENSHTEIN || metric == RF_INDEL || metric == RF_LCS_SEQ || (JS::kF64 && metric == RF_FUZZ_RATIO);
    if (sw_join() && device_metric && !queries->wide && !corpus->wide) {
        DeviceGuard guard(corpus->device);
        if (!guard.ok) {
            set_error("cannot select the corpus' device");
            return RF_ERR_NO_DEVICE;
        }
        ScratchSet sc(st);
        // the rows' slots and lengths (take_rows_len_kernel); the lengths come home
        TakeParams tp{};
        tp.s.data = queries->d_data;
        tp.s.tiles = queries->uniform ? nullptr : queries->d_tiles;
        tp.s.uniform_len = queries->uniform_len;
        tp.s.uniform_tile_bytes = (uint32_t)tile_bytes(queries->uniform_len);
        tp.n_slots = queries->uniform ? queries->n_tiles * (uint32_t)kWave : (uint32_t)queries->n_slots;
        uint32_t* d_idx = nullptr;
        RF_HIP(sc.get(&d_idx, (size_t)m * sizeof(uint32_t)));
        RF_HIP(sc.get(&tp.row_slot, (size_t)m * sizeof(uint32_t)));
        RF_HIP(sc.get(&tp.row_len, (size_t)m * sizeof(uint32_t)));
        if (!queries->uniform)
            if (const rf_status s = corpus_take_slot_of(queries, st, &tp.slot_of); s != RF_OK) return s;
        std::vector<uint32_t> lens((size_t)m);
        hipError_t e = hipMemcpyAsync(d_idx, qidx.data(), (size_t)m * sizeof(uint32_t), hipMemcpyHostToDevice, st);
        tp.idx = d_idx, tp.m = m;
        if (e == hipSuccess) e = launch_take_rows_len(tp, st);
        if (e == hipSuccess) e = copy_home(lens.data(), tp.row_len, (size_t)m * sizeof(uint32_t), st);
        else (void)hipStreamSynchronize(st);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            set_error(std::string(JS::kName) + ", query lengths: " + hipGetErrorString(e));
            return e == hipErrorOutOfMemory ? RF_ERR_OOM : RF_ERR_HIP;
        }
        // one plan per distinct length: plan() reads of a byte comparator its metric and its length (the query's head and bytes only for kernels no fused road runs)
        struct LenPlan {
            bool planned = false, fusable = false;
            uint32_t tile_begin = 0, tile_end = 0;
        };
        LenPlan by_len[kJoinMaxLen + 1];
        ScanParams plan0{};
        RawKind raw0 = RAW_LEV;
        bool have_plan0 = false;
        std::vector<JoinQuery> fused;
        for (size_t j = 0; j < (size_t)m; ++j) {
            const uint32_t len = lens[j];
            if (len > kJoinMaxLen) {
                rest.push_back((uint32_t)j);
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
                const rf_status s = plan(&probe, corpus, op, args, JS::kF64, &p, &raw);
                if (s == RF_ERR_UNSUPPORTED) return s;
                if (s == RF_OK && fusable_base(raw, 1, p.long_words_pad) && p.early && p.has_cutoff && !p.band) {
                    lp.fusable = true;
                    lp.tile_begin = p.tile_begin, lp.tile_end = std::min(p.tile_end, corpus->n_tiles);
                    if (lp.tile_begin >= lp.tile_end) lp.tile_begin = lp.tile_end = 0;
                    if (!have_plan0) plan0 = p, raw0 = raw, have_plan0 = true;
                }
            }
            if (lp.fusable)
                fused.push_back(JoinQuery{len, (uint32_t)j, qidx[j], lp.tile_begin, lp.tile_end});
            else
                rest.push_back((uint32_t)j);
        }
        if (!fused.empty()) {
            join_sort(fused);
            const uint64_t cap = std::min<uint64_t>(capacity, (uint64_t)fused.size() * corpus->n);
            if (const rf_status s = join_device(raw0, plan0, queries, corpus, fused, tp.row_slot, tp.row_len, flags, cap, sc, st, &triples, &total, &n_batches, &n_groups); s != RF_OK)
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

}  // extern "C"

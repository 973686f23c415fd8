// rf_api_filter_multi.hip -- rf_filter_multi_u32 / rf_filter_multi_f64: the (index, score) pairs within the cutoff of each of q queries, fusable queries 4
// (then 2) to a pass over the corpus (rf_filter_multi.hip), every other query through rf_filter_u32 / rf_filter_f64 (rf_host.hpp has the shared declarations).
// Product code: never includes or links anything from oracle/.
#include <algorithm>

#include "rf_host.hpp"

#include "rf_filter_multi_rows.hpp"

extern "C" {

constexpr size_t kHeadPlaneWins = size_t(1) << 25;  // candidates of a single-length corpus from which small-cutoff Levenshtein queries go per query (see head_plane_wins below)
constexpr size_t kHeadPlaneWinsF64 = size_t(3) << 23;  // the same for the f64 plans of rf_filter_multi_f64 (25.2 M: see head_plane_wins below)
// A/B switch: 0 sends every query down the per-query road (identical results)
static bool sw_filter_multi() { static const bool v = env_on("RF_FILTER_MULTI"); return v; }
// A/B switch of the f64 planner: 0 fuses every fusable query of rf_filter_multi_f64, also the shapes its measured routing rules send per query
static bool sw_filter_multi_f64_route() { static const bool v = env_on("RF_FILTER_MULTI_F64_ROUTE"); return v; }

// The one shape the fused road lost (tools/bench_filter_multi.py, profiles/filter_multi.txt): Levenshtein under a small cutoff over a LARGE single-length
// corpus, where rf_filter_u32 takes its first look from the 8-byte head plane and compacts lanes (6-8 B per pair, 8 columns) while a fused group reads
// the payload's 16-byte first chunk: 100 M x 64, cutoff 3, 16 / 256 queries 5.67 / 89.5 ms fused against 3.00 / 53.7 ms per query; at 10 M the fused
// road still wins (0.92 / 14.1 against 1.64 / 23.9 ms).  Between the two sizes the boundary is interpolated from those four times (fixed cost + slope of
// either road: about 2^25 candidates for a group of four); the one size measured beside it, 30 M, is level at 16 queries and 1.10 x at 256
// (profiles/filter_multi_copy.txt).  A query whose length window is empty stays fused: it launches nothing.
// The f64 plans (tools/bench_filter_multi_f64.py, profiles/filter_multi_f64.txt; 16 / 256 queries of 64 symbols): rf_filter_f64 takes the same head-plane road
// for such a query -- first_check <= 8 is normalized_similarity >= 0.95 over 64-symbol candidates, and RF_TRACE_PLAN shows heads8=1 for its scans -- and the
// fused road, which also pays an f64 division per look, falls behind EARLIER.  normalized_similarity >= 0.95, fused (RF_FILTER_MULTI_F64_ROUTE=0) against the loop: 20 M
// 1.39 / 20.4 ms against 1.93 / 27.0 (1.39 / 1.33 x), 24 M 1.65 / 24.2 against 1.72 / 30.6 (1.04 / 1.27 x; second run 1.12 / 1.13 x), 30 M 2.02 / 30.0 against
// 1.98 / 32.5 (0.98 / 1.08 x; first session 0.96 / 1.03 x: at 16 queries the fused road LOSES), 100 M 6.24 / 96.9 against 3.02 / 49.7 (0.48 / 0.51 x).  So the
// boundary sits between the last size where both query counts win by more than the spread, 24 M, and the first where one loses, 30 M: 3 x 2^23 = 25.2 M.
// A cutoff whose first look comes later (normalized_similarity >= 0.9: first_check 10, no head plane per query) stays fused at every size: 100 M 8.58 / 135.9 ms
// against 11.01 / 172.2 (1.28 / 1.27 x).
static bool head_plane_wins(const ScanParams& p, RawKind raw, const rf_corpus* corpus, bool norm)
{
    return raw == RAW_LEV && corpus->uniform && corpus->n >= (norm ? kHeadPlaneWinsF64 : kHeadPlaneWins) && p.first_check <= 8 && p.tile_begin < p.tile_end && (!norm || sw_filter_multi_f64_route());
}

// ... and the argument checks of the two: everything is decided before the corpus is looked at or a device is touched, and before anything is written
static rf_status check_filter_multi_args(const char* fn, bool f64, const rf_comparator* const* cs, uint32_t q, const rf_corpus* corpus, rf_op op, const rf_args* args_in,
                                         uint64_t capacity, const uint64_t* out_index, const void* out_score, const uint64_t* out_count, rf_filter_order order, rf_args* args)
{
    const std::string name(fn);
    if (!cs || !corpus || !args_in || !out_count) {
        set_error(name + ": null handle, args or count");
        return RF_ERR_INVALID_ARG;
    }
    if (capacity && (!out_index || !out_score)) {
        set_error(name + ": null output with a non-zero capacity");
        return RF_ERR_INVALID_ARG;
    }
    if ((int)order < 0 || (int)order > (int)RF_FILTER_ANY) {
        set_error(name + ": unknown order");
        return RF_ERR_INVALID_ARG;
    }
    const std::string usize_only = name + ": usize-valued metrics only (jaro / jaro_winkler / fuzz ratio: rf_filter_f64)";
    if (const rf_status s = check_multi_members(fn, f64, usize_only.c_str(), cs, q, op); s != RF_OK) return s;
    *args = sanitized_args(args_in, false);
    return RF_OK;
}

// What rf_filter_multi_u32 and rf_filter_multi_f64 share, after their argument checks: plan every query (a refusal comes before a count is written), run the fused
// groups and bring their counters and key rows home.  `norm` (rf_filter_multi_f64): f64-valued plans and the normalized kernels.  Fused: plans under a tight cutoff
// (`early`), but for the shapes head_plane_wins() sends per query.
struct FusedFilter {
    MultiPlan plan;
    uint32_t seg_cap = 0;                       // keys a row can hold: min(capacity, n)
    // the results at home.  Row r = the r-th fused member in group order: count(r) is its true number of matches, keys(r) its first min(count, seg_cap) keys in
    // the order of arrival -- (score, ~score or norm_key) << 32 | local index
    std::vector<uint8_t> home;
    std::vector<uint64_t> big;  // (the two-step road: [fused][width], width = the longest list held)
    size_t ctl_bytes = 0, width = 0;
    bool one_copy = true;
    uint32_t count(uint32_t r) const { return reinterpret_cast<const uint32_t*>(home.data())[(size_t)r * kFilterMultiLine32]; }
    uint64_t* keys(uint32_t r) { return one_copy ? reinterpret_cast<uint64_t*>(home.data() + ctl_bytes) + (size_t)r * seg_cap : big.data() + (size_t)r * width; }
};
static rf_status filter_multi_fused(bool norm, const rf_comparator* const* cs, uint32_t q, const rf_corpus* corpus, rf_op op, const rf_args* args, uint64_t capacity,
                                    uint64_t* out_count, hipStream_t st, FusedFilter* out)
{
    MultiPlan& mp = out->plan;
    if (corpus->n != 0)
        if (const rf_status s = plan_multi(MultiAsk{norm, true, sw_filter_multi(), head_plane_wins}, cs, q, corpus, op, args, &mp); s != RF_OK) return s;
    for (uint32_t i = 0; i < q; ++i) out_count[i] = 0;
    if (corpus->n == 0) return RF_OK;
    const std::vector<ScanParams>& ps = mp.ps;
    const std::vector<std::vector<uint32_t>>& groups = mp.g.groups;
    const uint32_t fused = mp.fused;
    mp.trace(norm ? "filter_multi_f64" : "filter_multi", "", "");

    // ---- the fused groups: everything enqueued, then the results home
    const uint32_t seg_cap = out->seg_cap = (uint32_t)std::min<uint64_t>(capacity, corpus->n);
    if (fused) {
        DeviceGuard guard(corpus->device);
        if (!guard.ok) {
            set_error("cannot select the corpus' device");
            return RF_ERR_NO_DEVICE;
        }
        ScratchSet sc(st);
        // one block: [fused counter lines | fused segments of seg_cap keys], row r = the r-th fused member in group order
        constexpr size_t kLine = kFilterMultiLine32 * sizeof(uint32_t);
        constexpr size_t kOneCopyBytes = 256u << 10;
        const size_t ctl_bytes = out->ctl_bytes = (size_t)fused * kLine, seg_bytes = (size_t)fused * seg_cap * sizeof(uint64_t);
        uint8_t* block = nullptr;
        RF_HIP(sc.get(&block, ctl_bytes + seg_bytes));
        uint32_t* d_count = reinterpret_cast<uint32_t*>(block);
        uint64_t* d_cand = reinterpret_cast<uint64_t*>(block + ctl_bytes);
        hipError_t e = hipMemsetAsync(d_count, 0, ctl_bytes, st);
        rf_status status = RF_OK;
        uint32_t row = 0;
        for (const auto& g : groups) {
            if (e != hipSuccess) break;
            const uint32_t i = g[0];
            FilterMultiParams fp{};
            fp.s = ps[i];
            ScanParams& p = fp.s;
            p.out = nullptr, p.prefill_none = 0, p.tile_step = 1;
            p.multi_q = (uint32_t)g.size();
            p.topk_desc = op == RF_OP_SIMILARITY;  // (not read under norm: both normalized ops store the ascending norm_key)
            fp.norm = norm ? 1u : 0u;
            // the union of the members' length windows (plan(): a member's tiles outside its own are None by their length alone; an empty window: tile_begin == tile_end)
            uint32_t t0 = corpus->n_tiles, t1 = 0;
            for (size_t m = 0; m < g.size() && status == RF_OK; ++m) {
                const ScanParams& pm = ps[g[m]];
                p.multi_len1[m] = pm.len1;
                if (pm.tile_begin < pm.tile_end) t0 = std::min(t0, pm.tile_begin), t1 = std::max(t1, std::min(pm.tile_end, corpus->n_tiles));
                status = comparator_device_pm(mp.eff[g[m]], corpus->device, &p.multi_pm[m]);
            }
            if (status != RF_OK) break;
            p.tile_begin = t0, p.tile_end = std::max(t0, t1);
            fp.count = d_count + (size_t)row * kFilterMultiLine32;
            fp.cand = seg_cap ? d_cand + (size_t)row * seg_cap : nullptr;
            fp.seg_cap = seg_cap;
            e = launch_filter_multi(mp.raws[i], p.len1 <= 32, fp, st);
            row += (uint32_t)g.size();
        }
        std::vector<uint8_t>& home = out->home;
        std::vector<uint64_t>& big = out->big;
        size_t& width = out->width = seg_cap;
        const bool one_copy = out->one_copy = seg_bytes <= kOneCopyBytes;
        if (status == RF_OK && e == hipSuccess) {
            home.resize(one_copy ? ctl_bytes + seg_bytes : ctl_bytes);
            e = copy_home(home.data(), block, home.size(), st);
            if (e == hipSuccess && !one_copy) {
                // the counters say how much of the segments is filled: the first `width` keys of EVERY segment in one strided copy, whatever the number of rows
                width = 0;
                for (uint32_t r = 0; r < fused; ++r)
                    width = std::max<size_t>(width, std::min(reinterpret_cast<const uint32_t*>(home.data())[(size_t)r * kFilterMultiLine32], seg_cap));
                if (width) {
                    big.resize((size_t)fused * width);
                    e = hipMemcpy2DAsync(big.data(), width * sizeof(uint64_t), d_cand, (size_t)seg_cap * sizeof(uint64_t), width * sizeof(uint64_t), fused,
                                         hipMemcpyDeviceToHost, st);
                    const hipError_t es = hipStreamSynchronize(st);
                    if (e == hipSuccess) e = es;
                }
            }
        } else {
            (void)hipStreamSynchronize(st);
        }
        if (status != RF_OK) return status;
        if (e != hipSuccess) {
            (void)hipGetLastError();
            set_error(std::string("filter, fused queries: ") + hipGetErrorString(e));
            return e == hipErrorOutOfMemory ? RF_ERR_OOM : RF_ERR_HIP;
        }
    }
    return RF_OK;
}

// Row j is rf_filter_u32(cs[j], ..., RF_MEM_HOST, order, ...).  Queries are planned as rf_topk_multi_u32 plans them and grouped under its rules (filter_multi_fused), with ONE
// difference: here a query is fused when plan() set `early` -- the cutoff is tight -- and goes per query when it did not.  Under a tight cutoff nearly every
// tile dies for all members at the first look, the rare passer costs one atomic per tile and member, and the compact lists need no n-entry vector; without one
// (or under a loose one) every candidate would be appended and rf_filter_u32's scan + compaction is the better road.  OSA, Damerau-Levenshtein, general weight
// tables, queries beyond 64 symbols, u32 queries with overflow-class symbols and the odd one left over take rf_filter_u32 itself.
// A call: one memset of the members' counters, one scan per fused group into the group's counters and segments, then the results home -- counters and segments
// in ONE copy while the segments are small (kOneCopyBytes), else the counters first and then the filled part of all segments in one strided copy -- and the ordering
// and widening (index_base in 64 bits) on the host: the lists are short by construction.  All scratch is the call's own (ScratchSet): nothing of the corpus'
// per-stream caches is leased.
rf_status rf_filter_multi_u32(const rf_comparator* const* cs, uint32_t q, const rf_corpus* corpus, rf_op op, const rf_args* args_in, uint64_t index_base,
                              uint64_t capacity, uint64_t* out_index, uint32_t* out_score, uint64_t* out_count, rf_filter_order order, void* stream)
try {
    rf_args args_v;
    const rf_args* args = &args_v;
    if (const rf_status s = check_filter_multi_args("rf_filter_multi_u32", false, cs, q, corpus, op, args_in, capacity, out_index, out_score, out_count, order, &args_v); s != RF_OK) return s;
    if (q == 0) return RF_OK;
    FusedFilter fz;
    if (const rf_status s = filter_multi_fused(false, cs, q, corpus, op, args, capacity, out_count, (hipStream_t)stream, &fz); s != RF_OK) return s;
    if (corpus->n == 0) return RF_OK;
    // order and decode as rf_filter_u32 does: by index ascending, or best score first with ties by index (a plain sort of the keys)
    {
        const bool desc = op == RF_OP_SIMILARITY;
        uint32_t row = 0;
        for (const auto& g : fz.plan.g.groups)
            for (uint32_t j : g) {
                const uint32_t r = row++;
                const uint32_t count = fz.count(r), have = std::min(count, fz.seg_cap);
                uint64_t* keys = fz.keys(r);
                if (order == RF_FILTER_BY_SCORE)
                    std::sort(keys, keys + have);
                else if (order == RF_FILTER_BY_INDEX)
                    std::sort(keys, keys + have, [](uint64_t a, uint64_t b) { return (uint32_t)a < (uint32_t)b; });
                for (uint32_t m = 0; m < have; ++m) {
                    const uint32_t hi = (uint32_t)(keys[m] >> 32);
                    out_index[(size_t)j * capacity + m] = index_base + (uint32_t)keys[m];
                    out_score[(size_t)j * capacity + m] = desc ? ~hi : hi;
                }
                out_count[j] = count;
            }
    }

    // ---- everything else: the single-query filter, one call per query
    for (uint32_t j = 0; j < q; ++j) {
        if (fz.plan.g.taken[j]) continue;
        const rf_status s = rf_filter_u32(cs[j], corpus, op, args, index_base, capacity, capacity ? out_index + (size_t)j * capacity : nullptr,
                                          capacity ? out_score + (size_t)j * capacity : nullptr, out_count + j, RF_MEM_HOST, order, stream);
        if (s != RF_OK) return s;
    }
    return RF_OK;
}
RF_ABI_CATCH

// Row j is rf_filter_f64(cs[j], ..., RF_MEM_HOST, order, ...): the same pairs, the same doubles bit for bit, in the same order.  The grouping is
// rf_filter_multi_u32's with the f64-valued plans -- plan() sets `early` from the f64 cutoff: a normalized distance below 0.7 (Levenshtein) / 0.4 (LCS family) still
// allowed -- and, as in rf_topk_multi_f64, a fusable query must keep every maximum of its scan within 65535: the kernel keeps or drops a candidate by emit_fin's
// own f64 compare and stores norm_key(dist, maximum) (rf_norm_key.hpp), which the host orders and turns back into the double (rf_filter_multi_rows.hpp).  jaro /
// jaro_winkler, OSA, Damerau-Levenshtein, general weight tables, queries beyond 64 symbols, no cutoff (NaN) or a loose one, a maximum beyond 65535 and the odd one
// left over take rf_filter_f64 itself.
rf_status rf_filter_multi_f64(const rf_comparator* const* cs, uint32_t q, const rf_corpus* corpus, rf_op op, const rf_args* args_in, uint64_t index_base,
                              uint64_t capacity, uint64_t* out_index, double* out_score, uint64_t* out_count, rf_filter_order order, void* stream)
try {
    rf_args args_v;
    const rf_args* args = &args_v;
    if (const rf_status s = check_filter_multi_args("rf_filter_multi_f64", true, cs, q, corpus, op, args_in, capacity, out_index, out_score, out_count, order, &args_v); s != RF_OK) return s;
    if (q == 0) return RF_OK;
    FusedFilter fz;
    if (const rf_status s = filter_multi_fused(true, cs, q, corpus, op, args, capacity, out_count, (hipStream_t)stream, &fz); s != RF_OK) return s;
    if (corpus->n == 0) return RF_OK;
    // order and decode (rf_filter_multi_rows.hpp); which value a member returns is its plan's op (a fuzz ratio: the similarity)
    uint32_t row = 0;
    for (const auto& g : fz.plan.g.groups)
        for (uint32_t j : g) {
            const uint32_t r = row++;
            const uint32_t count = fz.count(r), have = std::min(count, fz.seg_cap);
            const bool as_distance = op == RF_OP_NORMALIZED_DISTANCE && cs[j]->metric != RF_FUZZ_RATIO;
            if (have) filter_multi_f64_row(fz.keys(r), have, order, as_distance, index_base, out_index + (size_t)j * capacity, out_score + (size_t)j * capacity);
            out_count[j] = count;
        }

    // ---- everything else: the single-query filter, one call per query
    for (uint32_t j = 0; j < q; ++j) {
        if (fz.plan.g.taken[j]) continue;
        const rf_status s = rf_filter_f64(cs[j], corpus, op, args, index_base, capacity, capacity ? out_index + (size_t)j * capacity : nullptr,
                                          capacity ? out_score + (size_t)j * capacity : nullptr, out_count + j, RF_MEM_HOST, order, stream);
        if (s != RF_OK) return s;
    }
    return RF_OK;
}
RF_ABI_CATCH

}  // extern "C"

// rf_api_topk_multi.hip -- rf_topk_multi_u32 / rf_topk_multi_f64: the k best candidates of each of q queries, fusable queries 4 (then 2) to
// a pass over the corpus (rf_topk_multi.hip), every other query through rf_topk_u32 / rf_topk_f64 (rf_host.hpp has the shared declarations).
// Also what the four fused multi-query entry points share (rf_api_filter_multi.hip has the other two): their planner, plan_multi, and the
// checks of op and members, check_multi_members.
// Product code: never includes or links anything from oracle/.
#include "rf_host.hpp"

#include "rf_norm_key.hpp"

extern "C" {

// A/B switch: 0 sends every query down the per-query road (identical results)
static bool sw_topk_multi() { static const bool v = env_on("RF_TOPK_MULTI"); return v; }

// Resolves and plans every query once and groups the fusable ones (rf_multi_group.hpp).  What plan() refuses on every road -- a query beyond what a kernel
// holds, weights or lengths beyond the u32 results -- is refused here, RF_ERR_UNSUPPORTED, at the first such query: the entry points ask before they write
// a count, so that a refused call leaves its outputs as they were.  A query that resolve() cannot lower (overflow-class symbols need a translated image of
// the corpus) or that does not plan for another reason is no refusal: it goes to the single-query call, which serves it or reports why not.
rf_status plan_multi(const MultiAsk& ask, const rf_comparator* const* cs, uint32_t q, const rf_corpus* corpus, rf_op op, const rf_args* args, MultiPlan* out)
{
    out->ps.assign(q, ScanParams{});
    out->raws.assign(q, RAW_LEV);
    out->eff.assign(q, nullptr);
    out->holds.assign(q, nullptr);
    std::vector<MultiQuery> qs(q, MultiQuery{});
    for (uint32_t i = 0; i < q; ++i) {
        if (resolve(cs[i], corpus, &out->eff[i], &out->holds[i]) != RF_OK) continue;
        const ScanParams& p = out->ps[i];
        const rf_status s = plan(out->eff[i], corpus, op, args, ask.norm, &out->ps[i], &out->raws[i]);
        if (s == RF_ERR_UNSUPPORTED) return s;
        if (s != RF_OK || !ask.fuse) continue;
        qs[i] = multi_query(out->raws[i], out->eff[i]->words, p, (p.early != 0) == ask.early);
        if (ask.norm && qs[i].fusable) qs[i].fusable = norm_key_fits(p.fin_mS, p.fin_mM, p.len1, corpus->max_len);
        if (ask.veto && qs[i].fusable) qs[i].fusable = !ask.veto(p, out->raws[i], corpus, ask.norm);
    }
    out->g = group_queries(qs, (size_t)kMaxMulti, false);  // (rows are independent here, so unlike run_many_multi's a group's members need not be neighbours)
    out->fused = 0;
    for (const auto& g : out->g.groups) out->fused += (uint32_t)g.size();
    return RF_OK;
}
void MultiPlan::trace(const char* road, const std::string& before, const std::string& after) const
{
    if (!sw_trace_plan()) return;
    std::string sizes;
    for (const auto& grp : g.groups) sizes += (sizes.empty() ? "" : ",") + std::to_string(grp.size());
    const uint32_t q = (uint32_t)ps.size();
    std::fprintf(stderr, "[rf plan] %s: q=%u%s fused_groups=[%s] per_query=%u%s\n", road, q, before.c_str(), sizes.c_str(), q - fused, after.c_str());
}

// The argument checks the four entry points `fn` share, in the order all of them test: op against the result type, then member by member a null comparator
// before its metric.  `usize_only`: the u32 entry points' text for a metric whose values are f64.
rf_status check_multi_members(const char* fn, bool f64, const char* usize_only, const rf_comparator* const* cs, uint32_t q, rf_op op)
{
    const std::string name(fn);
    if (!f64 && op != RF_OP_DISTANCE && op != RF_OP_SIMILARITY) {
        set_error(name + ": op must be RF_OP_DISTANCE or RF_OP_SIMILARITY");
        return RF_ERR_INVALID_ARG;
    }
    if ((int)op < 0 || (int)op > (int)RF_OP_NORMALIZED_SIMILARITY) {
        set_error("unknown rf_op");
        return RF_ERR_INVALID_ARG;
    }
    const bool norm_op = op == RF_OP_NORMALIZED_DISTANCE || op == RF_OP_NORMALIZED_SIMILARITY;
    // (a null or unacceptable comparator anywhere in the list is an error whatever q's other members are)
    for (uint32_t i = 0; i < q; ++i) {
        if (!cs[i]) {
            set_error(name + ": null comparator");
            return RF_ERR_INVALID_ARG;
        }
        const rf_metric m = cs[i]->metric;
        const bool f64_valued = m == RF_JARO || m == RF_JARO_WINKLER || m == RF_FUZZ_RATIO;
        if (!f64) {
            if (f64_valued) {
                set_error(usize_only);
                return RF_ERR_INVALID_ARG;
            }
        } else if (m == RF_FUZZ_RATIO) {
            if (op != RF_OP_SIMILARITY && op != RF_OP_NORMALIZED_SIMILARITY) {
                set_error("RatioBatchComparator only has similarity (fuzz.rs:115-149)");
                return RF_ERR_INVALID_ARG;
            }
        } else if (!f64_valued && !norm_op) {
            set_error(name + ": distance and similarity of levenshtein / indel / lcs_seq / osa / damerau_levenshtein are u32-valued (" + name.substr(0, name.size() - 3) + "u32)");
            return RF_ERR_INVALID_ARG;
        }
    }
    return RF_OK;
}
// ... and the top-k family's: everything is decided before the corpus is looked at or a device is touched.  Nothing is written before every output is known to be
// there; like rf_many_multi_*, only a non-empty corpus needs the row arrays, and q == 0 -- which writes nothing -- needs none.
static rf_status check_topk_multi_args(const char* fn, bool f64, const rf_comparator* const* cs, uint32_t q, const rf_corpus* corpus, rf_op op, const rf_args* args_in, uint32_t k,
                                       const void* out_score, const uint64_t* out_index, const uint32_t* out_count, rf_args* args)
{
    if (!cs || !corpus || !args_in) {
        set_error(std::string(fn) + ": null handle or args");
        return RF_ERR_INVALID_ARG;
    }
    if (k == 0) {
        set_error("top-k: k must be at least 1");
        return RF_ERR_INVALID_ARG;
    }
    if (const rf_status s = check_multi_members(fn, f64, "top-k: usize-valued metrics only (jaro / jaro_winkler / fuzz ratio: rf_topk_f64)", cs, q, op); s != RF_OK) return s;
    if (q != 0 && (!out_count || (corpus->n != 0 && (!out_score || !out_index)))) {
        set_error(std::string(fn) + ": null output");
        return RF_ERR_INVALID_ARG;
    }
    *args = sanitized_args(args_in, false);
    return RF_OK;
}

// What rf_topk_multi_u32 and rf_topk_multi_f64 share, after their argument checks: plan every query (a refusal comes before a count is written), run the
// fused groups and bring their keys home.  `norm` (rf_topk_multi_f64): f64-valued plans and the normalized kernels.  Fused: plans without a tight cutoff (a
// head-plane early-out scan per query is far faster than any fused full scan), k <= 64.
struct FusedTopk {
    MultiPlan plan;
    std::vector<uint64_t> keys;  // [fused rows in group order][k], best first, ~0 = empty
};
static rf_status topk_multi_fused(bool norm, const rf_comparator* const* cs, uint32_t q, const rf_corpus* corpus, rf_op op, const rf_args* args, uint32_t k,
                                  uint32_t* out_count, hipStream_t st, FusedTopk* out)
{
    MultiPlan& mp = out->plan;
    if (corpus->n != 0)
        if (const rf_status s = plan_multi(MultiAsk{norm, false, sw_topk_multi() && k <= (uint32_t)kWave, nullptr}, cs, q, corpus, op, args, &mp); s != RF_OK) return s;
    for (uint32_t i = 0; i < q; ++i) out_count[i] = 0;
    if (corpus->n == 0) return RF_OK;
    const std::vector<ScanParams>& ps = mp.ps;
    const std::vector<std::vector<uint32_t>>& groups = mp.g.groups;
    const uint32_t fused = mp.fused;
    const uint32_t n_tiles = corpus->n_tiles;
    const uint32_t sample_tiles = sw_topk_sample();
    const bool sample = !groups.empty() && sample_tiles && n_tiles >= 8 * sample_tiles;  // topk_core's rule (a fused group never has a tight cutoff)
    mp.trace(norm ? "topk_multi_f64" : "topk_multi", " k=" + std::to_string(k), sample ? " sample=1" : " sample=0");

    // ---- the fused groups: everything enqueued, one copy home
    std::vector<uint64_t>& keys = out->keys;
    keys.assign((size_t)fused * k, ~0ull);
    hipError_t e = hipSuccess;
    rf_status status = RF_OK;
    if (fused) {
        DeviceGuard guard(corpus->device);
        if (!guard.ok) {
            set_error("cannot select the corpus' device");
            return RF_ERR_NO_DEVICE;
        }
        ScratchSet sc(st);
        // One group's scratch, reused by the next (stream order): [kMaxMulti bound lines | kMaxMulti counter lines | kMaxMulti segments], and the
        // keys of every group.  A segment holds a full k-entry list from every workgroup of the larger launch (rf_topk_multi.hip topk_multi_grid:
        // at most 32 workgroups per CU, 4 MiB per query at k = 64 on 256 CUs).
        const uint32_t grid_main = (uint32_t)topk_multi_grid(n_tiles);
        const uint32_t seg_cap = grid_main * k;  // (the sample's grid is never larger)
        const size_t ctl_bytes = 2 * (size_t)kMaxMulti * 128;
        uint8_t* ctl = nullptr;
        uint64_t *cand = nullptr, *d_keys = nullptr;
        RF_HIP(sc.get(&ctl, ctl_bytes));
        RF_HIP(sc.get(&cand, (size_t)kMaxMulti * seg_cap * sizeof(uint64_t)));
        RF_HIP(sc.get(&d_keys, keys.size() * sizeof(uint64_t)));
        uint32_t row = 0;
        for (const auto& g : groups) {
            const uint32_t i = g[0];
            TopkMultiParams tp{};
            tp.s = ps[i];
            ScanParams& p = tp.s;
            p.out = nullptr, p.early = 0, p.prefill_none = 0;
            p.tile_begin = 0, p.tile_end = n_tiles, p.tile_step = 1;
            p.multi_q = (uint32_t)g.size();
            p.topk_k = k;
            p.topk_desc = op == RF_OP_SIMILARITY;  // (not read under norm: both normalized ops order by ascending norm_key)
            tp.norm = norm ? 1u : 0u;
            p.key_index_base = 0;  // index_base is added on the host, in 64 bits
            for (size_t m = 0; m < g.size() && status == RF_OK; ++m) {
                p.multi_len1[m] = ps[g[m]].len1;
                status = comparator_device_pm(mp.eff[g[m]], corpus->device, &p.multi_pm[m]);
            }
            if (status != RF_OK) break;
            tp.bound = reinterpret_cast<uint64_t*>(ctl);
            tp.count = reinterpret_cast<uint32_t*>(ctl + (size_t)kMaxMulti * 128);
            tp.cand = cand;
            tp.seg_cap = seg_cap;
            e = hipMemsetAsync(tp.bound, 0xFF, (size_t)kMaxMulti * 128, st);
            if (e == hipSuccess) e = hipMemsetAsync(tp.count, 0, (size_t)kMaxMulti * 128, st);
            const bool narrow = p.len1 <= 32;
            if (e == hipSuccess && sample) {
                TopkMultiParams ts = tp;
                ts.s.tile_step = n_tiles / sample_tiles;
                ts.sample = 1;
                e = launch_topk_multi(mp.raws[i], narrow, ts, st);
                if (e == hipSuccess) e = launch_topk_multi_select(ts, nullptr, st);
            }
            if (e == hipSuccess) e = launch_topk_multi(mp.raws[i], narrow, tp, st);
            if (e == hipSuccess) e = launch_topk_multi_select(tp, d_keys + (size_t)row * k, st);
            if (e != hipSuccess) break;
            row += (uint32_t)g.size();
        }
        if (status == RF_OK && e == hipSuccess) e = copy_home(keys.data(), d_keys, keys.size() * sizeof(uint64_t), st);
        else (void)hipStreamSynchronize(st);
        if (status != RF_OK) return status;
        if (e != hipSuccess) {
            set_error(std::string("top-k, fused queries: ") + hipGetErrorString(e));
            return e == hipErrorOutOfMemory ? RF_ERR_OOM : RF_ERR_HIP;
        }
    }
    return RF_OK;
}

// Row j is rf_topk_u32(cs[j], ...).  Queries are planned as run_many_multi plans them and fused under its rules -- single-word Levenshtein /
// LCS-family recurrences that agree on the kernel family, finishing, factor and word width, no long pattern, no tight cutoff (a head-plane
// early-out scan per query is far faster than any fused full scan) -- in groups of 4, then 2; k > 64, u32 queries with overflow-class
// symbols, OSA, Damerau-Levenshtein, general weight tables, queries beyond 64 symbols and the odd one left over take rf_topk_u32 itself.
// A fused group: [sample pass over every (tiles / RF_TOPK_SAMPLE)-th tile + selection into the bounds], main pass, selection into the keys.
// All scratch is the call's own (ScratchSet): nothing of the corpus' per-stream caches is leased, so handles stay shareable by host threads
// and the lock order of rf_host.hpp is not involved.  Every fusable shape runs fused: in the same-session comparison with a loop of rf_topk_u32
// (tools/bench_topk_multi.py, profiles/topk_multi.txt: 16 queries, k = 16, 10 k .. 100 M candidates, single-length and ragged) the fused road
// was the faster one for every family and size, by more than the spread between repetitions -- 1.02 x (64-bit Levenshtein, 100 M) to 3.4 x (10 k).
rf_status rf_topk_multi_u32(const rf_comparator* const* cs, uint32_t q, const rf_corpus* corpus, rf_op op, const rf_args* args_in, uint32_t k,
                            uint64_t index_base, uint32_t* out_score, uint64_t* out_index, uint32_t* out_count, void* stream)
try {
    rf_args args_v;
    const rf_args* args = &args_v;
    if (const rf_status s = check_topk_multi_args("rf_topk_multi_u32", false, cs, q, corpus, op, args_in, k, out_score, out_index, out_count, &args_v); s != RF_OK) return s;
    if (q == 0) return RF_OK;
    FusedTopk fz;
    if (const rf_status s = topk_multi_fused(false, cs, q, corpus, op, args, k, out_count, (hipStream_t)stream, &fz); s != RF_OK) return s;
    if (corpus->n == 0) return RF_OK;
    const std::vector<uint64_t>& keys = fz.keys;
    // decode as rf_topk_u32 does
    const bool desc = op == RF_OP_SIMILARITY;
    uint32_t row = 0;
    for (const auto& g : fz.plan.g.groups)
        for (uint32_t j : g) {
            const uint64_t* best = keys.data() + (size_t)row++ * k;
            uint32_t m = 0;
            for (; m < k && best[m] != ~0ull; ++m) {
                const uint32_t hi = (uint32_t)(best[m] >> 32);
                out_score[(size_t)j * k + m] = desc ? ~hi : hi;
                out_index[(size_t)j * k + m] = index_base + (uint32_t)best[m];
            }
            out_count[j] = m;
        }

    // ---- everything else: the single-query top-k, one call per query
    for (uint32_t j = 0; j < q; ++j) {
        if (fz.plan.g.taken[j]) continue;
        const rf_status s = rf_topk_u32(cs[j], corpus, op, args, k, index_base, out_score + (size_t)j * k, out_index + (size_t)j * k, out_count + j, nullptr, RF_MEM_HOST, stream);
        if (s != RF_OK) return s;
    }
    return RF_OK;
}
RF_ABI_CATCH

// Row j is rf_topk_f64(cs[j], ...): the same values bit for bit in the same (score, index) order.  The grouping is rf_topk_multi_u32's with the
// f64-valued plans; a fusable query must also keep every maximum of its scan within 65535, because the in-scan lists order by the 32-bit
// image norm_key(dist, maximum) of the normalized distance (rf_norm_key.hpp: exact and order-preserving up to there).  Both normalized ops
// rank by ascending key; the host turns a key back into its reduced fraction a / b and (double)a / (double)b is the double emit_fin divides
// out of dist and maximum, so nothing of the score is lost in the 32 bits.  jaro / jaro_winkler, OSA, Damerau-Levenshtein, general weight
// tables, queries beyond 64 symbols, tight cutoffs (early-out plans), k > 64, a maximum beyond 65535 and the odd one left over take
// rf_topk_f64 itself.  Every fusable shape runs fused: in the same-session comparison with a loop of rf_topk_f64 (tools/bench_topk_multi_f64.py,
// profiles/topk_multi_f64.txt: 16 queries, k = 16, 10 k .. 100 M candidates, single-length and ragged, Indel / Levenshtein / ratio) the fused road was the
// faster one for every family and size, 2.0 x (64-bit Levenshtein, 100 M) to 15 x (10 k), and costs 0-12 % over the u32 fused kernel on the same corpus.
rf_status rf_topk_multi_f64(const rf_comparator* const* cs, uint32_t q, const rf_corpus* corpus, rf_op op, const rf_args* args_in, uint32_t k,
                            uint64_t index_base, double* out_score, uint64_t* out_index, uint32_t* out_count, void* stream)
try {
    rf_args args_v;
    const rf_args* args = &args_v;
    if (const rf_status s = check_topk_multi_args("rf_topk_multi_f64", true, cs, q, corpus, op, args_in, k, out_score, out_index, out_count, &args_v); s != RF_OK) return s;
    if (q == 0) return RF_OK;
    FusedTopk fz;
    if (const rf_status s = topk_multi_fused(true, cs, q, corpus, op, args, k, out_count, (hipStream_t)stream, &fz); s != RF_OK) return s;
    if (corpus->n == 0) return RF_OK;
    // decode (decode_norm_keys, rf_host.hpp, shared with rf_join_topk_f64): norm_key_ratio(key) is the key's fraction a / b, the normalized distance; which value the
    // member returns is its plan's op (a fuzz ratio: the similarity)
    uint32_t row = 0;
    for (const auto& g : fz.plan.g.groups)
        for (uint32_t j : g)
            out_count[j] = decode_norm_keys(fz.keys.data() + (size_t)row++ * k, k, cs[j]->metric, op, index_base, out_score + (size_t)j * k, out_index + (size_t)j * k);

    // ---- everything else: the single-query top-k, one call per query
    for (uint32_t j = 0; j < q; ++j) {
        if (fz.plan.g.taken[j]) continue;
        uint64_t count = 0;
        const rf_status s = rf_topk_f64(cs[j], corpus, op, args, k, index_base, out_score + (size_t)j * k, out_index + (size_t)j * k, &count, nullptr, RF_MEM_HOST, stream);
        if (s != RF_OK) return s;
        out_count[j] = (uint32_t)count;
    }
    return RF_OK;
}
RF_ABI_CATCH

}  // extern "C"

// rf_api_filter_multi.hip -- rf_filter_multi_u32: the (index, score) pairs within the cutoff of each of q queries, fusable queries 4 (then 2) to a
// pass over the corpus (rf_filter_multi.hip), every other query through rf_filter_u32 (rf_host.hpp has the shared declarations).
// Product code: never includes or links anything from oracle/.
#include <algorithm>

#include "rf_host.hpp"

extern "C" {

constexpr size_t kHeadPlaneWins = size_t(1) << 25;  // candidates of a single-length corpus from which small-cutoff Levenshtein queries go per query (see the planner below)
// A/B switch: 0 sends every query down the per-query road (identical results)
static bool sw_filter_multi() { static const bool v = env_on("RF_FILTER_MULTI"); return v; }

// Row j is rf_filter_u32(cs[j], ..., RF_MEM_HOST, order, ...).  Queries are planned as rf_topk_multi_u32 plans them and grouped under its rules, with ONE
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
    // ---- arguments: everything here is decided before the corpus is looked at or a device is touched, and before anything is written
    if (!cs || !corpus || !args_in || !out_count) {
        set_error("rf_filter_multi_u32: null handle, args or count");
        return RF_ERR_INVALID_ARG;
    }
    if (capacity && (!out_index || !out_score)) {
        set_error("rf_filter_multi_u32: null output with a non-zero capacity");
        return RF_ERR_INVALID_ARG;
    }
    if ((int)order < 0 || (int)order > (int)RF_FILTER_ANY) {
        set_error("rf_filter_multi_u32: unknown order");
        return RF_ERR_INVALID_ARG;
    }
    if (op != RF_OP_DISTANCE && op != RF_OP_SIMILARITY) {
        set_error("rf_filter_multi_u32: op must be RF_OP_DISTANCE or RF_OP_SIMILARITY");
        return RF_ERR_INVALID_ARG;
    }
    if (q == 0) return RF_OK;
    for (uint32_t i = 0; i < q; ++i) {
        if (!cs[i]) {
            set_error("rf_filter_multi_u32: null comparator");
            return RF_ERR_INVALID_ARG;
        }
        if (cs[i]->metric == RF_JARO || cs[i]->metric == RF_JARO_WINKLER || cs[i]->metric == RF_FUZZ_RATIO) {
            set_error("rf_filter_multi_u32: usize-valued metrics only (jaro / jaro_winkler / fuzz ratio: rf_filter_f64)");
            return RF_ERR_INVALID_ARG;
        }
    }
    for (uint32_t i = 0; i < q; ++i) out_count[i] = 0;
    if (corpus->n == 0) return RF_OK;
    const rf_args args_v = sanitized_args(args_in, false), *args = &args_v;

    // ---- plan every query; which ones can be fused
    std::vector<ScanParams> ps(q);
    std::vector<RawKind> raws(q, RAW_LEV);
    std::vector<const rf_comparator*> eff(q, nullptr);
    std::vector<ComparatorRef> holds(q);
    std::vector<char> fusable(q, 0);
    if (sw_filter_multi())
        for (uint32_t i = 0; i < q; ++i) {
            // (a query that does not resolve -- overflow-class symbols need a translated image of the corpus -- or does not plan goes to
            // rf_filter_u32, which serves it or reports why not)
            if (resolve(cs[i], corpus, &eff[i], &holds[i]) != RF_OK) continue;
            if (plan(eff[i], corpus, op, args, false, &ps[i], &raws[i]) != RF_OK) continue;
            fusable[i] = (raws[i] == RAW_LEV || raws[i] == RAW_LCS) && eff[i]->words == 1 && !ps[i].long_words_pad && ps[i].early;
            // The one shape the fused road lost (tools/bench_filter_multi.py, profiles/filter_multi.txt): Levenshtein under a small cutoff over a LARGE single-length
            // corpus, where rf_filter_u32 takes its first look from the 8-byte head plane and compacts lanes (6-8 B per pair, 8 columns) while a fused group reads
            // the payload's 16-byte first chunk: 100 M x 64, cutoff 3, 16 / 256 queries 5.67 / 89.5 ms fused against 3.00 / 53.7 ms per query; at 10 M the fused
            // road still wins (0.92 / 14.1 against 1.64 / 23.9 ms).  Between the two sizes the boundary is interpolated from those four times (fixed cost + slope of
            // either road: about 2^25 candidates for a group of four); the one size measured beside it, 30 M, is level at 16 queries and 1.10 x at 256
            // (profiles/filter_multi_copy.txt).  A query whose length window is empty stays fused: it launches nothing.
            if (fusable[i] && raws[i] == RAW_LEV && corpus->uniform && corpus->n >= kHeadPlaneWins && ps[i].first_check <= 8 && ps[i].tile_begin < ps[i].tile_end)
                fusable[i] = 0;
        }
    auto same_group = [&](uint32_t a, uint32_t b) {
        return raws[a] == raws[b] && ps[a].finish == ps[b].finish && ps[a].factor == ps[b].factor && ps[a].op == ps[b].op &&
               (ps[a].len1 <= 32) == (ps[b].len1 <= 32);
    };
    // (rows are independent, so a group's members need not be neighbours)
    std::vector<std::vector<uint32_t>> groups;
    std::vector<char> taken(q, 0);
    for (uint32_t i = 0; i < q; ++i) {
        if (taken[i] || !fusable[i]) continue;
        std::vector<uint32_t> g{i};
        for (uint32_t j = i + 1; j < q && g.size() < (size_t)kMaxMulti; ++j)
            if (!taken[j] && fusable[j] && same_group(i, j)) g.push_back(j);
        if (g.size() == 3) g.pop_back();
        if (g.size() < 2) continue;  // the odd one left over
        for (uint32_t m : g) taken[m] = 1;
        groups.push_back(std::move(g));
    }
    uint32_t fused = 0;
    for (const auto& g : groups) fused += (uint32_t)g.size();
    if (sw_trace_plan()) {
        std::string sizes;
        for (const auto& g : groups) sizes += (sizes.empty() ? "" : ",") + std::to_string(g.size());
        std::fprintf(stderr, "[rf plan] filter_multi: q=%u fused_groups=[%s] per_query=%u\n", q, sizes.c_str(), q - fused);
    }

    // ---- the fused groups: everything enqueued, then the results home
    hipStream_t st = (hipStream_t)stream;
    const bool desc = op == RF_OP_SIMILARITY;
    const uint32_t seg_cap = (uint32_t)std::min<uint64_t>(capacity, corpus->n);
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
        const size_t ctl_bytes = (size_t)fused * kLine, seg_bytes = (size_t)fused * seg_cap * sizeof(uint64_t);
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
            p.topk_desc = desc;
            // the union of the members' length windows (plan(): a member's tiles outside its own are None by their length alone; an empty window: tile_begin == tile_end)
            uint32_t t0 = corpus->n_tiles, t1 = 0;
            for (size_t m = 0; m < g.size() && status == RF_OK; ++m) {
                const ScanParams& pm = ps[g[m]];
                p.multi_len1[m] = pm.len1;
                if (pm.tile_begin < pm.tile_end) t0 = std::min(t0, pm.tile_begin), t1 = std::max(t1, std::min(pm.tile_end, corpus->n_tiles));
                status = comparator_device_pm(eff[g[m]], corpus->device, &p.multi_pm[m]);
            }
            if (status != RF_OK) break;
            p.tile_begin = t0, p.tile_end = std::max(t0, t1);
            fp.count = d_count + (size_t)row * kFilterMultiLine32;
            fp.cand = seg_cap ? d_cand + (size_t)row * seg_cap : nullptr;
            fp.seg_cap = seg_cap;
            e = launch_filter_multi(raws[i], p.len1 <= 32, fp, st);
            row += (uint32_t)g.size();
        }
        std::vector<uint8_t> home;
        std::vector<uint64_t> big;  // (the two-step road: [fused][width], width = the longest list held)
        size_t width = seg_cap;
        const bool one_copy = seg_bytes <= kOneCopyBytes;
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
            for (uint32_t i = 0; i < q; ++i) out_count[i] = 0;
            set_error(std::string("filter, fused queries: ") + hipGetErrorString(e));
            return e == hipErrorOutOfMemory ? RF_ERR_OOM : RF_ERR_HIP;
        }
        // order and decode as rf_filter_u32 does: by index ascending, or best score first with ties by index (a plain sort of the keys)
        const uint32_t* counts = reinterpret_cast<const uint32_t*>(home.data());
        row = 0;
        for (const auto& g : groups)
            for (uint32_t j : g) {
                const uint32_t r = row++;
                const uint32_t count = counts[(size_t)r * kFilterMultiLine32], have = std::min(count, seg_cap);
                uint64_t* keys = one_copy ? reinterpret_cast<uint64_t*>(home.data() + ctl_bytes) + (size_t)r * seg_cap : big.data() + (size_t)r * width;
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
        if (taken[j]) continue;
        const rf_status s = rf_filter_u32(cs[j], corpus, op, args, index_base, capacity, capacity ? out_index + (size_t)j * capacity : nullptr,
                                          capacity ? out_score + (size_t)j * capacity : nullptr, out_count + j, RF_MEM_HOST, order, stream);
        if (s != RF_OK) return s;
    }
    return RF_OK;
}
RF_ABI_CATCH

}  // extern "C"

// rapidfuzz_amd.hpp -- header-only C++17 facade over the C ABI of rfgpu.h that mirrors the reference's names:
//   rapidfuzz::distance::{levenshtein, indel, lcs_seq, damerau_levenshtein, hamming, prefix, postfix, jaro, jaro_winkler}::{Args, BatchComparator, distance, ...}
//   rapidfuzz::fuzz::{ratio, RatioBatchComparator}
// `Option<T>` becomes std::optional<T>; the one-vs-many entry points take a rapidfuzz::Corpus.
// Reference: rapidfuzz-rs v0.5.0, e.g. src/distance/levenshtein.rs:86-148 (Args, WeightTable), :1636-1818
// (BatchComparator), src/fuzz.rs:48-150.  Every score is computed by the HIP kernels behind rfgpu.h.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <optional>
#include <stdexcept>
#include <string>
#include <string_view>
#include <vector>

#include "rfgpu.h"

namespace rapidfuzz {

struct Error : std::runtime_error {
    rf_status status;
    Error(rf_status s, const char* msg) : std::runtime_error(msg), status(s) {}
};
inline void check(rf_status s)
{
    if (s != RF_OK) throw Error(s, rf_last_error());
}

/// The device-resident candidate set (what the user's `for candidate in corpus` loop walks in the reference).
class Corpus {
public:
    Corpus(const std::vector<std::string_view>& candidates, int device = 0)
    {
        std::vector<uint8_t> bytes;
        std::vector<uint64_t> offsets{0};
        for (auto c : candidates) {
            bytes.insert(bytes.end(), c.begin(), c.end());
            offsets.push_back(bytes.size());
        }
        check(rf_corpus_pack(bytes.data(), offsets.data(), candidates.size(), device, &h_));
    }
    /// candidates as code points (`s.chars()` in the reference): one u32 per element, the corpus keeps its own alphabet
    Corpus(const std::vector<std::u32string_view>& candidates, int device = 0)
    {
        std::vector<uint32_t> elems;
        std::vector<uint64_t> offsets{0};
        for (auto c : candidates) {
            elems.insert(elems.end(), c.begin(), c.end());
            offsets.push_back(elems.size());
        }
        check(rf_corpus_pack_u32(elems.data(), offsets.data(), candidates.size(), device, &h_));
    }
    /// a packed corpus written by save()
    static Corpus load(const std::string& path, int device = 0)
    {
        Corpus c;
        check(rf_corpus_load(path.c_str(), device, &c.h_));
        return c;
    }
    void save(const std::string& path) const { check(rf_corpus_save(h_, path.c_str())); }
    /// n rows of `len` bytes already in device memory
    Corpus(const void* d_rows, size_t n, size_t len, size_t stride, int device = 0, void* stream = nullptr)
    {
        check(rf_corpus_pack_rows_device(d_rows, n, len, stride, device, stream, &h_));
    }
    /// ragged candidates already in device memory: candidate i = d_bytes[d_offsets[i] .. d_offsets[i + 1]) (n + 1 offsets, on the device too; n_elems
    /// bytes are readable at d_bytes).  The corpus the string_view constructor builds from the same arrays on the host.
    static Corpus from_device_ragged(const uint8_t* d_bytes, uint64_t n_elems, const uint64_t* d_offsets, size_t n, int device = 0, void* stream = nullptr)
    {
        Corpus c;
        check(rf_corpus_pack_device(d_bytes, n_elems, d_offsets, n, device, stream, &c.h_));
        return c;
    }
    /// the same over code points (u32 elements): the corpus the u32string_view constructor builds
    static Corpus from_device_ragged(const uint32_t* d_elems, uint64_t n_elems, const uint64_t* d_offsets, size_t n, int device = 0, void* stream = nullptr)
    {
        Corpus c;
        check(rf_corpus_pack_u32_device(d_elems, n_elems, d_offsets, n, device, stream, &c.h_));
        return c;
    }
    Corpus(const Corpus&) = delete;
    Corpus& operator=(const Corpus&) = delete;
    Corpus(Corpus&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    ~Corpus() { rf_corpus_free(h_); }
    size_t size() const { return rf_corpus_count(h_); }
    const rf_corpus* handle() const { return h_; }
    /// packed over code points (the u32string_view constructor, or a file saved from such a corpus): read with take_u32
    bool wide() const { return rf_corpus_is_wide(h_) != 0; }
    /// The candidates behind the indices a topk / filter call returned -- the `c` of the reference's `for c in corpus`, read back out of the
    /// packed form: row j is candidate indices[j] - index_base (any order, repeats allowed).
    std::vector<std::string> take(const std::vector<uint64_t>& indices, uint64_t index_base = 0, void* stream = nullptr) const
    {
        return rows<std::string, uint8_t>(rf_corpus_take, indices, index_base, stream);
    }
    /// the same as code points: the symbols of a wide corpus, the bytes of a byte corpus zero-extended
    std::vector<std::u32string> take_u32(const std::vector<uint64_t>& indices, uint64_t index_base = 0, void* stream = nullptr) const
    {
        return rows<std::u32string, uint32_t>(rf_corpus_take_u32, indices, index_base, stream);
    }
    /// their lengths, in elements
    std::vector<uint32_t> lengths(const std::vector<uint64_t>& indices, uint64_t index_base = 0, void* stream = nullptr) const
    {
        std::vector<uint32_t> out(indices.size());
        uint32_t none = 0;
        check(rf_corpus_lengths(h_, indices.empty() ? &index_base : indices.data(), indices.size(), index_base, out.empty() ? &none : out.data(), stream));
        return out;
    }

private:
    Corpus() = default;
    template <class Str, class Elem, class Fn>
    std::vector<Str> rows(Fn fn, const std::vector<uint64_t>& indices, uint64_t index_base, void* stream) const
    {
        // (indices == NULL means "every candidate" in the C ABI: an empty list stays an empty list here)
        const uint64_t* idx = indices.empty() ? &index_base : indices.data();
        std::vector<uint64_t> offsets(indices.size() + 1, 0);
        check(fn(h_, idx, indices.size(), index_base, nullptr, 0, offsets.data(), RF_MEM_HOST, stream));  // the sizing call
        std::vector<Elem> data(offsets.back());
        if (!data.empty()) check(fn(h_, idx, indices.size(), index_base, data.data(), data.size(), offsets.data(), RF_MEM_HOST, stream));
        std::vector<Str> out;
        out.reserve(indices.size());
        for (size_t j = 0; j < indices.size(); ++j)
            out.emplace_back(reinterpret_cast<const typename Str::value_type*>(data.data()) + offsets[j], (size_t)(offsets[j + 1] - offsets[j]));
        return out;
    }
    rf_corpus* h_ = nullptr;
};

namespace detail {

struct WeightTable {  // levenshtein.rs:128-148
    size_t insertion_cost = 1, deletion_cost = 1, substitution_cost = 1;
};

/// `Args::default().score_cutoff(x).score_hint(y).weights(&w).prefix_weight(p)`
template <class T>
struct Args {
    std::optional<T> cutoff, hint;
    WeightTable w;
    double pw = 0.1;
    uint32_t flags = 0;
    Args score_cutoff(T v) const { Args a = *this; a.cutoff = v; return a; }
    Args score_hint(T v) const { Args a = *this; a.hint = v; return a; }
    Args weights(const WeightTable& t) const { Args a = *this; a.w = t; return a; }
    Args prefix_weight(double p) const { Args a = *this; a.pw = p; return a; }
    /// hamming only, `Args::pad(true)` (hamming.rs:112-118).  Without it a candidate of another length than the query is the reference's
    /// Err(DifferentLengthArgs): the single-candidate methods throw Error(RF_ERR_INVALID_ARG), *_many leaves its entry empty, *_filter_* and *_topk_* drop it
    Args pad(bool on = true) const { Args a = *this; a.flags = on ? (a.flags | RF_FLAG_HAMMING_PAD) : (a.flags & ~RF_FLAG_HAMMING_PAD); return a; }
    rf_args to_c() const
    {
        rf_args a;
        rf_args_default(&a);
        if constexpr (std::is_floating_point_v<T>) {
            if (cutoff) a.cutoff_f64 = *cutoff;
            if (hint) a.score_hint_f64 = *hint;
        } else {
            if (cutoff) a.cutoff_usize = *cutoff;
            if (hint) a.score_hint_usize = *hint;
        }
        a.insertion_cost = w.insertion_cost;
        a.deletion_cost = w.deletion_cost;
        a.substitution_cost = w.substitution_cost;
        a.prefix_weight = pw;
        a.flags = flags;
        return a;
    }
};

/// a triple of the joins by f64 score (rf_join_f64): `score` is the double normalized_*_filter_many (or the f64 metric's filter) reports for the pair
struct JoinTripleF64 {
    uint64_t query, candidate;
    double score;
};

template <rf_metric M, bool FloatMetric>
class BatchComparator {
public:
    using usize_result = std::conditional_t<FloatMetric, double, size_t>;
    using JoinTripleF64 = detail::JoinTripleF64;
    explicit BatchComparator(std::string_view s1)  // BatchComparator::new
    {
        check(rf_comparator_new(M, reinterpret_cast<const uint8_t*>(s1.data()), s1.size(), &h_));
    }
    explicit BatchComparator(std::u32string_view s1)  // BatchComparator::new(s1.chars())
    {
        check(rf_comparator_new_u32(M, reinterpret_cast<const uint32_t*>(s1.data()), s1.size(), &h_));
    }
    BatchComparator(const BatchComparator& o) { check(rf_comparator_clone(o.h_, &h_)); }  // #[derive(Clone)]
    BatchComparator& operator=(const BatchComparator&) = delete;
    ~BatchComparator() { rf_comparator_free(h_); }

    // ---- one-vs-many: out[i] = this-><op>_with_args(candidate_i, args)
    std::vector<std::optional<usize_result>> distance_many(const Corpus& c, const Args<usize_result>& a = {}) const
    {
        return many<usize_result>(c, RF_OP_DISTANCE, a.to_c());
    }
    std::vector<std::optional<usize_result>> similarity_many(const Corpus& c, const Args<usize_result>& a = {}) const
    {
        return many<usize_result>(c, RF_OP_SIMILARITY, a.to_c());
    }
    std::vector<std::optional<double>> normalized_distance_many(const Corpus& c, const Args<double>& a = {}) const
    {
        return many<double>(c, RF_OP_NORMALIZED_DISTANCE, a.to_c());
    }
    std::vector<std::optional<double>> normalized_similarity_many(const Corpus& c, const Args<double>& a = {}) const
    {
        return many<double>(c, RF_OP_NORMALIZED_SIMILARITY, a.to_c());
    }

    // ---- only the candidates within the cutoff: the reference user's `corpus.iter().enumerate().filter_map(|(i, c)| scorer.<op>_with_args(c, &args).map(|v| (i, v)))`
    // as ONE device pass that never builds the n-entry vector of Nones (rf_filter_u32 / rf_filter_f64); pairs in ascending index order (or `order`)
    std::vector<std::pair<uint64_t, usize_result>> distance_filter_many(const Corpus& c, const Args<usize_result>& a = {}, rf_filter_order order = RF_FILTER_BY_INDEX) const
    {
        return filter<usize_result>(c, RF_OP_DISTANCE, a.to_c(), order);
    }
    std::vector<std::pair<uint64_t, usize_result>> similarity_filter_many(const Corpus& c, const Args<usize_result>& a = {}, rf_filter_order order = RF_FILTER_BY_INDEX) const
    {
        return filter<usize_result>(c, RF_OP_SIMILARITY, a.to_c(), order);
    }
    std::vector<std::pair<uint64_t, double>> normalized_distance_filter_many(const Corpus& c, const Args<double>& a = {}, rf_filter_order order = RF_FILTER_BY_INDEX) const
    {
        return filter<double>(c, RF_OP_NORMALIZED_DISTANCE, a.to_c(), order);
    }
    std::vector<std::pair<uint64_t, double>> normalized_similarity_filter_many(const Corpus& c, const Args<double>& a = {}, rf_filter_order order = RF_FILTER_BY_INDEX) const
    {
        return filter<double>(c, RF_OP_NORMALIZED_SIMILARITY, a.to_c(), order);
    }

    // ---- many queries x one corpus: res[j][i] = scorers[j].<op>_with_args(candidate_i, args), one call (rf_many_multi_*)
    static std::vector<std::vector<std::optional<usize_result>>> distance_many_multi(const std::vector<const BatchComparator*>& scorers,
                                                                                      const Corpus& c, const Args<usize_result>& a = {})
    {
        const rf_args ca = a.to_c();
        std::vector<const rf_comparator*> hs;
        for (const BatchComparator* s : scorers) hs.push_back(s->h_);
        std::vector<std::vector<std::optional<usize_result>>> res(scorers.size(), std::vector<std::optional<usize_result>>(c.size()));
        if constexpr (FloatMetric) {
            std::vector<double> out(scorers.size() * c.size());
            check(rf_many_multi_f64(hs.data(), (uint32_t)hs.size(), c.handle(), RF_OP_DISTANCE, &ca, out.data(), RF_MEM_HOST, nullptr));
            for (size_t j = 0; j < scorers.size(); ++j)
                for (size_t i = 0; i < c.size(); ++i)
                    if (!std::isnan(out[j * c.size() + i])) res[j][i] = out[j * c.size() + i];
        } else {
            std::vector<uint32_t> out(scorers.size() * c.size());
            check(rf_many_multi_u32(hs.data(), (uint32_t)hs.size(), c.handle(), RF_OP_DISTANCE, &ca, out.data(), RF_MEM_HOST, nullptr));
            for (size_t j = 0; j < scorers.size(); ++j)
                for (size_t i = 0; i < c.size(); ++i)
                    if (out[j * c.size() + i] != RF_NONE_U32 && !(M == RF_HAMMING && out[j * c.size() + i] == RF_DIFFERENT_LENGTH_U32)) res[j][i] = out[j * c.size() + i];
        }
        return res;
    }

    // ---- the k best candidates of every query, one call (rf_topk_multi_u32): res[j] = (index_base + index, score) pairs of scorers[j], best first -- ordered by
    // (score ascending, index ascending), at most k of them.  Fusable queries share passes over the corpus; no [q][n] matrix is built.  usize metrics only.
    static std::vector<std::vector<std::pair<uint64_t, size_t>>> distance_topk_multi(const std::vector<const BatchComparator*>& scorers, const Corpus& c, uint32_t k,
                                                                                      const Args<usize_result>& a = {}, uint64_t index_base = 0)
    {
        return topk_multi(scorers, c, k, RF_OP_DISTANCE, a.to_c(), index_base);
    }
    /// the same by similarity: (score descending, index ascending)
    static std::vector<std::vector<std::pair<uint64_t, size_t>>> similarity_topk_multi(const std::vector<const BatchComparator*>& scorers, const Corpus& c, uint32_t k,
                                                                                        const Args<usize_result>& a = {}, uint64_t index_base = 0)
    {
        return topk_multi(scorers, c, k, RF_OP_SIMILARITY, a.to_c(), index_base);
    }

    // ---- the same for the f64-valued scores (rf_topk_multi_f64): res[j] = (index_base + index, score) pairs, normalized distance ascending / normalized
    // similarity descending, ties by index; bit for bit the doubles normalized_*_many returns.  Fusable queries (see rfgpu.h) share passes over the corpus.
    static std::vector<std::vector<std::pair<uint64_t, double>>> normalized_distance_topk_multi(const std::vector<const BatchComparator*>& scorers, const Corpus& c, uint32_t k,
                                                                                                 const Args<double>& a = {}, uint64_t index_base = 0)
    {
        return topk_multi_f64(scorers, c, k, RF_OP_NORMALIZED_DISTANCE, a.to_c(), index_base);
    }
    static std::vector<std::vector<std::pair<uint64_t, double>>> normalized_similarity_topk_multi(const std::vector<const BatchComparator*>& scorers, const Corpus& c, uint32_t k,
                                                                                                   const Args<double>& a = {}, uint64_t index_base = 0)
    {
        return topk_multi_f64(scorers, c, k, RF_OP_NORMALIZED_SIMILARITY, a.to_c(), index_base);
    }

    // ---- the candidates within the cutoff for every query, one call (rf_filter_multi_u32): res[j] = distance_filter_many of scorers[j] -- (index_base + index,
    // score) pairs, in `order`.  Queries under a tight cutoff share passes over the corpus, 4 (or 2) to a pass; no [q][n] matrix is built.  usize metrics only.
    static std::vector<std::vector<std::pair<uint64_t, size_t>>> distance_filter_multi(const std::vector<const BatchComparator*>& scorers, const Corpus& c,
                                                                                        const Args<usize_result>& a = {}, rf_filter_order order = RF_FILTER_BY_INDEX,
                                                                                        uint64_t index_base = 0)
    {
        return filter_multi(scorers, c, RF_OP_DISTANCE, a.to_c(), order, index_base);
    }
    static std::vector<std::vector<std::pair<uint64_t, size_t>>> similarity_filter_multi(const std::vector<const BatchComparator*>& scorers, const Corpus& c,
                                                                                          const Args<usize_result>& a = {}, rf_filter_order order = RF_FILTER_BY_INDEX,
                                                                                          uint64_t index_base = 0)
    {
        return filter_multi(scorers, c, RF_OP_SIMILARITY, a.to_c(), order, index_base);
    }

    // ---- the same for the f64-valued scores (rf_filter_multi_f64): res[j] = normalized_*_filter_many of scorers[j] -- (index_base + index, score) pairs, in
    // `order`, bit for bit the doubles normalized_*_many returns.  Queries under a tight cutoff (see rfgpu.h) share passes over the corpus.
    static std::vector<std::vector<std::pair<uint64_t, double>>> normalized_distance_filter_multi(const std::vector<const BatchComparator*>& scorers, const Corpus& c,
                                                                                                   const Args<double>& a = {}, rf_filter_order order = RF_FILTER_BY_INDEX,
                                                                                                   uint64_t index_base = 0)
    {
        return filter_multi_f64(scorers, c, RF_OP_NORMALIZED_DISTANCE, a.to_c(), order, index_base);
    }
    static std::vector<std::vector<std::pair<uint64_t, double>>> normalized_similarity_filter_multi(const std::vector<const BatchComparator*>& scorers, const Corpus& c,
                                                                                                     const Args<double>& a = {}, rf_filter_order order = RF_FILTER_BY_INDEX,
                                                                                                     uint64_t index_base = 0)
    {
        return filter_multi_f64(scorers, c, RF_OP_NORMALIZED_SIMILARITY, a.to_c(), order, index_base);
    }

    // ---- all pairs of two packed corpora within the cutoff, one call (rf_join_u32): the triples (query row, candidate, score) -- what distance_filter_many of
    // a comparator over row `query` of `queries` reports for `candidate` -- ascending by (position in query_indices, candidate) or, RF_JOIN_ANY, as they arrived.
    // `queries` and `c` may be the same corpus (a self-join; `upper` then keeps each unordered pair once and no (i, i)).  query_indices: the rows to join, nullptr = every row (an empty list: no pair).  The
    // cutoff is required.  The usize metrics' triples carry a size_t (rf_join_u32); jaro / jaro_winkler's, and every normalized_*_join's, a double (rf_join_f64).
    struct JoinTriple {
        uint64_t query, candidate;
        size_t score;
    };
    using join_result = std::conditional_t<FloatMetric, JoinTripleF64, JoinTriple>;
    static std::vector<join_result> distance_join(const Corpus& queries, const Corpus& c, const Args<usize_result>& a, bool upper = false, rf_join_order order = RF_JOIN_BY_QUERY,
                                                 const std::vector<uint64_t>* query_indices = nullptr, uint64_t query_base = 0, uint64_t index_base = 0)
    {
        return join<join_result>(queries, c, RF_OP_DISTANCE, a.to_c(), upper, order, query_indices, query_base, index_base);
    }
    static std::vector<join_result> similarity_join(const Corpus& queries, const Corpus& c, const Args<usize_result>& a, bool upper = false, rf_join_order order = RF_JOIN_BY_QUERY,
                                                   const std::vector<uint64_t>* query_indices = nullptr, uint64_t query_base = 0, uint64_t index_base = 0)
    {
        return join<join_result>(queries, c, RF_OP_SIMILARITY, a.to_c(), upper, order, query_indices, query_base, index_base);
    }
    // ---- the same by normalized score (rf_join_f64): "every pair with normalized_similarity >= 0.9" -- bit for bit the doubles normalized_*_filter_many reports
    static std::vector<JoinTripleF64> normalized_distance_join(const Corpus& queries, const Corpus& c, const Args<double>& a, bool upper = false, rf_join_order order = RF_JOIN_BY_QUERY,
                                                               const std::vector<uint64_t>* query_indices = nullptr, uint64_t query_base = 0, uint64_t index_base = 0)
    {
        return join<JoinTripleF64>(queries, c, RF_OP_NORMALIZED_DISTANCE, a.to_c(), upper, order, query_indices, query_base, index_base);
    }
    static std::vector<JoinTripleF64> normalized_similarity_join(const Corpus& queries, const Corpus& c, const Args<double>& a, bool upper = false, rf_join_order order = RF_JOIN_BY_QUERY,
                                                                 const std::vector<uint64_t>* query_indices = nullptr, uint64_t query_base = 0, uint64_t index_base = 0)
    {
        return join<JoinTripleF64>(queries, c, RF_OP_NORMALIZED_SIMILARITY, a.to_c(), upper, order, query_indices, query_base, index_base);
    }

    // ---- the k best candidates of `c` for every row of the packed corpus `queries`, one call (rf_join_topk_u32): res[j] = (index_base + index, score) pairs of row
    // query_indices[j] (nullptr = every row; an empty list: no row) -- what distance_topk_multi of a comparator over that row returns, ordered by (score ascending,
    // index ascending), at most k of them.  No cutoff is needed.  `queries` and `c` may be the same corpus; `no_self` then never offers a row its own candidate
    // (compared by row index), so every record gets its k nearest OTHER records.  The usize metrics' pairs carry a size_t (rf_join_topk_u32); jaro / jaro_winkler's,
    // and every normalized_*_join_topk's, a double (rf_join_topk_f64).
    static std::vector<std::vector<std::pair<uint64_t, usize_result>>> distance_join_topk(const Corpus& queries, const Corpus& c, uint32_t k, const Args<usize_result>& a = {},
                                                                                           bool no_self = false, const std::vector<uint64_t>* query_indices = nullptr,
                                                                                           uint64_t index_base = 0)
    {
        return join_topk<usize_result>(queries, c, k, RF_OP_DISTANCE, a.to_c(), no_self, query_indices, index_base);
    }
    /// the same by similarity: (score descending, index ascending)
    static std::vector<std::vector<std::pair<uint64_t, usize_result>>> similarity_join_topk(const Corpus& queries, const Corpus& c, uint32_t k, const Args<usize_result>& a = {},
                                                                                             bool no_self = false, const std::vector<uint64_t>* query_indices = nullptr,
                                                                                             uint64_t index_base = 0)
    {
        return join_topk<usize_result>(queries, c, k, RF_OP_SIMILARITY, a.to_c(), no_self, query_indices, index_base);
    }
    // ---- the same by normalized score (rf_join_topk_f64): "each record's best matches by normalized_similarity" -- bit for bit the doubles, and the order, of
    // normalized_*_topk_multi of comparators over the same rows.  Over a ragged corpus this ranking differs from distance_join_topk's.
    static std::vector<std::vector<std::pair<uint64_t, double>>> normalized_distance_join_topk(const Corpus& queries, const Corpus& c, uint32_t k, const Args<double>& a = {},
                                                                                                bool no_self = false, const std::vector<uint64_t>* query_indices = nullptr,
                                                                                                uint64_t index_base = 0)
    {
        return join_topk<double>(queries, c, k, RF_OP_NORMALIZED_DISTANCE, a.to_c(), no_self, query_indices, index_base);
    }
    static std::vector<std::vector<std::pair<uint64_t, double>>> normalized_similarity_join_topk(const Corpus& queries, const Corpus& c, uint32_t k, const Args<double>& a = {},
                                                                                                  bool no_self = false, const std::vector<uint64_t>* query_indices = nullptr,
                                                                                                  uint64_t index_base = 0)
    {
        return join_topk<double>(queries, c, k, RF_OP_NORMALIZED_SIMILARITY, a.to_c(), no_self, query_indices, index_base);
    }

    // ---- the reference's per-candidate methods (a one-candidate corpus through the same kernels)
    std::optional<usize_result> distance_with_args(std::string_view s2, const Args<usize_result>& a) const
    {
        return many<usize_result>(Corpus({s2}), RF_OP_DISTANCE, a.to_c(), true)[0];
    }
    std::optional<usize_result> similarity_with_args(std::string_view s2, const Args<usize_result>& a) const
    {
        return many<usize_result>(Corpus({s2}), RF_OP_SIMILARITY, a.to_c(), true)[0];
    }
    std::optional<double> normalized_distance_with_args(std::string_view s2, const Args<double>& a) const
    {
        return many<double>(Corpus({s2}), RF_OP_NORMALIZED_DISTANCE, a.to_c(), true)[0];
    }
    std::optional<double> normalized_similarity_with_args(std::string_view s2, const Args<double>& a) const
    {
        return many<double>(Corpus({s2}), RF_OP_NORMALIZED_SIMILARITY, a.to_c(), true)[0];
    }
    usize_result distance(std::string_view s2) const { return *distance_with_args(s2, {}); }
    usize_result similarity(std::string_view s2) const { return *similarity_with_args(s2, {}); }
    double normalized_distance(std::string_view s2) const { return *normalized_distance_with_args(s2, {}); }
    double normalized_similarity(std::string_view s2) const { return *normalized_similarity_with_args(s2, {}); }

    const rf_comparator* handle() const { return h_; }

private:
    template <class T>
    std::vector<std::optional<T>> many(const Corpus& c, rf_op op, const rf_args& a, bool throw_different_length = false) const
    {
        // (hamming without pad: a candidate of another length is neither a value nor None -- RF_DIFFERENT_LENGTH_*, rfgpu.h)
        std::vector<std::optional<T>> res(c.size());
        if constexpr (std::is_floating_point_v<T>) {
            std::vector<double> out(c.size());
            check(rf_many_f64(h_, c.handle(), op, &a, out.data(), RF_MEM_HOST, nullptr));
            for (size_t i = 0; i < out.size(); ++i) {
                if (M == RF_HAMMING && throw_different_length && rfgpu_is_different_length_f64(out[i])) throw Error(RF_ERR_INVALID_ARG, "Differing length arguments provided");
                if (!std::isnan(out[i])) res[i] = out[i];
            }
        } else {
            std::vector<uint32_t> out(c.size());
            check(rf_many_u32(h_, c.handle(), op, &a, out.data(), RF_MEM_HOST, nullptr));
            for (size_t i = 0; i < out.size(); ++i) {
                if (M == RF_HAMMING && out[i] == RF_DIFFERENT_LENGTH_U32) {
                    if (throw_different_length) throw Error(RF_ERR_INVALID_ARG, "Differing length arguments provided");
                    continue;
                }
                if (out[i] != RF_NONE_U32) res[i] = out[i];
            }
        }
        return res;
    }
    static std::vector<std::vector<std::pair<uint64_t, size_t>>> topk_multi(const std::vector<const BatchComparator*>& scorers, const Corpus& c, uint32_t k, rf_op op,
                                                                            const rf_args& a, uint64_t index_base)
    {
        static_assert(!FloatMetric, "rf_topk_multi_u32 serves the usize-valued metrics");
        std::vector<const rf_comparator*> hs;
        for (const BatchComparator* s : scorers) hs.push_back(s->h_);
        const size_t q = hs.size();
        if (q == 0) return {};  // (an empty vector has no data(): the C ABI refuses a null list even of no queries)
        std::vector<uint32_t> score(q * k), count(q);
        std::vector<uint64_t> index(q * k);
        check(rf_topk_multi_u32(hs.data(), (uint32_t)q, c.handle(), op, &a, k, index_base, score.data(), index.data(), count.data(), nullptr));
        std::vector<std::vector<std::pair<uint64_t, size_t>>> res(q);
        for (size_t j = 0; j < q; ++j)
            for (uint32_t m = 0; m < count[j]; ++m) res[j].emplace_back(index[j * k + m], (size_t)score[j * k + m]);
        return res;
    }
    static std::vector<std::vector<std::pair<uint64_t, double>>> topk_multi_f64(const std::vector<const BatchComparator*>& scorers, const Corpus& c, uint32_t k, rf_op op,
                                                                                const rf_args& a, uint64_t index_base)
    {
        std::vector<const rf_comparator*> hs;
        for (const BatchComparator* s : scorers) hs.push_back(s->h_);
        const size_t q = hs.size();
        if (q == 0) return {};  // (an empty vector has no data(): the C ABI refuses a null list even of no queries)
        std::vector<double> score(q * k);
        std::vector<uint32_t> count(q);
        std::vector<uint64_t> index(q * k);
        check(rf_topk_multi_f64(hs.data(), (uint32_t)q, c.handle(), op, &a, k, index_base, score.data(), index.data(), count.data(), nullptr));
        std::vector<std::vector<std::pair<uint64_t, double>>> res(q);
        for (size_t j = 0; j < q; ++j)
            for (uint32_t m = 0; m < count[j]; ++m) res[j].emplace_back(index[j * k + m], score[j * k + m]);
        return res;
    }
    static std::vector<std::vector<std::pair<uint64_t, size_t>>> filter_multi(const std::vector<const BatchComparator*>& scorers, const Corpus& c, rf_op op, const rf_args& a,
                                                                              rf_filter_order order, uint64_t index_base)
    {
        static_assert(!FloatMetric, "rf_filter_multi_u32 serves the usize-valued metrics");
        std::vector<const rf_comparator*> hs;
        for (const BatchComparator* s : scorers) hs.push_back(s->h_);
        const size_t q = hs.size();
        if (q == 0) return {};  // (an empty vector has no data(): the C ABI refuses a null list even of no queries)
        // (a first guess per row: fused rows sit under a tight cutoff and are short, and q rows of it are allocated here and on the device)
        uint64_t cap = std::clamp<uint64_t>(c.size() / 4096, 64, 1u << 12);
        for (;;) {  // (the device reports the true counts: at most one repeat, with room for the largest)
            std::vector<uint64_t> index(q * cap), count(q);
            std::vector<uint32_t> score(q * cap);
            check(rf_filter_multi_u32(hs.data(), (uint32_t)q, c.handle(), op, &a, index_base, cap, index.data(), score.data(), count.data(), order, nullptr));
            const uint64_t most = *std::max_element(count.begin(), count.end());
            if (most > cap) { cap = most; continue; }
            std::vector<std::vector<std::pair<uint64_t, size_t>>> res(q);
            for (size_t j = 0; j < q; ++j)
                for (uint64_t m = 0; m < count[j]; ++m) res[j].emplace_back(index[j * cap + m], (size_t)score[j * cap + m]);
            return res;
        }
    }
    // (every *_join_topk: Value picks the call -- size_t rf_join_topk_u32, double rf_join_topk_f64)
    template <class Value>
    static std::vector<std::vector<std::pair<uint64_t, Value>>> join_topk(const Corpus& queries, const Corpus& c, uint32_t k, rf_op op, const rf_args& a, bool no_self,
                                                                          const std::vector<uint64_t>* query_indices, uint64_t index_base)
    {
        constexpr bool f64 = std::is_floating_point_v<Value>;
        static_assert(f64 || !FloatMetric, "rf_join_topk_u32 serves the usize-valued metrics");
        using Score = std::conditional_t<f64, double, uint32_t>;
        if (query_indices && query_indices->empty()) return {};  // (an empty selection is no row; only a null pointer asks for every row)
        const uint64_t* qi = query_indices ? query_indices->data() : nullptr;
        const uint64_t m = query_indices ? query_indices->size() : queries.size();
        const uint32_t flags = no_self ? RF_JOIN_NO_SELF : 0u;
        std::vector<Score> score(m * k);
        std::vector<uint32_t> count(m);
        std::vector<uint64_t> index(m * k);
        if constexpr (f64)
            check(rf_join_topk_f64(M, queries.handle(), qi, m, c.handle(), op, &a, flags, k, index_base, score.data(), index.data(), count.data(), nullptr));
        else
            check(rf_join_topk_u32(M, queries.handle(), qi, m, c.handle(), op, &a, flags, k, index_base, score.data(), index.data(), count.data(), nullptr));
        std::vector<std::vector<std::pair<uint64_t, Value>>> res(m);
        for (size_t j = 0; j < m; ++j)
            for (uint32_t t = 0; t < count[j]; ++t) res[j].emplace_back(index[j * k + t], (Value)score[j * k + t]);
        return res;
    }
    // (every *_join: Triple picks the call -- JoinTriple rf_join_u32, JoinTripleF64 rf_join_f64)
    template <class Triple>
    static std::vector<Triple> join(const Corpus& queries, const Corpus& c, rf_op op, const rf_args& a, bool upper, rf_join_order order,
                                    const std::vector<uint64_t>* query_indices, uint64_t query_base, uint64_t index_base)
    {
        constexpr bool f64 = std::is_same_v<Triple, JoinTripleF64>;
        static_assert(f64 || !FloatMetric, "rf_join_u32 serves the usize-valued metrics");
        using Score = std::conditional_t<f64, double, uint32_t>;
        if (query_indices && query_indices->empty()) return {};  // (an empty selection is no pair; only a null pointer asks for every row)
        const uint64_t* qi = query_indices ? query_indices->data() : nullptr;
        const uint64_t m = query_indices ? query_indices->size() : queries.size();
        const uint32_t flags = upper ? RF_JOIN_UPPER : 0u;
        uint64_t count = 0;
        auto call = [&](uint64_t cap, uint64_t* query, uint64_t* index, Score* score) {
            if constexpr (f64)
                check(rf_join_f64(M, queries.handle(), qi, m, c.handle(), op, &a, flags, query_base, index_base, cap, query, index, score, &count, order, nullptr));
            else
                check(rf_join_u32(M, queries.handle(), qi, m, c.handle(), op, &a, flags, query_base, index_base, cap, query, index, score, &count, order, nullptr));
        };
        call(0, nullptr, nullptr, nullptr);  // (a pure count first: the call reports the true number of pairs)
        std::vector<Triple> res;
        if (count == 0) return res;
        std::vector<uint64_t> query(count), index(count);
        std::vector<Score> score(count);
        const uint64_t cap = count;
        call(cap, query.data(), index.data(), score.data());
        res.reserve(std::min(cap, count));
        for (uint64_t t = 0; t < std::min(cap, count); ++t) res.push_back(Triple{query[t], index[t], (decltype(Triple::score))score[t]});
        return res;
    }
    static std::vector<std::vector<std::pair<uint64_t, double>>> filter_multi_f64(const std::vector<const BatchComparator*>& scorers, const Corpus& c, rf_op op,
                                                                                  const rf_args& a, rf_filter_order order, uint64_t index_base)
    {
        std::vector<const rf_comparator*> hs;
        for (const BatchComparator* s : scorers) hs.push_back(s->h_);
        const size_t q = hs.size();
        if (q == 0) return {};  // (an empty vector has no data(): the C ABI refuses a null list even of no queries)
        uint64_t cap = std::clamp<uint64_t>(c.size() / 4096, 64, 1u << 12);
        for (;;) {  // (the device reports the true counts: at most one repeat, with room for the largest)
            std::vector<uint64_t> index(q * cap), count(q);
            std::vector<double> score(q * cap);
            check(rf_filter_multi_f64(hs.data(), (uint32_t)q, c.handle(), op, &a, index_base, cap, index.data(), score.data(), count.data(), order, nullptr));
            const uint64_t most = *std::max_element(count.begin(), count.end());
            if (most > cap) { cap = most; continue; }
            std::vector<std::vector<std::pair<uint64_t, double>>> res(q);
            for (size_t j = 0; j < q; ++j)
                for (uint64_t m = 0; m < count[j]; ++m) res[j].emplace_back(index[j * cap + m], score[j * cap + m]);
            return res;
        }
    }
    template <class T>
    std::vector<std::pair<uint64_t, T>> filter(const Corpus& c, rf_op op, const rf_args& a, rf_filter_order order) const
    {
        uint64_t cap = std::max<uint64_t>(1024, c.size() / 64), n = 0;
        for (;;) {  // (the device reports the true number of matches: at most one repeat)
            std::vector<uint64_t> idx(cap);
            std::vector<std::pair<uint64_t, T>> res;
            if constexpr (std::is_floating_point_v<T>) {
                std::vector<double> val(cap);
                check(rf_filter_f64(h_, c.handle(), op, &a, 0, cap, idx.data(), val.data(), &n, RF_MEM_HOST, order, nullptr));
                if (n > cap) { cap = n; continue; }
                for (uint64_t i = 0; i < n; ++i) res.emplace_back(idx[i], val[i]);
            } else {
                std::vector<uint32_t> val(cap);
                check(rf_filter_u32(h_, c.handle(), op, &a, 0, cap, idx.data(), val.data(), &n, RF_MEM_HOST, order, nullptr));
                if (n > cap) { cap = n; continue; }
                for (uint64_t i = 0; i < n; ++i) res.emplace_back(idx[i], (T)val[i]);
            }
            return res;
        }
    }
    rf_comparator* h_ = nullptr;
};

template <rf_metric M, bool F>
struct Module {
    using WeightTable = detail::WeightTable;
    template <class T>
    using Args = detail::Args<T>;
    using BatchComparator = detail::BatchComparator<M, F>;
    using R = std::conditional_t<F, double, size_t>;
    static R distance(std::string_view s1, std::string_view s2) { return BatchComparator(s1).distance(s2); }
    static std::optional<R> distance_with_args(std::string_view s1, std::string_view s2, const Args<R>& a)
    {
        return BatchComparator(s1).distance_with_args(s2, a);
    }
    static R similarity(std::string_view s1, std::string_view s2) { return BatchComparator(s1).similarity(s2); }
    static std::optional<R> similarity_with_args(std::string_view s1, std::string_view s2, const Args<R>& a)
    {
        return BatchComparator(s1).similarity_with_args(s2, a);
    }
    static double normalized_distance(std::string_view s1, std::string_view s2) { return BatchComparator(s1).normalized_distance(s2); }
    static double normalized_similarity(std::string_view s1, std::string_view s2) { return BatchComparator(s1).normalized_similarity(s2); }
};

}  // namespace detail

namespace distance {
using levenshtein = detail::Module<RF_LEVENSHTEIN, false>;    // src/distance/levenshtein.rs
using indel = detail::Module<RF_INDEL, false>;                // src/distance/indel.rs
using lcs_seq = detail::Module<RF_LCS_SEQ, false>;            // src/distance/lcs_seq.rs
using damerau_levenshtein = detail::Module<RF_DAMERAU_LEVENSHTEIN, false>;  // src/distance/damerau_levenshtein.rs
using hamming = detail::Module<RF_HAMMING, false>;            // src/distance/hamming.rs (Args::pad)
using prefix = detail::Module<RF_PREFIX, false>;              // src/distance/prefix.rs
using postfix = detail::Module<RF_POSTFIX, false>;            // src/distance/postfix.rs
using jaro = detail::Module<RF_JARO, true>;                   // src/distance/jaro.rs
using jaro_winkler = detail::Module<RF_JARO_WINKLER, true>;   // src/distance/jaro_winkler.rs
}  // namespace distance

namespace fuzz {
/// src/fuzz.rs:98-150 (similarity only; reproduces fuzz.rs:141 unless RF_FLAG_RATIO_INDEL_NORMALIZATION is set)
class RatioBatchComparator {
public:
    explicit RatioBatchComparator(std::string_view s1) : c_(s1) {}
    std::vector<std::optional<double>> similarity_many(const Corpus& c, const detail::Args<double>& a = {}) const
    {
        return c_.similarity_many(c, a);
    }
    double similarity(std::string_view s2) const { return *c_.similarity_with_args(s2, {}); }
    /// the k best candidates of every scorer, one call (rf_topk_multi_f64): (index_base + index, ratio) pairs, ratio descending, ties by index
    static std::vector<std::vector<std::pair<uint64_t, double>>> similarity_topk_multi(const std::vector<const RatioBatchComparator*>& scorers, const Corpus& c, uint32_t k,
                                                                                        const detail::Args<double>& a = {}, uint64_t index_base = 0)
    {
        std::vector<const detail::BatchComparator<RF_FUZZ_RATIO, true>*> inner;
        for (const RatioBatchComparator* s : scorers) inner.push_back(&s->c_);
        return detail::BatchComparator<RF_FUZZ_RATIO, true>::normalized_similarity_topk_multi(inner, c, k, a, index_base);
    }
    /// the candidates whose ratio reaches the cutoff (rf_filter_f64): (index, ratio) pairs, in `order`
    std::vector<std::pair<uint64_t, double>> similarity_filter_many(const Corpus& c, const detail::Args<double>& a = {}, rf_filter_order order = RF_FILTER_BY_INDEX) const
    {
        return c_.normalized_similarity_filter_many(c, a, order);
    }
    /// the same for every scorer, one call (rf_filter_multi_f64): res[j] = similarity_filter_many of scorers[j], indices offset by index_base
    static std::vector<std::vector<std::pair<uint64_t, double>>> similarity_filter_multi(const std::vector<const RatioBatchComparator*>& scorers, const Corpus& c,
                                                                                          const detail::Args<double>& a = {}, rf_filter_order order = RF_FILTER_BY_INDEX,
                                                                                          uint64_t index_base = 0)
    {
        std::vector<const detail::BatchComparator<RF_FUZZ_RATIO, true>*> inner;
        for (const RatioBatchComparator* s : scorers) inner.push_back(&s->c_);
        return detail::BatchComparator<RF_FUZZ_RATIO, true>::normalized_similarity_filter_multi(inner, c, a, order, index_base);
    }
    /// every pair (row of `queries`, candidate of `c`) whose ratio reaches the cutoff, one call (rf_join_f64); see BatchComparator::distance_join
    using JoinTripleF64 = detail::JoinTripleF64;
    static std::vector<JoinTripleF64> similarity_join(const Corpus& queries, const Corpus& c, const detail::Args<double>& a, bool upper = false, rf_join_order order = RF_JOIN_BY_QUERY,
                                                      const std::vector<uint64_t>* query_indices = nullptr, uint64_t query_base = 0, uint64_t index_base = 0)
    {
        return detail::BatchComparator<RF_FUZZ_RATIO, true>::similarity_join(queries, c, a, upper, order, query_indices, query_base, index_base);
    }
    static std::vector<JoinTripleF64> normalized_similarity_join(const Corpus& queries, const Corpus& c, const detail::Args<double>& a, bool upper = false,
                                                                 rf_join_order order = RF_JOIN_BY_QUERY, const std::vector<uint64_t>* query_indices = nullptr,
                                                                 uint64_t query_base = 0, uint64_t index_base = 0)
    {
        return detail::BatchComparator<RF_FUZZ_RATIO, true>::normalized_similarity_join(queries, c, a, upper, order, query_indices, query_base, index_base);
    }
    /// the k best candidates of `c` by ratio for every row of the packed corpus `queries`, one call (rf_join_topk_f64); see BatchComparator::distance_join_topk
    static std::vector<std::vector<std::pair<uint64_t, double>>> similarity_join_topk(const Corpus& queries, const Corpus& c, uint32_t k, const detail::Args<double>& a = {},
                                                                                       bool no_self = false, const std::vector<uint64_t>* query_indices = nullptr,
                                                                                       uint64_t index_base = 0)
    {
        return detail::BatchComparator<RF_FUZZ_RATIO, true>::similarity_join_topk(queries, c, k, a, no_self, query_indices, index_base);
    }
    static std::vector<std::vector<std::pair<uint64_t, double>>> normalized_similarity_join_topk(const Corpus& queries, const Corpus& c, uint32_t k, const detail::Args<double>& a = {},
                                                                                                  bool no_self = false, const std::vector<uint64_t>* query_indices = nullptr,
                                                                                                  uint64_t index_base = 0)
    {
        return detail::BatchComparator<RF_FUZZ_RATIO, true>::normalized_similarity_join_topk(queries, c, k, a, no_self, query_indices, index_base);
    }

private:
    detail::BatchComparator<RF_FUZZ_RATIO, true> c_;
};
/// fuzz::ratio (src/fuzz.rs:48-85) = normalized Indel similarity
inline double ratio(std::string_view s1, std::string_view s2) { return distance::indel::normalized_similarity(s1, s2); }
}  // namespace fuzz

}  // namespace rapidfuzz

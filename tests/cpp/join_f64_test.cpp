// normalized_distance_join / normalized_similarity_join and the ratio's and jaro's *_join of the C++ facade (include/rapidfuzz_amd.hpp) over rf_join_f64.
// Without a GPU it checks that the calls compile (members of a class template exist only once used), that the C call's argument checks answer without a
// device and write nothing; with a GPU (argv[1] == "gpu") a small self-join by normalized_similarity_join, by normalized_distance_join and by the ratio's
// similarity_join equals values computed here from the rows' known edit counts, bit for bit.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <tuple>
#include <type_traits>
#include <utility>

#include "rapidfuzz_amd.hpp"

using namespace rapidfuzz;
using Lev = distance::levenshtein::BatchComparator;
using Indel = distance::indel::BatchComparator;
using Jaro = distance::jaro::BatchComparator;
using JaroWinkler = distance::jaro_winkler::BatchComparator;
using Ratio = fuzz::RatioBatchComparator;
using F64Args = distance::levenshtein::Args<double>;
using Triples = std::vector<std::tuple<uint64_t, uint64_t, double>>;

#define EXPECT(c)                                                     \
    do {                                                              \
        if (!(c)) {                                                   \
            std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                 \
        }                                                             \
    } while (0)

static Triples flat(const std::vector<detail::JoinTripleF64>& r)
{
    Triples t;
    for (const auto& x : r) t.emplace_back(x.query, x.candidate, x.score);
    return t;
}

int main(int argc, char** argv)
{
    const bool gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    if (!gpu) {
        rf_args a;
        rf_args_default(&a);
        a.cutoff_f64 = 0.9;
        double score[2] = {7, 7};
        uint64_t query[2] = {7, 7}, index[2] = {7, 7}, count = 9, rows[2] = {0, 1};
        alignas(16) static unsigned char never_read[2][8192];  // stand in for the corpora: the calls below are refused (or answered) before they look at one
        const rf_corpus* q = reinterpret_cast<const rf_corpus*>(never_read[0]);
        const rf_corpus* c = reinterpret_cast<const rf_corpus*>(never_read[1]);
        const rf_op NS = RF_OP_NORMALIZED_SIMILARITY, ND = RF_OP_NORMALIZED_DISTANCE;
        EXPECT(rf_join_f64(RF_LEVENSHTEIN, q, rows, 2, c, NS, &a, 0, 0, 0, 2, query, index, score, &count, (rf_join_order)7, nullptr) == RF_ERR_INVALID_ARG);
        EXPECT(rf_join_f64(RF_LEVENSHTEIN, q, rows, 2, c, NS, &a, 0, 0, 0, 2, nullptr, index, score, &count, RF_JOIN_BY_QUERY, nullptr) == RF_ERR_INVALID_ARG);
        EXPECT(rf_join_f64(RF_LEVENSHTEIN, q, rows, 2, c, NS, &a, 0, 0, 0, 2, query, index, nullptr, &count, RF_JOIN_BY_QUERY, nullptr) == RF_ERR_INVALID_ARG);
        EXPECT(rf_join_f64(RF_LEVENSHTEIN, q, rows, 2, c, RF_OP_DISTANCE, &a, 0, 0, 0, 2, query, index, score, &count, RF_JOIN_BY_QUERY, nullptr) == RF_ERR_INVALID_ARG);
        EXPECT(std::strstr(rf_last_error(), "rf_join_u32") != nullptr);  // (the message points to the u32 call)
        EXPECT(rf_join_f64(RF_INDEL, q, rows, 2, c, RF_OP_SIMILARITY, &a, 0, 0, 0, 2, query, index, score, &count, RF_JOIN_BY_QUERY, nullptr) == RF_ERR_INVALID_ARG);
        EXPECT(rf_join_f64(RF_FUZZ_RATIO, q, rows, 2, c, ND, &a, 0, 0, 0, 2, query, index, score, &count, RF_JOIN_BY_QUERY, nullptr) == RF_ERR_INVALID_ARG);
        EXPECT(rf_join_f64((rf_metric)99, q, rows, 2, c, NS, &a, 0, 0, 0, 2, query, index, score, &count, RF_JOIN_BY_QUERY, nullptr) == RF_ERR_INVALID_ARG);
        EXPECT(rf_join_f64(RF_LEVENSHTEIN, q, rows, 2, c, NS, &a, 2u, 0, 0, 2, query, index, score, &count, RF_JOIN_BY_QUERY, nullptr) == RF_ERR_INVALID_ARG);
        rf_args nan_cutoff = a;
        nan_cutoff.cutoff_f64 = std::numeric_limits<double>::quiet_NaN();
        EXPECT(rf_join_f64(RF_LEVENSHTEIN, q, rows, 2, c, NS, &nan_cutoff, 0, 0, 0, 2, query, index, score, &count, RF_JOIN_BY_QUERY, nullptr) == RF_ERR_INVALID_ARG);
        EXPECT(rf_join_f64(RF_JARO, q, rows, 2, c, RF_OP_DISTANCE, &nan_cutoff, 0, 0, 0, 2, query, index, score, &count, RF_JOIN_BY_QUERY, nullptr) == RF_ERR_INVALID_ARG);
        EXPECT(rf_join_f64(RF_LEVENSHTEIN, q, rows, 0, c, NS, &a, 0, 0, 0, 2, query, index, score, &count, RF_JOIN_BY_QUERY, nullptr) == RF_OK);
        EXPECT(count == 9 && score[0] == 7 && score[1] == 7 && index[1] == 7 && query[0] == 7);
        // the facade's functions exist and are well-formed: naming them instantiates them
        auto f1 = &Lev::normalized_distance_join;
        auto f2 = &Indel::normalized_similarity_join;
        auto f3 = &Ratio::similarity_join;
        auto f4 = &Ratio::normalized_similarity_join;
        auto f5 = &Jaro::distance_join;
        auto f6 = &Jaro::similarity_join;
        auto f7 = &JaroWinkler::normalized_distance_join;
        auto f8 = &JaroWinkler::normalized_similarity_join;
        auto f9 = &Lev::distance_join;  // (still the u32 call's triples)
        EXPECT(f1 && f2 && f3 && f4 && f5 && f6 && f7 && f8 && f9);
        static_assert(std::is_same_v<decltype(Lev::distance_join(std::declval<Corpus&>(), std::declval<Corpus&>(), {}))::value_type, Lev::JoinTriple>);
        static_assert(std::is_same_v<decltype(Jaro::distance_join(std::declval<Corpus&>(), std::declval<Corpus&>(), {}))::value_type, detail::JoinTripleF64>);
        std::printf("join_f64 ok (cpu)\n");
        return 0;
    }
    // rows of 10 symbols whose edit counts are known: 1 = row 0 with one substitution, 2 = row 0 with two, 1 -> 2 is one more substitution at a place
    // where 1 already differs plus one elsewhere; 3 shares no symbol with the others
    //                                     0             1             2             3
    const std::vector<std::string> rows{"abcdefghij", "abcdefghiX", "abcdefghXY", "zzzzzzzzzz"};
    std::vector<std::string_view> views(rows.begin(), rows.end());
    Corpus corpus(views);
    const double one = 1.0 / 10.0, two = 2.0 / 10.0;
    {   // Levenshtein: d(0,1) = 1, d(0,2) = 2, d(1,2) = 2 (i -> X, X -> Y), everything against row 3 is 10
        const auto sim = flat(Lev::normalized_similarity_join(corpus, corpus, F64Args{}.score_cutoff(0.75), true));
        EXPECT((sim == Triples{{0, 1, 1.0 - one}, {0, 2, 1.0 - two}, {1, 2, 1.0 - two}}));
        const auto dist = flat(Lev::normalized_distance_join(corpus, corpus, F64Args{}.score_cutoff(0.25), true));
        EXPECT((dist == Triples{{0, 1, one}, {0, 2, two}, {1, 2, two}}));
        const auto full = flat(Lev::normalized_similarity_join(corpus, corpus, F64Args{}.score_cutoff(0.85)));
        EXPECT((full == Triples{{0, 0, 1.0}, {0, 1, 1.0 - one}, {1, 0, 1.0 - one}, {1, 1, 1.0}, {2, 2, 1.0}, {3, 3, 1.0}}));
        // rows in any order with repeats, bases beyond 32 bits; the flag compares the candidate with the ROW's index
        const uint64_t base = (1ull << 32) + 5;
        const std::vector<uint64_t> pick{2, 0, 2, 1};
        const auto picked = flat(Lev::normalized_similarity_join(corpus, corpus, F64Args{}.score_cutoff(0.75), true, RF_JOIN_BY_QUERY, &pick, base, base));
        EXPECT((picked == Triples{{base, base + 1, 1.0 - one}, {base, base + 2, 1.0 - two}, {base + 1, base + 2, 1.0 - two}}));
        const std::vector<uint64_t> none;
        EXPECT(Lev::normalized_similarity_join(corpus, corpus, F64Args{}.score_cutoff(0.75), false, RF_JOIN_BY_QUERY, &none).empty());
        bool refused = false;
        try {
            (void)Lev::normalized_similarity_join(corpus, corpus, F64Args{});  // no cutoff
        } catch (const Error& e) {
            refused = e.status == RF_ERR_INVALID_ARG;
        }
        EXPECT(refused);
    }
    {   // the ratio (the inner lcs_seq comparator's normalization: 1 - (10 - lcs) / 10): lcs(0,1) = 9, lcs(0,2) = 8, lcs(1,2) = 9 ("abcdefghX")
        const auto r = flat(Ratio::similarity_join(corpus, corpus, F64Args{}.score_cutoff(0.85), true));
        EXPECT((r == Triples{{0, 1, 1.0 - one}, {1, 2, 1.0 - one}}));
        const auto n = flat(Ratio::normalized_similarity_join(corpus, corpus, F64Args{}.score_cutoff(0.75), true));
        EXPECT((n == Triples{{0, 1, 1.0 - one}, {0, 2, 1.0 - two}, {1, 2, 1.0 - one}}));
        // ... and with the documented Indel normalization: 1 - (20 - 2 lcs) / 20
        F64Args indel_norm = F64Args{}.score_cutoff(0.85);
        indel_norm.flags |= RF_FLAG_RATIO_INDEL_NORMALIZATION;
        const auto d = flat(Ratio::similarity_join(corpus, corpus, indel_norm, true));
        EXPECT((d == Triples{{0, 1, 1.0 - 2.0 / 20.0}, {1, 2, 1.0 - 2.0 / 20.0}}));
    }
    {   // jaro_winkler goes per query: equal to the loop of its own filter
        Triples exp;
        for (uint64_t qi = 0; qi < rows.size(); ++qi)
            for (const auto& p : JaroWinkler(rows[qi]).similarity_filter_many(corpus, F64Args{}.score_cutoff(0.9))) exp.emplace_back(qi, p.first, p.second);
        EXPECT(flat(JaroWinkler::similarity_join(corpus, corpus, F64Args{}.score_cutoff(0.9))) == exp);
        EXPECT(exp.size() >= 6);
    }
    std::printf("join_f64 ok (gpu)\n");
    return 0;
}

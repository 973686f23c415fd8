// normalized_distance_join_topk / normalized_similarity_join_topk of the C++ facade (include/rapidfuzz_amd.hpp) over rf_join_topk_f64, the ratio's
// similarity_join_topk and jaro's distance_join_topk / similarity_join_topk.  Without a GPU it checks that the calls compile (members of a class template exist only
// once used), that the C call's argument checks answer without a device and that an empty selection of rows is an empty result; with a GPU (argv[1] == "gpu") every
// row equals -- the doubles compared with == -- the facade's normalized_*_topk_multi of one scorer over the same row, on a 6-string corpus joined with itself (with
// and without no_self) and on a 700-string corpus, for a selection of rows in any order with repeats and a base beyond 32 bits.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>

#include "rapidfuzz_amd.hpp"

using namespace rapidfuzz;
using Lev = distance::levenshtein::BatchComparator;
using Indel = distance::indel::BatchComparator;
using Jaro = distance::jaro::BatchComparator;
using Ratio = fuzz::RatioBatchComparator;
using LevArgs = distance::levenshtein::Args<double>;
using IndelArgs = distance::indel::Args<double>;
using Row = std::vector<std::pair<uint64_t, double>>;

#define EXPECT(c)                                                     \
    do {                                                              \
        if (!(c)) {                                                   \
            std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                 \
        }                                                             \
    } while (0)

// the loop the call stands for: one scorer per selected row, its top-k over the corpus (k + 1 and the row's own entry dropped under no_self)
template <class Scorer, class A>
static std::vector<Row> loop(const std::vector<std::string>& rows, const std::vector<uint64_t>& pick, const Corpus& c, uint32_t k, const A& a, bool similarity, bool no_self,
                             uint64_t ibase)
{
    std::vector<Row> res;
    for (uint64_t qi : pick) {
        Scorer s(rows[qi]);
        const auto full =
            (similarity ? Scorer::normalized_similarity_topk_multi({&s}, c, k + 1, a, ibase) : Scorer::normalized_distance_topk_multi({&s}, c, k + 1, a, ibase))[0];
        Row r;
        for (const auto& p : full)
            if (r.size() < k && !(no_self && p.first == ibase + qi)) r.push_back(p);
        res.push_back(r);
    }
    return res;
}
static std::vector<Row> ratio_loop(const std::vector<std::string>& rows, const std::vector<uint64_t>& pick, const Corpus& c, uint32_t k, uint64_t ibase)
{
    std::vector<Row> res;
    for (uint64_t qi : pick) {
        Ratio s(rows[qi]);
        res.push_back(Ratio::similarity_topk_multi({&s}, c, k, {}, ibase)[0]);
    }
    return res;
}

static std::vector<uint64_t> all_rows(size_t n)
{
    std::vector<uint64_t> v(n);
    for (size_t i = 0; i < n; ++i) v[i] = i;
    return v;
}

int main(int argc, char** argv)
{
    const bool gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    if (!gpu) {
        rf_args a;
        rf_args_default(&a);
        double score[4] = {7, 7, 7, 7};
        uint32_t count[2] = {9, 9};
        uint64_t index[4] = {7, 7, 7, 7}, rows[2] = {0, 1};
        alignas(16) static unsigned char never_read[2][8192];  // stand in for the corpora: the calls below are refused (or answered) before they look at one
        const rf_corpus* q = reinterpret_cast<const rf_corpus*>(never_read[0]);
        const rf_corpus* c = reinterpret_cast<const rf_corpus*>(never_read[1]);
        const rf_op ns = RF_OP_NORMALIZED_SIMILARITY;
        EXPECT(rf_join_topk_f64(RF_LEVENSHTEIN, q, rows, 2, c, ns, &a, 0, 0, 0, score, index, count, nullptr) == RF_ERR_INVALID_ARG);  // k == 0
        EXPECT(rf_join_topk_f64(RF_LEVENSHTEIN, q, rows, 2, c, RF_OP_DISTANCE, &a, 0, 2, 0, score, index, count, nullptr) == RF_ERR_INVALID_ARG);
        EXPECT(rf_join_topk_f64(RF_FUZZ_RATIO, q, rows, 2, c, RF_OP_NORMALIZED_DISTANCE, &a, 0, 2, 0, score, index, count, nullptr) == RF_ERR_INVALID_ARG);
        EXPECT(rf_join_topk_f64(RF_LEVENSHTEIN, q, rows, 2, c, ns, &a, RF_JOIN_UPPER, 2, 0, score, index, count, nullptr) == RF_ERR_INVALID_ARG);
        EXPECT(rf_join_topk_f64(RF_LEVENSHTEIN, q, rows, 2, c, ns, &a, RF_JOIN_NO_SELF, 2, 0, score, nullptr, count, nullptr) == RF_ERR_INVALID_ARG);
        EXPECT(rf_join_topk_f64(RF_JARO, q, rows, 0, c, RF_OP_DISTANCE, &a, RF_JOIN_NO_SELF, 2, 0, nullptr, nullptr, nullptr, nullptr) == RF_OK);
        EXPECT(count[0] == 9 && count[1] == 9 && score[0] == 7 && index[3] == 7);
        // the facade's functions exist and are well-formed: naming them instantiates them
        auto dj = &Lev::normalized_distance_join_topk;
        auto sj = &Indel::normalized_similarity_join_topk;
        auto rj = &Ratio::similarity_join_topk;
        auto rn = &Ratio::normalized_similarity_join_topk;
        auto jd = &Jaro::distance_join_topk;
        auto js = &Jaro::similarity_join_topk;
        auto ud = &Lev::distance_join_topk;  // (the u32 call's entry keeps its type)
        std::vector<std::vector<std::pair<uint64_t, size_t>>> (*u32_type)(const Corpus&, const Corpus&, uint32_t, const distance::levenshtein::Args<size_t>&, bool,
                                                                            const std::vector<uint64_t>*, uint64_t) = ud;
        EXPECT(dj != nullptr && sj != nullptr && rj != nullptr && rn != nullptr && jd != nullptr && js != nullptr && u32_type != nullptr);
        std::printf("join_topk_f64 ok (cpu)\n");
        return 0;
    }
    const uint64_t base = (1ull << 32) + 5;
    size_t entries = 0;
    {   // six strings joined with themselves
        const std::vector<std::string> six{"kitten", "mitten", "", "sitting", "kitten", "bitten"};
        std::vector<std::string_view> views(six.begin(), six.end());
        Corpus corpus(views);
        const auto every = all_rows(six.size());
        for (uint32_t k : {1u, 2u, 6u, 9u})
            for (bool no_self : {false, true}) {
                const auto got = Lev::normalized_similarity_join_topk(corpus, corpus, k, LevArgs{}, no_self);
                EXPECT(got == (loop<Lev>(six, every, corpus, k, LevArgs{}, true, no_self, 0)));
                for (const auto& r : got) entries += r.size();
            }
        const auto nearest = Lev::normalized_distance_join_topk(corpus, corpus, 1, LevArgs{}, true);
        // (the empty row: every candidate is at normalized distance 1.0, the smallest index wins)
        EXPECT(nearest.size() == 6 && (nearest[0] == Row{{4, 0.0}}) && (nearest[4] == Row{{0, 0.0}}) && (nearest[1] == Row{{0, 1.0 / 6.0}}) && (nearest[2] == Row{{0, 1.0}}));
        // rows in any order, with repeats, no_self on: the candidate is compared with the ROW's index, not with its place in the list
        const std::vector<uint64_t> pick{4, 0, 4, 5, 1};
        for (bool no_self : {false, true})
            EXPECT(Lev::normalized_distance_join_topk(corpus, corpus, 2, LevArgs{}, no_self, &pick, base) == (loop<Lev>(six, pick, corpus, 2, LevArgs{}, false, no_self, base)));
        const std::vector<uint64_t> none;
        EXPECT(Lev::normalized_similarity_join_topk(corpus, corpus, 2, LevArgs{}, false, &none).empty());  // an empty selection is no row
        // an optional cutoff: rows may come back short
        const auto cut = Lev::normalized_distance_join_topk(corpus, corpus, 6, LevArgs{}.score_cutoff(0.2), true);
        EXPECT(cut == (loop<Lev>(six, every, corpus, 6, LevArgs{}.score_cutoff(0.2), false, true, 0)));
        EXPECT(cut[2].empty() && cut[0].size() == 3);
        EXPECT(Ratio::similarity_join_topk(corpus, corpus, 3) == ratio_loop(six, every, corpus, 3, 0));
    }
    {   // queries of one corpus against the 700 candidates of another
        std::vector<std::string> cands;
        const std::string words[3] = {"kitten", "sitting", "mitten"};
        for (int i = 0; i < 700; ++i) {
            std::string w = words[i % 3];
            std::rotate(w.begin(), w.begin() + i % w.size(), w.end());
            if (i % 5 == 0) w += std::to_string(i);
            cands.push_back(i % 67 == 11 ? "kitten" : (i % 71 == 13 ? "mitten" : w));
        }
        std::vector<std::string_view> views(cands.begin(), cands.end());
        Corpus corpus(views);
        const std::vector<std::string> qs{"kitten", "mitten", "sitting", "", "kitten", "ittenk5"};
        std::vector<std::string_view> qviews(qs.begin(), qs.end());
        Corpus queries(qviews);
        const auto every = all_rows(qs.size());
        for (uint32_t k : {1u, 16u, 64u, 65u}) {
            const auto got = Lev::normalized_similarity_join_topk(queries, corpus, k);
            EXPECT(got == (loop<Lev>(qs, every, corpus, k, LevArgs{}, true, false, 0)));
            for (const auto& r : got) entries += r.size();
        }
        EXPECT(Indel::normalized_distance_join_topk(queries, corpus, 5) == (loop<Indel>(qs, every, corpus, 5, IndelArgs{}, false, false, 0)));
        EXPECT(Indel::normalized_similarity_join_topk(queries, corpus, 5, IndelArgs{}, false, nullptr, base) == (loop<Indel>(qs, every, corpus, 5, IndelArgs{}, true, false, base)));
        EXPECT(Ratio::similarity_join_topk(queries, corpus, 16, {}, false, nullptr, base) == ratio_loop(qs, every, corpus, 16, base));
        EXPECT(Ratio::normalized_similarity_join_topk(queries, corpus, 16, {}, false, nullptr, base) == ratio_loop(qs, every, corpus, 16, base));
        const auto jaro = Jaro::similarity_join_topk(queries, corpus, 4);
        EXPECT(jaro.size() == qs.size() && jaro[0].size() == 4 && jaro[0][0].second == 1.0);
    }
    EXPECT(entries > 400);
    std::printf("join_topk_f64 ok (gpu)\n");
    return 0;
}

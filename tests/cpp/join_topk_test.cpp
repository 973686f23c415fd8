// distance_join_topk / similarity_join_topk of the C++ facade (include/rapidfuzz_amd.hpp) over rf_join_topk_u32.  Without a GPU it checks that the calls compile
// (members of a class template exist only once used), that the C call's argument checks answer without a device and that an empty selection of rows is an empty
// result; with a GPU (argv[1] == "gpu") every row equals the facade's distance_topk_multi / similarity_topk_multi of one scorer over the same row, on a 6-string corpus joined
// with itself (with and without no_self) and on a 700-string corpus, for a selection of rows in any order with repeats and a base beyond 32 bits.
#include <cstdio>
#include <cstring>
#include <string>

#include "rapidfuzz_amd.hpp"

using namespace rapidfuzz;
using Lev = distance::levenshtein::BatchComparator;
using Indel = distance::indel::BatchComparator;
using LevArgs = distance::levenshtein::Args<size_t>;
using IndelArgs = distance::indel::Args<size_t>;
using Row = std::vector<std::pair<uint64_t, size_t>>;

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
        const auto full = (similarity ? Scorer::similarity_topk_multi({&s}, c, k + 1, a, ibase) : Scorer::distance_topk_multi({&s}, c, k + 1, a, ibase))[0];
        Row r;
        for (const auto& p : full)
            if (r.size() < k && !(no_self && p.first == ibase + qi)) r.push_back(p);
        res.push_back(r);
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
        uint32_t score[4] = {7, 7, 7, 7}, count[2] = {9, 9};
        uint64_t index[4] = {7, 7, 7, 7}, rows[2] = {0, 1};
        alignas(16) static unsigned char never_read[2][8192];  // stand in for the corpora: the calls below are refused (or answered) before they look at one
        const rf_corpus* q = reinterpret_cast<const rf_corpus*>(never_read[0]);
        const rf_corpus* c = reinterpret_cast<const rf_corpus*>(never_read[1]);
        EXPECT(rf_join_topk_u32(RF_LEVENSHTEIN, q, rows, 2, c, RF_OP_DISTANCE, &a, 0, 0, 0, score, index, count, nullptr) == RF_ERR_INVALID_ARG);  // k == 0
        EXPECT(rf_join_topk_u32(RF_LEVENSHTEIN, q, rows, 2, c, RF_OP_NORMALIZED_DISTANCE, &a, 0, 2, 0, score, index, count, nullptr) == RF_ERR_INVALID_ARG);
        EXPECT(rf_join_topk_u32(RF_JARO, q, rows, 2, c, RF_OP_DISTANCE, &a, 0, 2, 0, score, index, count, nullptr) == RF_ERR_INVALID_ARG);
        EXPECT(rf_join_topk_u32(RF_LEVENSHTEIN, q, rows, 2, c, RF_OP_DISTANCE, &a, RF_JOIN_UPPER, 2, 0, score, index, count, nullptr) == RF_ERR_INVALID_ARG);
        EXPECT(rf_join_topk_u32(RF_LEVENSHTEIN, q, rows, 2, c, RF_OP_DISTANCE, &a, RF_JOIN_NO_SELF, 2, 0, score, nullptr, count, nullptr) == RF_ERR_INVALID_ARG);
        EXPECT(rf_join_topk_u32(RF_LEVENSHTEIN, q, rows, 0, c, RF_OP_DISTANCE, &a, RF_JOIN_NO_SELF, 2, 0, nullptr, nullptr, nullptr, nullptr) == RF_OK);
        EXPECT(count[0] == 9 && count[1] == 9 && score[0] == 7 && index[3] == 7);
        // the facade's functions exist and are well-formed: naming them instantiates them
        auto dj = &Lev::distance_join_topk;
        auto sj = &Indel::similarity_join_topk;
        EXPECT(dj != nullptr && sj != nullptr);
        std::printf("join_topk ok (cpu)\n");
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
                const auto got = Lev::distance_join_topk(corpus, corpus, k, LevArgs{}, no_self);
                EXPECT(got == (loop<Lev>(six, every, corpus, k, LevArgs{}, false, no_self, 0)));
                for (const auto& r : got) entries += r.size();
            }
        const auto nearest = Lev::distance_join_topk(corpus, corpus, 1, LevArgs{}, true);
        EXPECT(nearest.size() == 6 && (nearest[0] == Row{{4, 0}}) && (nearest[4] == Row{{0, 0}}) && (nearest[1] == Row{{0, 1}}) && (nearest[2] == Row{{0, 6}}));
        // rows in any order, with repeats, no_self on: the candidate is compared with the ROW's index, not with its place in the list
        const std::vector<uint64_t> pick{4, 0, 4, 5, 1};
        for (bool no_self : {false, true})
            EXPECT(Lev::distance_join_topk(corpus, corpus, 2, LevArgs{}, no_self, &pick, base) == (loop<Lev>(six, pick, corpus, 2, LevArgs{}, false, no_self, base)));
        const std::vector<uint64_t> none;
        EXPECT(Lev::distance_join_topk(corpus, corpus, 2, LevArgs{}, false, &none).empty());  // an empty selection is no row
        // an optional cutoff: rows may come back short
        const auto cut = Lev::distance_join_topk(corpus, corpus, 6, LevArgs{}.score_cutoff(1), true);
        EXPECT(cut == (loop<Lev>(six, every, corpus, 6, LevArgs{}.score_cutoff(1), false, true, 0)));
        EXPECT(cut[2].empty() && cut[0].size() == 3);
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
            const auto got = Lev::distance_join_topk(queries, corpus, k);
            EXPECT(got == (loop<Lev>(qs, every, corpus, k, LevArgs{}, false, false, 0)));
            for (const auto& r : got) entries += r.size();
        }
        EXPECT(Indel::distance_join_topk(queries, corpus, 5) == (loop<Indel>(qs, every, corpus, 5, IndelArgs{}, false, false, 0)));
        EXPECT(Indel::similarity_join_topk(queries, corpus, 5, IndelArgs{}, false, nullptr, base) == (loop<Indel>(qs, every, corpus, 5, IndelArgs{}, true, false, base)));
    }
    EXPECT(entries > 400);
    std::printf("join_topk ok (gpu)\n");
    return 0;
}

// distance_join / similarity_join of the C++ facade (include/rapidfuzz_amd.hpp) over rf_join_u32.  Without a GPU it checks that the calls compile (members of
// a class template exist only once used), that the C call's argument checks answer without a device and that an empty selection of rows is an empty result;
// with a GPU (argv[1] == "gpu") the triples equal a loop of the facade's single-query distance_filter_many over the rows, on a 6-string corpus and a
// 700-string corpus, with and without `upper`, for a selection of rows in any order with repeats, and with bases beyond 32 bits.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <tuple>

#include "rapidfuzz_amd.hpp"

using namespace rapidfuzz;
using Lev = distance::levenshtein::BatchComparator;
using Indel = distance::indel::BatchComparator;
using LevArgs = distance::levenshtein::Args<size_t>;
using IndelArgs = distance::indel::Args<size_t>;
using Triples = std::vector<std::tuple<uint64_t, uint64_t, size_t>>;

#define EXPECT(c)                                                     \
    do {                                                              \
        if (!(c)) {                                                   \
            std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                 \
        }                                                             \
    } while (0)

template <class Scorer>
static Triples flat(const std::vector<typename Scorer::JoinTriple>& r)
{
    Triples t;
    for (const auto& x : r) t.emplace_back(x.query, x.candidate, x.score);
    return t;
}

// the loop the join stands for: one scorer per selected row, its filter over the corpus
template <class Scorer, class A>
static Triples loop(const std::vector<std::string>& rows, const std::vector<uint64_t>& pick, const Corpus& c, const A& a, bool similarity, bool upper, uint64_t qbase, uint64_t ibase)
{
    Triples t;
    for (uint64_t qi : pick) {
        Scorer s(rows[qi]);
        for (const auto& p : similarity ? s.similarity_filter_many(c, a, RF_FILTER_BY_INDEX) : s.distance_filter_many(c, a, RF_FILTER_BY_INDEX))
            if (!upper || p.first > qi) t.emplace_back(qbase + qi, ibase + p.first, p.second);
    }
    return t;
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
        a.cutoff_usize = 2;
        uint32_t score[2] = {7, 7};
        uint64_t query[2] = {7, 7}, index[2] = {7, 7}, count = 9, rows[2] = {0, 1};
        alignas(16) static unsigned char never_read[2][8192];  // stand in for the corpora: the calls below are refused (or answered) before they look at one
        const rf_corpus* q = reinterpret_cast<const rf_corpus*>(never_read[0]);
        const rf_corpus* c = reinterpret_cast<const rf_corpus*>(never_read[1]);
        EXPECT(rf_join_u32(RF_LEVENSHTEIN, q, rows, 2, c, RF_OP_DISTANCE, &a, 0, 0, 0, 2, query, index, score, &count, (rf_join_order)7, nullptr) == RF_ERR_INVALID_ARG);
        EXPECT(rf_join_u32(RF_LEVENSHTEIN, q, rows, 2, c, RF_OP_DISTANCE, &a, 0, 0, 0, 2, nullptr, index, score, &count, RF_JOIN_BY_QUERY, nullptr) == RF_ERR_INVALID_ARG);
        EXPECT(rf_join_u32(RF_LEVENSHTEIN, q, rows, 2, c, RF_OP_NORMALIZED_DISTANCE, &a, 0, 0, 0, 2, query, index, score, &count, RF_JOIN_BY_QUERY, nullptr) == RF_ERR_INVALID_ARG);
        EXPECT(rf_join_u32(RF_JARO, q, rows, 2, c, RF_OP_DISTANCE, &a, 0, 0, 0, 2, query, index, score, &count, RF_JOIN_BY_QUERY, nullptr) == RF_ERR_INVALID_ARG);
        EXPECT(rf_join_u32(RF_LEVENSHTEIN, q, rows, 2, c, RF_OP_DISTANCE, &a, 2u, 0, 0, 2, query, index, score, &count, RF_JOIN_BY_QUERY, nullptr) == RF_ERR_INVALID_ARG);
        EXPECT(rf_join_u32(RF_LEVENSHTEIN, q, rows, 0, c, RF_OP_DISTANCE, &a, 0, 0, 0, 2, query, index, score, &count, RF_JOIN_BY_QUERY, nullptr) == RF_OK);
        EXPECT(count == 9 && score[0] == 7 && index[1] == 7 && query[0] == 7);
        // the facade's functions exist and are well-formed: naming them instantiates them
        auto dj = &Lev::distance_join;
        auto sj = &Indel::similarity_join;
        EXPECT(dj != nullptr && sj != nullptr);
        std::printf("join ok (cpu)\n");
        return 0;
    }
    const uint64_t base = (1ull << 32) + 5;
    size_t triples = 0;
    {   // six strings joined with themselves
        const std::vector<std::string> six{"kitten", "mitten", "", "sitting", "kitten", "bitten"};
        std::vector<std::string_view> views(six.begin(), six.end());
        Corpus corpus(views);
        const auto every = all_rows(six.size());
        for (size_t cutoff : {0u, 1u, 3u})
            for (bool upper : {false, true}) {
                const auto got = flat<Lev>(Lev::distance_join(corpus, corpus, LevArgs{}.score_cutoff(cutoff), upper));
                EXPECT(got == (loop<Lev>(six, every, corpus, LevArgs{}.score_cutoff(cutoff), false, upper, 0, 0)));
                triples += got.size();
            }
        const auto d = flat<Lev>(Lev::distance_join(corpus, corpus, LevArgs{}.score_cutoff(1), true));
        EXPECT((d == Triples{{0, 1, 1}, {0, 4, 0}, {0, 5, 1}, {1, 4, 1}, {1, 5, 1}, {4, 5, 1}}));
        // rows in any order, with repeats, the flag on: the candidate is compared with the ROW's index, not with its place in the list
        const std::vector<uint64_t> pick{4, 0, 4, 5, 1};
        for (bool upper : {false, true})
            EXPECT(flat<Lev>(Lev::distance_join(corpus, corpus, LevArgs{}.score_cutoff(1), upper, RF_JOIN_BY_QUERY, &pick, base, base)) ==
                   (loop<Lev>(six, pick, corpus, LevArgs{}.score_cutoff(1), false, upper, base, base)));
        const std::vector<uint64_t> none;
        EXPECT(Lev::distance_join(corpus, corpus, LevArgs{}.score_cutoff(1), false, RF_JOIN_BY_QUERY, &none).empty());  // an empty selection is no pair
        bool refused = false;
        try {
            (void)Lev::distance_join(corpus, corpus, LevArgs{});  // no cutoff
        } catch (const Error& e) {
            refused = e.status == RF_ERR_INVALID_ARG;
        }
        EXPECT(refused);
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
        for (size_t cutoff : {0u, 1u, 2u}) {
            const auto got = flat<Lev>(Lev::distance_join(queries, corpus, LevArgs{}.score_cutoff(cutoff)));
            EXPECT(got == (loop<Lev>(qs, every, corpus, LevArgs{}.score_cutoff(cutoff), false, false, 0, 0)));
            triples += got.size();
        }
        EXPECT(flat<Indel>(Indel::distance_join(queries, corpus, IndelArgs{}.score_cutoff(2))) == (loop<Indel>(qs, every, corpus, IndelArgs{}.score_cutoff(2), false, false, 0, 0)));
        EXPECT(flat<Indel>(Indel::similarity_join(queries, corpus, IndelArgs{}.score_cutoff(12))) == (loop<Indel>(qs, every, corpus, IndelArgs{}.score_cutoff(12), true, false, 0, 0)));
        auto any = flat<Lev>(Lev::distance_join(queries, corpus, LevArgs{}.score_cutoff(1), false, RF_JOIN_ANY));
        std::sort(any.begin(), any.end());
        EXPECT(any == (loop<Lev>(qs, every, corpus, LevArgs{}.score_cutoff(1), false, false, 0, 0)));
    }
    EXPECT(triples > 100);
    std::printf("join ok (gpu)\n");
    return 0;
}

// filter_multi of the C++ facade (include/rapidfuzz_amd.hpp) over rf_filter_multi_u32.  Without a GPU it checks that the call compiles, that its
// argument checks answer without a device (an unknown order, a null row array) and that an empty list of scorers is an empty result; with a GPU
// (argv[1] == "gpu") every row equals the single-query facade call of the same scorer, on a 5-string corpus and a 700-string corpus.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>

#include "rapidfuzz_amd.hpp"

using namespace rapidfuzz;
using Lev = distance::levenshtein::BatchComparator;
using Indel = distance::indel::BatchComparator;
using LevArgs = distance::levenshtein::Args<size_t>;
using IndelArgs = distance::indel::Args<size_t>;

#define EXPECT(c)                                                     \
    do {                                                              \
        if (!(c)) {                                                   \
            std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                 \
        }                                                             \
    } while (0)

// rows of the facade's multi call against a loop of its single-query call; index_base shifts the multi call's indices
template <class Scorer, class A>
static bool rows_equal(const std::vector<const Scorer*>& scorers, const Corpus& c, const A& a, rf_filter_order order, bool similarity, uint64_t base, size_t* pairs)
{
    const auto multi = similarity ? Scorer::similarity_filter_multi(scorers, c, a, order, base) : Scorer::distance_filter_multi(scorers, c, a, order, base);
    if (multi.size() != scorers.size()) return false;
    for (size_t j = 0; j < scorers.size(); ++j) {
        auto one = similarity ? scorers[j]->similarity_filter_many(c, a, order) : scorers[j]->distance_filter_many(c, a, order);
        for (auto& p : one) p.first += base;
        if (multi[j] != one) return false;
        *pairs += one.size();
    }
    return true;
}

int main(int argc, char** argv)
{
    const bool gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    Lev kitten("kitten"), mitten("mitten"), sitting("sitting"), empty("");
    if (!gpu) {
        rf_args a;
        rf_args_default(&a);
        const rf_comparator* hs[2] = {kitten.handle(), mitten.handle()};
        uint32_t score[2] = {7, 7};
        uint64_t index[2] = {7, 7}, count[2] = {9, 9};
        alignas(16) static unsigned char never_read[8192];  // stands in for a corpus: the calls below are refused (or answered) before they look at one
        const rf_corpus* fake = reinterpret_cast<const rf_corpus*>(never_read);
        EXPECT(rf_filter_multi_u32(hs, 2, fake, RF_OP_DISTANCE, &a, 0, 1, index, score, count, (rf_filter_order)7, nullptr) == RF_ERR_INVALID_ARG);
        EXPECT(rf_filter_multi_u32(hs, 2, fake, RF_OP_DISTANCE, &a, 0, 1, nullptr, score, count, RF_FILTER_BY_INDEX, nullptr) == RF_ERR_INVALID_ARG);
        EXPECT(rf_filter_multi_u32(hs, 2, fake, RF_OP_NORMALIZED_DISTANCE, &a, 0, 1, index, score, count, RF_FILTER_BY_INDEX, nullptr) == RF_ERR_INVALID_ARG);
        EXPECT(rf_filter_multi_u32(hs, 0, fake, RF_OP_DISTANCE, &a, 0, 1, index, score, count, RF_FILTER_BY_INDEX, nullptr) == RF_OK);
        EXPECT(count[0] == 9 && count[1] == 9 && score[0] == 7 && index[1] == 7);
        std::printf("filter_multi ok (cpu)\n");
        return 0;
    }
    const uint64_t base = (1ull << 40) + 5;
    size_t pairs = 0;
    {   // five strings
        const std::vector<std::string> five{"kitten", "mitten", "", "sitting", "kitten"};
        std::vector<std::string_view> views(five.begin(), five.end());
        Corpus corpus(views);
        const std::vector<const Lev*> scorers{&kitten, &mitten, &sitting, &empty};
        for (size_t cutoff : {0u, 1u, 3u, 100u})
            for (rf_filter_order order : {RF_FILTER_BY_INDEX, RF_FILTER_BY_SCORE}) EXPECT(rows_equal(scorers, corpus, LevArgs{}.score_cutoff(cutoff), order, false, base, &pairs));
        const auto d = Lev::distance_filter_multi(scorers, corpus, LevArgs{}.score_cutoff(1));
        EXPECT((d[0] == std::vector<std::pair<uint64_t, size_t>>{{0, 0}, {1, 1}, {4, 0}}));
        EXPECT((d[3] == std::vector<std::pair<uint64_t, size_t>>{{2, 0}}));
        EXPECT(rows_equal(scorers, corpus, LevArgs{}, RF_FILTER_BY_INDEX, false, 0, &pairs));  // no cutoff: every candidate, per query
    }
    {   // 700 candidates: rotations of three words with a counter behind some of them, and copies of the queries at distant indices
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
        const std::vector<const Lev*> scorers{&kitten, &mitten, &sitting, &empty, &kitten};  // a group of four and one left over
        for (size_t cutoff : {0u, 1u, 2u})
            for (rf_filter_order order : {RF_FILTER_BY_INDEX, RF_FILTER_BY_SCORE}) {
                EXPECT(rows_equal(scorers, corpus, LevArgs{}.score_cutoff(cutoff), order, false, base, &pairs));
            }
        EXPECT(rows_equal(scorers, corpus, LevArgs{}.score_cutoff(5), RF_FILTER_BY_SCORE, true, 0, &pairs));
        Indel a("kitten"), b("sitting"), c("mitten");  // three Indel scorers: a group of two and one on its own
        const std::vector<const Indel*> indels{&a, &b, &c};
        EXPECT(rows_equal(indels, corpus, IndelArgs{}.score_cutoff(2), RF_FILTER_BY_INDEX, false, base, &pairs));
        const auto d = Lev::distance_filter_multi(scorers, corpus, LevArgs{}.score_cutoff(0));
        EXPECT(d[0].size() >= 10 && d[0] == d[4] && d[0][0].second == 0);
        EXPECT(Lev::distance_filter_multi({}, corpus, LevArgs{}.score_cutoff(1)).empty());
    }
    EXPECT(pairs > 100);
    std::printf("filter_multi ok (gpu)\n");
    return 0;
}

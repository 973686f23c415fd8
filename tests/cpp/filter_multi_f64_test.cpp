// The f64 filter_multi entry points of the C++ facade (include/rapidfuzz_amd.hpp) over rf_filter_multi_f64.  Without a GPU it checks that the calls
// compile, that the argument checks answer without a device (an unknown order, a null row array, a u32-valued op) and that an empty list of scorers is
// an empty result; with a GPU (argv[1] == "gpu") every row of normalized_distance_filter_multi, normalized_similarity_filter_multi and
// fuzz::RatioBatchComparator::similarity_filter_multi equals the facade's own single-query filter of the same scorer -- the same indices, the same doubles.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>

#include "rapidfuzz_amd.hpp"

using namespace rapidfuzz;
using Lev = distance::levenshtein::BatchComparator;
using Indel = distance::indel::BatchComparator;
using Ratio = fuzz::RatioBatchComparator;
using FArgs = distance::levenshtein::Args<double>;

#define EXPECT(c)                                                     \
    do {                                                              \
        if (!(c)) {                                                   \
            std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                 \
        }                                                             \
    } while (0)

static bool same(const std::vector<std::pair<uint64_t, double>>& a, std::vector<std::pair<uint64_t, double>> b, uint64_t base)
{
    for (auto& p : b) p.first += base;
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (a[i].first != b[i].first || std::memcmp(&a[i].second, &b[i].second, sizeof(double)) != 0) return false;
    return true;
}

// rows of the facade's multi call against a loop of its single-query call; index_base shifts the multi call's indices
template <class Scorer>
static bool rows_equal(const std::vector<const Scorer*>& scorers, const Corpus& c, const FArgs& a, rf_filter_order order, bool similarity, uint64_t base, size_t* pairs)
{
    const auto multi = similarity ? Scorer::normalized_similarity_filter_multi(scorers, c, a, order, base) : Scorer::normalized_distance_filter_multi(scorers, c, a, order, base);
    if (multi.size() != scorers.size()) return false;
    for (size_t j = 0; j < scorers.size(); ++j) {
        const auto one = similarity ? scorers[j]->normalized_similarity_filter_many(c, a, order) : scorers[j]->normalized_distance_filter_many(c, a, order);
        if (!same(multi[j], one, base)) return false;
        *pairs += one.size();
    }
    return true;
}
static bool ratio_rows_equal(const std::vector<const Ratio*>& scorers, const Corpus& c, const FArgs& a, rf_filter_order order, uint64_t base, size_t* pairs)
{
    const auto multi = Ratio::similarity_filter_multi(scorers, c, a, order, base);
    if (multi.size() != scorers.size()) return false;
    for (size_t j = 0; j < scorers.size(); ++j) {
        const auto one = scorers[j]->similarity_filter_many(c, a, order);
        if (!same(multi[j], one, base)) return false;
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
        a.cutoff_f64 = 0.9;
        const rf_comparator* hs[2] = {kitten.handle(), mitten.handle()};
        double score[2] = {7, 7};
        uint64_t index[2] = {7, 7}, count[2] = {9, 9};
        alignas(16) static unsigned char never_read[8192];  // stands in for a corpus: the calls below are refused (or answered) before they look at one
        const rf_corpus* fake = reinterpret_cast<const rf_corpus*>(never_read);
        EXPECT(rf_filter_multi_f64(hs, 2, fake, RF_OP_NORMALIZED_SIMILARITY, &a, 0, 1, index, score, count, (rf_filter_order)7, nullptr) == RF_ERR_INVALID_ARG);
        EXPECT(rf_filter_multi_f64(hs, 2, fake, RF_OP_NORMALIZED_SIMILARITY, &a, 0, 1, nullptr, score, count, RF_FILTER_BY_INDEX, nullptr) == RF_ERR_INVALID_ARG);
        EXPECT(rf_filter_multi_f64(hs, 2, fake, RF_OP_DISTANCE, &a, 0, 1, index, score, count, RF_FILTER_BY_INDEX, nullptr) == RF_ERR_INVALID_ARG);
        EXPECT(rf_filter_multi_f64(hs, 0, fake, RF_OP_NORMALIZED_SIMILARITY, &a, 0, 1, index, score, count, RF_FILTER_BY_INDEX, nullptr) == RF_OK);
        EXPECT(count[0] == 9 && count[1] == 9 && score[0] == 7 && index[1] == 7);
        std::printf("filter_multi_f64 ok (cpu)\n");
        return 0;
    }
    const uint64_t base = (1ull << 40) + 5;
    size_t pairs = 0;
    {   // five strings
        const std::vector<std::string> five{"kitten", "mitten", "", "sitting", "kitten"};
        std::vector<std::string_view> views(five.begin(), five.end());
        Corpus corpus(views);
        const std::vector<const Lev*> scorers{&kitten, &mitten, &sitting, &empty};
        for (double cutoff : {1.0, 0.8, 0.5, 0.0})
            for (rf_filter_order order : {RF_FILTER_BY_INDEX, RF_FILTER_BY_SCORE}) {
                EXPECT(rows_equal(scorers, corpus, FArgs{}.score_cutoff(cutoff), order, true, base, &pairs));
                EXPECT(rows_equal(scorers, corpus, FArgs{}.score_cutoff(1.0 - cutoff), order, false, base, &pairs));
            }
        const auto s = Lev::normalized_similarity_filter_multi(scorers, corpus, FArgs{}.score_cutoff(0.8));
        EXPECT((s[0] == std::vector<std::pair<uint64_t, double>>{{0, 1.0}, {1, 1.0 - 1.0 / 6.0}, {4, 1.0}}));
        EXPECT((s[3] == std::vector<std::pair<uint64_t, double>>{{2, 1.0}}));
        EXPECT(rows_equal(scorers, corpus, FArgs{}, RF_FILTER_BY_INDEX, true, 0, &pairs));  // no cutoff: every candidate, per query
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
        for (double cutoff : {1.0, 0.8, 0.7})
            for (rf_filter_order order : {RF_FILTER_BY_INDEX, RF_FILTER_BY_SCORE}) {
                EXPECT(rows_equal(scorers, corpus, FArgs{}.score_cutoff(cutoff), order, true, base, &pairs));
                EXPECT(rows_equal(scorers, corpus, FArgs{}.score_cutoff(1.0 - cutoff), order, false, base, &pairs));
            }
        Indel a("kitten"), b("sitting"), c("mitten");  // three Indel scorers: a group of two and one on its own
        const std::vector<const Indel*> indels{&a, &b, &c};
        EXPECT(rows_equal(indels, corpus, FArgs{}.score_cutoff(0.8), RF_FILTER_BY_INDEX, true, base, &pairs));
        EXPECT(rows_equal(indels, corpus, FArgs{}.score_cutoff(0.2), RF_FILTER_BY_SCORE, false, 0, &pairs));
        Ratio ra("kitten"), rb("sitting"), rc("mitten"), rd("kitten");
        const std::vector<const Ratio*> ratios{&ra, &rb, &rc, &rd};
        for (rf_filter_order order : {RF_FILTER_BY_INDEX, RF_FILTER_BY_SCORE}) EXPECT(ratio_rows_equal(ratios, corpus, FArgs{}.score_cutoff(0.8), order, base, &pairs));
        const auto r = Ratio::similarity_filter_multi(ratios, corpus, FArgs{}.score_cutoff(1.0));
        EXPECT(r[0].size() >= 10 && r[0] == r[3] && r[0][0].second == 1.0);
        const auto d = Lev::normalized_distance_filter_multi(scorers, corpus, FArgs{}.score_cutoff(0.0));
        EXPECT(d[0].size() >= 10 && d[0] == d[4] && d[0][0].second == 0.0);
        EXPECT(Lev::normalized_similarity_filter_multi({}, corpus, FArgs{}.score_cutoff(0.9)).empty());
        EXPECT(Ratio::similarity_filter_multi({}, corpus, FArgs{}.score_cutoff(0.9)).empty());
    }
    EXPECT(pairs > 100);
    std::printf("filter_multi_f64 ok (gpu)\n");
    return 0;
}

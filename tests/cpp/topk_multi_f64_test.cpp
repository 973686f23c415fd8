// normalized_*_topk_multi of the C++ facade (include/rapidfuzz_amd.hpp) over rf_topk_multi_f64.  Without a GPU it checks that the calls compile, that
// the argument checks answer without a device (k == 0, a u32-valued op) and that an empty list of scorers is an empty result; with a GPU
// (argv[1] == "gpu") every row equals a sort of normalized_*_many() of the same scorer by (score, index), bit for bit.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>

#include "rapidfuzz_amd.hpp"

using namespace rapidfuzz;
using Lev = distance::levenshtein::BatchComparator;
using Indel = distance::indel::BatchComparator;
using Ratio = fuzz::RatioBatchComparator;

#define EXPECT(c)                                                     \
    do {                                                              \
        if (!(c)) {                                                   \
            std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                 \
        }                                                             \
    } while (0)

static std::vector<std::pair<uint64_t, double>> sorted(const std::vector<std::optional<double>>& all, uint32_t k, bool similarity, uint64_t base)
{
    std::vector<std::pair<uint64_t, double>> v;
    for (size_t i = 0; i < all.size(); ++i)
        if (all[i]) v.emplace_back(base + i, *all[i]);
    std::stable_sort(v.begin(), v.end(), [&](const auto& a, const auto& b) { return similarity ? a.second > b.second : a.second < b.second; });
    if (v.size() > k) v.resize(k);
    return v;
}

int main(int argc, char** argv)
{
    const bool gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    Lev kitten("kitten"), mitten("mitten"), sitting("sitting"), empty("");
    if (!gpu) {
        rf_args a;
        rf_args_default(&a);
        const rf_comparator* hs[2] = {kitten.handle(), mitten.handle()};
        double score[2] = {9.0, 9.0};
        uint32_t count[2] = {9, 9};
        uint64_t index[2];
        alignas(16) static unsigned char never_read[8192];  // stands in for a corpus: the calls below are answered before they look at one
        const rf_corpus* corpus = reinterpret_cast<const rf_corpus*>(never_read);
        EXPECT(rf_topk_multi_f64(hs, 2, corpus, RF_OP_NORMALIZED_SIMILARITY, &a, 0, 0, score, index, count, nullptr) == RF_ERR_INVALID_ARG);
        EXPECT(rf_topk_multi_f64(hs, 2, corpus, RF_OP_DISTANCE, &a, 1, 0, score, index, count, nullptr) == RF_ERR_INVALID_ARG);
        EXPECT(rf_topk_multi_f64(hs, 0, corpus, RF_OP_NORMALIZED_SIMILARITY, &a, 1, 0, score, index, count, nullptr) == RF_OK);
        EXPECT(count[0] == 9 && count[1] == 9 && score[0] == 9.0 && score[1] == 9.0);
        std::printf("topk_multi_f64 ok (cpu)\n");
        return 0;
    }
    // 200 candidates: rotations of three words with a counter behind some of them, and copies of the queries at distant indices
    std::vector<std::string> cands;
    const std::string words[3] = {"kitten", "sitting", "mitten"};
    for (int i = 0; i < 200; ++i) {
        std::string w = words[i % 3];
        std::rotate(w.begin(), w.begin() + i % w.size(), w.end());
        if (i % 5 == 0) w += std::to_string(i);
        cands.push_back(i % 67 == 11 ? "kitten" : (i % 71 == 13 ? "mitten" : w));
    }
    std::vector<std::string_view> views(cands.begin(), cands.end());
    Corpus corpus(views);
    const uint64_t base = (1ull << 40) + 5;
    {   // four scorers: one fused group
        const std::vector<const Lev*> scorers{&kitten, &mitten, &sitting, &empty};
        for (uint32_t k : {1u, 16u, 65u, 300u}) {
            const auto d = Lev::normalized_distance_topk_multi(scorers, corpus, k, {}, base);
            const auto s = Lev::normalized_similarity_topk_multi(scorers, corpus, k);
            EXPECT(d.size() == 4 && s.size() == 4);
            for (size_t j = 0; j < 4; ++j) {
                EXPECT(d[j] == sorted(scorers[j]->normalized_distance_many(corpus), k, false, base));
                EXPECT(s[j] == sorted(scorers[j]->normalized_similarity_many(corpus), k, true, 0));
            }
        }
        const auto cut = Lev::normalized_distance_topk_multi(scorers, corpus, 16, distance::levenshtein::Args<double>{}.score_cutoff(0.0));
        EXPECT(cut[0].size() >= 2 && cut[0][0].second == 0.0 && cut[3].empty());
    }
    {   // three Indel scorers: a group of two and one on its own
        Indel a("kitten"), b("sitting"), c("mitten");
        const std::vector<const Indel*> scorers{&a, &b, &c};
        const auto s = Indel::normalized_similarity_topk_multi(scorers, corpus, 16);
        for (size_t j = 0; j < 3; ++j) EXPECT(s[j] == sorted(scorers[j]->normalized_similarity_many(corpus), 16, true, 0));
    }
    {   // the ratio
        Ratio a("kitten"), b("sitting");
        const auto s = Ratio::similarity_topk_multi({&a, &b}, corpus, 16, {}, base);
        EXPECT(s.size() == 2 && s[0] == sorted(a.similarity_many(corpus), 16, true, base) && s[1] == sorted(b.similarity_many(corpus), 16, true, base));
    }
    EXPECT(Lev::normalized_distance_topk_multi({}, corpus, 4).empty());
    try {
        (void)Lev::normalized_distance_topk_multi({&kitten}, corpus, 0);
        return 1;
    } catch (const Error& e) {
        EXPECT(e.status == RF_ERR_INVALID_ARG);
    }
    std::printf("topk_multi_f64 ok (gpu)\n");
    return 0;
}

// topk_multi of the C++ facade (include/rapidfuzz_amd.hpp) over rf_topk_multi_u32.  Without a GPU it checks that the call compiles, that its
// argument checks answer without a device (k == 0) and that an empty list of scorers is an empty result; with a GPU (argv[1] == "gpu") every row
// equals a sort of distance_many() of the same scorer by (score, index).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>

#include "rapidfuzz_amd.hpp"

using namespace rapidfuzz;
using Lev = distance::levenshtein::BatchComparator;
using Indel = distance::indel::BatchComparator;

#define EXPECT(c)                                                     \
    do {                                                              \
        if (!(c)) {                                                   \
            std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                 \
        }                                                             \
    } while (0)

template <class Scorer>
static std::vector<std::pair<uint64_t, size_t>> sorted_many(const Scorer& s, const Corpus& c, uint32_t k, bool similarity, uint64_t base)
{
    const auto all = similarity ? s.similarity_many(c) : s.distance_many(c);
    std::vector<std::pair<uint64_t, size_t>> v;
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
        uint32_t score[2], count[2] = {9, 9};
        uint64_t index[2];
        alignas(16) static unsigned char never_read[8192];  // stands in for a corpus: the call below is refused before it looks at one
        EXPECT(rf_topk_multi_u32(hs, 2, reinterpret_cast<const rf_corpus*>(never_read), RF_OP_DISTANCE, &a, 0, 0, score, index, count, nullptr) == RF_ERR_INVALID_ARG);
        EXPECT(rf_topk_multi_u32(hs, 0, reinterpret_cast<const rf_corpus*>(never_read), RF_OP_DISTANCE, &a, 1, 0, score, index, count, nullptr) == RF_OK);
        EXPECT(count[0] == 9 && count[1] == 9);
        std::printf("topk_multi ok (cpu)\n");
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
            const auto d = Lev::distance_topk_multi(scorers, corpus, k, {}, base);
            const auto s = Lev::similarity_topk_multi(scorers, corpus, k);
            EXPECT(d.size() == 4 && s.size() == 4);
            for (size_t j = 0; j < 4; ++j) {
                EXPECT(d[j] == sorted_many(*scorers[j], corpus, k, false, base));
                EXPECT(s[j] == sorted_many(*scorers[j], corpus, k, true, 0));
            }
        }
        const auto cut = Lev::distance_topk_multi(scorers, corpus, 16, distance::levenshtein::Args<size_t>{}.score_cutoff(0));
        EXPECT(cut[0].size() >= 2 && cut[0][0].second == 0 && cut[3].empty());
    }
    {   // three Indel scorers: a group of two and one on its own
        Indel a("kitten"), b("sitting"), c("mitten");
        const std::vector<const Indel*> scorers{&a, &b, &c};
        const auto d = Indel::distance_topk_multi(scorers, corpus, 16);
        for (size_t j = 0; j < 3; ++j) EXPECT(d[j] == sorted_many(*scorers[j], corpus, 16, false, 0));
    }
    EXPECT(Lev::distance_topk_multi({}, corpus, 4).empty());
    try {
        (void)Lev::distance_topk_multi({&kitten}, corpus, 0);
        return 1;
    } catch (const Error& e) {
        EXPECT(e.status == RF_ERR_INVALID_ARG);
    }
    std::printf("topk_multi ok (gpu)\n");
    return 0;
}

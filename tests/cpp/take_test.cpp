// take / take_u32 / lengths of the C++ facade (include/rapidfuzz_amd.hpp) over rf_corpus_take.  Without a GPU it checks that the calls compile and that the
// argument checks answer without a device (a null offsets array, an index outside the corpus, an unknown out_mem) with nothing written; with a GPU
// (argv[1] == "gpu") the rows equal the strings the corpus was packed from, on a ragged byte corpus and on a corpus of code points.
#include <cstdio>
#include <cstring>
#include <string>

#include "rapidfuzz_amd.hpp"

using namespace rapidfuzz;

#define EXPECT(c)                                                     \
    do {                                                              \
        if (!(c)) {                                                   \
            std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                 \
        }                                                             \
    } while (0)

int main(int argc, char** argv)
{
    const bool gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    if (!gpu) {
        alignas(16) static unsigned char never_read[16384];  // stands in for a corpus of no candidates: the calls below are refused (or answered) without a device
        const rf_corpus* fake = reinterpret_cast<const rf_corpus*>(never_read);
        const uint64_t idx[2] = {3, 4};
        uint64_t offsets[3] = {7, 7, 7};
        uint8_t bytes[4] = {9, 9, 9, 9};
        uint32_t elems[4] = {9, 9, 9, 9}, lens[2] = {9, 9};
        EXPECT(rf_corpus_take(fake, idx, 2, 0, bytes, 4, nullptr, RF_MEM_HOST, nullptr) == RF_ERR_INVALID_ARG);
        EXPECT(rf_corpus_take(fake, idx, 2, 0, bytes, 4, offsets, RF_MEM_HOST, nullptr) == RF_ERR_INVALID_ARG);  // no candidate 3 in an empty corpus
        EXPECT(rf_corpus_take_u32(fake, idx, 2, 4, elems, 4, offsets, RF_MEM_HOST, nullptr) == RF_ERR_INVALID_ARG);  // 3 lies below the base
        EXPECT(rf_corpus_take(fake, nullptr, 0, 0, bytes, 4, offsets, (rf_mem)5, nullptr) == RF_ERR_INVALID_ARG);
        EXPECT(rf_corpus_lengths(fake, idx, 2, 0, lens, nullptr) == RF_ERR_INVALID_ARG);
        EXPECT(offsets[0] == 7 && offsets[2] == 7 && bytes[0] == 9 && elems[3] == 9 && lens[1] == 9);
        EXPECT(rf_corpus_take(fake, idx, 0, 0, bytes, 4, offsets, RF_MEM_HOST, nullptr) == RF_OK && offsets[0] == 0 && offsets[1] == 7);
        EXPECT(rf_corpus_is_wide(fake) == 0 && rf_corpus_is_wide(nullptr) == 0);
        std::printf("take ok (cpu)\n");
        return 0;
    }
    {   // a ragged byte corpus: every length 0..69 ten times, bytes over all 256 values
        std::vector<std::string> cands;
        for (int i = 0; i < 700; ++i) {
            std::string s(i % 70, '\0');
            for (size_t b = 0; b < s.size(); ++b) s[b] = (char)((i * 131 + b * 7 + (b % 3 ? 0 : i)) & 0xFF);
            cands.push_back(s);
        }
        std::vector<std::string_view> views(cands.begin(), cands.end());
        Corpus corpus(views);
        EXPECT(!corpus.wide());
        std::vector<uint64_t> all(cands.size());
        for (size_t i = 0; i < all.size(); ++i) all[i] = i;
        EXPECT(corpus.take(all) == cands);
        const uint64_t base = (1ull << 40) + 5;
        const std::vector<uint64_t> some{base + 699, base + 0, base + 70, base + 699, base + 33};
        const auto rows = corpus.take(some, base);
        EXPECT(rows.size() == 5 && rows[0] == cands[699] && rows[1].empty() && rows[2].empty() && rows[3] == cands[699] && rows[4] == cands[33]);
        EXPECT((corpus.lengths(some, base) == std::vector<uint32_t>{69, 0, 0, 69, 33}));
        const auto wide_rows = corpus.take_u32(some, base);  // the bytes, zero-extended
        EXPECT(wide_rows.size() == 5 && wide_rows[4].size() == 33);
        for (size_t b = 0; b < 33; ++b) EXPECT(wide_rows[4][b] == (char32_t)(unsigned char)cands[33][b]);
        EXPECT(corpus.take({}).empty() && corpus.take_u32({}).empty() && corpus.lengths({}).empty());
        bool refused = false;
        try {
            corpus.take({700});
        } catch (const Error& e) {
            refused = e.status == RF_ERR_INVALID_ARG;
        }
        EXPECT(refused);
    }
    {   // code points: Greek, Cyrillic, one beyond the BMP
        std::vector<std::u32string> cands;
        for (int i = 0; i < 300; ++i) {
            std::u32string s;
            for (int b = 0; b < i % 41; ++b) s.push_back((b + i) % 5 == 0 ? U'\U0001F600' : (char32_t)(((b * 3 + i) % 2 ? 0x391 : 0x410) + (b * 7 + i) % 30));
            cands.push_back(s);
        }
        std::vector<std::u32string_view> views(cands.begin(), cands.end());
        Corpus corpus(views);
        EXPECT(corpus.wide());
        std::vector<uint64_t> all(cands.size());
        for (size_t i = 0; i < all.size(); ++i) all[i] = cands.size() - 1 - i;
        const auto rows = corpus.take_u32(all);
        EXPECT(rows.size() == cands.size());
        for (size_t i = 0; i < rows.size(); ++i) EXPECT(rows[i] == cands[cands.size() - 1 - i]);
        const auto lens = corpus.lengths(all);
        for (size_t i = 0; i < lens.size(); ++i) EXPECT(lens[i] == cands[cands.size() - 1 - i].size());
        bool refused = false;
        try {
            corpus.take({0});  // bytes of a corpus of code points
        } catch (const Error& e) {
            refused = e.status == RF_ERR_INVALID_ARG;
        }
        EXPECT(refused);
    }
    std::printf("take ok (gpu)\n");
    return 0;
}

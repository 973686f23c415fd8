// The hamming / prefix / postfix modules of the C++ facade (include/rapidfuzz_amd.hpp).  Without a GPU it checks that the modules and Args::pad compile
// against the C ABI and that what is decided on the host answers without a device (hamming's Err(DifferentLengthArgs) from the single-candidate call);
// with a GPU (argv[1] == "gpu") one case per metric from the reference's own examples, through the free functions, a BatchComparator over a corpus and
// the filter.
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
    using HArgs = distance::hamming::Args<size_t>;
    EXPECT(HArgs().pad().to_c().flags == RF_FLAG_HAMMING_PAD && HArgs().pad().pad(false).to_c().flags == 0);
    EXPECT(HArgs().pad().score_cutoff(3).to_c().cutoff_usize == 3);
    EXPECT(rfgpu_is_different_length_f64(0.5) == 0);
    {
        const uint64_t bits = RF_DIFFERENT_LENGTH_F64_BITS, none = RF_NONE_F64_BITS;
        double err, nan;
        std::memcpy(&err, &bits, 8), std::memcpy(&nan, &none, 8);
        EXPECT(rfgpu_is_different_length_f64(err) == 1 && rfgpu_is_different_length_f64(nan) == 0 && std::isnan(err) && std::isnan(nan));
    }
    distance::hamming::BatchComparator ham("hamming");
    distance::prefix::BatchComparator pre("prefix");
    distance::postfix::BatchComparator post("postfix");
    EXPECT(rf_comparator_metric(ham.handle()) == RF_HAMMING && rf_comparator_metric(pre.handle()) == RF_PREFIX && rf_comparator_metric(post.handle()) == RF_POSTFIX);
    if (!gpu) {
        std::printf("compare facade ok (cpu)\n");
        return 0;
    }
    // hamming.rs tests `diff` and `unequal_length`
    EXPECT(distance::hamming::distance("hamming", "hammers") == 3);
    EXPECT(ham.distance_with_args("hammers", HArgs().score_cutoff(3)) == std::optional<size_t>(3));
    EXPECT(ham.distance_with_args("hammers", HArgs().score_cutoff(2)) == std::nullopt);
    EXPECT(distance::hamming::BatchComparator("ham").distance_with_args("hamming", HArgs().pad()) == std::optional<size_t>(4));
    bool threw = false;
    try {
        (void)distance::hamming::distance("ham", "hamming");
    } catch (const Error& e) {
        threw = e.status == RF_ERR_INVALID_ARG && std::string(e.what()) == "Differing length arguments provided";
    }
    EXPECT(threw);
    // prefix.rs / postfix.rs doc examples
    EXPECT(distance::prefix::similarity("prefix", "preference") == 4 && pre.similarity("preference") == 4);
    EXPECT(distance::postfix::similarity("postfix", "prefix") == 3 && post.similarity("prefix") == 3);
    EXPECT(distance::prefix::distance("prefix", "preference") == 6 && distance::postfix::normalized_similarity("postfix", "prefix") == 1.0 - 4.0 / 7.0);
    // over a corpus: an Err candidate has no entry in *_many and is dropped by the filter
    Corpus corpus({"hamming", "hammers", "ham", "humming", ""});
    const auto d = ham.distance_many(corpus);
    EXPECT(d.size() == 5 && d[0] == std::optional<size_t>(0) && d[1] == std::optional<size_t>(3) && !d[2] && d[3] == std::optional<size_t>(1) && !d[4]);
    const auto dp = ham.distance_many(corpus, HArgs().pad());
    EXPECT(dp[2] == std::optional<size_t>(4) && dp[4] == std::optional<size_t>(7));
    const auto f = ham.distance_filter_many(corpus, HArgs().score_cutoff(1));
    EXPECT(f.size() == 2 && f[0].first == 0 && f[0].second == 0 && f[1].first == 3 && f[1].second == 1);
    const auto ps = pre.similarity_many(Corpus({"preference", "prefix", "", "xprefix"}));
    EXPECT(ps[0] == std::optional<size_t>(4) && ps[1] == std::optional<size_t>(6) && ps[2] == std::optional<size_t>(0) && ps[3] == std::optional<size_t>(0));
    const auto qs = post.similarity_many(Corpus({"prefix", "postfix", "", "postfixy"}));
    EXPECT(qs[0] == std::optional<size_t>(3) && qs[1] == std::optional<size_t>(7) && qs[2] == std::optional<size_t>(0) && qs[3] == std::optional<size_t>(0));
    std::printf("compare facade ok (gpu)\n");
    return 0;
}

// Compiles the two Corpus::from_device_ragged overloads of the C++ facade against librfgpu.so.  Without a GPU: the argument errors that answer before a device
// is touched arrive as rapidfuzz::Error with RF_ERR_INVALID_ARG.  With a GPU (argv[1] == "gpu"): candidates copied to device memory, offsets that start above
// 0, packed in place over bytes and over code points, read back with take / take_u32 and scored against the corpus the host constructors build.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "rapidfuzz_amd.hpp"

using namespace rapidfuzz;

#define EXPECT(c)                                                     \
    do {                                                              \
        if (!(c)) {                                                   \
            std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                 \
        }                                                             \
    } while (0)

template <class Fn>
static bool invalid_arg(Fn&& fn, const char* who)
{
    try {
        fn();
    } catch (const Error& e) {
        return e.status == RF_ERR_INVALID_ARG && std::strncmp(e.what(), who, std::strlen(who)) == 0;
    }
    return false;
}

template <class T>
static T* to_device(const std::vector<T>& v)
{
    T* d = nullptr;
    if (hipMalloc(&d, std::max<size_t>(1, v.size()) * sizeof(T)) != hipSuccess) return nullptr;
    if (!v.empty() && hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    return d;
}

int main(int argc, char** argv)
{
    const bool gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    uint64_t fake_offsets[4] = {0, 1, 2, 3};  // (never read: each call below is refused first)
    const uint8_t* no_bytes = nullptr;
    const uint32_t* no_elems = nullptr;
    EXPECT(invalid_arg([&] { Corpus::from_device_ragged(no_bytes, 3, fake_offsets, 3); }, "rf_corpus_pack_device:"));
    EXPECT(invalid_arg([&] { Corpus::from_device_ragged(no_elems, 3, fake_offsets, 3); }, "rf_corpus_pack_u32_device:"));
    EXPECT(invalid_arg([&] { Corpus::from_device_ragged(reinterpret_cast<const uint8_t*>(fake_offsets), 3, nullptr, 3); }, "rf_corpus_pack_device:"));
    EXPECT(invalid_arg([&] { Corpus::from_device_ragged(reinterpret_cast<const uint32_t*>(fake_offsets), 3, nullptr, 3); }, "rf_corpus_pack_u32_device:"));
    if (!gpu) {
        std::printf("device ragged facade ok (cpu)\n");
        return 0;
    }
    const std::vector<std::string_view> words{"sitting", "", "mitten", "kitchen", "a", "sixteen symbols!", "seventeen symbols"};
    const std::vector<std::u32string_view> chars{U"sitting", U"", U"κίτρινο", U"kitchen", U"\U0001F600", U"sixteen symbols!", U"seventeen symbols"};
    std::vector<uint8_t> bytes{'x', 'y', 'z'};  // three elements in front of the window
    std::vector<uint32_t> elems{'x', 'y', 'z'};
    std::vector<uint64_t> off8{bytes.size()}, off32{elems.size()};
    std::vector<uint64_t> all;
    for (size_t i = 0; i < words.size(); ++i) {
        bytes.insert(bytes.end(), words[i].begin(), words[i].end());
        off8.push_back(bytes.size());
        elems.insert(elems.end(), chars[i].begin(), chars[i].end());
        off32.push_back(elems.size());
        all.push_back(i);
    }
    uint8_t* d_bytes = to_device(bytes);
    uint32_t* d_elems = to_device(elems);
    uint64_t *d_off8 = to_device(off8), *d_off32 = to_device(off32);
    EXPECT(d_bytes && d_elems && d_off8 && d_off32);
    {
        Corpus dev = Corpus::from_device_ragged(d_bytes, bytes.size(), d_off8, words.size());
        Corpus host(words);
        EXPECT(dev.size() == words.size() && !dev.wide());
        const std::vector<std::string> back = dev.take(all);
        for (size_t i = 0; i < words.size(); ++i) EXPECT(back[i] == words[i]);
        distance::levenshtein::BatchComparator scorer("kitten");
        EXPECT(scorer.distance_many(dev) == scorer.distance_many(host));
        EXPECT(invalid_arg([&] { Corpus::from_device_ragged(d_bytes, bytes.size() - 1, d_off8, words.size()); }, "rf_corpus_pack_device:"));
    }
    {
        Corpus dev = Corpus::from_device_ragged(d_elems, elems.size(), d_off32, chars.size());
        EXPECT(dev.size() == chars.size() && dev.wide());
        const std::vector<std::u32string> back = dev.take_u32(all);
        for (size_t i = 0; i < chars.size(); ++i) EXPECT(back[i] == chars[i]);
        EXPECT(invalid_arg([&] { Corpus::from_device_ragged(d_elems, elems.size() - 1, d_off32, chars.size()); }, "rf_corpus_pack_u32_device:"));
    }
    (void)hipFree(d_bytes), (void)hipFree(d_elems), (void)hipFree(d_off8), (void)hipFree(d_off32);
    std::printf("device ragged facade ok (gpu)\n");
    return 0;
}

// Host build of rf_dl_cell.hpp: the very inlines the gfx950 kernels of rf_damerau.hip compile, run column by column on the CPU and held
// to a plain full-matrix Lowrance-Wagner implementation of the unrestricted Damerau-Levenshtein distance.  Covers the field-width edges
// of the packed cell (max(len1, len2) = 253, 254 in 8-bit fields; 254, 255, 300 in 16-bit fields) and the query lengths at which the
// kernels change templates.  tests/test_dl_cell.py builds and runs it, once plainly and once under -fsanitize=address,undefined.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <random>
#include <vector>

#include "../../rapidfuzz_rs_amd/csrc/rf_dl_cell.hpp"

using Str = std::vector<uint8_t>;

// Lowrance-Wagner, the whole (n + 2) x (m + 2) matrix
static uint32_t brute(const Str& a, const Str& b)
{
    const size_t n = a.size(), m = b.size();
    const uint32_t inf = (uint32_t)(n + m);
    std::vector<std::vector<uint32_t>> H(n + 2, std::vector<uint32_t>(m + 2, 0));
    std::map<uint8_t, size_t> da;
    H[0][0] = inf;
    for (size_t i = 0; i <= n; ++i) H[i + 1][0] = inf, H[i + 1][1] = (uint32_t)i;
    for (size_t j = 0; j <= m; ++j) H[0][j + 1] = inf, H[1][j + 1] = (uint32_t)j;
    for (size_t i = 1; i <= n; ++i) {
        size_t db = 0;
        for (size_t j = 1; j <= m; ++j) {
            const size_t k = da.count(b[j - 1]) ? da[b[j - 1]] : 0, l = db;
            uint32_t cost = 1;
            if (a[i - 1] == b[j - 1]) cost = 0, db = j;
            H[i + 1][j + 1] = std::min(std::min(H[i][j] + cost, H[i + 1][j] + 1), std::min(H[i][j + 1] + 1, H[k][l] + (uint32_t)((i - k - 1) + 1 + (j - l - 1))));
        }
        da[a[i - 1]] = i;
    }
    return H[n + 1][m + 1];
}

// the kernels' loop: columns = candidate symbols, one packed cell per query position
template <class Cell>
static uint32_t by_cells(const Str& query, const Str& cand)
{
    const uint32_t len1 = (uint32_t)query.size(), len2 = (uint32_t)cand.size();
    std::vector<typename Cell::word> cell(len1);
    for (uint32_t y = 1; y <= len1; ++y) cell[y - 1] = Cell::first(y);
    for (uint32_t x = 1; x <= len2; ++x) {
        rf::DlColumn s;
        s.begin<Cell>(x);
        for (uint32_t y = 1; y <= len1; ++y) cell[y - 1] = rf::dl_step<Cell>(s, cell[y - 1], query[y - 1] == cand[x - 1], y);
    }
    return len1 ? Cell::row(cell[len1 - 1]) : len2;
}

static long checked = 0, bad = 0;
static void check(const Str& q, const Str& c)
{
    const uint32_t want = brute(q, c);
    const uint32_t mx = (uint32_t)std::max(q.size(), c.size());
    if (mx <= rf::DlCell8::kMaxLen) {
        const uint32_t got = by_cells<rf::DlCell8>(q, c);
        ++checked;
        if (got != want && ++bad <= 10) std::printf("8-bit cell: len1 %zu len2 %zu: %u, expected %u\n", q.size(), c.size(), got, want);
    }
    const uint32_t got = by_cells<rf::DlCell16>(q, c);
    ++checked;
    if (got != want && ++bad <= 10) std::printf("16-bit cell: len1 %zu len2 %zu: %u, expected %u\n", q.size(), c.size(), got, want);
}

static Str random_str(std::mt19937& rng, size_t len, int sym)
{
    Str s(len);
    for (auto& v : s) v = (uint8_t)(rng() % sym);
    return s;
}
// `base` after `edits` rounds of: swap two adjacent symbols and put a random one between them (the case that separates this metric from OSA)
static Str planted(std::mt19937& rng, Str s, int edits, int sym, size_t clip)
{
    for (int e = 0; e < edits && s.size() >= 2; ++e) {
        const size_t p = rng() % (s.size() - 1);
        std::swap(s[p], s[p + 1]);
        s.insert(s.begin() + p + 1, (uint8_t)(rng() % sym));
    }
    if (s.size() > clip) s.resize(clip);
    return s;
}

int main()
{
    static_assert(rf::DlCell8::kMaxLen == 254 && rf::DlCell16::kMaxLen == 65534, "field widths");
    std::mt19937 rng(20240611);
    auto S = [](const char* t) { Str s; for (; *t; ++t) s.push_back((uint8_t)*t); return s; };
    // known answers (the reference's own tests)
    struct { const char *a, *b; uint32_t d; } known[] = {{"", "", 0}, {"aaaa", "", 4}, {"aaaa", "aaaa", 0}, {"aaaa", "aaa", 1}, {"aaaa", "aaab", 1},
                                                         {"abaa", "baaa", 1}, {"aaaa", "bbbb", 4}, {"CA", "ABC", 2}};
    for (const auto& k : known) {
        if (brute(S(k.a), S(k.b)) != k.d || by_cells<rf::DlCell8>(S(k.a), S(k.b)) != k.d || by_cells<rf::DlCell16>(S(k.b), S(k.a)) != k.d) {
            std::printf("known answer %s / %s != %u\n", k.a, k.b, k.d);
            ++bad;
        }
        ++checked;
    }
    // the query lengths at which the kernels change templates, against short and long candidates, over small and large alphabets
    const size_t qlens[] = {0, 1, 16, 17, 64, 65};
    for (int sym : {2, 4, 62})
        for (size_t ql : qlens)
            for (int rep = 0; rep < 40; ++rep) {
                const Str q = random_str(rng, ql, sym);
                check(q, random_str(rng, rng() % 81, sym));
                check(q, planted(rng, q, 4, sym, 64));
                check(random_str(rng, rng() % 81, sym), q);
            }
    // random pairs, lengths 0..80
    for (int sym : {2, 3, 4, 62})
        for (int rep = 0; rep < 1500; ++rep) check(random_str(rng, rng() % 81, sym), random_str(rng, rng() % 81, sym));
    // the field-width edges: max(len1, len2) = 253, 254 (8-bit fields still hold), 255 and 300 (16-bit fields only), long side as query and as candidate
    for (size_t mx : {(size_t)253, (size_t)254, (size_t)255, (size_t)300})
        for (int sym : {2, 4, 62})
            for (size_t other : {(size_t)0, (size_t)1, (size_t)20, (size_t)64, mx - 1, mx}) {
                const Str lg = random_str(rng, mx, sym);
                check(lg, random_str(rng, other, sym));
                check(random_str(rng, other, sym), lg);
                check(lg, planted(rng, lg, 6, sym, mx));
                // the worst case for the fields: nothing matches, every entry reaches its maximum
                check(Str(mx, 1), Str(other, 2));
                check(Str(other, 2), Str(mx, 1));
            }
    std::printf("pairs checked %ld\nmismatches %ld\n", checked, bad);
    return bad ? 1 : 0;
}

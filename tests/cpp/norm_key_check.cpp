// norm_key_check.cpp -- rf_norm_key.hpp on the host: the f64-seeded key against its integer definition, the key's order against the order
// of the doubles emit_fin produces, and norm_key_ratio as the key's inverse.  Exhaustive for maximum <= 1024; Farey neighbours (fractions
// 1 / (b d) apart, the closest two ratios can be) with both denominators in 60000 .. 65535; dist == maximum, maximum == 0 and the whole
// row of maximum == 65535.  Prints "mismatches 0" when everything holds.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <vector>

#include "../../rapidfuzz_rs_amd/csrc/rf_norm_key.hpp"

namespace {

uint64_t g_mismatches = 0;
void fail(const char* what, uint32_t dist, uint32_t maximum)
{
    if (++g_mismatches <= 20) std::printf("MISMATCH %s at dist %u maximum %u\n", what, dist, maximum);
}

uint64_t bits(double d)
{
    uint64_t b;
    std::memcpy(&b, &d, sizeof b);
    return b;
}

// what emit_fin computes (rf_device.hpp): dist / maximum, 0.0 when maximum == 0
double norm_dist(uint32_t dist, uint32_t maximum) { return maximum == 0 ? 0.0 : (double)dist / (double)maximum; }

uint32_t key_by_definition(uint32_t dist, uint32_t maximum)
{
    if (maximum == 0) return 0;
    const uint64_t x = ((uint64_t)dist << 32) / maximum;
    return (uint32_t)std::min<uint64_t>(x, 0xFFFFFFFFull);
}

struct Seen {
    uint32_t key;
    double nd;
};
std::vector<Seen> g_seen;

void check_pair(uint32_t dist, uint32_t maximum)
{
    const uint32_t key = rf::norm_key(dist, maximum);
    if (key != key_by_definition(dist, maximum)) fail("key != definition", dist, maximum);
    if (rf::norm_key_scaled(dist, maximum, rf::norm_key_scale(maximum)) != key) fail("scaled form", dist, maximum);
    const rf::NormRatio r = rf::norm_key_ratio(key);
    const uint32_t g = maximum == 0 ? 1 : std::gcd(dist, maximum);
    const uint32_t a = maximum == 0 ? 0 : dist / g, b = maximum == 0 ? 1 : maximum / g;
    if (r.a != a || r.b != b) fail("norm_key_ratio != reduced fraction", dist, maximum);
    const double nd = norm_dist(dist, maximum);
    if (r.b == 0 || bits((double)r.a / (double)r.b) != bits(nd)) fail("a / b has other bits than dist / maximum", dist, maximum);
    g_seen.push_back(Seen{key, nd});
}

// key order == double order of nd == reversed double order of 1.0 - nd, equal keys <=> equal doubles: over everything seen so far
void check_order(const char* what)
{
    std::sort(g_seen.begin(), g_seen.end(), [](const Seen& x, const Seen& y) { return x.key < y.key; });
    for (size_t i = 1; i < g_seen.size(); ++i) {
        const Seen &x = g_seen[i - 1], &y = g_seen[i];
        const double sx = 1.0 - x.nd, sy = 1.0 - y.nd;
        const bool ok = x.key == y.key ? (bits(x.nd) == bits(y.nd) && bits(sx) == bits(sy)) : (x.nd < y.nd && sx > sy);
        if (!ok) {
            if (++g_mismatches <= 20) std::printf("MISMATCH order (%s): keys %u %u, nd %.17g %.17g\n", what, x.key, y.key, x.nd, y.nd);
        }
    }
    std::printf("%s: %zu pairs in key order\n", what, g_seen.size());
}

uint64_t mod_inverse(uint64_t a, uint64_t m)  // a^-1 mod m, gcd(a, m) == 1
{
    int64_t t = 0, nt = 1, r = (int64_t)m, nr = (int64_t)(a % m);
    while (nr != 0) {
        const int64_t q = r / nr;
        const int64_t t2 = t - q * nt, r2 = r - q * nr;
        t = nt, nt = t2, r = nr, nr = r2;
    }
    return (uint64_t)(t < 0 ? t + (int64_t)m : t);
}

}  // namespace

int main()
{
    // 1. exhaustive: every maximum <= 1024, every dist <= maximum
    for (uint32_t maximum = 0; maximum <= 1024; ++maximum)
        for (uint32_t dist = 0; dist <= maximum; ++dist) check_pair(dist, maximum);
    check_order("exhaustive to 1024");

    // 2. Farey neighbours a / b < c / d with b c - a d == 1, both denominators in 60000 .. 65535
    uint64_t farey = 0;
    uint64_t lcg = 0x2545F4914F6CDD1Dull;
    auto next = [&] { return (uint32_t)((lcg = lcg * 6364136223846793005ull + 1442695040888963407ull) >> 33); };
    auto neighbours = [&](uint32_t b, uint32_t d) {
        if (b == d || std::gcd(b, d) != 1) return;
        const uint64_t c = mod_inverse(b, d);  // b c == 1 (mod d)
        const uint64_t a = ((uint64_t)b * c - 1) / d;
        if ((uint64_t)b * c - a * d != 1 || a > b || c > d) {
            fail("farey construction", b, d);
            return;
        }
        check_pair((uint32_t)a, b);
        check_pair((uint32_t)c, d);
        if (!(rf::norm_key((uint32_t)a, b) < rf::norm_key((uint32_t)c, d))) fail("farey neighbours share a key or swap", b, d);
        ++farey;
    };
    for (uint32_t b = 65535; b > 65535 - 40; --b)
        for (uint32_t d = 65535; d > 65535 - 40; --d) neighbours(b, d);
    while (farey < 12000) neighbours(60000 + next() % 5536, 60000 + next() % 5536);
    std::printf("farey neighbour pairs: %llu\n", (unsigned long long)farey);
    check_order("with the farey neighbours");

    // 3. the edges: dist == maximum for every maximum, the whole row of maximum == 65535, maximum == 0
    for (uint32_t maximum = 0; maximum <= 65535; ++maximum) check_pair(maximum, maximum);
    for (uint32_t dist = 0; dist <= 65535; ++dist) check_pair(dist, 65535);
    check_pair(0, 0);
    if (rf::norm_key(0, 0) != 0 || rf::norm_key(65535, 65535) != 0xFFFFFFFFu || rf::norm_key(1, 1) != 0xFFFFFFFFu) fail("edge keys", 0, 0);
    if (rf::norm_key(65534, 65535) > 0xFFFFFFFFu - 65536u + 1u) fail("the ratio below the clamp", 65534, 65535);
    check_order("with the edges");

    std::printf("mismatches %llu\n", (unsigned long long)g_mismatches);
    return g_mismatches == 0 ? 0 : 1;
}

// rf_norm_key.hpp -- the 32-bit image of a normalized score dist / maximum (dist <= maximum <= 65535) that rf_topk_multi_f64's in-scan lists
// order by, and its inverse.  Host and device compile the same inlines (tests/cpp/norm_key_check.cpp runs them against the integer
// definition), so this file includes nothing of HIP.
//
//   norm_key(dist, maximum) = 0                                               when maximum == 0 (the reference's 0.0, details/distance.rs:246-250)
//                             min(floor(dist * 2^32 / maximum), 0xFFFFFFFF)   otherwise, in exact integer arithmetic
//
// Two distinct reduced fractions with denominators <= 65535 differ by at least 1 / 65535^2 > 2^-32, so distinct ratios get distinct keys in
// the same order, equal ratios (5/20, 10/40) the same key, and the clamp at dist == maximum collides with nothing (the next ratio below is
// at most 2^32 - 65536).  norm_key_ratio() gives the reduced fraction a / b back: (double)a / (double)b is the correctly rounded quotient of
// the same real number as (double)dist / (double)maximum, i.e. the very bits emit_fin (rf_device.hpp) produces, and 1.0 - that stays
// injective and monotone (ratios are >= 2^-32 apart, doubles near 1 are 2^-53 apart).  Ascending key is therefore exactly ascending
// normalized_distance and exactly descending normalized_similarity, ties included.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RF_NK_HD __host__ __device__ __forceinline__
#else
#define RF_NK_HD inline
#endif

namespace rf {

constexpr uint32_t kNormKeyMaxMaximum = 65535;  // the largest maximum the key is exact for
// May a scan of a query of len1 symbols over candidates of up to max_len order by the key?  Its maximum is fin_mS * (len1 + len2) + fin_mM * max(len1, len2)
// (rf_device.hpp "Finishing") and grows with the candidate's length, so the longest candidate decides.
RF_NK_HD bool norm_key_fits(int32_t fin_mS, int32_t fin_mM, uint64_t len1, uint64_t max_len)
{
    return (uint64_t)fin_mS * (len1 + max_len) + (uint64_t)fin_mM * (len1 > max_len ? len1 : max_len) <= kNormKeyMaxMaximum;
}

// The computation: x = dist * 2^32 / maximum from ONE f64 multiply with scale = 2^32 / maximum (a division per maximum, not per
// candidate: the kernel's maximum is tile-uniform), then one multiply-compare step.  The product is within 2^-20 of x (two roundings of
// 2^-53 relative on a value below 2^32) and the fractional part of x is j / maximum with j < maximum, at least 2^-16 away from the next
// integer: the truncated product is floor(x), or floor(x) - 1 when x is an integer and the product fell just below it.
RF_NK_HD double norm_key_scale(uint32_t maximum) { return maximum == 0 ? 0.0 : 4294967296.0 / (double)maximum; }
RF_NK_HD uint32_t norm_key_scaled(uint32_t dist, uint32_t maximum, double scale)
{
    if (maximum == 0) return 0;
    if (dist >= maximum) return 0xFFFFFFFFu;  // the clamp (x = 2^32)
    uint32_t est = (uint32_t)((double)dist * scale);  // (x <= 2^32 - 65536 here: the conversion is in range, and so is est + 1)
    if ((uint64_t)(est + 1u) * maximum <= ((uint64_t)dist << 32)) ++est;
    return est;
}
RF_NK_HD uint32_t norm_key(uint32_t dist, uint32_t maximum) { return norm_key_scaled(dist, maximum, norm_key_scale(maximum)); }

// The unique reduced fraction a / b with b <= 65535 in [key / 2^32, (key + 1) / 2^32); 0xFFFFFFFF -> 1 / 1.  A fraction with b <= 65535
// below (key + 1) / 2^32 is below it by at least 1 / (b * 2^32) > 2^-49, so the half-open interval holds the same such fractions as the
// closed [key * 2^17, (key + 1) * 2^17 - 1] / 2^49, and the fraction of the smallest denominator in a closed interval is what the
// continued-fraction walk yields: take floor(lo) and continue with the reciprocals of the remainders until an integer lies inside
// (about 20 steps; a unit-step Stern-Brocot walk would need up to 65535).  A key norm_key() does not produce yields the simplest
// fraction of its interval, whatever its denominator.
struct NormRatio {
    uint32_t a, b;
};
RF_NK_HD NormRatio norm_key_ratio(uint32_t key)
{
    if (key == 0xFFFFFFFFu) return NormRatio{1u, 1u};
    uint64_t ln = (uint64_t)key << 17, ld = 1ull << 49, hn = (((uint64_t)key + 1) << 17) - 1, hd = 1ull << 49;  // lo = ln / ld <= hi = hn / hd
    uint64_t p1 = 1, q1 = 0, p2 = 0, q2 = 1;  // the convergents before the current term
    for (;;) {
        const uint64_t f = ln / ld, r = ln % ld;
        uint64_t term = f;
        bool last = r == 0;            // lo is an integer: the simplest number of the interval
        if (!last && (f + 1) * hd <= hn) {  // an integer inside (lo, hi]
            term = f + 1;
            last = true;
        }
        const uint64_t p = term * p1 + p2, q = term * q1 + q2;
        if (last) return NormRatio{(uint32_t)p, (uint32_t)q};
        p2 = p1, q2 = q1, p1 = p, q1 = q;
        // f < lo <= hi < f + 1: x = f + 1 / y with y in [1 / (hi - f), 1 / (lo - f)]
        const uint64_t nln = hd, nld = hn - f * hd, nhn = ld, nhd = r;
        ln = nln, ld = nld, hn = nhn, hd = nhd;
    }
}

}  // namespace rf

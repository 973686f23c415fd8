// rf_filter_multi_rows.hpp -- what rf_filter_multi_f64 does on the host with one fused member's key row: order it as asked and turn every key
// (norm_key(dist, maximum) << 32 | local index, rf_norm_key.hpp) back into the pair rf_filter_f64 returns.  Includes nothing of HIP, so a plain
// host program can run it (tests/cpp/filter_multi_f64_rows_check.cpp).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/rfgpu.h"
#include "rf_norm_key.hpp"

namespace rf {

// keys[0 .. have): reordered in place.  Both normalized ops store the ascending key -- a smaller key is a smaller normalized distance, i.e. the better
// score for either op -- so RF_FILTER_BY_SCORE (best first, ties by ascending index) is a plain sort of the 64-bit keys, RF_FILTER_BY_INDEX a sort by
// the low word (indices are unique within a row) and RF_FILTER_ANY leaves the order of arrival.  The key's reduced fraction a / b is the normalized
// distance: (double)a / (double)b are the bits emit_fin (rf_device.hpp) divides out of dist and maximum, and `as_distance` (normalized_distance of a
// metric that is no fuzz ratio) returns it as it is, everything else 1.0 - it -- rf_topk_multi_f64's decode.
inline void filter_multi_f64_row(uint64_t* keys, size_t have, rf_filter_order order, bool as_distance, uint64_t index_base, uint64_t* out_index, double* out_score)
{
    if (order == RF_FILTER_BY_SCORE)
        std::sort(keys, keys + have);
    else if (order == RF_FILTER_BY_INDEX)
        std::sort(keys, keys + have, [](uint64_t a, uint64_t b) { return (uint32_t)a < (uint32_t)b; });
    for (size_t m = 0; m < have; ++m) {
        const NormRatio r = norm_key_ratio((uint32_t)(keys[m] >> 32));
        const double nd = (double)r.a / (double)r.b;
        out_index[m] = index_base + (uint32_t)keys[m];
        out_score[m] = as_distance ? nd : 1.0 - nd;
    }
}

}  // namespace rf

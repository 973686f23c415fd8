// rf_dl_cell.hpp -- one cell of the unrestricted Damerau-Levenshtein recurrence (damerau_levenshtein.rs:111-168, the linear-space
// algorithm of Zhao and Sahni), in the orientation of rf_long.hip's Wagner-Fischer kernels: the CANDIDATE's symbols are the columns
// x = 1 .. len2 that stream by, the state is a row over the QUERY positions y = 1 .. len1.  Host and device compile the same inlines
// (tests/cpp/dl_cell_check.cpp runs them against a full-matrix implementation), so this file includes nothing of HIP.
//
// With H[x][y] the distance between the first x candidate symbols and the first y query symbols,
//   H[x][y] = H[x-1][y-1]                                                   if c_x == q_y, else
//             1 + min(H[x-1][y-1], H[x][y-1], H[x-1][y])                    and the two transposition terms that can win:
//             H[k-1][y-2] + (x - k)       when q_{y-1} == c_x,  k = last column before x that held q_y        (A)
//             H[x-2][l-1] + (y - l)       when c_{x-1} == q_y,  l = last query position before y that holds c_x  (B)
// Both are costs of real edit scripts, so taking each whenever its condition holds is exact.  k is a property of the query POSITION
// y -- "the last column that held the symbol q_y" -- so it needs no per-lane hash map: it is written exactly where the cell's own
// compare hits, and in one column hits only write it and misses only read it.  Per query position the state is four numbers:
//   row   H[x-1][y], replaced by H[x][y]           row2  H[x-2][y], replaced by H[x-1][y]
//   fr    H[k-1][y-2] as of the last hit at y      col   k (1-based; 0 = no column held q_y yet)
// every one at most max(len1, len2) + 1, so they share one machine word: four 8-bit fields of a u32 while max(len1, len2) <= 254,
// four 16-bit fields of a u64 up to 65534.  "Infinity" (H outside the matrix) is the field's all-ones value, above every real entry.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RF_DL_HD __host__ __device__ __forceinline__
#else
#define RF_DL_HD inline
#endif

namespace rf {

template <typename W, int kBits>
struct DlCell {
    using word = W;
    static constexpr uint32_t kInf = (1u << kBits) - 1u;       // the all-ones field
    static constexpr uint32_t kMaxLen = kInf - 1u;             // longest string (query or candidate) the fields hold
    static RF_DL_HD uint32_t row(W c) { return (uint32_t)c & kInf; }
    static RF_DL_HD uint32_t row2(W c) { return (uint32_t)(c >> kBits) & kInf; }
    static RF_DL_HD uint32_t fr(W c) { return (uint32_t)(c >> (2 * kBits)) & kInf; }
    static RF_DL_HD uint32_t col(W c) { return (uint32_t)(c >> (3 * kBits)) & kInf; }
    static RF_DL_HD W pack(uint32_t row, uint32_t row2, uint32_t fr, uint32_t col)
    {
        return (W)row | ((W)row2 << kBits) | ((W)fr << (2 * kBits)) | ((W)col << (3 * kBits));
    }
    // before the first column: row 0 of the matrix (H[0][y] = y), nothing above it, no hit yet
    static RF_DL_HD W first(uint32_t y) { return pack(y, kInf, kInf, 0); }
};
using DlCell8 = DlCell<uint32_t, 8>;
using DlCell16 = DlCell<uint64_t, 16>;

// what one column carries down the query positions
struct DlColumn {
    uint32_t x;         // the column, 1-based
    uint32_t diag;      // H[x-1][y-1]
    uint32_t diag2;     // H[x-1][y-2]
    uint32_t left;      // H[x][y-1]
    uint32_t row2_prev; // H[x-2][y-1]
    uint32_t t_less_l;  // term (B)'s H[x-2][l-1] - l for the last hit l of this column (mod 2^32; infinity before the first hit)
    bool hit_prev;      // q_{y-1} == c_x
    template <class Cell>
    RF_DL_HD void begin(uint32_t column)
    {
        x = column;
        diag = column - 1;
        diag2 = Cell::kInf;
        left = column;
        row2_prev = column >= 2 ? column - 2 : Cell::kInf;
        t_less_l = Cell::kInf;
        hit_prev = false;
    }
};

// query position y (1-based) of column s.x: `c` is the position's cell as the previous column left it, `hit` is q_y == c_x.
// Returns the cell to keep; s.left is H[x][y].
template <class Cell>
RF_DL_HD typename Cell::word dl_step(DlColumn& s, typename Cell::word c, bool hit, uint32_t y)
{
    using W = typename Cell::word;
    const uint32_t up = Cell::row(c), r2 = Cell::row2(c), k = Cell::col(c);
    uint32_t m = (s.diag < s.left ? s.diag : s.left);
    m = (up < m ? up : m) + 1;
    const uint32_t a = Cell::fr(c) + (s.x - k);  // (A)
    const uint32_t b = s.t_less_l + y;           // (B)
    if (s.hit_prev && a < m) m = a;
    if (k + 1 == s.x && b < m) m = b;
    const uint32_t val = hit ? s.diag : m;
    // a miss keeps (fr, col) and shifts row -> row2; a hit also notes the column and H[x-1][y-2] for a later (A)
    constexpr int kB = (int)(sizeof(W) * 2);  // bits per field
    const W low = (W)val | ((W)up << kB);
    const W high_mask = ~(W)0 << (2 * kB);
    const W out = hit ? (low | ((W)s.diag2 << (2 * kB)) | ((W)s.x << (3 * kB))) : (low | (c & high_mask));
    s.t_less_l = hit ? s.row2_prev - y : s.t_less_l;
    s.hit_prev = hit;
    s.diag2 = s.diag;
    s.diag = up;
    s.left = val;
    s.row2_prev = r2;
    return out;
}

}  // namespace rf

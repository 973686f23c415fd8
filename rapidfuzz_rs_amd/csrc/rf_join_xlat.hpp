// rf_join_xlat.hpp -- the symbol-level row map of the join calls' device road (rf_api_join.hip builds it once per call, rf_join.hip join_pm_kernel and
// join_bad_kernel read it): which row of the SCANNED corpus' LDS table the symbol behind a stored byte of the QUERY corpus owns, whatever the kind -- bytes or
// `char` -- of either corpus.  Plain arithmetic over plain views, no HIP call: tests/cpp/join_xlat_check.cpp drives it with plain g++.
//
//   stored byte s      what the query corpus' payload holds: sigma_q[id], id = the byte itself (byte corpus) or the symbol's id in that corpus' alphabet (`char`)
//   the symbol         inv_sigma_q[s] for a byte corpus; sym_of_id[inv_sigma_q[s]] for a `char` corpus; NOT KNOWN from the byte when the id is the overflow id
//   its id over there  resolve()'s rule (rf_api.hip), to the letter: a byte corpus takes the code points 0..255 as they are and cannot hold a symbol above
//                      0xFF; a `char` corpus looks the symbol up in its alphabet; a symbol it lumped into its overflow class cannot be told apart from the
//                      others there; a symbol it does not store at all gets kXlatAbsentId, an id no candidate byte has
//   row_of[s]          sigma_c[that id]
//   bad[s]             1: the symbol cannot be placed exactly -- s is the queries' overflow id, or the symbol is in the scanned corpus' overflow class, or it is
//                      above 0xFF and the scanned corpus holds bytes.  A row of Q that holds such a byte goes down the per-query road.
//   any_bad            some stored value the query corpus may hold is bad: only then are the rows looked at (join_bad_kernel)
// Two byte corpora: row_of[s] == sigma_c[inv_sigma_q[s]] and nothing is bad.
// row_of of a bad value, and of a value the query corpus never stores (an id of a `char` corpus no symbol has), is never read: it is the absent row when the
// scanned corpus is `char`, else 0.
#pragma once

#include <stdint.h>

#include "rf_take_addr.hpp"

namespace rf {

constexpr uint32_t kXlatOverflowId = 254;          // rf_host.hpp kOverflowId
constexpr uint32_t kXlatAbsentId = 255;            // rf_host.hpp kAbsentId
constexpr uint32_t kXlatNoSymbol = 0xFFFFFFFFu;    // sym_of_id of an id no symbol has (the reserved symbol: no corpus stores it)

// One corpus as the map needs it
struct JoinXlatCorpus {
    bool wide;                  // a `char` corpus: the stored byte is sigma[id in the alphabet]
    const uint8_t* sigma;       // 256 bytes: id (byte corpora: the byte) -> stored byte; a permutation
    const uint32_t* sym_of_id;  // `char`: 256 u32, id -> symbol, kXlatNoSymbol for an id not in use (the overflow id and the absent id among them); bytes: not read
    bool has_overflow;          // `char`: some symbols share kXlatOverflowId
};

struct JoinXlat {
    uint8_t row_of[256];
    uint8_t bad[256];
    bool any_bad;
};

// lookup(symbol) -> the symbol's id in the scanned `char` corpus' alphabet, kXlatOverflowId when it is in that corpus' overflow class, kXlatAbsentId when the
// corpus does not store it at all.  Not called when the scanned corpus holds bytes.
// false: the scanned `char` corpus' absent row sigma_c[kXlatAbsentId] is also the row of an id in use, so an absent symbol could match a candidate byte (sigma
// is no permutation); *out is untouched and the caller must not fuse.
template <class Lookup>
inline bool join_xlat_build(const JoinXlatCorpus& q, const JoinXlatCorpus& c, Lookup&& lookup, JoinXlat* out)
{
    if (c.wide)
        for (uint32_t id = 0; id < 256; ++id) {
            const bool in_use = id == kXlatOverflowId ? c.has_overflow : (id != kXlatAbsentId && c.sym_of_id[id] != kXlatNoSymbol);
            if (in_use && c.sigma[id] == c.sigma[kXlatAbsentId]) return false;
        }
    uint8_t inv_q[256];
    take_inverse_sigma(q.sigma, inv_q);
    const uint8_t no_row = c.wide ? c.sigma[kXlatAbsentId] : (uint8_t)0;
    JoinXlat x;
    x.any_bad = false;
    for (uint32_t s = 0; s < 256; ++s) {
        const uint32_t id_q = inv_q[s];
        x.row_of[s] = no_row, x.bad[s] = 0;
        uint32_t sym;
        if (!q.wide) {
            sym = id_q;
        } else if (id_q == kXlatOverflowId) {
            if (q.has_overflow) x.bad[s] = 1, x.any_bad = true;  // (without the class the value is never stored)
            continue;
        } else if (id_q == kXlatAbsentId || q.sym_of_id[id_q] == kXlatNoSymbol) {
            continue;  // never stored
        } else {
            sym = q.sym_of_id[id_q];
        }
        uint32_t id_c;
        if (!c.wide) {
            if (sym > 0xFF) {
                x.bad[s] = 1, x.any_bad = true;
                continue;
            }
            id_c = sym;
        } else {
            id_c = lookup(sym);
            if (id_c == kXlatOverflowId) {
                x.bad[s] = 1, x.any_bad = true;
                continue;
            }
        }
        x.row_of[s] = c.sigma[id_c & 0xFFu];
    }
    *out = x;
    return true;
}

}  // namespace rf

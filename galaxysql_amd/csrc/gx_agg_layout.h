/*
 * gx_agg_layout.h — the one definition of the per-group aggregate state
 * record: which funcs exist and what they return, how a list of them lays
 * out into a record, and how a record slot decodes to an output value.
 * AggOp, GroupJoinOp and the frame window's whole-partition frame hold an
 * AggLayout; every accumulate / emit parameter struct embeds its AggRecDesc.
 *
 * The record is AoS, `stride` u64s: per aggregate one value slot (two for
 * SUM_DEC / AVG_DEC: {lo, hi} of the 128-bit sum), then one "seen" slot for
 * the funcs that start NULL (AVG's is its count). A fresh record is a copy
 * of `tmpl`: the value slots' identities, seen = 0.
 *
 * Plain C++, compiled for host and device alike (host g++: -I include).
 */
#ifndef GX_AGG_LAYOUT_H
#define GX_AGG_LAYOUT_H

#include <stdint.h>

#include "../../include/gxop.h"

#if defined(__HIPCC__)
#define GX_HD __host__ __device__
#else
#define GX_HD
#endif

#define GX_MAX_COLS 16

/* ---- funcs --------------------------------------------------------------- */

GX_HD static inline bool agg_func_is_dec(int32_t func) {
    return func == GX_AGG_SUM_DEC || func == GX_AGG_AVG_DEC;
}

/* additive: the state takes plain (non-returning) adds only. SUM_DEC /
 * AVG_DEC are NOT: their carry needs the returning add of agg_rmw */
GX_HD static inline bool agg_func_additive(int32_t func) {
    return func == GX_AGG_COUNT_ROW || func == GX_AGG_COUNT_COL ||
           func == GX_AGG_SUM_I64 || func == GX_AGG_SUM_I64N ||
           func == GX_AGG_SUM_F64 || func == GX_AGG_AVG_F64;
}
GX_HD static inline bool agg_func_adds_f64(int32_t func) {
    return func == GX_AGG_SUM_F64 || func == GX_AGG_AVG_F64;
}

/* starts NULL and has a seen slot; the others are valid from their identity */
GX_HD static inline bool agg_func_tracks_null(int32_t func) {
    return !(func == GX_AGG_COUNT_ROW || func == GX_AGG_COUNT_COL ||
             func == GX_AGG_SUM_I64 || func == GX_AGG_BIT_AND ||
             func == GX_AGG_BIT_OR || func == GX_AGG_BIT_XOR);
}

/* the bits a value slot starts from */
GX_HD static inline unsigned long long agg_func_identity(int32_t func) {
    switch (func) {
    case GX_AGG_MIN_I64: return 0x7FFFFFFFFFFFFFFFull; /* INT64_MAX */
    case GX_AGG_MAX_I64: return 0x8000000000000000ull; /* INT64_MIN */
    case GX_AGG_MIN_F64: return 0x7FF0000000000000ull; /* +Inf */
    case GX_AGG_MAX_F64: return 0xFFF0000000000000ull; /* -Inf */
    case GX_AGG_BIT_AND: return ~0ull;
    default: return 0ull;
    }
}

/* result column type of a plain aggregate func (the window-only funcs are
 * the window ops' own cases) */
GX_HD static inline int32_t agg_func_result_type(int32_t func) {
    if (agg_func_is_dec(func)) return GX_DECIMAL;
    switch (func) {
    case GX_AGG_SUM_F64: case GX_AGG_MIN_F64: case GX_AGG_MAX_F64:
    case GX_AGG_AVG_F64:
        return GX_F64;
    default:
        return GX_I64;
    }
}

/* ---- record descriptor (what the kernels read) --------------------------- */

struct AggRecDesc {
    int32_t n_aggs;
    int32_t stride;                  /* record size in u64s */
    int32_t func[GX_MAX_COLS];
    int32_t val_off[GX_MAX_COLS];
    int32_t seen_off[GX_MAX_COLS];   /* -1 = always-valid agg */
};

/* ---- layout (host side) -------------------------------------------------- */

struct AggLayout {
    AggRecDesc desc;
    unsigned long long tmpl[3 * GX_MAX_COLS]; /* <= 3 slots per agg */
    bool tmpl_zero;                           /* tmpl is all zero bits */

    /* base funcs: no DISTINCT variant, no scale in the upper bits */
    void build(const int32_t *base_funcs, int n) {
        int32_t off = 0;
        desc = AggRecDesc();
        for (int k = 0; k < 3 * GX_MAX_COLS; k++) tmpl[k] = 0ull;
        desc.n_aggs = n;
        for (int a = 0; a < n; a++) {
            const int32_t f = base_funcs[a];
            desc.func[a] = f;
            desc.val_off[a] = off;
            tmpl[off++] = agg_func_identity(f);
            if (agg_func_is_dec(f)) off++; /* {lo, hi}: hi follows lo */
            desc.seen_off[a] = agg_func_tracks_null(f) ? off++ : -1;
        }
        desc.stride = off > 0 ? off : 1;
        tmpl_zero = true;
        for (int32_t k = 0; k < desc.stride; k++)
            if (tmpl[k] != 0ull) tmpl_zero = false;
    }

    /* the same records seen through aggregates agg_idx[0..k) only */
    AggRecDesc select(const int32_t *agg_idx, int k) const {
        AggRecDesc d = AggRecDesc();
        d.n_aggs = k;
        d.stride = desc.stride;
        for (int i = 0; i < k; i++) {
            d.func[i] = desc.func[agg_idx[i]];
            d.val_off[i] = desc.val_off[agg_idx[i]];
            d.seen_off[i] = desc.seen_off[agg_idx[i]];
        }
        return d;
    }
};

/* ---- record slot -> output value ------------------------------------------
 * NULL iff the func has a seen slot and it is 0. The seen slot of a
 * null-tracking SUM may hold more than 1 (the transposed accumulate adds to
 * it): only AVG, whose slot is its count, reads more than "non-zero".
 * A NULL decodes to zero bits, which is 0 and 0.0 alike. The DECIMAL funcs'
 * 40-byte decode is k_agg_emit's own. */
struct AggDecoded {
    unsigned long long bits; /* an I64, or the bit pattern of an F64 */
    bool isnull;
};

GX_HD static inline AggDecoded agg_decode(int32_t func,
                                          const unsigned long long *rec,
                                          int32_t val_off, int32_t seen_off) {
    AggDecoded d;
    const unsigned long long seen = seen_off >= 0 ? rec[seen_off] : 1ull;
    d.isnull = seen == 0ull;
    d.bits = d.isnull ? 0ull : rec[val_off];
    if (func == GX_AGG_AVG_F64 && !d.isnull) {
        double sum;
        __builtin_memcpy(&sum, &d.bits, 8);
        sum /= (double)seen;
        __builtin_memcpy(&d.bits, &sum, 8);
    }
    return d;
}

#endif /* GX_AGG_LAYOUT_H */

/*
 * gxhip_scan.inc — vectorized filter + project (included by gxhip.hip).
 *
 * The GPU fusion of the reference's vectorized filter/projection stage
 * (executor/vectorized/, VectorizedFilterExec; SURVEY.md §8f row 1): one
 * streaming pass evaluates the AND of predicates (SQL semantics: NULL
 * fails every comparison), ballot-compacts the selection, and writes the
 * projected columns in the same kernel — no selection-vector round trip
 * through HBM.
 */

namespace {

#define GX_MAX_PREDS 8

/* predicate half of a scan: shared by k_scan and the fused probe-scan
 * kernel, which takes it next to the join's ProbeParams */
struct ScanPreds {
    int32_t n_preds;
    int32_t pred_cmp[GX_MAX_PREDS];
    int64_t pred_i64[GX_MAX_PREDS];
    double  pred_f64[GX_MAX_PREDS];
    const uint8_t *pred_pat[GX_MAX_PREDS];
    int32_t pred_plen[GX_MAX_PREDS];
    DevColView pred_view[GX_MAX_PREDS];
};

struct ScanParams {
    int64_t n;
    ScanPreds preds;
    int32_t n_projs;
    int32_t proj_op[GX_MAX_COLS];
    int32_t proj_scale[GX_MAX_COLS];
    DevColView proj_a[GX_MAX_COLS];
    DevColView proj_b[GX_MAX_COLS];
    DevColView proj_c[GX_MAX_COLS];
    DevColView proj_d[GX_MAX_COLS];
    void *out_vals[GX_MAX_COLS];
    uint8_t *out_nulls[GX_MAX_COLS];
    uint32_t *out_rowids;   /* selected source rows (for slice post-gather) */
    uint32_t cap;
    uint32_t *counter;
    uint32_t *err;      /* wide-DECIMAL fence flag (counter word + 1) */
};

__device__ static const int64_t d_POW10[19] = {1LL,10LL,100LL,1000LL,
    10000LL,100000LL,1000000LL,10000000LL,100000000LL,1000000000LL,
    10000000000LL,100000000000LL,1000000000000LL,10000000000000LL,
    100000000000000LL,1000000000000000LL,10000000000000000LL,
    100000000000000000LL,1000000000000000000LL};

/* device mirrors of oracle/gx_oracle.cpp dec40_to_scaled/scaled_to_dec40
 * (DecimalBox "simple" 40-B layout; DecimalBox.java doAddToSum1/2).
 * Wide-DECIMAL fence: values needing a third integer word (integers > 18)
 * or more than 18 total significant digits do not fit the scaled-int64
 * fast path — the reference falls back to full 9-limb Decimal arithmetic
 * there (DecimalBox.java:43-71); we flag *err and the host rejects the
 * chunk loudly instead of silently truncating. */
__device__ static inline int64_t dec40_to_scaled_dev(const uint8_t *p,
                                                     int scale,
                                                     uint32_t *err) {
    const int32_t *w = (const int32_t *)p;
    uint8_t integers = p[36];
    uint8_t isneg = p[39];
    int64_t ip, fr;
    if (integers > 9) {
        ip = (int64_t)w[0] * 1000000000LL + w[1];
        fr = w[2];
    } else {
        ip = w[0];
        fr = w[1];
    }
    if (integers > 18 || ip >= d_POW10[18 - scale]) {
        atomicOr(err, 1u);
        return 0;
    }
    int64_t v = ip * d_POW10[scale] + fr / d_POW10[9 - scale];
    return isneg ? -v : v;
}

__device__ static inline void scaled_to_dec40_dev(int64_t v, int scale,
                                                  uint8_t *p) {
    for (int k = 0; k < 5; k++) ((uint64_t *)p)[k] = 0;
    uint8_t isneg = v < 0;
    uint64_t a = isneg ? (uint64_t)(-v) : (uint64_t)v;
    int64_t ip = (int64_t)(a / (uint64_t)d_POW10[scale]);
    int64_t fr = (int64_t)(a % (uint64_t)d_POW10[scale]) * d_POW10[9 - scale];
    int32_t *w = (int32_t *)p;
    uint8_t integers;
    if (ip >= 1000000000LL) {
        w[0] = (int32_t)(ip / 1000000000LL);
        w[1] = (int32_t)(ip % 1000000000LL);
        w[2] = (int32_t)fr;
        integers = 18;
    } else {
        w[0] = (int32_t)ip;
        w[1] = (int32_t)fr;
        w[2] = 0;
        integers = 9;
    }
    p[36] = integers;
    p[37] = (uint8_t)scale;
    p[38] = (uint8_t)scale;
    p[39] = isneg;
}

__device__ static inline bool cmp_i64(int64_t a, int32_t cmp, int64_t b) {
    switch (cmp) {
    case GX_CMP_LT: return a < b;
    case GX_CMP_LE: return a <= b;
    case GX_CMP_GT: return a > b;
    case GX_CMP_GE: return a >= b;
    case GX_CMP_EQ: return a == b;
    default: return a != b;
    }
}
__device__ static inline bool cmp_f64(double a, int32_t cmp, double b) {
    switch (cmp) {
    case GX_CMP_LT: return a < b;
    case GX_CMP_LE: return a <= b;
    case GX_CMP_GT: return a > b;
    case GX_CMP_GE: return a >= b;
    case GX_CMP_EQ: return a == b;
    default: return a != b;
    }
}

__device__ static inline bool scan_row_passes(const ScanPreds &P, int64_t i) {
    for (int p = 0; p < P.n_preds; p++) {
        const DevColView &c = P.pred_view[p];
        if (col_is_null(c, i)) return false; /* SQL: NULL fails */
        bool ok;
        switch (c.type) {
        case GX_I64:
            ok = cmp_i64(((const int64_t *)c.values)[i], P.pred_cmp[p],
                         P.pred_i64[p]);
            break;
        case GX_I32:
            ok = cmp_i64((int64_t)((const int32_t *)c.values)[i],
                         P.pred_cmp[p], P.pred_i64[p]);
            break;
        case GX_SLICE: {
            /* LIKE '%pat%': naive byte search (p_name is ~30 B) */
            int32_t b = slice_begin(c, i), e = c.offsets[i];
            int32_t len = e - b, pl = P.pred_plen[p];
            const uint8_t *pat = P.pred_pat[p];
            ok = false;
            for (int32_t st = 0; st + pl <= len && !ok; st++) {
                bool m = true;
                for (int32_t k = 0; k < pl && m; k++)
                    m = c.bytes[b + st + k] == pat[k];
                ok = m;
            }
            break; }
        default:
            ok = cmp_f64(((const double *)c.values)[i], P.pred_cmp[p],
                         P.pred_f64[p]);
            break;
        }
        if (!ok) return false;
    }
    return true;
}

/* The value of a register-sized projection at source row `src`: a COPY of
 * an I64/I32/F64 column, REV_F64, REV_SCALED4, Q9_AMOUNT4 or Q1_CHARGE6. The
 * one place
 * these expressions are computed: proj_store (k_scan, k_gather_proj) stores
 * what this returns and the group-join probe-scan accumulates it, so all
 * three are bit-identical. A NULL input gives isnull and the value the
 * expression has over zeros. */
__device__ static inline AggVal proj_value(int32_t op, const DevColView &a,
                                           const DevColView &b,
                                           const DevColView &cc,
                                           const DevColView &dd, int64_t src) {
    AggVal v;
    v.bits = 0;
    v.hi = 0; /* SUM_DEC / AVG_DEC never take a projection's value */
    v.type = GX_I64;
    switch (op) {
    case GX_PROJ_COPY:
        v.type = a.type;
        v.isnull = col_is_null(a, src);
        if (!v.isnull)
            v.bits = a.type == GX_I32
                ? (unsigned long long)(int64_t)((const int32_t *)a.values)[src]
                : ((const unsigned long long *)a.values)[src];
        break;
    case GX_PROJ_REV_F64: {
        v.type = GX_F64;
        v.isnull = col_is_null(a, src) || col_is_null(b, src);
        double av = v.isnull ? 0 : ((const double *)a.values)[src];
        double bv = v.isnull ? 0 : ((const double *)b.values)[src];
        v.bits = __builtin_bit_cast(unsigned long long, av * (1.0 - bv));
        break; }
    case GX_PROJ_REV_SCALED4: {
        v.isnull = col_is_null(a, src) || col_is_null(b, src);
        int64_t av = v.isnull ? 0 : ((const int64_t *)a.values)[src];
        int64_t bv = v.isnull ? 0 : ((const int64_t *)b.values)[src];
        v.bits = (uint64_t)av * (uint64_t)(100 - bv);
        break; }
    case GX_PROJ_Q1_CHARGE6: {
        v.isnull = col_is_null(a, src) || col_is_null(b, src) ||
                   col_is_null(cc, src);
        int64_t av = v.isnull ? 0 : ((const int64_t *)a.values)[src];
        int64_t bv = v.isnull ? 0 : ((const int64_t *)b.values)[src];
        int64_t cv = v.isnull ? 0 : ((const int64_t *)cc.values)[src];
        v.bits = (uint64_t)av * (uint64_t)(100 - bv) * (uint64_t)(100 + cv);
        break; }
    case GX_PROJ_Q9_AMOUNT4: {
        v.isnull = col_is_null(a, src) || col_is_null(b, src) ||
                   col_is_null(cc, src) || col_is_null(dd, src);
        int64_t av = v.isnull ? 0 : ((const int64_t *)a.values)[src];
        int64_t bv = v.isnull ? 0 : ((const int64_t *)b.values)[src];
        int64_t cv = v.isnull ? 0 : ((const int64_t *)cc.values)[src];
        int64_t dv = v.isnull ? 0 : ((const int64_t *)dd.values)[src];
        v.bits = (unsigned long long)(
            (int64_t)((uint64_t)av * (uint64_t)(100 - bv)) -
            (int64_t)((uint64_t)cv * (uint64_t)dv * 100u));
        break; }
    default: /* not a register-sized expression: callers never pass one */
        v.isnull = true;
        break;
    }
    return v;
}

/* Evaluate one projection at source row `src` and store it at output row
 * `at`. k_scan and the fused probe-scan gather both call it. SLICE copies
 * are not handled here (gathered in a post-pass). */
__device__ static inline void proj_store(int32_t op, int32_t scale,
                                         const DevColView &a,
                                         const DevColView &b,
                                         const DevColView &cc,
                                         const DevColView &dd, int64_t src,
                                         void *out_vals, uint8_t *out_nulls,
                                         int64_t at, uint32_t *err) {
    switch (op) {
    case GX_PROJ_COPY: {
        if (a.type == GX_SLICE) break; /* gathered post-pass */
        if (a.type == GX_DECIMAL) {
            bool nn = col_is_null(a, src);
            if (out_nulls) out_nulls[at] = nn;
            for (int k = 0; k < 5; k++)
                ((uint64_t *)out_vals)[(size_t)at * 5 + k] =
                    nn ? 0 : ((const uint64_t *)a.values)[src * 5 + k];
            break;
        }
        AggVal v = proj_value(op, a, b, cc, dd, src);
        if (out_nulls) out_nulls[at] = v.isnull;
        if (a.type == GX_I32) ((int32_t *)out_vals)[at] = (int32_t)v.bits;
        else ((unsigned long long *)out_vals)[at] = v.bits;
        break; }
    case GX_PROJ_REV_F64:
    case GX_PROJ_REV_SCALED4:
    case GX_PROJ_Q9_AMOUNT4:
    case GX_PROJ_Q1_CHARGE6: {
        AggVal v = proj_value(op, a, b, cc, dd, src);
        if (out_nulls) out_nulls[at] = v.isnull;
        ((unsigned long long *)out_vals)[at] = v.bits;
        break; }
    case GX_PROJ_DEC_TO_SCALED: {
        bool nn = col_is_null(a, src);
        if (out_nulls) out_nulls[at] = nn;
        ((int64_t *)out_vals)[at] = nn ? 0
            : dec40_to_scaled_dev((const uint8_t *)a.values +
                                  (size_t)src * 40, scale, err);
        break; }
    case GX_PROJ_SCALED_TO_DEC: {
        bool nn = col_is_null(a, src);
        if (out_nulls) out_nulls[at] = nn;
        uint8_t *dst = (uint8_t *)out_vals + (size_t)at * 40;
        if (nn)
            for (int k = 0; k < 5; k++) ((uint64_t *)dst)[k] = 0;
        else
            scaled_to_dec40_dev(((const int64_t *)a.values)[src], scale, dst);
        break; }
    }
}

/* ---- fused scan + probe kernel (gxop_join_probe_scan fast path) --------
 * Grid-strides over the RAW rows in three wave-synchronous stages, so the
 * emitted probe index is the raw row id and no projected column is
 * materialized for rows the join drops.
 *
 * 1. Stream: a wave takes a tile of 64*R rows per iteration, row =
 *    tile + r*64 + lane, so every load is a plain coalesced wave-wide
 *    access whatever the column pointers' alignment. All R key loads and
 *    the R loads of a predicate column are issued before the first use
 *    (R x 768 B in flight per wave instead of 768 B), then the rows that
 *    pass issue their bloom-word loads together.
 * 2. Compact: rows that pass the predicates, have a non-NULL key and pass
 *    the bloom are ballot-compacted into a per-wave LDS queue of
 *    (raw row id, key).
 * 3. Walk: whenever the queue holds >= 64 entries (and once at the end for
 *    the rest) the wave pops 64, one per lane, and runs the bucket walk
 *    (probe_key) on them: the random HBM line of the bucket is fetched
 *    with every lane busy, not for the ~5 of 64 lanes that survive Q3's
 *    predicate and bloom.
 *
 * Survivors of the predicates (not of the bloom) are counted per wave in a
 * register and added to *kept once per wave. */
#define GX_PS_R 2                          /* rows per lane per iteration */
#define GX_PS_TILE (64 * GX_PS_R)          /* rows per wave per iteration */
#define GX_PS_BLOCK_ROWS (256 * GX_PS_R)   /* rows per block per iteration */
/* grid cap: one pass of the full grid covers 4096 * 256 * R rows
 * (2,097,152 at R = 2); longer inputs grid-stride */
#define GX_PS_GRID_CAP 4096
/* queue: up to 63 carried entries + one iteration's worst case (64*R) */
#define GX_PS_QCAP (64 + GX_PS_TILE)
/* emit stage per wave: the largest that keeps queue (192 x 12 B) + stage
 * (384 x 8 B) per wave, 21,504 B per block, at 7 blocks per CU inside the
 * 160 KB of LDS, i.e. the 7 waves/SIMD the registers allow. Measured
 * (profiles/README.md Round 5): the stage size moves the step more than R
 * does, one atomicAdd on the pair counter per flush. */
#define GX_PS_STAGE 384

static inline int gx_ps_grid(int64_t n) {
    int64_t g = (n + GX_PS_BLOCK_ROWS - 1) / GX_PS_BLOCK_ROWS;
    if (g > GX_PS_GRID_CAP) g = GX_PS_GRID_CAP;
    if (g < 1) g = 1;
    return (int)g;
}

/* AND the scan predicates into `pass` (bit r = row row0 + r*64) for the
 * lane's R rows. Same semantics as scan_row_passes (a NULL value fails),
 * but column by column: the R loads of a column go out back to back.
 * Rows at or past n never load; their bits are already clear. */
__device__ static inline uint32_t scan_rows_pass_wide(const ScanPreds &S,
                                                      int64_t row0, int64_t n,
                                                      uint32_t pass) {
    for (int p = 0; p < S.n_preds; p++) {
        const DevColView &c = S.pred_view[p];
        const int32_t cmp = S.pred_cmp[p];
        uint32_t ok = 0;
        uint8_t nl[GX_PS_R];
#pragma unroll
        for (int r = 0; r < GX_PS_R; r++) {
            const int64_t row = row0 + r * 64;
            nl[r] = (c.has_nulls && row < n) ? c.nulls[row] : (uint8_t)0;
        }
        switch (c.type) {
        case GX_I64: {
            int64_t v[GX_PS_R];
#pragma unroll
            for (int r = 0; r < GX_PS_R; r++) {
                const int64_t row = row0 + r * 64;
                v[r] = row < n ? ((const int64_t *)c.values)[row] : 0;
            }
#pragma unroll
            for (int r = 0; r < GX_PS_R; r++)
                if (!nl[r] && cmp_i64(v[r], cmp, S.pred_i64[p])) ok |= 1u << r;
            break; }
        case GX_I32: {
            int32_t v[GX_PS_R];
#pragma unroll
            for (int r = 0; r < GX_PS_R; r++) {
                const int64_t row = row0 + r * 64;
                v[r] = row < n ? ((const int32_t *)c.values)[row] : 0;
            }
#pragma unroll
            for (int r = 0; r < GX_PS_R; r++)
                if (!nl[r] && cmp_i64((int64_t)v[r], cmp, S.pred_i64[p]))
                    ok |= 1u << r;
            break; }
        default: {
            double v[GX_PS_R];
#pragma unroll
            for (int r = 0; r < GX_PS_R; r++) {
                const int64_t row = row0 + r * 64;
                v[r] = row < n ? ((const double *)c.values)[row] : 0.0;
            }
#pragma unroll
            for (int r = 0; r < GX_PS_R; r++)
                if (!nl[r] && cmp_f64(v[r], cmp, S.pred_f64[p])) ok |= 1u << r;
            break; }
        }
        pass &= ok;
    }
    return pass;
}

/* The three stages, shared by k_probe_scan and the group-join's
 * k_gj_probe_scan: they differ only in `flush`, what a full pair stage (and
 * the last, partial one) does with its (raw row, build position) pairs. */
template <class Flush>
__device__ static inline void probe_scan_body(const ProbeParams &P,
                                              const ScanPreds &S,
                                              uint32_t *kept,
                                              const Flush &flush) {
    __shared__ uint32_t s_pairs[2][4][GX_PS_STAGE]; /* [p/b][wave][slot] */
    __shared__ int64_t s_qkey[4][GX_PS_QCAP];       /* [wave][queue slot] */
    __shared__ uint32_t s_qrow[4][GX_PS_QCAP];
    const int wid = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    EmitStage E;
    E.s_p = s_pairs[0][wid];
    E.s_b = s_pairs[1][wid];
    E.cnt = 0;
    E.lane = lane;
    int64_t *qkey = s_qkey[wid];
    uint32_t *qrow = s_qrow[wid];
    uint32_t qcnt = 0;   /* wave-uniform */
    uint32_t n_kept = 0; /* wave-uniform */

    const int64_t n = P.n_probe;
    const DevColView &kc = P.probe_keys.col[0];
    const int64_t *keys = (const int64_t *)kc.values;
    const uint64_t *bloom = (const uint64_t *)P.bloom;
    /* SLICE CONTAINS does not suit the column-wise form: per row instead */
    bool wide = true;
    for (int p = 0; p < S.n_preds; p++)
        if (S.pred_view[p].type == GX_SLICE) wide = false;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;

    const int64_t stride = (int64_t)gridDim.x * GX_PS_BLOCK_ROWS;
    for (int64_t tile = blockIdx.x * (int64_t)GX_PS_BLOCK_ROWS +
                        (int64_t)wid * GX_PS_TILE;
         tile < n; tile += stride) { /* wave-uniform trip count */
        const int64_t row0 = tile + lane;

        /* 1. stream: keys (and their null bytes), then the predicates */
        int64_t key[GX_PS_R];
        uint32_t pass = 0, knull = 0;
#pragma unroll
        for (int r = 0; r < GX_PS_R; r++) {
            const int64_t row = row0 + r * 64;
            const bool in = row < n;
            key[r] = in ? keys[row] : 0;
            if (in) pass |= 1u << r;
            if (kc.has_nulls && in && kc.nulls[row]) knull |= 1u << r;
        }
        if (wide) {
            pass = scan_rows_pass_wide(S, row0, n, pass);
        } else {
#pragma unroll
            for (int r = 0; r < GX_PS_R; r++)
                if (((pass >> r) & 1u) && !scan_row_passes(S, row0 + r * 64))
                    pass &= ~(1u << r);
        }
#pragma unroll
        for (int r = 0; r < GX_PS_R; r++)
            n_kept += (uint32_t)__popcll(__ballot((pass >> r) & 1u));

        /* bloom words of the live rows, all loads before the first test */
        uint32_t live = pass & ~knull; /* a NULL key matches nothing */
        if (bloom) {
            uint64_t word[GX_PS_R], bits[GX_PS_R];
#pragma unroll
            for (int r = 0; r < GX_PS_R; r++) {
                const uint64_t x = bloom_mix(key[r]);
                bits[r] = bloom_bits(x, P.bloom_k);
                word[r] = ((live >> r) & 1u)
                    ? bloom[bloom_word(x, P.bloom_mask)] : 0ull;
            }
#pragma unroll
            for (int r = 0; r < GX_PS_R; r++)
                if ((word[r] & bits[r]) != bits[r]) live &= ~(1u << r);
        }

        /* 2. compact the live rows into the wave's queue (slots qcnt..) */
#pragma unroll
        for (int r = 0; r < GX_PS_R; r++) {
            const bool want = (live >> r) & 1u;
            const unsigned long long m = __ballot(want);
            if (want) {
                const uint32_t at = qcnt + (uint32_t)__popcll(m & lt_mask);
                qkey[at] = key[r];
                qrow[at] = (uint32_t)(row0 + r * 64);
            }
            qcnt += (uint32_t)__popcll(m);
        }

        /* 3. dense walk: pop 64 from the tail while a full wave's worth is
         * queued; at most 63 entries carry over, so qcnt never passes
         * 63 + 64*R < GX_PS_QCAP */
        while (qcnt >= 64) {
            qcnt -= 64;
            probe_key<GX_PS_STAGE>(P, E, true, qrow[qcnt + lane],
                                   qkey[qcnt + lane], flush);
        }
    }
    /* remainder */
    if (qcnt) {
        const bool active = (uint32_t)lane < qcnt;
        probe_key<GX_PS_STAGE>(P, E, active, active ? qrow[lane] : 0u,
                               active ? qkey[lane] : 0, flush);
    }
    flush(P, E);
    if (lane == 0 && n_kept) atomicAdd(kept, n_kept);
}

__global__ void __launch_bounds__(256)
k_probe_scan(ProbeParams P, ScanPreds S, uint32_t *kept) {
    probe_scan_body(P, S, kept, PairListFlush());
}

/* ---- group-join probe-scan (gxop_groupjoin_probe_scan fast path) -------
 * The same stream / compact / walk, but a full pair stage is ACCUMULATED,
 * not written out: each lane takes one staged (raw row, build position),
 * evaluates the aggregate-input projections at the raw row and applies them
 * to records[position]. The group of a matched row IS its build position,
 * so no pair list, no projected intermediate and no second hash table ever
 * reach HBM, and every lane is busy during the random record RMWs just as
 * the dense walk keeps every lane busy during the bucket fetch.
 *
 * The per-aggregate projection views are too large for the kernel-argument
 * segment next to ProbeParams and ScanPreds (together past 4 KB), so they
 * travel in a small device buffer read through wave-uniform loads. */
struct GJAccum {
    AggRecDesc R;                   /* first: the buffer's leading bytes */
    int32_t op[GX_MAX_COLS];        /* the input's projection (unused for
                                       COUNT(*)) */
    DevColView a[GX_MAX_COLS];
    DevColView b[GX_MAX_COLS];
    DevColView c[GX_MAX_COLS];
    DevColView d[GX_MAX_COLS];
    unsigned long long *records;
    uint32_t *used;                 /* NULL: the op reads "matched" from its
                                       COUNT(*) word (GroupJoinOp::count_off) */
    unsigned long long *matches;    /* cumulative (row, position) matches */
    /* transposed accumulate (agg_add_transposed): the lane-group width, 0
     * where the record is too wide or an aggregate is not additive, and
     * the slots that take f64 adds */
    int32_t t_width;
    uint32_t t_f64;
};

struct AccumFlush {
    const GJAccum *A;
    __device__ inline void operator()(const ProbeParams &,
                                      EmitStage &E) const {
        if (E.cnt == 0) return;
        const GJAccum &G = *A;
        if (G.t_width) {
            /* 64 staged pairs at a time, one per lane: every raw-column
             * load (and the used word's) goes out before the first atomic,
             * then the wave turns round so that a record's slots leave in
             * adjacent lanes of one instruction */
            for (uint32_t i0 = 0; i0 < E.cnt; i0 += 64) { /* wave-uniform */
                const uint32_t i = i0 + (uint32_t)E.lane;
                const bool active = i < E.cnt;
                const int64_t row = active ? (int64_t)E.s_p[i] : 0;
                const uint32_t pos = active ? E.s_b[i] : 0u;
                const uint32_t w = 1u << (pos & 31);
                uint32_t seen_w = w;
                if (G.used && active) seen_w = G.used[pos >> 5];
                AggSlotOps o;
                agg_slot_ops_clear(o);
#pragma unroll
                for (int a = 0; a < GX_AGG_T_SLOTS; a++) {
                    if (a >= G.R.n_aggs || !active) continue;
                    AggVal v;
                    v.bits = 0;
                    v.hi = 0;
                    v.type = GX_I64;
                    v.isnull = false;
                    if (G.R.func[a] != GX_AGG_COUNT_ROW)
                        v = proj_value(G.op[a], G.a[a], G.b[a], G.c[a],
                                       G.d[a], row);
                    agg_slot_ops_put(o, G.R.func[a], G.R.val_off[a],
                                     G.R.seen_off[a], v);
                }
                if ((seen_w & w) == 0) atomicOr(&G.used[pos >> 5], w);
                agg_add_transposed(G.records, G.R.stride, G.t_width, G.t_f64,
                                   pos, o, E.lane);
            }
            if (E.lane == 0) atomicAdd(G.matches, (unsigned long long)E.cnt);
            E.cnt = 0;
            return;
        }
        for (uint32_t i = (uint32_t)E.lane; i < E.cnt; i += 64) {
            const int64_t row = E.s_p[i];
            const uint32_t pos = E.s_b[i];
            const uint32_t w = 1u << (pos & 31);
            /* test-then-set: one RMW */
            if (G.used && (G.used[pos >> 5] & w) == 0)
                atomicOr(&G.used[pos >> 5], w);
            unsigned long long *rec = G.records + (size_t)pos * G.R.stride;
            for (int a = 0; a < G.R.n_aggs; a++) {
                AggVal v;
                v.bits = 0;
                v.hi = 0;
                v.type = GX_I64;
                v.isnull = false;
                if (G.R.func[a] != GX_AGG_COUNT_ROW)
                    v = proj_value(G.op[a], G.a[a], G.b[a], G.c[a], G.d[a],
                                   row);
                agg_rmw(G.R.func[a], rec, G.R.val_off[a], G.R.seen_off[a],
                        v);
            }
        }
        if (E.lane == 0) atomicAdd(G.matches, (unsigned long long)E.cnt);
        E.cnt = 0;
    }
};

__global__ void __launch_bounds__(256)
k_gj_probe_scan(ProbeParams P, ScanPreds S, uint32_t *kept,
                const GJAccum *A) {
    AccumFlush flush;
    flush.A = A;
    probe_scan_body(P, S, kept, flush);
}

/* Materialize the fused probe's pair list: probe-side output columns are
 * the scan's projections evaluated at the raw row id (side 0), build-side
 * columns are plain gathers at the build position (side 1, a COPY). */
struct ProjGatherParams {
    const uint32_t *pidx;
    const uint32_t *bidx;
    int64_t n;
    int32_t n_cols;
    int32_t side[GX_MAX_COLS];
    int32_t op[GX_MAX_COLS];
    int32_t scale[GX_MAX_COLS];
    DevColView a[GX_MAX_COLS];
    DevColView b[GX_MAX_COLS];
    DevColView c[GX_MAX_COLS];
    DevColView d[GX_MAX_COLS];
    void *out_vals[GX_MAX_COLS];
    uint8_t *out_nulls[GX_MAX_COLS];
};

__global__ void k_gather_proj(ProjGatherParams G) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < G.n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t pi = G.pidx[i];
        const int64_t bi = G.bidx[i];
        for (int c = 0; c < G.n_cols; c++)
            proj_store(G.op[c], G.scale[c], G.a[c], G.b[c], G.c[c], G.d[c],
                       G.side[c] ? bi : pi, G.out_vals[c], G.out_nulls[c], i,
                       nullptr);
    }
}

/* ---- gather + insert (gxop_groupjoin_build_probe_scan fast path) -------
 * k_gather_proj and k_join_insert in one pass over the fused probe's pair
 * list: pair i evaluates every consumed column (register-sized: proj_value)
 * at its raw row / build position, all loads issued before anything else,
 * writes the values to row i of the group-join's build store (adjacent
 * lanes, adjacent rows) and inserts (key, i) from the register. The random
 * loads then ride beside the insert's atomics, which set the pace. The
 * column loops are unrolled over GX_JIP_MAX_COLS so the values stay in
 * registers; wider schemas take the composed path. */
#define GX_JIP_MAX_COLS 8

__global__ void __launch_bounds__(256)
k_join_insert_proj(JoinInsertParams P, ProjGatherParams G, int32_t key_col) {
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    /* wave-uniform trip count: the spill append ballots across the wave */
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;;
         i += stride) {
        const bool live = i < P.n;
        if (!__ballot(live)) break;
        unsigned long long val[GX_JIP_MAX_COLS];
        uint32_t nullm = 0;
        int64_t key = 0;
        if (live) {
            const int64_t pi = G.pidx[i];
            const int64_t bi = G.bidx[i];
#pragma unroll
            for (int c = 0; c < GX_JIP_MAX_COLS; c++) {
                val[c] = 0;
                if (c < G.n_cols) {
                    const AggVal v = proj_value(G.op[c], G.a[c], G.b[c],
                                                G.c[c], G.d[c],
                                                G.side[c] ? bi : pi);
                    val[c] = v.bits;
                    if (v.isnull) nullm |= 1u << c;
                }
            }
#pragma unroll
            for (int c = 0; c < GX_JIP_MAX_COLS; c++) {
                if (c < G.n_cols) {
                    if (G.out_nulls[c])
                        G.out_nulls[c][i] = (uint8_t)((nullm >> c) & 1u);
                    /* as proj_store: an I32 COPY stores 4 B, all else 8 B */
                    if (G.op[c] == GX_PROJ_COPY && G.a[c].type == GX_I32)
                        ((int32_t *)G.out_vals[c])[i] = (int32_t)val[c];
                    else
                        ((unsigned long long *)G.out_vals[c])[i] = val[c];
                    if (c == key_col) key = (int64_t)val[c];
                }
            }
        }
        /* the key column is null-free (a fast-path condition): every live
         * row is inserted */
        const uint32_t b = (uint32_t)gx_mix(gx_hash_i64(key)) & P.mask;
        join_insert_row(P, live, key, b, i, lane);
    }
}

__global__ void k_scan(ScanParams P) {
    /* per-wave LDS staging of surviving row indices, then each flush
     * writes the projected columns coalesced (same batching rationale as
     * the probe's emit stage) */
    __shared__ uint32_t s_rows[4][GX_EMIT_STAGE];
    const int wid = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    uint32_t *stage = s_rows[wid];
    uint32_t cnt = 0;

    auto flush = [&]() {
        if (cnt == 0) return;
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(P.counter, cnt);
        base = (uint32_t)__shfl((int)base, 0, 64);
        for (uint32_t k = (uint32_t)lane; k < cnt; k += 64) {
            uint32_t at = base + k;
            if (at >= P.cap) continue;
            int64_t src = stage[k];
            if (P.out_rowids) P.out_rowids[at] = (uint32_t)src;
            for (int c = 0; c < P.n_projs; c++)
                proj_store(P.proj_op[c], P.proj_scale[c], P.proj_a[c],
                           P.proj_b[c], P.proj_c[c], P.proj_d[c], src,
                           P.out_vals[c], P.out_nulls[c], at, P.err);
        }
        cnt = 0;
    };

    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t base_i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;;
         base_i += stride) {
        bool active = base_i < P.n;
        if (!__ballot(active)) break;
        bool want = active && scan_row_passes(P.preds, base_i);
        unsigned long long m = __ballot(want);
        uint32_t add = (uint32_t)__popcll(m);
        if (cnt + add > GX_EMIT_STAGE) flush();
        if (want)
            stage[cnt + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] =
                (uint32_t)base_i;
        cnt += add;
    }
    flush();
}

struct ScanOp : gx_op {
    gx_scan_cfg cfg;
    std::vector<gx_pred> preds;
    std::vector<gx_proj> projs;
    std::vector<int32_t> input_types, out_types;
    /* last-allocated first (see DevBuf: destruction order and the pool) */
    std::vector<DevBuf> d_pats;
    DevBuf d_scan_tmp, d_rowids, d_meta;
    bool has_slice_out = false;

    ScanOp(const gx_scan_cfg *c) : gx_op(OP_SCAN, c->device, c->stream), cfg(*c) {
        preds.assign(c->preds, c->preds + c->n_preds);
        projs.assign(c->projs, c->projs + c->n_projs);
        input_types.assign(c->input_types, c->input_types + c->n_input_cols);
        for (auto &p : projs) {
            switch (p.op) {
            case GX_PROJ_COPY: out_types.push_back(input_types[p.a]); break;
            case GX_PROJ_REV_F64: out_types.push_back(GX_F64); break;
            case GX_PROJ_SCALED_TO_DEC: out_types.push_back(GX_DECIMAL); break;
            case GX_PROJ_Q1_CHARGE6: out_types.push_back(GX_I64); break;
            default: out_types.push_back(GX_I64); break;
            }
            if (out_types.back() == GX_SLICE) has_slice_out = true;
        }
    }

    int upload_patterns() {
        if (!d_pats.empty()) return 0;
        for (auto &p : preds) {
            d_pats.emplace_back();
            if (p.cmp == GX_CMP_CONTAINS && p.v_bytes && p.v_len > 0) {
                DevBuf &b = d_pats.back();
                if (b.grow((size_t)p.v_len, stream)) return -1;
                HIP_OK(hipMemcpyAsync(b.p, p.v_bytes, (size_t)p.v_len,
                                      hipMemcpyHostToDevice, stream));
            }
        }
        return 0;
    }

    /* predicate constants + the staged chunk's predicate columns */
    int fill_preds(ScanPreds &S, const StagedChunk &st) {
        std::memset(&S, 0, sizeof(S));
        if (upload_patterns()) return -1;
        S.n_preds = (int32_t)preds.size();
        for (size_t p = 0; p < preds.size(); p++) {
            S.pred_cmp[p] = preds[p].cmp;
            S.pred_i64[p] = preds[p].v_i64;
            S.pred_f64[p] = preds[p].v_f64;
            S.pred_pat[p] = (const uint8_t *)d_pats[p].p;
            S.pred_plen[p] = preds[p].v_len;
            S.pred_view[p] = st.views[preds[p].col];
        }
        return 0;
    }

    /* projection p's output is null-free when none of the raw columns it
     * reads carries nulls (SLICE outputs keep their nulls: the slice
     * gather writes them) */
    bool proj_null_free(size_t p, const StagedChunk &st) const {
        const gx_proj &pr = projs[p];
        if (out_types[p] == GX_SLICE) return false;
        bool nf = !st.views[pr.a].has_nulls;
        if (pr.op == GX_PROJ_REV_F64 || pr.op == GX_PROJ_REV_SCALED4 ||
            pr.op == GX_PROJ_Q9_AMOUNT4 || pr.op == GX_PROJ_Q1_CHARGE6)
            nf = nf && !st.views[pr.b].has_nulls;
        if (pr.op == GX_PROJ_Q9_AMOUNT4 || pr.op == GX_PROJ_Q1_CHARGE6)
            nf = nf && !st.views[pr.c].has_nulls;
        if (pr.op == GX_PROJ_Q9_AMOUNT4)
            nf = nf && !st.views[pr.d].has_nulls;
        return nf;
    }

    int consume(const gx_chunk *ch, gx_result **out) {
        *out = nullptr;
        if (ensure_device(device)) return -1;
        const int64_t n = ch->n_rows;
        StagedChunk st;
        if (st.stage(ch, stream)) return -1;
        if (d_meta.grow(8, stream)) return -1;
        /* pass 1 would count; instead allocate full-capacity output and
         * shrink by the counter (filters keep a bounded fraction and
         * the buffers come from the pool) */
        std::vector<uint8_t> null_free;
        for (size_t c = 0; c < projs.size(); c++)
            null_free.push_back(proj_null_free(c, st));
        auto h = alloc_result_cols(out_types, n, device, stream, &null_free);
        if (!h) return -1;
        HIP_OK(hipMemsetAsync(d_meta.p, 0, 8, stream));
        ScanParams P;
        std::memset(&P, 0, sizeof(P));
        P.n = n;
        if (fill_preds(P.preds, st)) return -1;
        P.n_projs = (int32_t)projs.size();
        for (size_t c = 0; c < projs.size(); c++) {
            P.proj_op[c] = projs[c].op;
            P.proj_a[c] = st.views[projs[c].a];
            if (projs[c].op == GX_PROJ_DEC_TO_SCALED ||
                projs[c].op == GX_PROJ_SCALED_TO_DEC)
                P.proj_scale[c] = projs[c].c;   /* c = scale, not a col */
            else if (projs[c].op != GX_PROJ_COPY)
                P.proj_b[c] = st.views[projs[c].b];
            if (projs[c].op == GX_PROJ_Q9_AMOUNT4) {
                P.proj_c[c] = st.views[projs[c].c];
                P.proj_d[c] = st.views[projs[c].d];
            }
            if (projs[c].op == GX_PROJ_Q1_CHARGE6)
                P.proj_c[c] = st.views[projs[c].c];
            P.out_vals[c] = h->bufs[c * 2].p;
            P.out_nulls[c] = (uint8_t *)h->bufs[c * 2 + 1].p;
        }
        P.cap = (uint32_t)n;
        P.counter = (uint32_t *)d_meta.p;
        P.err = (uint32_t *)d_meta.p + 1;
        P.out_rowids = nullptr;
        if (has_slice_out) {
            if (d_rowids.grow((size_t)std::max<int64_t>(n, 1) * 4, stream))
                return -1;
            P.out_rowids = (uint32_t *)d_rowids.p;
        }
        if (n > 0)
            hipLaunchKernelGGL(k_scan, dim3(gx_grid(n)), dim3(256), 0,
                               stream, P);
        uint32_t meta[2] = {0, 0};
        if (n > 0) {
            HIP_OK(hipMemcpyAsync(meta, d_meta.p, 8,
                                  hipMemcpyDeviceToHost, stream));
            HIP_OK(hipStreamSynchronize(stream));
        }
        if (meta[1]) {
            gx_set_err("wide DECIMAL: value exceeds 18 significant "
                       "digits / the DecimalBox simple layout; the "
                       "scaled-int64 fast path cannot represent it "
                       "(reference falls back to full Decimal "
                       "arithmetic, DecimalBox.java:43-71)");
            return -1;
        }
        uint32_t kept = meta[0];
        h->res.chunk.n_rows = (int32_t)kept;
        for (size_t c = 0; c < projs.size(); c++) {
            if (out_types[c] != GX_SLICE) continue;
            if (gather_slice_col(st.views[projs[c].a],
                                 (const uint32_t *)d_rowids.p, 0, kept,
                                 h.get(), c, d_scan_tmp, stream))
                return -1;
        }
        give_result(std::move(h), out);
        return 0;
    }
};

/* ---- fused scan + probe (gxop_join_probe_scan) ------------------------ */

/* The fast path's conditions (gxop.h): fast_i64 inline-bucket table, plain
 * INNER/SEMI equi-join, probe key = COPY of a raw I64 column, no SLICE
 * anywhere on the output, no DEC_TO_SCALED projection (its wide-DECIMAL
 * fence must fire for every surviving row; late evaluation would only see
 * the matched ones), device-resident input. Anything else runs the
 * composed scan -> probe sequence. */
bool probe_scan_fast_ok(const JoinOp *j, const ScanOp *s,
                        const gx_chunk *raw) {
    if (!j->built || !j->fast_i64 || j->pass_nothing || j->pass_through)
        return false;
    const gx_join_cfg &c = j->cfg;
    if (c.build_outer || c.single_join || !j->conds.empty()) return false;
    if (c.join_type != GX_JOIN_INNER && c.join_type != GX_JOIN_SEMI)
        return false;
    if (raw->n_rows <= 0 || raw->n_blocks != (int32_t)s->input_types.size())
        return false;
    for (int32_t b = 0; b < raw->n_blocks; b++)
        if (raw->blocks[b].mem != GX_MEM_DEVICE) return false;
    const gx_proj &kp = s->projs[(size_t)j->probe_key_cols[0]];
    if (kp.op != GX_PROJ_COPY || s->input_types[kp.a] != GX_I64) return false;
    /* Q1_CHARGE6: the fused gather's operand wiring knows the expressions
     * it was built for; a scan with this one runs the composed sequence
     * (so does gxop_groupjoin_build_probe_scan, which asks here first) */
    for (size_t p = 0; p < s->projs.size(); p++)
        if (s->projs[p].op == GX_PROJ_DEC_TO_SCALED ||
            s->projs[p].op == GX_PROJ_Q1_CHARGE6 ||
            s->out_types[p] == GX_SLICE)
            return false;
    std::vector<JoinOp::OutSpec> specs = j->projected_specs();
    if (specs.size() > GX_MAX_COLS) return false;
    for (auto &sp : specs)
        if (sp.type == GX_SLICE) return false;
    return true;
}

/* Stage 1 of the fused probe: k_probe_scan over the staged raw chunk. On
 * return the (raw row, build position) pairs of the *n_out matches sit in
 * j->d_pidx / j->d_bpos (until the op's next probe), *n_kept holds the rows
 * that passed the predicates, the join's stats are advanced and the stream
 * is drained. */
int probe_scan_pairs(JoinOp *j, ScanOp *s, const StagedChunk &st,
                     int64_t *n_out, int64_t *n_kept) {
    hipStream_t stream = j->stream;
    const int64_t n = st.n_rows;
    ScanPreds S;
    if (s->fill_preds(S, st)) return -1;
    const gx_proj &kp = s->projs[(size_t)j->probe_key_cols[0]];

    /* first attempt sized like gxop_join_probe's, on the raw row count */
    uint32_t cap = (uint32_t)std::min<int64_t>(
        std::max<int64_t>((int64_t)n * 2, 1 << 16), INT64_C(1) << 31);
    if (j->d_meta.grow(16, stream)) return -1;
    for (int attempt = 0; attempt < 4; attempt++) {
        if (j->d_pidx.grow((size_t)cap * 4, stream) ||
            j->d_bpos.grow((size_t)cap * 4, stream)) return -1;
        HIP_OK(hipMemsetAsync(j->d_meta.p, 0, 16, stream));
        ProbeParams P;
        std::memset(&P, 0, sizeof(P));
        P.table = (const JoinEntry *)j->d_table.p;
        P.entries = (const JoinEntry *)j->d_entries.p;
        P.mask = j->mask;
        P.n_probe = n;
        P.bloom = (const uint32_t *)j->d_bloom.p;
        P.bloom_mask = j->bloom_mask;
        P.bloom_k = j->bloom_k;
        P.fast_i64 = 1;
        P.build_keys = j->key_views(j->build, j->build_key_cols);
        P.probe_keys.n = 1;
        P.probe_keys.col[0] = st.views[kp.a];
        P.join_type = j->cfg.join_type;
        P.semi_join = j->cfg.join_type == GX_JOIN_SEMI;
        P.anti_null_col = -1;
        P.out_probe = (uint32_t *)j->d_pidx.p;
        P.out_build = (uint32_t *)j->d_bpos.p;
        P.cap = cap;
        P.counter = (uint32_t *)j->d_meta.p;
        P.err = (uint32_t *)j->d_meta.p + 1;
        if (!j->ev0) {
            HIP_OK(hipEventCreate(&j->ev0));
            HIP_OK(hipEventCreate(&j->ev1));
        }
        HIP_OK(hipEventRecord(j->ev0, stream));
        hipLaunchKernelGGL(k_probe_scan, dim3(gx_ps_grid(n)), dim3(256), 0,
                           stream, P, S, (uint32_t *)j->d_meta.p + 2);
        HIP_OK(hipEventRecord(j->ev1, stream));
        uint32_t meta[3];
        HIP_OK(hipMemcpyAsync(meta, j->d_meta.p, 12, hipMemcpyDeviceToHost,
                              stream));
        HIP_OK(hipStreamSynchronize(stream));
        {
            float ms = 0;
            HIP_OK(hipEventElapsedTime(&ms, j->ev0, j->ev1));
            j->probe_kernel_ms += ms;
            j->probe_launches++;
        }
        if (meta[0] > cap) { cap = meta[0]; continue; } /* exact-size retry */

        *n_out = meta[0];
        j->probe_rows_total += meta[2];
        j->matches_total += meta[0];
        *n_kept = meta[2];
        return 0;
    }
    gx_set_err("probe_scan: pair list still short after 4 resizes");
    return -1;
}

/* the source half of ProjGatherParams for the fused probe's pair list: per
 * output column of `specs`, the scan projection it evaluates at the raw row
 * or the build column it gathers (G zeroed by the caller; out_vals /
 * out_nulls are the caller's) */
void fill_proj_gather(ProjGatherParams &G, const JoinOp *j, const ScanOp *s,
                      const StagedChunk &st,
                      const std::vector<JoinOp::OutSpec> &specs,
                      int64_t n_out) {
    G.pidx = (const uint32_t *)j->d_pidx.p;
    G.bidx = (const uint32_t *)j->d_bpos.p;
    G.n = n_out;
    G.n_cols = (int32_t)specs.size();
    for (size_t c = 0; c < specs.size(); c++) {
        if (!specs[c].outer) { /* build side: plain gather */
            G.side[c] = 1;
            G.op[c] = GX_PROJ_COPY;
            G.a[c] = j->build.view(specs[c].src);
            continue;
        }
        const gx_proj &pr = s->projs[(size_t)specs[c].src];
        G.side[c] = 0;
        G.op[c] = pr.op;
        G.a[c] = st.views[pr.a];
        if (pr.op == GX_PROJ_SCALED_TO_DEC)
            G.scale[c] = pr.c;   /* c = scale, not a col */
        else if (pr.op != GX_PROJ_COPY)
            G.b[c] = st.views[pr.b];
        if (pr.op == GX_PROJ_Q9_AMOUNT4) {
            G.c[c] = st.views[pr.c];
            G.d[c] = st.views[pr.d];
        }
    }
}

/* is output column `sp` of the fused probe null-free? (as in the scan and
 * the join) */
bool probe_scan_col_null_free(const JoinOp *j, const ScanOp *s,
                              const StagedChunk &st,
                              const JoinOp::OutSpec &sp) {
    return sp.outer ? s->proj_null_free((size_t)sp.src, st)
                    : !j->build.view(sp.src).has_nulls;
}

int probe_scan_fused(JoinOp *j, ScanOp *s, const gx_chunk *raw,
                     gx_result **out, int64_t *n_kept) {
    if (ensure_device(j->device)) return -1;
    hipStream_t stream = j->stream;
    StagedChunk st;
    if (st.stage(raw, stream)) return -1; /* device-resident: zero copy */
    int64_t n_out = 0;
    if (probe_scan_pairs(j, s, st, &n_out, n_kept)) return -1;

    std::vector<JoinOp::OutSpec> specs = j->projected_specs();
    std::vector<int32_t> otypes;
    std::vector<uint8_t> null_free;
    for (auto &sp : specs) {
        otypes.push_back(sp.type);
        null_free.push_back(probe_scan_col_null_free(j, s, st, sp));
    }
    auto h = alloc_result_cols(otypes, n_out, j->device, stream, &null_free);
    if (!h) return -1;
    if (n_out > 0) {
        ProjGatherParams G;
        std::memset(&G, 0, sizeof(G));
        fill_proj_gather(G, j, s, st, specs, n_out);
        for (size_t c = 0; c < specs.size(); c++) {
            G.out_vals[c] = h->bufs[c * 2].p;
            G.out_nulls[c] = (uint8_t *)h->bufs[c * 2 + 1].p;
        }
        hipLaunchKernelGGL(k_gather_proj, dim3(gx_grid(n_out)), dim3(256),
                           0, stream, G);
        /* the pair lists are reused by the next probe: drain first */
        HIP_OK(hipStreamSynchronize(stream));
    }
    give_result(std::move(h), out);
    return 0;
}

/* ---- fused scan + group-join probe (gxop_groupjoin_probe_scan) -------- */

/* The fast path's conditions (gxop_hip.h): the op built the inline-bucket
 * table (one I64 key, no NULL in the consumed key column), the key is a
 * COPY of a raw I64 column, every aggregate input is a register-sized
 * projection (proj_value), no DEC_TO_SCALED projection anywhere (its
 * wide-DECIMAL fence must see every surviving row), device-resident input
 * of fewer than 2^31 rows. */
bool gj_probe_scan_fast_ok(const GroupJoinOp *g, const ScanOp *s,
                           const gx_chunk *raw) {
    if (!g->inline_tab || g->jop->pass_nothing) return false;
    if (raw->n_rows <= 0 || (int64_t)raw->n_rows >= (INT64_C(1) << 31) ||
        raw->n_blocks != (int32_t)s->input_types.size())
        return false;
    for (int32_t b = 0; b < raw->n_blocks; b++)
        if (raw->blocks[b].mem != GX_MEM_DEVICE) return false;
    const gx_proj &kp = s->projs[(size_t)g->jop->probe_key_cols[0]];
    if (kp.op != GX_PROJ_COPY || s->input_types[kp.a] != GX_I64) return false;
    for (auto &pr : s->projs)
        if (pr.op == GX_PROJ_DEC_TO_SCALED || pr.op == GX_PROJ_Q1_CHARGE6)
            return false; /* Q1_CHARGE6: as in probe_scan_fast_ok */
    for (auto &sp : g->aggs) {
        if (sp.input_col < 0) continue;
        const gx_proj &pr = s->projs[(size_t)sp.input_col];
        const int32_t t = s->out_types[(size_t)sp.input_col];
        switch (pr.op) {
        case GX_PROJ_COPY:
            if (t != GX_I64 && t != GX_I32 && t != GX_F64) return false;
            break;
        case GX_PROJ_REV_F64: case GX_PROJ_REV_SCALED4:
        case GX_PROJ_Q9_AMOUNT4:
            break;
        default:
            return false;
        }
    }
    return true;
}

int gj_probe_scan_fused(GroupJoinOp *g, ScanOp *s, const gx_chunk *raw,
                        int64_t *n_kept) {
    if (ensure_device(g->device)) return -1;
    hipStream_t stream = g->stream;
    JoinOp *j = g->jop.get();
    StagedChunk st;
    if (st.stage(raw, stream)) return -1; /* device-resident: zero copy */
    const int64_t n = st.n_rows;
    ScanPreds S;
    if (s->fill_preds(S, st)) return -1;
    const gx_proj &kp = s->projs[(size_t)j->probe_key_cols[0]];

    ProbeParams P;
    std::memset(&P, 0, sizeof(P));
    P.table = (const JoinEntry *)j->d_table.p;
    P.entries = (const JoinEntry *)j->d_entries.p;
    P.mask = j->mask;
    P.n_probe = n;
    P.bloom = (const uint32_t *)j->d_bloom.p;
    P.bloom_mask = j->bloom_mask;
    P.bloom_k = j->bloom_k;
    P.fast_i64 = 1;
    P.probe_keys.n = 1;
    P.probe_keys.col[0] = st.views[kp.a];
    P.join_type = GX_JOIN_INNER; /* every match is a pair; LEFT only
                                    changes the emission */
    P.anti_null_col = -1;

    GJAccum A;
    std::memset(&A, 0, sizeof(A));
    A.R = g->layout.desc;
    for (size_t a = 0; a < g->aggs.size(); a++) {
        if (g->aggs[a].input_col < 0) continue;
        const gx_proj &pr = s->projs[(size_t)g->aggs[a].input_col];
        A.op[a] = pr.op;
        A.a[a] = st.views[pr.a];
        if (pr.op != GX_PROJ_COPY) A.b[a] = st.views[pr.b];
        if (pr.op == GX_PROJ_Q9_AMOUNT4) {
            A.c[a] = st.views[pr.c];
            A.d[a] = st.views[pr.d];
        }
    }
    bool additive = A.R.stride <= GX_AGG_T_SLOTS;
    for (size_t a = 0; a < g->aggs.size(); a++)
        additive = additive && agg_func_additive(g->aggs[a].func);
    if (additive) {
        A.t_width = A.R.stride <= 1 ? 1 : A.R.stride == 2 ? 2 : 4;
        for (size_t a = 0; a < g->aggs.size(); a++)
            if (agg_func_adds_f64(g->aggs[a].func))
                A.t_f64 |= 1u << A.R.val_off[a];
    }
    A.records = (unsigned long long *)g->d_records.p;
    A.used = g->count_off >= 0 ? nullptr : (uint32_t *)g->d_used.p;
    A.matches = (unsigned long long *)g->d_meta.p;
    if (g->d_accum.grow(sizeof(A), stream)) return -1;
    /* `A` outlives the copy: finish_probe drains the stream below */
    HIP_OK(hipMemcpyAsync(g->d_accum.p, &A, sizeof(A), hipMemcpyHostToDevice,
                          stream));
    HIP_OK(hipMemsetAsync((char *)g->d_meta.p + 8, 0, 4, stream));
    if (!g->ev0) {
        HIP_OK(hipEventCreate(&g->ev0));
        HIP_OK(hipEventCreate(&g->ev1));
    }
    HIP_OK(hipEventRecord(g->ev0, stream));
    hipLaunchKernelGGL(k_gj_probe_scan, dim3(gx_ps_grid(n)), dim3(256), 0,
                       stream, P, S, (uint32_t *)g->d_meta.p + 2,
                       (const GJAccum *)g->d_accum.p);
    HIP_OK(hipEventRecord(g->ev1, stream));
    if (g->finish_probe(n_kept)) return -1;
    g->rows_total += *n_kept;
    return 0;
}

/* ---- join1's matches straight into the group-join's build
 *      (gxop_groupjoin_build_probe_scan) -------------------------------- */

/* The fast path's conditions that can be told before the probe (gxop_hip.h):
 * the producer join's own fused fast path, a group-join that has consumed
 * nothing and would build the inline-bucket table, a null-free key
 * projection, register-sized consumed columns only (at most
 * GX_JIP_MAX_COLS), one device and stream. GX_GJ_BUILD_FUSED=0, read per
 * call, turns it off. */
bool gj_build_probe_scan_fast_ok(const GroupJoinOp *g, const JoinOp *j,
                                 const ScanOp *s, const gx_chunk *raw,
                                 const StagedChunk &st) {
    const char *e = getenv("GX_GJ_BUILD_FUSED");
    if (e && e[0] == '0') return false;
    if (!probe_scan_fast_ok(j, s, raw)) return false;
    if (g->built || g->jop->built || g->jop->build.n_rows != 0 ||
        !g->inline_ok)
        return false;
    if (g->device != j->device || g->stream != j->stream) return false;
    const std::vector<JoinOp::OutSpec> specs = j->projected_specs();
    if (specs.size() > GX_JIP_MAX_COLS) return false;
    for (size_t c = 0; c < specs.size(); c++) {
        const JoinOp::OutSpec &sp = specs[c];
        if (sp.type != GX_I64 && sp.type != GX_I32 && sp.type != GX_F64)
            return false;
        if (sp.outer && s->projs[(size_t)sp.src].op == GX_PROJ_SCALED_TO_DEC)
            return false;
    }
    /* the consumed key column must come out null-free, else do_build
     * would not choose the inline-bucket table */
    const int kc = g->jop->build_key_cols[0];
    return probe_scan_col_null_free(j, s, st, specs[(size_t)kc]);
}

/* Size the group-join's (empty) build store for exactly n rows whose
 * column c carries a nulls buffer unless null_free[c]: what appending the
 * composed sequence's result would leave, before any row is written. */
int gj_store_size_exact(DevStore &store, int64_t n,
                        const std::vector<uint8_t> &null_free) {
    if (store.reserve(n)) return -1;
    for (size_t c = 0; c < store.cols.size(); c++) {
        DevColumn &col = store.cols[c];
        col.has_nulls = !null_free[c];
        if (col.has_nulls && col.nulls.grow((size_t)n, store.stream))
            return -1;
    }
    store.n_rows = n;
    return 0;
}

int gj_build_probe_scan_fused(GroupJoinOp *g, JoinOp *j, ScanOp *s,
                              const StagedChunk &st, int64_t *n_kept,
                              int64_t *n_consumed) {
    hipStream_t stream = j->stream;
    int64_t n = 0;
    if (probe_scan_pairs(j, s, st, &n, n_kept)) return -1;
    *n_consumed = n;
    /* an empty consumed side builds as an empty consume would */
    if (n == 0) return g->do_build();

    const std::vector<JoinOp::OutSpec> specs = j->projected_specs();
    std::vector<uint8_t> null_free;
    for (auto &sp : specs)
        null_free.push_back(probe_scan_col_null_free(j, s, st, sp));
    DevStore &store = g->jop->build;
    if (gj_store_size_exact(store, n, null_free)) return -1;

    ProjGatherParams G;
    std::memset(&G, 0, sizeof(G));
    fill_proj_gather(G, j, s, st, specs, n);
    for (size_t c = 0; c < specs.size(); c++) {
        G.out_vals[c] = store.cols[c].values.p;
        G.out_nulls[c] = store.cols[c].has_nulls
            ? (uint8_t *)store.cols[c].nulls.p : nullptr;
    }
    const int32_t key_col = (int32_t)g->jop->build_key_cols[0];
    g->build_fused = true;
    /* sizes and zeroes table, spill list and bloom for n, launches the
     * insert through the lambda, then the spill passes, records, d_meta */
    return g->do_build_with([&](const JoinInsertParams &IP) {
        hipLaunchKernelGGL(k_join_insert_proj, dim3(gx_grid(IP.n)), dim3(256),
                           0, stream, IP, G, key_col);
    });
}

} // namespace

extern "C" {

int gxop_groupjoin_build_probe_scan(gx_op *groupjoin, gx_op *join,
                                    gx_op *scan, const gx_chunk *raw_chunk,
                                    int64_t *n_scan_kept,
                                    int64_t *n_consumed) {
    if (!groupjoin || groupjoin->kind != OP_GROUPJOIN) { gx_set_err("not a groupjoin op"); return -1; }
    if (!join || join->kind != OP_JOIN) { gx_set_err("not a join op"); return -1; }
    if (!scan || scan->kind != OP_SCAN) { gx_set_err("not a scan op"); return -1; }
    if (!raw_chunk) { gx_set_err("groupjoin_build_probe_scan: null argument"); return -1; }
    GroupJoinOp *g = static_cast<GroupJoinOp *>(groupjoin);
    ScanOp *s = static_cast<ScanOp *>(scan);
    JoinOp *j = join->variant == 0 ? static_cast<JoinOp *>(join) : nullptr;
    int64_t kept = 0, consumed = 0;
    {
        std::unique_lock<std::mutex> lj(join->mu, std::defer_lock);
        std::unique_lock<std::mutex> lg(groupjoin->mu, std::defer_lock);
        std::lock(lj, lg);
        if (g->built) { gx_set_err("groupjoin_build_probe_scan: already built"); return -1; }
        /* the fast path checks nothing the composed sequence would
         * reject: types and build state are tested the same way first */
        const bool shape_ok = j && j->built &&
            (j->cfg.build_outer ? j->inner_types : j->outer_types) ==
                s->out_types &&
            j->output_types() == g->build_types &&
            join->device == scan->device && join->stream == scan->stream;
        if (shape_ok) {
            if (ensure_device(j->device)) return -1;
            StagedChunk st; /* device-resident on the fast path: zero copy */
            bool fast = true;
            for (int32_t b = 0; b < raw_chunk->n_blocks && fast; b++)
                fast = raw_chunk->blocks[b].mem == GX_MEM_DEVICE;
            if (fast && st.stage(raw_chunk, j->stream)) return -1;
            if (fast && gj_build_probe_scan_fast_ok(g, j, s, raw_chunk, st)) {
                int rc = gj_build_probe_scan_fused(g, j, s, st, &kept,
                                                   &consumed);
                if (rc) return rc;
                if (n_scan_kept) *n_scan_kept = kept;
                if (n_consumed) *n_consumed = consumed;
                return 0;
            }
        }
    }
    /* composed sequence, each step under its own op's lock */
    gx_result *t = nullptr;
    int rc = gxop_join_probe_scan(join, scan, raw_chunk, &t, &kept);
    if (rc) return rc;
    if (t) {
        consumed = t->chunk.n_rows;
        rc = gxop_groupjoin_consume(groupjoin, &t->chunk);
        gxop_result_release(t);
        if (rc) return rc;
    }
    rc = gxop_groupjoin_build(groupjoin);
    if (rc) return rc;
    if (n_scan_kept) *n_scan_kept = kept;
    if (n_consumed) *n_consumed = consumed;
    return 0;
}

int gxop_groupjoin_build_was_fused(gx_op *groupjoin) {
    if (!groupjoin || groupjoin->kind != OP_GROUPJOIN) { gx_set_err("not a groupjoin op"); return -1; }
    return static_cast<GroupJoinOp *>(groupjoin)->build_fused ? 1 : 0;
}

int gxop_groupjoin_probe_scan(gx_op *groupjoin, gx_op *scan,
                              const gx_chunk *raw_chunk,
                              int64_t *n_scan_kept, int64_t *n_matched) {
    if (!groupjoin || groupjoin->kind != OP_GROUPJOIN) { gx_set_err("not a groupjoin op"); return -1; }
    if (!scan || scan->kind != OP_SCAN) { gx_set_err("not a scan op"); return -1; }
    if (!raw_chunk) { gx_set_err("groupjoin_probe_scan: null argument"); return -1; }
    if (groupjoin->device != scan->device || groupjoin->stream != scan->stream) {
        gx_set_err("groupjoin_probe_scan: group-join and scan must share "
                   "device and stream");
        return -1;
    }
    GroupJoinOp *g = static_cast<GroupJoinOp *>(groupjoin);
    ScanOp *s = static_cast<ScanOp *>(scan);
    std::lock_guard<std::mutex> lk(groupjoin->mu);
    if (g->probe_types != s->out_types) {
        gx_set_err("groupjoin_probe_scan: scan's projected types differ "
                   "from the group-join's probe_types");
        return -1;
    }
    if (!g->built) { gx_set_err("probe before build"); return -1; }
    const int64_t before = g->matches_total;
    int64_t kept = 0;
    int rc;
    if (gj_probe_scan_fast_ok(g, s, raw_chunk)) {
        rc = gj_probe_scan_fused(g, s, raw_chunk, &kept);
    } else {
        /* composed sequence: scan, then probe with its projected chunk */
        gx_result *t = nullptr;
        rc = s->consume(raw_chunk, &t);
        if (rc) return rc;
        kept = t->chunk.n_rows;
        rc = g->probe(&t->chunk);
        gxop_result_release(t);
    }
    if (rc) return rc;
    if (n_scan_kept) *n_scan_kept = kept;
    if (n_matched) *n_matched = g->matches_total - before;
    return 0;
}

int gxop_join_probe_scan(gx_op *join, gx_op *scan, const gx_chunk *raw_chunk,
                         gx_result **out, int64_t *n_scan_kept) {
    if (!join || join->kind != OP_JOIN) { gx_set_err("not a join op"); return -1; }
    if (!scan || scan->kind != OP_SCAN) { gx_set_err("not a scan op"); return -1; }
    if (!raw_chunk || !out) { gx_set_err("probe_scan: null argument"); return -1; }
    *out = nullptr;
    if (join->device != scan->device || join->stream != scan->stream) {
        gx_set_err("probe_scan: join and scan must share device and stream");
        return -1;
    }
    ScanOp *s = static_cast<ScanOp *>(scan);
    std::lock_guard<std::mutex> lk(join->mu);
    JoinOp *j = join->variant == 0 ? static_cast<JoinOp *>(join) : nullptr;
    HybridJoinOp *hj = j ? nullptr : static_cast<HybridJoinOp *>(join);
    const gx_join_cfg &cfg = j ? j->cfg : hj->cfg;
    const std::vector<int32_t> &pt = cfg.build_outer
        ? (j ? j->inner_types : hj->inner_types)
        : (j ? j->outer_types : hj->outer_types);
    if (pt != s->out_types) {
        gx_set_err("probe_scan: scan's projected types differ from the "
                   "join's probe-side types");
        return -1;
    }
    if (!(j ? j->built : hj->built)) { gx_set_err("probe before build"); return -1; }
    int64_t kept = 0;
    int rc;
    if (j && probe_scan_fast_ok(j, s, raw_chunk)) {
        rc = probe_scan_fused(j, s, raw_chunk, out, &kept);
    } else {
        /* composed sequence: scan, then probe with its projected chunk */
        gx_result *t = nullptr;
        rc = s->consume(raw_chunk, &t);
        if (rc) return rc;
        kept = t->chunk.n_rows;
        rc = j ? j->probe(&t->chunk, out) : hj->probe(&t->chunk, out);
        gxop_result_release(t);
    }
    if (rc == 0 && n_scan_kept) *n_scan_kept = kept;
    return rc;
}

gx_op *gxop_scan_create(const gx_scan_cfg *cfg) {
    if (!cfg || cfg->n_preds > GX_MAX_PREDS || cfg->n_projs > GX_MAX_COLS ||
        cfg->n_projs <= 0) {
        gx_set_err("bad scan cfg");
        return nullptr;
    }
    for (int32_t i = 0; i < cfg->n_preds; i++) {
        const gx_pred &p = cfg->preds[i];
        if (p.col < 0 || p.col >= cfg->n_input_cols ||
            p.cmp < GX_CMP_LT || p.cmp > GX_CMP_CONTAINS) {
            gx_set_err("bad scan predicate (column or comparison)");
            return nullptr;
        }
    }
    for (int32_t i = 0; i < cfg->n_projs; i++) {
        const gx_proj &p = cfg->projs[i];
        if (p.op < GX_PROJ_COPY || p.op > GX_PROJ_Q1_CHARGE6 ||
            p.a < 0 || p.a >= cfg->n_input_cols ||
            ((p.op == GX_PROJ_REV_F64 || p.op == GX_PROJ_REV_SCALED4 ||
              p.op == GX_PROJ_Q9_AMOUNT4 || p.op == GX_PROJ_Q1_CHARGE6) &&
             (p.b < 0 || p.b >= cfg->n_input_cols)) ||
            (p.op == GX_PROJ_Q1_CHARGE6 &&
             (p.c < 0 || p.c >= cfg->n_input_cols))) {
            gx_set_err("bad scan projection (op or column)");
            return nullptr;
        }
    }
    if (cfg->device < 0) { gx_set_err("gxhip requires a GPU device"); return nullptr; }
    HIP_OK_NULL(hipSetDevice(cfg->device));
    return new ScanOp(cfg);
}
int gxop_scan_consume(gx_op *op, const gx_chunk *c, gx_result **out) {
    if (!op || op->kind != OP_SCAN) { gx_set_err("not a scan op"); return -1; }
    return static_cast<ScanOp *>(op)->consume(c, out);
}
int gxop_scan_close(gx_op *op) { delete op; return 0; }

} /* extern "C" */

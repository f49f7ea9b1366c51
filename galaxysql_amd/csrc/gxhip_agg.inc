/*
 * gxhip_agg.inc — GPU hash aggregation (included by gxhip.hip).
 *
 * Restates HashAggExec -> AggOpenHashMap.putChunk (AggOpenHashMap.java:
 * 100-139) + GroupOpenHashMap open addressing (GroupOpenHashMap.java:142-193)
 * + aggregator null/init semantics (calc/aggfunctions/*). Group ids are
 * first-claim order (nondeterministic across runs — parity is defined on the
 * result-row multiset, SURVEY.md §4).
 *
 * SIMT-safe streaming design: per consumed chunk, two kernels with no
 * intra-kernel waiting —
 *   k_agg_insert:     claim 16-B slots {tag, krow+1, gid} via one 64-bit CAS
 *                     on the first 8 bytes; ties compared via the persistent
 *                     PACKED key record (one random 16-B line) — key rows
 *                     are device-resident BEFORE the kernel launches, so a
 *                     losing lane always compares, never spins.
 *   k_agg_accumulate: re-probe (one 16-B slot load carries the gid), RMW the
 *                     per-group state with device-scope atomics.
 *
 * Key records: group keys of total fixed width <= 16 B pack into one 16-B
 * record (null values zeroed) + a 1-byte null mask in a separate SMALL array
 * (n rows -> L3-resident), so a compare costs one HBM line + one cached
 * byte. Wider/variable keys fall back to column-wise compare against the
 * keystore. Rehash re-inserts by gid into a 2x table (keys distinct, no
 * compare ambiguity); gids never move, so accumulated state never moves.
 */

namespace {

struct __align__(16) AggSlot {
    unsigned long long claim; /* {tag:32, krow+1:32}; 0 = empty */
    uint32_t gid;             /* written by the claimer; read next kernel */
    uint32_t pad;
};

__device__ __host__ static inline uint32_t agg_tag(int32_t h) {
    return ((uint32_t)h << 1) | 1u; /* nonzero */
}

struct __align__(16) PackedKey {
    unsigned long long lo, hi;
};

/* pack one chunk's group-key rows: values (nulls zeroed) + null mask +
 * Java row hash (Chunk.java:116-129 semantics via row_hash). */
__global__ void k_agg_pack(KeyViews keys, int64_t n, int64_t base,
                           PackedKey *packed, uint8_t *nullmask,
                           int32_t *hashes) {
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < n;
         r += (int64_t)gridDim.x * blockDim.x) {
        PackedKey p;
        p.lo = 0; p.hi = 0;
        uint8_t mask = 0;
        uint8_t *bytes = (uint8_t *)&p;
        int off = 0;
        for (int c = 0; c < keys.n; c++) {
            const DevColView &cv = keys.col[c];
            bool isnull = col_is_null(cv, r);
            if (isnull) mask |= (uint8_t)(1u << c);
            switch (cv.type) {
            case GX_I64: case GX_F64: {
                uint64_t v = isnull ? 0 : ((const uint64_t *)cv.values)[r];
                __builtin_memcpy(bytes + off, &v, 8);
                off += 8;
                break; }
            case GX_I32: {
                uint32_t v = isnull ? 0 : ((const uint32_t *)cv.values)[r];
                __builtin_memcpy(bytes + off, &v, 4);
                off += 4;
                break; }
            }
        }
        packed[base + r] = p;
        nullmask[base + r] = mask;
        hashes[r] = row_hash(keys, r);
    }
}

/* agg row hash: ALL rows hash (null cols contribute 0 per Block.hashCode) —
 * unlike the join's k_hash_rows, which zeroes null-key rows because they
 * never match. */
__global__ void k_agg_hash(KeyViews keys, int64_t n, int32_t *hashes) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        hashes[i] = row_hash(keys, i);
}

__device__ static inline bool packed_equal(const PackedKey *packed,
                                           const uint8_t *nullmask,
                                           int64_t a, int64_t b) {
    PackedKey pa = packed[a], pb = packed[b];
    if (pa.lo != pb.lo || pa.hi != pb.hi) return false;
    /* nullmask == NULL: no key column has carried a NULL so far, every
     * mask byte is 0 — skip the second random request */
    return !nullmask || nullmask[a] == nullmask[b];
}

/* Java Math.min/max semantics for doubles (NaN propagates, -0.0 < +0.0) */
__device__ static inline double jmin_f64(double a, double b) {
    if (a != a) return a;
    if (b != b) return b;
    if (a < b) return a;
    if (b < a) return b;
    /* a == b: the sign distinction only exists for +-0 (Math.min picks
     * -0.0); for any other equal pair return the value itself — the old
     * unconditional "-0.0" here returned the WRONG VALUE for equal
     * nonzero inputs (caught by the sliding-MAX sparse-table parity) */
    if (a == 0.0)
        return (__builtin_signbit(a) || __builtin_signbit(b)) ? -0.0 : a;
    return a;
}
__device__ static inline double jmax_f64(double a, double b) {
    if (a != a) return a;
    if (b != b) return b;
    if (a > b) return a;
    if (b > a) return b;
    if (a == 0.0)
        return (!__builtin_signbit(a) || !__builtin_signbit(b)) ? +0.0 : a;
    return a;
}

__device__ static inline void atomic_min_i64(long long *p, long long v) {
    atomicMin(p, v);
}
__device__ static inline void atomic_max_i64(long long *p, long long v) {
    atomicMax(p, v);
}
__device__ static inline void atomic_jmin_f64(unsigned long long *p, double v) {
    unsigned long long old = *p, assumed;
    do {
        assumed = old;
        double cur = __builtin_bit_cast(double, assumed);
        double nv = jmin_f64(cur, v);
        if (__builtin_bit_cast(unsigned long long, nv) == assumed) return;
        old = atomicCAS(p, assumed, __builtin_bit_cast(unsigned long long, nv));
    } while (old != assumed);
}
__device__ static inline void atomic_jmax_f64(unsigned long long *p, double v) {
    unsigned long long old = *p, assumed;
    do {
        assumed = old;
        double cur = __builtin_bit_cast(double, assumed);
        double nv = jmax_f64(cur, v);
        if (__builtin_bit_cast(unsigned long long, nv) == assumed) return;
        old = atomicCAS(p, assumed, __builtin_bit_cast(unsigned long long, nv));
    } while (old != assumed);
}

/* Per-group state is ONE AoS record (stride u64s): every aggregator's RMW
 * lands on the same 1-2 cache lines instead of one random line per agg
 * array. Null-tracking "seen" slots are plain stores of 1 (idempotent —
 * concurrent same-value stores are race-free), not atomics. */
struct AggAccumParams {
    const AggSlot *slots;
    int slot_records;             /* records indexed by SLOT, not gid */
    const uint32_t *slot_of_row;  /* from the insert pass — no re-probe */
    uint32_t mask;
    int use_packed;
    const PackedKey *packed;
    const uint8_t *nullmask;
    KeyViews keystore;
    const int32_t *hashes;
    int64_t base_krow;
    int64_t n;
    int global_group;          /* noGroupBy: everything is gid 0 */
    /* The aggregates applied: an AggRecDesc's five fields, loose. Embedding
     * the struct here keeps the bytes but changes how the kernel-argument
     * loads of k_agg_accumulate_local are split (24 VGPRs for 28,
     * profiles/README.md), so set_desc copies them instead. */
    int32_t n_aggs;
    int32_t stride;            /* record size in u64s */
    int32_t func[GX_MAX_COLS];
    int32_t val_off[GX_MAX_COLS];
    int32_t seen_off[GX_MAX_COLS];    /* -1 = always-valid agg */
    DevColView input[GX_MAX_COLS];    /* staged CURRENT-chunk value columns */
    unsigned long long *records;
    /* SUM_DEC / AVG_DEC over a GX_DECIMAL column (read by the *_dec kernels
     * only): the scale each record is brought to, the sticky fence word */
    uint8_t dec_scale[GX_MAX_COLS];
    uint32_t *dec_err;

    void set_desc(const AggRecDesc &R) {
        n_aggs = R.n_aggs;
        stride = R.stride;
        std::memcpy(func, R.func, sizeof(func));
        std::memcpy(val_off, R.val_off, sizeof(val_off));
        std::memcpy(seen_off, R.seen_off, sizeof(seen_off));
    }
};

/* One aggregate input value: `bits` holds an I64 value, a sign-extended I32
 * or the bit pattern of an F64, `type` says which. COUNT(*) takes none.
 * `hi` is read by SUM_DEC / AVG_DEC only: the upper half of the 128-bit
 * two's-complement value (an integer's sign extension, 0 or ~0). */
struct AggVal {
    unsigned long long bits;
    unsigned long long hi;
    int32_t type;
    bool isnull;
};

__device__ static inline int64_t aggval_i64(const AggVal &v) {
    return (int64_t)v.bits;
}
__device__ static inline double aggval_f64(const AggVal &v) {
    return v.type == GX_F64 ? __builtin_bit_cast(double, v.bits)
                            : (double)(int64_t)v.bits;
}

/* the value an aggregate of `func` reads from column c at row r (COUNT
 * reads only the null flag; a NULL value is never loaded). DEC: the caller
 * may hold a SUM_DEC / AVG_DEC and wants `hi` (see agg_apply). */
template <bool DEC = false>
__device__ static inline AggVal agg_load(int32_t func, const DevColView &c,
                                         int64_t r) {
    AggVal v;
    v.bits = 0;
    v.hi = 0;
    v.type = c.type;
    v.isnull = false;
    if (func == GX_AGG_COUNT_ROW) return v;
    v.isnull = col_is_null(c, r);
    if (v.isnull || func == GX_AGG_COUNT_COL || c.type == GX_SLICE) return v;
    v.bits = c.type == GX_I32
        ? (unsigned long long)(int64_t)((const int32_t *)c.values)[r]
        : ((const unsigned long long *)c.values)[r];
    if (DEC) v.hi = (unsigned long long)((int64_t)v.bits >> 63);
    return v;
}

/* SUM_DEC / AVG_DEC over a GX_DECIMAL column: decode the 40-B record (a
 * strided read: up to 9 words + the 4 layout bytes) to a 128-bit integer at
 * `scale`. A fenced value sets its bit in *err and reads as NULL. Only the
 * *_dec kernels carry it (see agg_apply). */
__device__ static inline AggVal agg_load_dec(const DevColView &c, int64_t r,
                                             int scale, uint32_t *err) {
    AggVal v;
    v.bits = 0;
    v.hi = 0;
    v.type = GX_DECIMAL;
    v.isnull = col_is_null(c, r);
    if (v.isnull) return v;
    gx_u128 mag;
    bool neg;
    const uint32_t fence = gx_dec40_to_u128(
        (const uint8_t *)c.values + (size_t)r * 40, scale, &mag, &neg);
    if (fence) {
        atomicOr(err, fence);
        v.isnull = true;
        return v;
    }
    if (neg) mag = gx_u128_neg(mag);
    v.bits = mag.lo;
    v.hi = mag.hi;
    return v;
}

/* The read-modify-write of one aggregate on its record, for a value however
 * it was obtained: a staged column (agg_apply) or a projection evaluated at
 * a raw row (the group-join probe-scan). DEC = false compiles the SUM_DEC /
 * AVG_DEC case out: the kernels of ops that cannot hold one (every op but a
 * gxop_agg created with one) keep the code they had without it. */
template <bool DEC = false>
__device__ static inline void agg_rmw(int32_t func, unsigned long long *rec,
                                      int32_t val_off, int32_t seen_off,
                                      const AggVal &v) {
    unsigned long long *vp = rec + val_off;
    if (func == GX_AGG_COUNT_ROW) {
        atomicAdd(vp, 1ull);
        return;
    }
    if (v.isnull) return;
    switch (func) {
    case GX_AGG_COUNT_COL:
        atomicAdd(vp, 1ull);
        break;
    case GX_AGG_SUM_I64:
        atomicAdd(vp, v.bits);
        break;
    case GX_AGG_SUM_I64N: /* null-init Sum: track seen */
        atomicAdd(vp, v.bits);
        if (seen_off >= 0) rec[seen_off] = 1ull;
        break;
    case GX_AGG_SUM_F64:
        atomicAdd((double *)vp, aggval_f64(v));
        rec[seen_off] = 1ull;
        break;
    case GX_AGG_MIN_I64:
        atomic_min_i64((long long *)vp, (long long)aggval_i64(v));
        rec[seen_off] = 1ull;
        break;
    case GX_AGG_MAX_I64:
        atomic_max_i64((long long *)vp, (long long)aggval_i64(v));
        rec[seen_off] = 1ull;
        break;
    case GX_AGG_MIN_F64:
        atomic_jmin_f64(vp, __builtin_bit_cast(double, v.bits));
        rec[seen_off] = 1ull;
        break;
    case GX_AGG_MAX_F64:
        atomic_jmax_f64(vp, __builtin_bit_cast(double, v.bits));
        rec[seen_off] = 1ull;
        break;
    case GX_AGG_BIT_AND: atomicAnd(vp, v.bits); break;
    case GX_AGG_BIT_OR: atomicOr(vp, v.bits); break;
    case GX_AGG_BIT_XOR: atomicXor(vp, v.bits); break;
    case GX_AGG_AVG_F64:
        /* state {sum f64, count u64}; the "seen" slot IS the count
         * (atomicAdd, not the idempotent plain store) — NULL iff 0 */
        atomicAdd((double *)vp, aggval_f64(v));
        atomicAdd(rec + seen_off, 1ull);
        break;
    case GX_AGG_SUM_DEC:
    case GX_AGG_AVG_DEC: {
        if (!DEC) break;
        /* state {lo, hi, seen | count}: a 128-bit two's-complement sum.
         * The returning add on lo tells this lane whether ITS add wrapped
         * lo; the carry joins the value's own upper half in one add on hi,
         * skipped when that is zero (non-negative values, and negative
         * ones whose add wraps lo). Addition mod 2^128 commutes and every
         * wrap of lo is seen by exactly one returning atomic, so the state
         * is exact under any interleaving. */
        const unsigned long long old = atomicAdd(vp, v.bits);
        const unsigned long long add_hi =
            v.hi + ((old + v.bits) < old ? 1ull : 0ull);
        if (add_hi != 0ull) atomicAdd(vp + 1, add_hi);
        if (func == GX_AGG_SUM_DEC) rec[seen_off] = 1ull;
        else atomicAdd(rec + seen_off, 1ull);
        break; }
    }
}

/* ---- transposed accumulate: one request per record line ----------------
 * Atomics execute at the memory side, one request per 64-B line that an
 * atomic INSTRUCTION touches (tools/micro_atomic.hip `records`, profiles/
 * README.md Round 7): a lane that walks its record with agg_rmw sends one
 * request per slot, while adjacent lanes of one instruction that cover the
 * slots of one record send one between them. So for a record of up to
 * GX_AGG_T_SLOTS u64 whose aggregates are all additive, 64 lanes that each
 * hold one (row, record) contribution first say what they add to every slot
 * (AggSlotOps), then agg_add_transposed turns the wave round: W = the power
 * of two >= stride, W passes, lane L of pass i serves slot L % W of the
 * contribution held by lane (L - L % W) + i. A pass is one f64 atomicAdd
 * under the mask of f64 slots and one u64 atomicAdd under the mask of
 * integer slots. The "seen" slot of a null-tracking SUM is ADDED 1 here
 * (it rides in the integer instruction) where agg_rmw stores 1: every
 * reader tests it against zero only, AVG's is a count either way. Which
 * funcs are additive: agg_func_additive (SUM_DEC / AVG_DEC are not, their
 * carry needs agg_rmw's returning add). */
#define GX_AGG_T_SLOTS 4

/* what one contribution adds to each slot of its record: bit s of `skip`
 * set = nothing (slot past the record, NULL input, idle lane) */
struct AggSlotOps {
    unsigned long long v[GX_AGG_T_SLOTS];
    uint32_t skip;
};

__device__ static inline void agg_slot_ops_clear(AggSlotOps &o) {
#pragma unroll
    for (int s = 0; s < GX_AGG_T_SLOTS; s++) o.v[s] = 0ull;
    o.skip = (1u << GX_AGG_T_SLOTS) - 1u;
}

/* enter one additive aggregate's value (agg_rmw's arithmetic, as operands) */
__device__ static inline void agg_slot_ops_put(AggSlotOps &o, int32_t func,
                                               int32_t val_off,
                                               int32_t seen_off,
                                               const AggVal &v) {
    if (func != GX_AGG_COUNT_ROW && v.isnull) return;
    unsigned long long x = v.bits;
    if (func == GX_AGG_COUNT_ROW || func == GX_AGG_COUNT_COL) x = 1ull;
    else if (agg_func_adds_f64(func))
        x = __builtin_bit_cast(unsigned long long, aggval_f64(v));
#pragma unroll
    for (int s = 0; s < GX_AGG_T_SLOTS; s++) { /* no dynamic index: VGPRs */
        if (s == val_off) { o.v[s] = x; o.skip &= ~(1u << s); }
        if (s == seen_off) { o.v[s] = 1ull; o.skip &= ~(1u << s); }
    }
}

/* Apply the wave's 64 contributions. Every lane of the wave calls it (an
 * idle lane passes a cleared `o`); `width` (1, 2 or 4), `stride` and
 * `f64_slots` (bit s = slot s takes an f64 add) are wave-uniform. Several
 * lanes of one instruction may address one word: each add lands. */
__device__ static inline void agg_add_transposed(unsigned long long *records,
                                                 int32_t stride, int32_t width,
                                                 uint32_t f64_slots,
                                                 uint32_t rec_index,
                                                 AggSlotOps o, int lane) {
    unsigned long long skip_of[GX_AGG_T_SLOTS]; /* per slot, bit = lane */
#pragma unroll
    for (int s = 0; s < GX_AGG_T_SLOTS; s++)
        skip_of[s] = __ballot((o.skip >> s) & 1u);
    /* width x width transpose inside each group of `width` lanes: after it
     * v[i] is what the group's lane i adds to THIS lane's slot */
#pragma unroll
    for (int b = 1; b < GX_AGG_T_SLOTS; b <<= 1) {
        const bool hi = (lane & b) != 0;
#pragma unroll
        for (int r = 0; r < GX_AGG_T_SLOTS; r++) {
            if ((r & b) == 0 && (r | b) < width) { /* wave-uniform */
                const unsigned long long got =
                    __shfl_xor(hi ? o.v[r] : o.v[r | b], b, 64);
                if (hi) o.v[r] = got;
                else o.v[r | b] = got;
            }
        }
    }
    const int slot = lane & (width - 1);
    const int lane0 = lane - slot;
    unsigned long long my_skip = skip_of[0];
#pragma unroll
    for (int s = 1; s < GX_AGG_T_SLOTS; s++)
        if (slot == s) my_skip = skip_of[s];
    const bool f64 = (f64_slots >> slot) & 1u;
    /* every cross-lane read stands before the first divergent branch */
    uint32_t at[GX_AGG_T_SLOTS];
#pragma unroll
    for (int i = 0; i < GX_AGG_T_SLOTS; i++)
        at[i] = (uint32_t)__shfl((int)rec_index,
                                 lane0 + (i < width ? i : 0), 64);
#pragma unroll
    for (int i = 0; i < GX_AGG_T_SLOTS; i++) {
        if (i < width && !((my_skip >> (lane0 + i)) & 1ull)) {
            unsigned long long *w = records + (size_t)at[i] * stride + slot;
            if (f64)
                atomicAdd((double *)w, __builtin_bit_cast(double, o.v[i]));
            else
                atomicAdd(w, o.v[i]);
        }
    }
}

/* DEC: the op has a SUM_DEC / AVG_DEC. Decided on the host, which then
 * launches the *_dec twin of the kernel: the 128-bit case of agg_rmw, the
 * high word of agg_load and the 40-B record decode exist only there, so the
 * kernels every other op runs are compiled as if the funcs did not exist. */
template <bool DEC = false>
__device__ static inline void agg_apply_rec(const AggAccumParams &P,
                                            unsigned long long *rec,
                                            int64_t r) {
    for (int a = 0; a < P.n_aggs; a++) {
        if (DEC && P.input[a].type == GX_DECIMAL &&
            agg_func_is_dec(P.func[a]))
            agg_rmw<DEC>(P.func[a], rec, P.val_off[a], P.seen_off[a],
                         agg_load_dec(P.input[a], r, P.dec_scale[a],
                                      P.dec_err));
        else
            agg_rmw<DEC>(P.func[a], rec, P.val_off[a], P.seen_off[a],
                         agg_load<DEC>(P.func[a], P.input[a], r));
    }
}

/* row r into the global record of group / slot / position `gid` */
template <bool DEC = false>
__device__ static inline void agg_apply(const AggAccumParams &P, uint32_t gid,
                                        int64_t r) {
    agg_apply_rec<DEC>(P, P.records + (size_t)gid * P.stride, r);
}

struct AggInsertParams {
    AggSlot *slots;
    uint32_t mask;
    int use_packed;
    const PackedKey *packed;   /* persistent, indexed by krow */
    const uint8_t *nullmask;
    KeyViews keystore;         /* generic fallback compare */
    const int32_t *hashes;     /* this chunk's row hashes */
    int64_t base_krow;
    int64_t n;
    uint32_t *overflow;        /* set when a probe exhausts the table */
    /* small-chunk mode: assign gids inline from a device counter (a hot
     * word is fine at CHUNK_SIZE~1000 rows) instead of the table-scan
     * compaction pass, whose cost scales with TABLE size per chunk. */
    int inline_gid;
    uint32_t *ngroups;
    uint32_t *krow_of_gid;
    uint32_t *slot_of_gid;     /* emission: record index per gid (slot mode) */
    uint32_t *slot_of_row;     /* found slot per chunk row (coalesced);
                                  lets accumulate skip the re-probe */
    /* FUSED accumulation (slot-records mode): RMW the state right at the
     * claim/match point — the records[slot] line is adjacent in time to the
     * slot line just touched, and the separate accumulate pass (one more
     * 600M-row stream + random read) disappears. Retry-safe: a row that
     * exhausts its probes writes GX_SLOT_FAIL and does NOT accumulate; the
     * rerun after the x2 rehash processes ONLY those rows (only_failed), so
     * every row accumulates exactly once even across retries (migrated
     * state moves with its slot). */
    int fuse_accum;
    int only_failed;
    AggAccumParams A;
};

#define GX_SLOT_FAIL 0xFFFFFFFFu

__device__ static inline bool agg_rows_equal(const AggInsertParams &P,
                                             int64_t a, int64_t b) {
    if (P.use_packed) return packed_equal(P.packed, P.nullmask, a, b);
    return rows_key_equal(P.keystore, a, P.keystore, b);
}

#define GX_GID_PENDING 0xFFFFFFFFu

template <bool DEC>
__device__ static inline void agg_insert_body(const AggInsertParams &P) {
    /* (see AggInsertParams.fuse_accum for the fused-accumulate contract) */
    /* Claims only — gid allocation is a SEPARATE compaction pass
     * (k_agg_gid_*): a per-claim atomicAdd on one ngroups word throttled
     * this kernel 12x (measured: 16.8 -> 1.1 ms on the C3 shape; a single
     * hot word serializes returning atomics, MI355X_MICROARCH.md row
     * "dequeue"). Plain-load fast path first: claims are MONOTONIC, so a
     * visible claim is trustworthy and a stale/empty read just falls
     * through to the coherent CAS. */
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < P.n;
         r += (int64_t)gridDim.x * blockDim.x) {
        if (P.only_failed && P.slot_of_row[r] != GX_SLOT_FAIL)
            continue;   /* retry pass: this row already claimed+accumulated */
        const int64_t krow = P.base_krow + r;
        const uint32_t tag = agg_tag(P.hashes[r]);
        const unsigned long long claim =
            ((unsigned long long)tag << 32) | (uint32_t)(krow + 1);
        uint32_t slot = (uint32_t)gx_mix(P.hashes[r]) & P.mask;
        uint32_t probes = 0;
        bool failed = false;
        while (true) {
            unsigned long long old = P.slots[slot].claim;
            if (old == 0ull)
                old = atomicCAS(&P.slots[slot].claim, 0ull, claim);
            if (old == 0ull) {
                if (P.inline_gid) {
                    uint32_t gid = atomicAdd(P.ngroups, 1u);
                    P.slots[slot].gid = gid;
                    P.krow_of_gid[gid] = (uint32_t)krow;
                    if (P.slot_of_gid)   /* slot-records mode only */
                        P.slot_of_gid[gid] = slot;
                } else {
                    P.slots[slot].gid = GX_GID_PENDING;
                }
                break;
            }
            if ((uint32_t)(old >> 32) == tag) {
                int64_t owner = (int64_t)(uint32_t)old - 1;
                if (agg_rows_equal(P, owner, krow))
                    break; /* same group */
            }
            if (++probes > (P.mask < 1023u ? P.mask : 1023u)) {
                /* Probe chains beyond ~1K only happen when the table is
                 * (near) full — a healthy 0.5-load table's longest chain
                 * is tens of slots — so give up EARLY instead of walking
                 * the whole table (a 2048-slot table + 5M incoming groups
                 * made every row walk all slots per growth attempt:
                 * quadratic). A rare false positive just costs one extra
                 * rehash. Host grows x4 and reruns; claims are
                 * idempotent, and with fuse_accum only THIS row is rerun
                 * (GX_SLOT_FAIL). */
                *P.overflow = 1u;
                failed = true;
                break;
            }
            slot = (slot + 1) & P.mask;
        }
        if (P.fuse_accum) {
            P.slot_of_row[r] = failed ? GX_SLOT_FAIL : slot;
            if (!failed) agg_apply<DEC>(P.A, slot, r);
        } else {
            P.slot_of_row[r] = slot;
        }
    }
}

__global__ void k_agg_insert(AggInsertParams P) {
    agg_insert_body<false>(P);
}
/* the same kernel for an op with a SUM_DEC / AVG_DEC (see agg_apply) */
__global__ void k_agg_insert_dec(AggInsertParams P) {
    agg_insert_body<true>(P);
}

/* gid compaction pass 1: count pending claims per slot tile (no hot word —
 * one LDS-reduced store per tile). */
#define GX_GID_TILE 4096

__global__ void k_agg_gid_count(const AggSlot *slots, int64_t n_slots,
                                uint32_t *tile_counts) {
    __shared__ uint32_t cnt;
    for (int64_t tile = blockIdx.x; tile * GX_GID_TILE < n_slots;
         tile += gridDim.x) {
        if (threadIdx.x == 0) cnt = 0;
        __syncthreads();
        int64_t base = tile * GX_GID_TILE;
        int64_t lim = n_slots - base < GX_GID_TILE ? n_slots - base : GX_GID_TILE;
        uint32_t mine = 0;
        for (int64_t j = threadIdx.x; j < lim; j += blockDim.x) {
            AggSlot s = slots[base + j];
            if (s.claim != 0ull && s.gid == GX_GID_PENDING) mine++;
        }
        atomicAdd(&cnt, mine);
        __syncthreads();
        if (threadIdx.x == 0) tile_counts[tile] = cnt;
        __syncthreads();
    }
}

/* single-block exclusive scan of tile counts (small: n_slots/4096 entries);
 * writes total new groups to *total. */
__global__ void k_agg_gid_scan(uint32_t *tile_counts, int64_t n_tiles,
                               uint32_t base_gid, uint32_t *total) {
    __shared__ uint32_t carry;
    if (threadIdx.x == 0) carry = base_gid;
    __syncthreads();
    /* serial chunked scan by one block: n_tiles is small (<= 256K) */
    for (int64_t start = 0; start < n_tiles; start += blockDim.x) {
        int64_t idx = start + threadIdx.x;
        uint32_t v = idx < n_tiles ? tile_counts[idx] : 0;
        /* inclusive scan within the block via LDS */
        __shared__ uint32_t buf[1024];
        buf[threadIdx.x] = v;
        __syncthreads();
        for (uint32_t off = 1; off < blockDim.x; off <<= 1) {
            uint32_t t = threadIdx.x >= off ? buf[threadIdx.x - off] : 0;
            __syncthreads();
            buf[threadIdx.x] += t;
            __syncthreads();
        }
        uint32_t incl = buf[threadIdx.x];
        if (idx < n_tiles) tile_counts[idx] = carry + incl - v; /* exclusive */
        __syncthreads();
        if (threadIdx.x == blockDim.x - 1) carry += incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

/* gid compaction pass 2: assign dense gids tile-locally. */
__global__ void k_agg_gid_assign(AggSlot *slots, int64_t n_slots,
                                 const uint32_t *tile_starts,
                                 uint32_t *krow_of_gid,
                                 uint32_t *slot_of_gid) {
    __shared__ uint32_t cursor;
    for (int64_t tile = blockIdx.x; tile * GX_GID_TILE < n_slots;
         tile += gridDim.x) {
        if (threadIdx.x == 0) cursor = tile_starts[tile];
        __syncthreads();
        int64_t base = tile * GX_GID_TILE;
        int64_t lim = n_slots - base < GX_GID_TILE ? n_slots - base : GX_GID_TILE;
        for (int64_t j = threadIdx.x; j < lim; j += blockDim.x) {
            AggSlot s = slots[base + j];
            if (s.claim != 0ull && s.gid == GX_GID_PENDING) {
                uint32_t gid = atomicAdd(&cursor, 1u);
                slots[base + j].gid = gid;
                krow_of_gid[gid] = (uint32_t)s.claim - 1;
                if (slot_of_gid)   /* slot-records mode only */
                    slot_of_gid[gid] = (uint32_t)(base + j);
            }
        }
        __syncthreads();
    }
}

/* rehash: migrate every occupied OLD slot (claim + gid, incl. PENDING ones
 * from a partially inserted chunk) into a fresh 2x table. Keys are
 * distinct-or-same-group, so claims need no compare. */
__global__ void k_agg_rehash(const AggSlot *old_slots, int64_t n_old,
                             AggSlot *slots, uint32_t mask,
                             KeyViews keystore,
                             const unsigned long long *old_records,
                             unsigned long long *new_records,
                             int32_t rec_stride, uint32_t *new_slot_of_gid) {
    for (int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; s < n_old;
         s += (int64_t)gridDim.x * blockDim.x) {
        AggSlot o = old_slots[s];
        if (o.claim == 0ull) continue;
        const int64_t krow = (int64_t)(uint32_t)o.claim - 1;
        const int32_t h = row_hash(keystore, krow);
        uint32_t slot = (uint32_t)gx_mix(h) & mask;
        while (true) {
            unsigned long long old = atomicCAS(&slots[slot].claim, 0ull, o.claim);
            if (old == 0ull) { slots[slot].gid = o.gid; break; }
            slot = (slot + 1) & mask;
        }
        if (rec_stride > 0) {
            /* slot-indexed per-group state moves WITH its slot */
            for (int32_t k = 0; k < rec_stride; k++)
                new_records[(size_t)slot * rec_stride + k] =
                    old_records[(size_t)s * rec_stride + k];
            if (o.gid != GX_GID_PENDING && new_slot_of_gid)
                new_slot_of_gid[o.gid] = slot;
        }
    }
}

/* initialize records [from, to) from a template (identity values, seen=0) */
struct AggInitParams {
    unsigned long long *records;
    int32_t stride;
    int64_t from, to;
    unsigned long long tmpl[3 * GX_MAX_COLS]; /* <= 3 slots per agg */
};

__global__ void k_agg_init(AggInitParams P) {
    int64_t total = (P.to - P.from) * P.stride;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x)
        P.records[P.from * P.stride + i] = P.tmpl[i % P.stride];
}

/* identity-initialize records [from, to) of buf, laid out by L */
static inline void agg_launch_init(const AggLayout &L, void *buf, int64_t from,
                                   int64_t to, hipStream_t stream) {
    if (to <= from) return;
    AggInitParams P;
    P.records = (unsigned long long *)buf;
    P.stride = L.desc.stride;
    P.from = from;
    P.to = to;
    std::memcpy(P.tmpl, L.tmpl, sizeof(P.tmpl));
    hipLaunchKernelGGL(k_agg_init, dim3(gx_grid((to - from) * P.stride)),
                       dim3(256), 0, stream, P);
}

/* the layout of an op's aggregate list (base funcs, <= GX_MAX_COLS) */
static inline AggLayout agg_layout_of(const std::vector<gx_agg_spec> &aggs) {
    int32_t funcs[GX_MAX_COLS];
    for (size_t a = 0; a < aggs.size(); a++) funcs[a] = aggs[a].func;
    AggLayout L;
    L.build(funcs, (int)aggs.size());
    return L;
}

/* dst[i] = the staged column aggregate i of a descriptor reads; COUNT(*)'s
 * stays as the caller zeroed it. agg_idx: the list the descriptor was
 * select()ed by, NULL = every aggregate of the op. */
static inline void agg_bind_inputs(DevColView *dst, const gx_agg_spec *aggs,
                                   const int32_t *agg_idx, int n,
                                   const std::vector<DevColView> &views) {
    for (int i = 0; i < n; i++) {
        const int32_t col = aggs[agg_idx ? agg_idx[i] : i].input_col;
        if (col >= 0) dst[i] = views[(size_t)col];
    }
}

template <bool DEC>
__device__ static inline void agg_accumulate_body(const AggAccumParams &P) {
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < P.n;
         r += (int64_t)gridDim.x * blockDim.x) {
        uint32_t rec = 0;
        if (!P.global_group)
            /* slot mode: the RMW target IS records[slot] — ONE random line
             * per row (the slots[slot].gid indirection cost a second;
             * measured on the Q18 shape via the group-join wide-entry
             * experiment, profiles/README.md) */
            rec = P.slot_records ? P.slot_of_row[r]
                                 : P.slots[P.slot_of_row[r]].gid;
        agg_apply<DEC>(P, rec, r);
    }
}

__global__ void k_agg_accumulate(AggAccumParams P) {
    agg_accumulate_body<false>(P);
}
__global__ void k_agg_accumulate_dec(AggAccumParams P) {
    agg_accumulate_body<true>(P);
}

/* ---- block-local pre-aggregation (few groups) ---------------------------
 * k_agg_accumulate sends every row's RMWs to records[gid]: with a handful of
 * groups (Q1's 4, a global aggregate's 1) all of them queue on the same few
 * L2 lines. Here a block keeps its own copy of the `groups` records in LDS,
 * accumulates its rows there with LDS atomics (agg_rmw itself, on the LDS
 * record) and merges each record it touched into records[gid] once, after
 * its last row: touched groups x stride global atomics per BLOCK instead of
 * n_aggs per ROW. The host launches it only when every gid of the chunk is
 * below `groups` (it knows n_groups_host), so there is no per-row fallback.
 *
 * Same-address LDS atomics of one instruction serialize as well, so the
 * block holds `replicas` (a power of two, up to GX_AGG_LOCAL_MAX_REPLICAS)
 * copies and thread t works on copy t % replicas; the flush folds the copies in registers before the one
 * global merge. Layout: lds[(replica * groups + gid) * stride + slot], then
 * one u32 "touched" marker per (replica, gid).
 *
 * Every func is a commutative monoid, so partial state folds and merges in
 * any order; SUM_DEC / AVG_DEC keep the carry rule of agg_rmw both in LDS
 * (returning ds add on lo) and at the merge (returning global add on lo with
 * the partial's lo, carry + the partial's hi into hi): addition mod 2^128
 * commutes, so the 128-bit state is exact as before. */
#define GX_AGG_LOCAL_LDS_BYTES (32 * 1024) /* 4 blocks/CU of 160 KiB */
#define GX_AGG_LOCAL_MAX_REPLICAS 16 /* measured: 4..16 best, 64 behind */

/* Measured (profiles/README.md "Low-cardinality GROUP BY"):
 * MAX_GROUPS: the count limit of the local group cap. The sweep has the
 *   local path ahead up to 1024 groups, by the least there (1.15x at the
 *   gate's chunk size); 1024 is also the reference planner's floor for the
 *   hint when it knows nothing (HashAggExecutorFactory MIN_HASH_TABLE_SIZE),
 *   which must not read as "few groups": 512.
 * MIN_ROWS: chunks of 2^18 rows or more at any group count up to the cap;
 *   MIN_ROWS_FEW: chunks of 2^16 rows or more at up to FEW_GROUPS groups
 *   (at 2^16 rows the flush of more groups no longer pays).
 * BLOCK_ROWS / BLOCKS_PER_CU: a block flushes touched groups x stride
 *   atomics once, so it gets at least this many rows and the grid at most
 *   this many blocks per CU. */
#define GX_AGG_LOCAL_MAX_GROUPS 512
#define GX_AGG_LOCAL_MIN_ROWS ((int64_t)1 << 18)
#define GX_AGG_LOCAL_MIN_ROWS_FEW ((int64_t)1 << 16)
#define GX_AGG_LOCAL_FEW_GROUPS 128
#define GX_AGG_LOCAL_BLOCK_ROWS 2048
#define GX_AGG_LOCAL_BLOCKS_PER_CU 4

struct AggLocalParams {
    AggAccumParams A;
    int32_t groups;                /* every gid of the chunk is below it */
    int32_t replicas;              /* power of two */
    unsigned long long tmpl[3 * GX_MAX_COLS]; /* identity record */
};

__host__ __device__ static inline size_t agg_local_lds_bytes(int32_t groups,
                                                             int32_t stride,
                                                             int32_t replicas) {
    return (size_t)replicas * groups * ((size_t)stride * 8 + 4);
}

/* fold one aggregate of one group over the block's replicas and merge the
 * partial into the global record. Runs on one thread per (group, agg). */
template <bool DEC>
__device__ static inline void agg_local_merge(const AggLocalParams &P,
                                              const unsigned long long *lds,
                                              const uint32_t *touched,
                                              int32_t g, int32_t a) {
    const int32_t func = P.A.func[a];
    const int32_t vo = P.A.val_off[a], so = P.A.seen_off[a];
    const int32_t stride = P.A.stride;
    unsigned long long acc = P.tmpl[vo], acc_hi = 0ull, seen = 0ull;
    bool any = false;
    for (int32_t rep = 0; rep < P.replicas; rep++) {
        const int32_t li = rep * P.groups + g;
        if (!touched[li]) continue;
        any = true;
        const unsigned long long *rec = lds + (size_t)li * stride;
        const unsigned long long x = rec[vo];
        if (so >= 0) seen += rec[so]; /* a flag (0/1) or AVG's count */
        switch (func) {
        case GX_AGG_SUM_F64: case GX_AGG_AVG_F64:
            acc = __builtin_bit_cast(unsigned long long,
                __builtin_bit_cast(double, acc) + __builtin_bit_cast(double, x));
            break;
        case GX_AGG_MIN_I64:
            if ((long long)x < (long long)acc) acc = x;
            break;
        case GX_AGG_MAX_I64:
            if ((long long)x > (long long)acc) acc = x;
            break;
        case GX_AGG_MIN_F64:
            acc = __builtin_bit_cast(unsigned long long,
                jmin_f64(__builtin_bit_cast(double, acc),
                         __builtin_bit_cast(double, x)));
            break;
        case GX_AGG_MAX_F64:
            acc = __builtin_bit_cast(unsigned long long,
                jmax_f64(__builtin_bit_cast(double, acc),
                         __builtin_bit_cast(double, x)));
            break;
        case GX_AGG_BIT_AND: acc &= x; break;
        case GX_AGG_BIT_OR: acc |= x; break;
        case GX_AGG_BIT_XOR: acc ^= x; break;
        case GX_AGG_SUM_DEC: case GX_AGG_AVG_DEC:
            if (DEC) {
                const unsigned long long lo = acc + x;
                acc_hi += rec[vo + 1] + (lo < acc ? 1ull : 0ull);
                acc = lo;
            }
            break;
        default: /* COUNT_ROW / COUNT_COL / SUM_I64 / SUM_I64N */
            acc += x;
            break;
        }
    }
    if (!any) return;
    unsigned long long *grec = P.A.records + (size_t)g * stride;
    unsigned long long *vp = grec + vo;
    /* a null-tracking aggregate whose inputs were all NULL here merges
     * nothing: its identity (MIN/MAX's +-Inf, INT64_MAX/MIN) stays in LDS
     * and `seen` stays as it was */
    if (so >= 0 && seen == 0ull) return;
    switch (func) {
    case GX_AGG_COUNT_ROW: case GX_AGG_COUNT_COL: case GX_AGG_SUM_I64:
        if (acc) atomicAdd(vp, acc);
        break;
    case GX_AGG_SUM_I64N:
        atomicAdd(vp, acc);
        if (so >= 0) grec[so] = 1ull;
        break;
    case GX_AGG_SUM_F64:
        atomicAdd((double *)vp, __builtin_bit_cast(double, acc));
        grec[so] = 1ull;
        break;
    case GX_AGG_AVG_F64: /* the count slot takes the partial COUNT */
        atomicAdd((double *)vp, __builtin_bit_cast(double, acc));
        atomicAdd(grec + so, seen);
        break;
    case GX_AGG_MIN_I64:
        atomic_min_i64((long long *)vp, (long long)acc);
        grec[so] = 1ull;
        break;
    case GX_AGG_MAX_I64:
        atomic_max_i64((long long *)vp, (long long)acc);
        grec[so] = 1ull;
        break;
    case GX_AGG_MIN_F64:
        atomic_jmin_f64(vp, __builtin_bit_cast(double, acc));
        grec[so] = 1ull;
        break;
    case GX_AGG_MAX_F64:
        atomic_jmax_f64(vp, __builtin_bit_cast(double, acc));
        grec[so] = 1ull;
        break;
    case GX_AGG_BIT_AND: atomicAnd(vp, acc); break;
    case GX_AGG_BIT_OR: atomicOr(vp, acc); break;
    case GX_AGG_BIT_XOR: atomicXor(vp, acc); break;
    case GX_AGG_SUM_DEC:
    case GX_AGG_AVG_DEC: {
        if (!DEC) break;
        /* agg_rmw's 128-bit case with v = {acc, acc_hi} */
        const unsigned long long old = atomicAdd(vp, acc);
        const unsigned long long add_hi =
            acc_hi + ((old + acc) < old ? 1ull : 0ull);
        if (add_hi != 0ull) atomicAdd(vp + 1, add_hi);
        if (func == GX_AGG_SUM_DEC) grec[so] = 1ull;
        else atomicAdd(grec + so, seen);
        break; }
    }
}

template <bool DEC>
__device__ static inline void agg_accumulate_local_body(
        const AggLocalParams &P) {
    extern __shared__ unsigned long long gx_agg_lds[];
    const int32_t stride = P.A.stride;
    const int32_t n_recs = P.replicas * P.groups;
    unsigned long long *lds = gx_agg_lds;
    uint32_t *touched = (uint32_t *)(lds + (size_t)n_recs * stride);
    for (int32_t i = threadIdx.x; i < n_recs * stride; i += blockDim.x)
        lds[i] = P.tmpl[i % stride];
    for (int32_t i = threadIdx.x; i < n_recs; i += blockDim.x)
        touched[i] = 0u;
    __syncthreads();

    const int32_t rep_base =
        (int32_t)(threadIdx.x & (uint32_t)(P.replicas - 1)) * P.groups;
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < P.A.n;
         r += (int64_t)gridDim.x * blockDim.x) {
        uint32_t gid = 0;
        if (!P.A.global_group) gid = P.A.slots[P.A.slot_of_row[r]].gid;
        if (gid >= (uint32_t)P.groups) continue; /* host contract; LDS bound */
        const int32_t li = rep_base + (int32_t)gid;
        unsigned long long *rec = lds + (size_t)li * stride;
        touched[li] = 1u; /* idempotent plain store */
        agg_apply_rec<DEC>(P.A, rec, r); /* agg_rmw's atomics, on LDS */
    }
    __syncthreads(); /* the one barrier after the loop: every thread is here */

    const int32_t items = P.groups * P.A.n_aggs;
    for (int32_t i = threadIdx.x; i < items; i += blockDim.x)
        agg_local_merge<DEC>(P, lds, touched, i / P.A.n_aggs,
                             i % P.A.n_aggs);
}

__global__ void __launch_bounds__(256)
k_agg_accumulate_local(AggLocalParams P) {
    agg_accumulate_local_body<false>(P);
}
__global__ void __launch_bounds__(256)
k_agg_accumulate_local_dec(AggLocalParams P) {
    agg_accumulate_local_body<true>(P);
}

/* Emission, one kernel for the whole result: each group's record (a random
 * line in slot mode) is read ONCE and every aggregate's value + null flag
 * written from it; with packed null-free keys the group-key columns come
 * out of the group's 16-B packed record as well (one random read per group
 * instead of one gather per key column). */
struct AggEmitParams {
    const unsigned long long *records;
    uint32_t n_groups;
    const uint32_t *slot_of_gid;   /* slot mode; NULL = records[gid] */
    AggRecDesc R;
    uint8_t dec_scale[GX_MAX_COLS];  /* SUM_DEC / AVG_DEC: input scale */
    void *out_vals[GX_MAX_COLS];
    uint8_t *out_nulls[GX_MAX_COLS];
    int32_t n_keys;                /* 0 = key columns gathered separately */
    int32_t key_type[GX_MAX_KEYS];
    const PackedKey *packed;
    const uint32_t *krow_of_gid;
    void *key_vals[GX_MAX_KEYS];
    uint8_t *key_nulls[GX_MAX_KEYS];
};

__global__ void k_agg_emit(AggEmitParams P) {
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < P.n_groups;
         g += gridDim.x * blockDim.x) {
        if (P.n_keys > 0) {
            const PackedKey pk = P.packed[P.krow_of_gid[g]];
            const uint8_t *bytes = (const uint8_t *)&pk;
            int off = 0;
            for (int c = 0; c < P.n_keys; c++) {
                P.key_nulls[c][g] = 0;
                if (P.key_type[c] == GX_I32) {
                    uint32_t v;
                    __builtin_memcpy(&v, bytes + off, 4);
                    ((uint32_t *)P.key_vals[c])[g] = v;
                    off += 4;
                } else {
                    uint64_t v;
                    __builtin_memcpy(&v, bytes + off, 8);
                    ((uint64_t *)P.key_vals[c])[g] = v;
                    off += 8;
                }
            }
        }
        const size_t rec_idx = P.slot_of_gid ? P.slot_of_gid[g] : g;
        const unsigned long long *rec = P.records + rec_idx * P.R.stride;
        for (int a = 0; a < P.R.n_aggs; a++) {
            const int32_t func = P.R.func[a], seen_off = P.R.seen_off[a];
            if (agg_func_is_dec(func)) {
                const bool isnull = rec[seen_off] == 0ull;
                P.out_nulls[a][g] = isnull;
                /* 40-B DecimalBlock record of the 128-bit state; AVG
                 * divides |sum| by the count, half-up at scale 4 */
                uint8_t *dst = (uint8_t *)P.out_vals[a] + (size_t)g * 40;
                if (isnull) { /* zero record, as every NULL DECIMAL */
                    for (int k = 0; k < 5; k++)
                        ((unsigned long long *)dst)[k] = 0ull;
                    continue;
                }
                gx_u128 mag;
                mag.lo = rec[P.R.val_off[a]];
                mag.hi = rec[P.R.val_off[a] + 1];
                const bool neg = (mag.hi >> 63) != 0ull;
                if (neg) mag = gx_u128_neg(mag);
                int scale = P.dec_scale[a];
                if (func == GX_AGG_AVG_DEC) {
                    mag = gx_dec_avg4(mag, rec[seen_off], scale);
                    scale = 4;
                }
                gx_u128_to_dec40(mag, neg, scale, dst);
                continue;
            }
            /* I64 results and F64 bit patterns alike */
            const AggDecoded d = agg_decode(func, rec, P.R.val_off[a],
                                            seen_off);
            P.out_nulls[a][g] = d.isnull;
            ((unsigned long long *)P.out_vals[a])[g] = d.bits;
        }
    }
}

/* ---- DISTINCT aggregates ------------------------------------------------
 * AggOpenHashMap.putChunk asks a per-aggregator DistinctSet — itself a
 * GroupOpenHashMap over (groupId, value) — whether the pair was seen, and
 * accumulates only when it was not (AggOpenHashMap.java:100-139,
 * operator/util/DistinctSet.java). Here: one device set per distinct INPUT
 * COLUMN (COUNT(DISTINCT x), SUM(DISTINCT x) share it), built like the group
 * table above and for the same reasons. Per consumed chunk, once the chunk's
 * gids are final:
 *   k_dist_pack:   one persistent 16-B record {gid, hash, value} per row,
 *                  resident BEFORE the insert launches (a losing lane always
 *                  compares against data already there, never waits).
 *   k_dist_insert: claim an 8-B slot {tag:32, drow+1:32} with one 64-bit
 *                  CAS; the winner applies that column's distinct aggs to
 *                  records[gid] through agg_apply (base funcs); a lane that
 *                  finds an equal owner drops its row. NULL values never
 *                  enter the set.
 * A bounded probe sets the overflow flag and leaves the row PENDING; the
 * host grows the slot array x4 (owners re-inserted by drow — distinct by
 * construction, no compare) and reruns only the pending rows, so every row
 * resolves exactly once and a win accumulates exactly once.
 * Value hash/equality are col_hash / col_eq of the value's type, i.e. what
 * a group-key column of that type gets. */

struct __align__(16) DistRec {
    uint32_t gid;
    int32_t hash;             /* pair hash; kept so growth never recomputes */
    unsigned long long value; /* fixed-width value bits (I32 zero-extended);
                                 unused for SLICE (compared via the store) */
};

#define GX_DIST_PENDING 0
#define GX_DIST_DONE 1

__device__ static inline int32_t dist_pair_hash(uint32_t gid, int32_t vh) {
    /* gids are dense small integers: scramble before combining, or
     * (gid, v) and (gid+1, v-31) would share a probe chain */
    return (int32_t)((uint32_t)gx_murmur3((int32_t)gid) * 31u + (uint32_t)vh);
}

__global__ void k_dist_pack(DevColView in, int64_t n, int64_t base,
                            const uint32_t *slot_of_row, const AggSlot *slots,
                            DistRec *recs, uint8_t *status) {
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < n;
         r += (int64_t)gridDim.x * blockDim.x) {
        DistRec rec;
        rec.gid = slot_of_row ? slots[slot_of_row[r]].gid : 0u;
        rec.hash = 0;
        rec.value = 0ull;
        const bool isnull = col_is_null(in, r);
        if (!isnull) {
            rec.hash = dist_pair_hash(rec.gid, col_hash(in, r));
            switch (in.type) {
            case GX_I64: case GX_F64:
                rec.value = ((const unsigned long long *)in.values)[r];
                break;
            case GX_I32:
                rec.value = ((const uint32_t *)in.values)[r];
                break;
            }
        }
        recs[base + r] = rec;
        status[r] = isnull ? GX_DIST_DONE : GX_DIST_PENDING;
    }
}

struct DistInsertParams {
    unsigned long long *slots;  /* {tag:32, drow+1:32}; 0 = empty */
    uint32_t mask;
    int32_t vtype;
    const DistRec *recs;        /* persistent, indexed by drow */
    DevColView store;           /* SLICE: persistent value column (by drow) */
    int64_t base_drow;
    int64_t n;
    uint8_t *status;            /* per chunk row: PENDING / DONE */
    uint32_t *ctl;              /* [0] overflow flag, [1] owners (occupancy) */
    AggAccumParams A;           /* this set's aggs, base funcs */
};

__device__ static inline bool dist_equal(const DistInsertParams &P,
                                         const DistRec &mine, int64_t drow,
                                         int64_t owner) {
    const DistRec o = P.recs[owner];
    if (o.gid != mine.gid) return false;
    switch (P.vtype) {
    case GX_F64: /* col_eq: IEEE ==, as for an F64 group key */
        return __builtin_bit_cast(double, o.value) ==
               __builtin_bit_cast(double, mine.value);
    case GX_SLICE:
        return col_eq(P.store, owner, P.store, drow);
    default:
        return o.value == mine.value;
    }
}

__global__ void k_dist_insert(DistInsertParams P) {
    __shared__ uint32_t block_wins;
    if (threadIdx.x == 0) block_wins = 0;
    __syncthreads();
    uint32_t wins = 0;
    const uint32_t max_probes = P.mask < 1023u ? P.mask : 1023u;
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < P.n;
         r += (int64_t)gridDim.x * blockDim.x) {
        if (P.status[r] != GX_DIST_PENDING) continue;
        /* the table is already known to be too small: leave the rest
         * PENDING instead of walking a full table 1K slots per row (a stale
         * read only costs this row its probes) */
        if (__hip_atomic_load(P.ctl, __ATOMIC_RELAXED,
                              __HIP_MEMORY_SCOPE_AGENT))
            continue;
        const int64_t drow = P.base_drow + r;
        const DistRec mine = P.recs[drow];
        const uint32_t tag = agg_tag(mine.hash);
        const unsigned long long claim =
            ((unsigned long long)tag << 32) | (uint32_t)(drow + 1);
        uint32_t slot = (uint32_t)gx_mix(mine.hash) & P.mask;
        uint32_t probes = 0;
        while (true) {
            /* plain load first: claims are monotonic (see k_agg_insert) */
            unsigned long long old = P.slots[slot];
            if (old == 0ull) old = atomicCAS(&P.slots[slot], 0ull, claim);
            if (old == 0ull) {
                /* first of its (group, value): the only lane that counts */
                agg_apply(P.A, mine.gid, r);
                wins++;
                P.status[r] = GX_DIST_DONE;
                break;
            }
            if ((uint32_t)(old >> 32) == tag &&
                dist_equal(P, mine, drow, (int64_t)(uint32_t)old - 1)) {
                P.status[r] = GX_DIST_DONE; /* seen before: drop */
                break;
            }
            if (++probes > max_probes) {
                P.ctl[0] = 1u; /* stays PENDING for the rerun after growth */
                break;
            }
            slot = (slot + 1) & P.mask;
        }
    }
    /* occupancy: one global add per block, not a hot word per claim */
    if (wins) atomicAdd(&block_wins, wins);
    __syncthreads();
    if (threadIdx.x == 0 && block_wins) atomicAdd(P.ctl + 1, block_wins);
}

/* growth: re-insert every owner by drow into the larger slot array */
__global__ void k_dist_rehash(const unsigned long long *old_slots,
                              int64_t n_old, unsigned long long *slots,
                              uint32_t mask, const DistRec *recs) {
    for (int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; s < n_old;
         s += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long c = old_slots[s];
        if (c == 0ull) continue;
        const int32_t h = recs[(int64_t)(uint32_t)c - 1].hash;
        uint32_t slot = (uint32_t)gx_mix(h) & mask;
        while (atomicCAS(&slots[slot], 0ull, c) != 0ull)
            slot = (slot + 1) & mask;
    }
}

/* DISTINCT func -> the base func whose state/accumulate/emit it shares;
 * -1 for a plain func */
static inline int32_t agg_distinct_base(int32_t f) {
    switch (f) {
    case GX_AGG_COUNT_DISTINCT: return GX_AGG_COUNT_COL;
    case GX_AGG_SUM_I64_DISTINCT: return GX_AGG_SUM_I64;
    case GX_AGG_SUM_I64N_DISTINCT: return GX_AGG_SUM_I64N;
    case GX_AGG_SUM_F64_DISTINCT: return GX_AGG_SUM_F64;
    case GX_AGG_AVG_F64_DISTINCT: return GX_AGG_AVG_F64;
    default: return -1;
    }
}
/* the other ops' creates reject these (gxop_agg only) */
static inline bool gx_agg_is_distinct(int32_t f) {
    return agg_distinct_base(f) >= 0;
}
/* SUM_DEC / AVG_DEC, with or without a scale in the upper 16 bits: gxop_agg
 * only as well (the other ops' emit kernels write 8-B values) */
static inline bool gx_agg_is_dec(int32_t f) {
    return agg_func_is_dec(f & 0xFFFF);
}

/* host side of one distinct set (one per distinct input column) */
struct DistSet {
    int32_t input_col = -1;
    int32_t vtype = GX_I64;
    std::vector<int32_t> agg_idx;  /* the op's aggs fed by this set */
    DevBuf d_ctl, d_slots, d_recs;
    DevStore store;                /* SLICE values, appended per chunk */
    int64_t n_slots = 0;
    int64_t n_drows = 0;           /* records written so far */
    uint32_t owners = 0;           /* occupancy, read back per attempt */
};

struct AggOp : gx_op {
    gx_agg_cfg cfg;
    std::vector<int32_t> group_cols_, input_types;
    std::vector<gx_agg_spec> aggs;

    /* DISTINCT: aggs[] holds BASE funcs (layout, accumulate and emission
     * work by base func); is_distinct[a] marks the ones fed by a DistSet */
    std::vector<uint8_t> is_distinct;
    bool has_distinct = false;

    /* device buffers, last-allocated first (see DevBuf: destruction order
     * and the pool); d_slots / d_records, d_hashes / d_slotidx and
     * d_krow_of_gid / d_slot_of_gid share a size class */
    DevBuf d_decerr;            /* DECIMAL-input fence word (sticky bits) */
    std::vector<DistSet> dsets; /* one per distinct input column */
    DevBuf d_dstatus;           /* per chunk row: distinct pass status */
    DevBuf d_slot_of_gid;      /* slot mode: record index per gid */
    DevBuf d_records;          /* AoS per-group state records */
    DevBuf d_slotidx, d_total, d_tiles, d_hashes, d_krow_of_gid, d_slots;
    DevBuf d_nullmask, d_packed;  /* packed fast-path key records */
    DevStore keystore;         /* appended group-key columns (for emit) */
    bool slot_records = false; /* records indexed by slot (narrow state) */
    AggLayout layout;          /* the AoS state record, over aggs[] */
    std::vector<int32_t> plain_idx; /* the aggs no DistSet feeds */
    /* SUM_DEC / AVG_DEC: aggs[] holds the base func, the scale that rode in
     * the spec's upper 16 bits is split off here once */
    uint8_t dec_scale[GX_MAX_COLS] = {0};
    bool has_dec = false;       /* consume launches the *_dec kernels */
    bool has_dec_input = false; /* one of them reads a GX_DECIMAL column:
                                   consume reads the fence word back */
    int64_t n_slots = 0;
    uint32_t mask = 0;
    uint32_t n_groups_host = 0;
    int64_t group_cap = 0;
    bool use_packed = false;
    bool emitted = false;
    bool global_agg_seeded = false;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    double kernel_ms = 0.0;
    int64_t consumes = 0, rows_total = 0;
    /* block-local pre-aggregation (k_agg_accumulate_local): GX_AGG_LOCAL at
     * create — -1 unset (gates apply), 0 never, 1 whenever the groups fit */
    int local_mode = -1;
    int32_t local_cap = 0;      /* most groups the local kernel takes */
    int32_t local_rep_max = GX_AGG_LOCAL_MAX_REPLICAS;
    int32_t local_cus = 0;      /* CU count, read at the first launch */
    int64_t local_rows = 0, local_launches = 0;
    int32_t local_replicas = 0; /* at the last launch */

    AggOp(const gx_agg_cfg *c) : gx_op(OP_AGG, c->device, c->stream), cfg(*c) {
        group_cols_.assign(c->group_cols, c->group_cols + c->n_group_cols);
        input_types.assign(c->input_types, c->input_types + c->n_input_cols);
        aggs.assign(c->aggs, c->aggs + c->n_aggs);
        is_distinct.assign(aggs.size(), 0);
        for (size_t a = 0; a < aggs.size(); a++) {
            dec_scale[a] = (uint8_t)((uint32_t)aggs[a].func >> 16);
            aggs[a].func &= 0xFFFF;
            if (!agg_func_is_dec(aggs[a].func)) continue;
            has_dec = true;
            if (input_types[aggs[a].input_col] == GX_DECIMAL)
                has_dec_input = true;
        }
        for (size_t a = 0; a < aggs.size(); a++) {
            int32_t base = agg_distinct_base(aggs[a].func);
            if (base < 0) continue;
            aggs[a].func = base;
            is_distinct[a] = 1;
            has_distinct = true;
            DistSet *ds = nullptr;
            for (auto &d : dsets)
                if (d.input_col == aggs[a].input_col) ds = &d;
            if (!ds) {
                dsets.emplace_back();
                ds = &dsets.back();
                ds->input_col = aggs[a].input_col;
                ds->vtype = input_types[ds->input_col];
                if (ds->vtype == GX_SLICE)
                    ds->store.init(1, &ds->vtype, stream);
            }
            ds->agg_idx.push_back((int32_t)a);
        }
        std::vector<int32_t> key_types;
        int width = 0;
        bool fixed = true;
        for (int32_t gc : group_cols_) {
            key_types.push_back(input_types[gc]);
            switch (input_types[gc]) {
            case GX_I64: case GX_F64: width += 8; break;
            case GX_I32: width += 4; break;
            default: fixed = false; break;
            }
        }
        /* single fixed-width key: the keystore column IS the packed form —
         * the generic col-compare reads one 8B line vs packed's 16B record
         * + mask byte, and the pack kernel (16B/row write) is skipped */
        use_packed = fixed && width <= 16 && group_cols_.size() <= 8
                     && group_cols_.size() >= 2;
        keystore.init((int32_t)key_types.size(), key_types.data(), stream);

        layout = agg_layout_of(aggs);
        for (size_t a = 0; a < aggs.size(); a++)
            if (!is_distinct[a]) plain_idx.push_back((int32_t)a);
        const int32_t stride = layout.desc.stride;
        /* slot-indexed state: the accumulate RMW lands on records[slot]
         * directly (one random line/row) and fuses into the insert pass.
         * Memory = n_slots x stride x 8 (2x the group count at load 0.5),
         * so gate on narrow state: records of up to GX_AGG_SLOT_STRIDE
         * u64s (default 4, clamped to 1..4; 2 = the pre-round-4 gate). */
        int32_t slot_stride_max = 4;
        if (const char *se = getenv("GX_AGG_SLOT_STRIDE")) {
            int v = atoi(se);
            if (v >= 1 && v <= 4) slot_stride_max = v;
        }
        slot_records = stride <= slot_stride_max && cfg.n_group_cols > 0;
        if (const char *le = getenv("GX_AGG_LOCAL")) {
            if (le[0] == '0' && !le[1]) local_mode = 0;
            else if (le[0] == '1' && !le[1]) local_mode = 1;
        }
        if (const char *re = getenv("GX_AGG_LOCAL_REPLICAS")) {
            /* bench knob: cap the replica count (1 = plain shared copy) */
            int v = atoi(re);
            if (v >= 1 && v <= GX_AGG_LOCAL_MAX_REPLICAS && (v & (v - 1)) == 0)
                local_rep_max = v;
        }
        local_cap = (int32_t)std::min<size_t>(
            GX_AGG_LOCAL_MAX_GROUPS,
            agg_local_lds_bytes(1, stride, 1) <= GX_AGG_LOCAL_LDS_BYTES
                ? GX_AGG_LOCAL_LDS_BYTES / agg_local_lds_bytes(1, stride, 1)
                : 0);
        /* a planner hint of few groups: keep even a narrow state gid-indexed
         * so its accumulate pass can run block-local (gxop.h,
         * expected_groups) */
        if (local_mode != 0 && cfg.expected_groups >= 1 &&
            cfg.expected_groups <= local_cap)
            slot_records = false;
        /* a distinct agg accumulates by gid from its own pass: state is
         * gid-indexed (gids never move) */
        if (has_distinct) slot_records = false;
    }
    ~AggOp() override {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
    }

    int64_t max_fill() const { return n_slots / 2; }

    /* identity-initialize records [from, to) of buf */
    int init_records(void *buf, int64_t from, int64_t to) {
        if (to <= from) return 0;
        if (layout.tmpl_zero) {
            const size_t rec_bytes = (size_t)layout.desc.stride * 8;
            HIP_OK(hipMemsetAsync((char *)buf + (size_t)from * rec_bytes, 0,
                                  (size_t)(to - from) * rec_bytes, stream));
            return 0;
        }
        agg_launch_init(layout, buf, from, to, stream);
        return 0;
    }
    int init_state_range(int64_t from, int64_t to) {
        return init_records(d_records.p, from, to);
    }

    int ensure_group_cap(int64_t need) {
        if (need <= group_cap) return 0;
        int64_t ncap = std::max<int64_t>(group_cap * 2, std::max<int64_t>(need, 1024));
        if (d_krow_of_gid.grow((size_t)ncap * 4, stream)) return -1;
        if (slot_records) {
            if (d_slot_of_gid.grow((size_t)ncap * 4, stream)) return -1;
            group_cap = ncap;
            return 0;
        }
        if (d_records.grow((size_t)ncap * layout.desc.stride * 8, stream))
            return -1;
        int64_t old = group_cap;
        group_cap = ncap;
        return init_state_range(old, ncap);
    }

    /* the fields agg_apply reads: aggregates idx[0..k) of the op, or all of
     * them (idx == NULL), over the staged chunk. The one place where an
     * index list meets both select() and the input binding. */
    void fill_accum_params(AggAccumParams &A, const StagedChunk &st,
                           const int32_t *idx = nullptr, int k = 0) {
        A.set_desc(idx ? layout.select(idx, k) : layout.desc);
        std::memset(A.input, 0, sizeof(A.input)); /* COUNT(*) binds none */
        std::memset(A.dec_scale, 0, sizeof(A.dec_scale));
        agg_bind_inputs(A.input, aggs.data(), idx, A.n_aggs, st.views);
        for (int i = 0; i < A.n_aggs; i++)
            A.dec_scale[i] = dec_scale[idx ? idx[i] : i];
        A.records = (unsigned long long *)d_records.p;
        A.dec_err = (uint32_t *)d_decerr.p;
    }

    /* any group-key column has carried a NULL so far (sticky per column;
     * checked after the chunk's keys are appended, so it covers both sides
     * of every compare) */
    bool keys_have_nulls() const {
        for (const auto &c : keystore.cols)
            if (c.has_nulls) return true;
        return false;
    }

    KeyViews keystore_views() const {
        KeyViews kv;
        kv.n = (int32_t)keystore.cols.size();
        for (int i = 0; i < kv.n; i++) kv.col[i] = keystore.view(i);
        return kv;
    }

    int ensure_table(int64_t min_groups, bool force_double = false) {
        if (!force_double && n_slots > 0 && min_groups <= max_fill()) return 0;
        int64_t ns = gx_pow2(std::max<int64_t>(min_groups * 2, 2048));
        /* overflow recovery grows x4: with a badly undersized hint the x2
         * ladder pays a full-chunk insert rerun per step */
        if (force_double) ns = std::max<int64_t>(ns, n_slots * 4);
        if (ns <= n_slots) return 0;
        const int32_t stride = layout.desc.stride;
        DevBuf new_slots, new_records;
        if (new_slots.grow((size_t)ns * sizeof(AggSlot), stream)) return -1;
        HIP_OK(hipMemsetAsync(new_slots.p, 0, (size_t)ns * sizeof(AggSlot), stream));
        if (slot_records) {
            if (new_records.grow((size_t)ns * stride * 8, stream)) return -1;
            if (init_records(new_records.p, 0, ns)) return -1;
        }
        if (n_slots > 0 && d_slots.p) {
            /* migrate occupied slots (incl. pending ones) + their state */
            hipLaunchKernelGGL(k_agg_rehash, dim3(gx_grid(n_slots)), dim3(256),
                               0, stream, (const AggSlot *)d_slots.p, n_slots,
                               (AggSlot *)new_slots.p, (uint32_t)(ns - 1),
                               keystore_views(),
                               (const unsigned long long *)d_records.p,
                               (unsigned long long *)new_records.p,
                               slot_records ? stride : 0,
                               (uint32_t *)d_slot_of_gid.p);
        }
        /* the rehash kernel reads the old table: drain before move
         * assignment returns it to the pool */
        HIP_OK(hipStreamSynchronize(stream));
        d_slots = std::move(new_slots);
        if (slot_records) d_records = std::move(new_records);
        n_slots = ns;
        mask = (uint32_t)(ns - 1);
        return 0;
    }

    /* grow one distinct set's slot array to >= min_slots (pow2), migrating
     * the owners */
    int dist_grow(DistSet &ds, int64_t min_slots) {
        int64_t ns = gx_pow2(std::max<int64_t>(min_slots, 2048));
        if (ns <= ds.n_slots) return 0;
        DevBuf fresh;
        if (fresh.grow((size_t)ns * 8, stream)) return -1;
        HIP_OK(hipMemsetAsync(fresh.p, 0, (size_t)ns * 8, stream));
        if (ds.n_slots > 0 && ds.owners > 0)
            hipLaunchKernelGGL(k_dist_rehash, dim3(gx_grid(ds.n_slots)),
                               dim3(256), 0, stream,
                               (const unsigned long long *)ds.d_slots.p,
                               ds.n_slots, (unsigned long long *)fresh.p,
                               (uint32_t)(ns - 1), (const DistRec *)ds.d_recs.p);
        /* the rehash reads the old array: drain before it returns to the
         * pool */
        HIP_OK(hipStreamSynchronize(stream));
        ds.d_slots = std::move(fresh);
        ds.n_slots = ns;
        return 0;
    }

    /* one chunk through one distinct set; the chunk's gids are final.
     * An error return leaves the set half-updated (n_drows and the SLICE
     * store already cover the chunk, its rows are unresolved): a failed
     * consume poisons the op, as it does for the group table — close it. */
    int distinct_pass(DistSet &ds, const StagedChunk &st, int64_t n,
                      bool no_group_by) {
        /* the claim word carries drow+1 in 32 bits — the group table's own
         * row limit; fail, never wrap */
        if (ds.n_drows + n >= 0xFFFFFFFFll) {
            gx_set_err("DISTINCT set: more than 2^32-2 input rows");
            return -1;
        }
        const int64_t base = ds.n_drows;
        const DevColView in = st.views[ds.input_col];
        if (ds.d_recs.grow((size_t)(base + n) * sizeof(DistRec), stream) ||
            d_dstatus.grow((size_t)n, stream))
            return -1;
        if (!ds.d_ctl.p) {
            if (ds.d_ctl.grow(8, stream)) return -1;
            HIP_OK(hipMemsetAsync(ds.d_ctl.p, 0, 8, stream));
        }
        if (ds.vtype == GX_SLICE) {
            gx_block vb = view_block(in);
            gx_chunk vc;
            vc.n_rows = (int32_t)n;
            vc.n_blocks = 1;
            vc.blocks = &vb;
            if (ds.store.append(&vc)) return -1;
        }
        ds.n_drows = base + n;
        hipLaunchKernelGGL(k_dist_pack, dim3(gx_grid(n)), dim3(256), 0, stream,
                           in, n, base,
                           no_group_by ? nullptr : (const uint32_t *)d_slotidx.p,
                           (const AggSlot *)d_slots.p, (DistRec *)ds.d_recs.p,
                           (uint8_t *)d_dstatus.p);
        /* size by ACTUAL occupancy (+ headroom; the overflow retry covers
         * the rest) — a chunk of duplicates must not buy a table sized for
         * "every row is new". Small chunks reserve their worst case, as
         * the group table does, so CHUNK_SIZE streams never retry. */
        const int64_t headroom = n < (int64_t)(1 << 18) ? n : 1024;
        int64_t want = ((int64_t)ds.owners + headroom) * 2;
        if (ds.n_slots == 0) /* every group holds at least one pair */
            want = std::max<int64_t>(want, cfg.expected_groups * 2);
        if (dist_grow(ds, want)) return -1;

        DistInsertParams IP;
        std::memset(&IP, 0, sizeof(IP));
        IP.vtype = ds.vtype;
        IP.base_drow = base;
        IP.n = n;
        IP.status = (uint8_t *)d_dstatus.p;
        IP.ctl = (uint32_t *)ds.d_ctl.p;
        /* every agg of the set reads ds.input_col, i.e. `in` */
        fill_accum_params(IP.A, st, ds.agg_idx.data(),
                          (int)ds.agg_idx.size());
        for (int attempt = 0;; attempt++) {
            IP.slots = (unsigned long long *)ds.d_slots.p;
            IP.mask = (uint32_t)(ds.n_slots - 1);
            IP.recs = (const DistRec *)ds.d_recs.p;
            if (ds.vtype == GX_SLICE) IP.store = ds.store.view(0);
            hipLaunchKernelGGL(k_dist_insert, dim3(gx_grid(n)), dim3(256), 0,
                               stream, IP);
            uint32_t ctl[2] = {0, 0};
            HIP_OK(hipMemcpyAsync(ctl, ds.d_ctl.p, 8, hipMemcpyDeviceToHost,
                                  stream));
            HIP_OK(hipStreamSynchronize(stream));
            ds.owners = ctl[1];
            if (!ctl[0]) break;
            if (attempt > 40) { gx_set_err("distinct set overflow loop"); return -1; }
            HIP_OK(hipMemsetAsync(ds.d_ctl.p, 0, 4, stream));
            /* x4, as the group table's overflow recovery */
            if (dist_grow(ds, std::max<int64_t>(ds.n_slots * 4,
                                                (int64_t)ds.owners * 4)))
                return -1;
        }
        return 0;
    }

    /* the accumulate pass of one chunk through k_agg_accumulate_local[_dec];
     * the caller has checked n_groups_host <= local_cap */
    int launch_local(const AggAccumParams &AP, int64_t n) {
        if (local_cus == 0) {
            int v = 0;
            HIP_OK(hipDeviceGetAttribute(
                &v, hipDeviceAttributeMultiprocessorCount, device));
            local_cus = v > 0 ? v : 1;
        }
        AggLocalParams LP;
        LP.A = AP;
        LP.groups = (int32_t)n_groups_host;
        std::memcpy(LP.tmpl, layout.tmpl, sizeof(LP.tmpl));
        const int32_t stride = layout.desc.stride;
        /* as many replicas as the LDS budget holds, up to the maximum (Q1's
         * 22-u64 record x 4 groups: 16; 128 groups of it: 1) */
        int32_t rep = 1;
        while (rep * 2 <= local_rep_max &&
               agg_local_lds_bytes(LP.groups, stride, rep * 2) <=
                   GX_AGG_LOCAL_LDS_BYTES)
            rep *= 2;
        LP.replicas = rep;
        const size_t lds = agg_local_lds_bytes(LP.groups, stride, rep);
        if (lds > GX_AGG_LOCAL_LDS_BYTES) {
            gx_set_err("agg local: state does not fit the LDS budget");
            return -1;
        }
        /* a block flushes touched groups x stride atomics once: give it
         * GX_AGG_LOCAL_BLOCK_ROWS rows or more to spread them over, and at
         * most GX_AGG_LOCAL_BLOCKS_PER_CU resident blocks' worth of blocks */
        const int64_t by_rows =
            (n + GX_AGG_LOCAL_BLOCK_ROWS - 1) / GX_AGG_LOCAL_BLOCK_ROWS;
        const int64_t blocks = std::max<int64_t>(
            1, std::min<int64_t>(by_rows, (int64_t)local_cus *
                                              GX_AGG_LOCAL_BLOCKS_PER_CU));
        auto k_local = has_dec ? k_agg_accumulate_local_dec
                               : k_agg_accumulate_local;
        hipLaunchKernelGGL(k_local, dim3((unsigned)blocks), dim3(256), lds,
                           stream, LP);
        HIP_OK(hipGetLastError());
        local_rows += n;
        local_launches++;
        local_replicas = rep;
        return 0;
    }

    int consume(const gx_chunk *ch) {
        if (ensure_device(device)) return -1;
        if ((int32_t)aggs.size() > GX_MAX_COLS) { gx_set_err("too many aggs"); return -1; }
        const int64_t n = ch->n_rows;
        if (n == 0) return 0;

        StagedChunk st;
        if (st.stage(ch, stream)) return -1;

        if (!ev0) {
            HIP_OK(hipEventCreate(&ev0));
            HIP_OK(hipEventCreate(&ev1));
        }
        HIP_OK(hipEventRecord(ev0, stream));
        if (has_dec_input && !d_decerr.p) {
            if (d_decerr.grow(4, stream)) return -1;
            HIP_OK(hipMemsetAsync(d_decerr.p, 0, 4, stream));
        }

        const bool no_group_by = group_cols_.empty();
        int64_t base_krow = keystore.n_rows;

        if (!no_group_by) {
            /* append key columns (for emit + generic compare) */
            std::vector<gx_block> kb;
            for (int32_t gc : group_cols_) kb.push_back(view_block(st.views[gc]));
            gx_chunk kc;
            kc.n_rows = (int32_t)n;
            kc.n_blocks = (int32_t)kb.size();
            kc.blocks = kb.data();
            if (keystore.append(&kc)) return -1;

            if (d_hashes.grow((size_t)n * 4, stream) ||
                d_slotidx.grow((size_t)n * 4, stream)) return -1;
            KeyViews chunk_keys;
            chunk_keys.n = (int32_t)group_cols_.size();
            for (size_t i = 0; i < group_cols_.size(); i++)
                chunk_keys.col[i] = st.views[group_cols_[i]];

            if (use_packed) {
                if (d_packed.grow((size_t)(base_krow + n) * sizeof(PackedKey), stream) ||
                    d_nullmask.grow((size_t)(base_krow + n), stream))
                    return -1;
                hipLaunchKernelGGL(k_agg_pack, dim3(gx_grid(n)), dim3(256), 0,
                                   stream, chunk_keys, n, base_krow,
                                   (PackedKey *)d_packed.p,
                                   (uint8_t *)d_nullmask.p, (int32_t *)d_hashes.p);
            } else {
                /* generic: hashes only; compare goes via keystore columns */
                hipLaunchKernelGGL(k_agg_hash, dim3(gx_grid(n)), dim3(256), 0,
                                   stream, chunk_keys, n, (int32_t *)d_hashes.p);
            }

            /* size by ACTUAL groups so far (+chunk-bounded headroom via the
             * overflow retry) — sizing for "every row could be a group"
             * built a 32 GB table for a 600M-row chunk */
            const bool small_chunk = n < (int64_t)(1 << 18);
            if (small_chunk) {
                /* inline gids need capacity for the worst case up front */
                if (ensure_table((int64_t)n_groups_host + n)) return -1;
                if (ensure_group_cap((int64_t)n_groups_host + n)) return -1;
            } else {
                if (ensure_table((int64_t)n_groups_host + 1024)) return -1;
            }
            if (d_total.grow(12, stream)) return -1;
            if (small_chunk)
                /* once, BEFORE the overflow-retry loop: gids assigned in a
                 * partial attempt must not be reissued on the rerun */
                HIP_OK(hipMemcpyAsync((char *)d_total.p + 8, &n_groups_host,
                                      4, hipMemcpyHostToDevice, stream));

            for (int attempt = 0;; attempt++) {
                HIP_OK(hipMemsetAsync((char *)d_total.p + 4, 0, 4, stream));
                AggInsertParams IP;
                std::memset(&IP, 0, sizeof(IP));
                IP.slots = (AggSlot *)d_slots.p;
                IP.mask = mask;
                IP.use_packed = (int)use_packed;
                IP.packed = (const PackedKey *)d_packed.p;
                IP.nullmask = keys_have_nulls()
                                  ? (const uint8_t *)d_nullmask.p : nullptr;
                IP.keystore = keystore_views();
                IP.hashes = (const int32_t *)d_hashes.p;
                IP.base_krow = base_krow;
                IP.n = n;
                IP.overflow = (uint32_t *)d_total.p + 1;
                IP.inline_gid = small_chunk ? 1 : 0;
                IP.ngroups = (uint32_t *)d_total.p + 2;
                IP.krow_of_gid = (uint32_t *)d_krow_of_gid.p;
                IP.slot_of_gid = (uint32_t *)d_slot_of_gid.p;
                IP.slot_of_row = (uint32_t *)d_slotidx.p;
                IP.fuse_accum = (int)slot_records;
                IP.only_failed = (slot_records && attempt > 0) ? 1 : 0;
                if (slot_records)
                    fill_accum_params(IP.A, st); /* records ptr per attempt
                                                    (rehash reallocates) */
                auto k_insert = slot_records && has_dec ? k_agg_insert_dec
                                                        : k_agg_insert;
                hipLaunchKernelGGL(k_insert, dim3(gx_grid(n)), dim3(256), 0,
                                   stream, IP);
                uint32_t ovf = 0;
                HIP_OK(hipMemcpyAsync(&ovf, (char *)d_total.p + 4, 4,
                                      hipMemcpyDeviceToHost, stream));
                HIP_OK(hipStreamSynchronize(stream));
                if (!ovf) break;
                if (attempt > 40) { gx_set_err("agg table overflow loop"); return -1; }
                if (ensure_table(0, /*force_double=*/true)) return -1;
            }

            if (small_chunk) {
                uint32_t total = 0;
                HIP_OK(hipMemcpyAsync(&total, (char *)d_total.p + 8, 4,
                                      hipMemcpyDeviceToHost, stream));
                HIP_OK(hipStreamSynchronize(stream));
                n_groups_host = total;
                goto accumulate;
            }
            {
            /* dense gid compaction over the slot table (no hot counter) */
            int64_t n_tiles = (n_slots + GX_GID_TILE - 1) / GX_GID_TILE;
            if (d_tiles.grow((size_t)n_tiles * 4, stream)) return -1;
            hipLaunchKernelGGL(k_agg_gid_count,
                               dim3((int)std::min<int64_t>(n_tiles, 4096)),
                               dim3(256), 0, stream,
                               (const AggSlot *)d_slots.p, n_slots,
                               (uint32_t *)d_tiles.p);
            hipLaunchKernelGGL(k_agg_gid_scan, dim3(1), dim3(1024), 0, stream,
                               (uint32_t *)d_tiles.p, n_tiles, n_groups_host,
                               (uint32_t *)d_total.p);
            uint32_t total = 0;
            HIP_OK(hipMemcpyAsync(&total, d_total.p, 4,
                                  hipMemcpyDeviceToHost, stream));
            HIP_OK(hipStreamSynchronize(stream));
            /* grow per-group state only now that the real count is known */
            if (ensure_group_cap(total)) return -1;
            hipLaunchKernelGGL(k_agg_gid_assign,
                               dim3((int)std::min<int64_t>(n_tiles, 4096)),
                               dim3(256), 0, stream,
                               (AggSlot *)d_slots.p, n_slots,
                               (const uint32_t *)d_tiles.p,
                               (uint32_t *)d_krow_of_gid.p,
                               (uint32_t *)d_slot_of_gid.p);
            n_groups_host = total;
            }
        accumulate:;
        } else {
            if (!global_agg_seeded) {
                if (ensure_group_cap(1)) return -1;
                n_groups_host = 1;
                global_agg_seeded = true;
            }
        }

        if (!slot_records) {
            /* gid-indexed state: separate accumulate pass (wide-state aggs
             * and the global aggregate) */
            AggAccumParams AP;
            std::memset(&AP, 0, sizeof(AP));
            AP.slots = (const AggSlot *)d_slots.p;
            AP.slot_records = 0;
            AP.slot_of_row = (const uint32_t *)d_slotidx.p;
            AP.mask = mask;
            AP.use_packed = (int)use_packed;
            AP.packed = (const PackedKey *)d_packed.p;
            AP.nullmask = keys_have_nulls()
                              ? (const uint8_t *)d_nullmask.p : nullptr;
            AP.keystore = keystore_views();
            AP.hashes = (const int32_t *)d_hashes.p;
            AP.base_krow = base_krow;
            AP.n = n;
            AP.global_group = (int)no_group_by;
            /* the distinct aggs are fed by the distinct pass */
            const int32_t k = (int32_t)plain_idx.size();
            fill_accum_params(AP, st, plain_idx.data(), k);
            auto k_accum = has_dec ? k_agg_accumulate_dec : k_agg_accumulate;
            /* few groups: accumulate block-local in LDS. n_groups_host
             * covers this chunk's gids (assigned above), so every row fits */
            const bool local =
                local_mode != 0 && k > 0 && n_groups_host >= 1 &&
                (int64_t)n_groups_host <= local_cap &&
                (local_mode == 1 || n >= GX_AGG_LOCAL_MIN_ROWS ||
                 (n >= GX_AGG_LOCAL_MIN_ROWS_FEW &&
                  n_groups_host <= GX_AGG_LOCAL_FEW_GROUPS));
            if (local) {
                if (launch_local(AP, n)) return -1;
            } else if (k > 0 || !has_distinct)
                hipLaunchKernelGGL(k_accum, dim3(gx_grid(n)), dim3(256), 0,
                                   stream, AP);
        }
        for (auto &ds : dsets)
            if (distinct_pass(ds, st, n, no_group_by)) return -1;
        HIP_OK(hipEventRecord(ev1, stream));
        uint32_t dec_fence = 0;
        if (has_dec_input)
            HIP_OK(hipMemcpyAsync(&dec_fence, d_decerr.p, 4,
                                  hipMemcpyDeviceToHost, stream));
        HIP_OK(hipStreamSynchronize(stream));
        if (dec_fence) {
            /* sticky on the device as well: the op is poisoned, like after
             * any failed consume */
            std::string what;
            if (dec_fence & GX_DEC_FENCE_FRAC)
                what += " [fractions fence: a value has more fraction "
                        "digits than the aggregate's scale]";
            if (dec_fence & GX_DEC_FENCE_WORDS)
                what += " [words fence: a record has more than 9 base-1e9 "
                        "words]";
            if (dec_fence & GX_DEC_FENCE_MAG)
                what += " [magnitude fence: |value x 10^scale| >= 10^29]";
            gx_set_err("SUM_DEC/AVG_DEC DECIMAL input rejected:" + what);
            return -1;
        }
        {
            float ms = 0;
            HIP_OK(hipEventElapsedTime(&ms, ev0, ev1));
            kernel_ms += ms;
            consumes++;
            rows_total += n;
        }
        return 0;
    }

    int next(gx_result **out) {
        *out = nullptr;
        if (emitted) return 0;
        emitted = true;
        if (ensure_device(device)) return -1;
        if (group_cols_.empty() && !global_agg_seeded) {
            /* SQL global aggregate over EMPTY input still emits one row
             * (COUNT=0, null-init aggs NULL) — consume() never ran, so
             * seed group 0 here (HashAggExec no-group-by contract; the
             * oracle emits the row; caught by deep-fuzz seed 100229) */
            if (ensure_group_cap(1)) return -1;
            n_groups_host = 1;
            global_agg_seeded = true;
        }
        const uint32_t ng = n_groups_host;
        std::vector<int32_t> otypes;
        for (int32_t gc : group_cols_) otypes.push_back(input_types[gc]);
        for (auto &sp : aggs) otypes.push_back(agg_func_result_type(sp.func));
        auto h = alloc_result_cols(otypes, ng, device, stream);
        if (!h) return -1;
        if (ng > 0) {
            AggEmitParams EP;
            std::memset(&EP, 0, sizeof(EP));
            size_t col = 0;
            /* packed null-free keys ride along in k_agg_emit */
            const bool packed_keys = use_packed && !keys_have_nulls();
            if (packed_keys) {
                EP.n_keys = (int32_t)group_cols_.size();
                EP.packed = (const PackedKey *)d_packed.p;
                EP.krow_of_gid = (const uint32_t *)d_krow_of_gid.p;
            }
            for (size_t kc = 0; kc < group_cols_.size(); kc++) {
                if (packed_keys) {
                    EP.key_type[kc] = otypes[kc];
                    EP.key_vals[kc] = h->bufs[col * 2].p;
                    EP.key_nulls[kc] = (uint8_t *)h->bufs[col * 2 + 1].p;
                    col++;
                    continue;
                }
                DevColView kv = keystore.view((int32_t)kc);
                if (kv.type == GX_SLICE) {
                    if (gather_slice_col(kv, (const uint32_t *)d_krow_of_gid.p,
                                         0, ng, h.get(), col,
                                         d_tiles /* reuse */, stream))
                        return -1;
                    col++;
                    continue;
                }
                hipLaunchKernelGGL(k_gather, dim3(gx_grid(ng)), dim3(256), 0, stream,
                                   kv,
                                   (const uint32_t *)d_krow_of_gid.p, (int64_t)ng,
                                   h->bufs[col * 2].p, (uint8_t *)h->bufs[col * 2 + 1].p, 0);
                col++;
            }
            EP.records = (const unsigned long long *)d_records.p;
            EP.n_groups = ng;
            EP.slot_of_gid = slot_records ? (const uint32_t *)d_slot_of_gid.p
                                          : nullptr;
            EP.R = layout.desc;
            for (size_t a = 0; a < aggs.size(); a++) {
                EP.dec_scale[a] = dec_scale[a];
                EP.out_vals[a] = h->bufs[col * 2].p;
                EP.out_nulls[a] = (uint8_t *)h->bufs[col * 2 + 1].p;
                col++;
            }
            if (EP.R.n_aggs > 0 || EP.n_keys > 0)
                hipLaunchKernelGGL(k_agg_emit, dim3(gx_grid(ng)), dim3(256), 0,
                                   stream, EP);
            HIP_OK(hipStreamSynchronize(stream));
        }
        give_result(std::move(h), out);
        return 0;
    }
};

} // namespace

extern "C" {

gx_op *gxop_agg_create(const gx_agg_cfg *cfg) {
    if (cfg)
        for (int32_t i = 0; i < cfg->n_aggs; i++) {
            int32_t f = cfg->aggs[i].func;
            if (agg_distinct_base(f) >= 0) {
                const int32_t col = cfg->aggs[i].input_col;
                if (col < 0 || col >= cfg->n_input_cols) {
                    gx_set_err("DISTINCT agg " + std::to_string(i) +
                               ": input_col " + std::to_string(col) +
                               " out of range");
                    return nullptr;
                }
                const int32_t t = cfg->input_types[col];
                const bool integral = t == GX_I64 || t == GX_I32;
                bool ok;
                switch (f) {
                case GX_AGG_COUNT_DISTINCT:
                    ok = integral || t == GX_F64 || t == GX_SLICE; break;
                case GX_AGG_SUM_I64_DISTINCT: case GX_AGG_SUM_I64N_DISTINCT:
                    ok = integral; break;
                default: /* SUM_F64 / AVG_F64 convert integers */
                    ok = integral || t == GX_F64; break;
                }
                if (!ok) {
                    gx_set_err("DISTINCT agg " + std::to_string(i) +
                               ": func " + std::to_string(f) +
                               " does not take input type " +
                               std::to_string(t));
                    return nullptr;
                }
                continue;
            }
            if (agg_func_is_dec(f & 0xFFFF)) {
                /* the input's decimal scale rides in the upper 16 bits */
                const int32_t base = f & 0xFFFF;
                const uint32_t scale = (uint32_t)f >> 16;
                const int32_t col = cfg->aggs[i].input_col;
                const char *name = base == GX_AGG_SUM_DEC ? "SUM_DEC"
                                                          : "AVG_DEC";
                if (scale > 9u) {
                    gx_set_err(std::string(name) + " agg " +
                               std::to_string(i) + ": scale " +
                               std::to_string(scale) +
                               " not supported (0..9, one fraction word)");
                    return nullptr;
                }
                if (base == GX_AGG_AVG_DEC && scale > 4u) {
                    gx_set_err("AVG_DEC agg " + std::to_string(i) +
                               ": scale " + std::to_string(scale) +
                               " not supported (the result has scale 4: "
                               "input scale 0..4)");
                    return nullptr;
                }
                if (col < 0 || col >= cfg->n_input_cols) {
                    gx_set_err(std::string(name) + " agg " +
                               std::to_string(i) + ": input_col " +
                               std::to_string(col) + " out of range");
                    return nullptr;
                }
                const int32_t t = cfg->input_types[col];
                if (t != GX_I64 && t != GX_I32 && t != GX_DECIMAL) {
                    gx_set_err(std::string(name) + " agg " +
                               std::to_string(i) +
                               ": does not take input type " +
                               std::to_string(t) +
                               " (I64, I32 or DECIMAL)");
                    return nullptr;
                }
                continue;
            }
            if ((f < GX_AGG_COUNT_ROW || f > GX_AGG_BIT_XOR) &&
                f != GX_AGG_SUM_I64N) {
                gx_set_err("unknown or window-only agg func in group-by");
                return nullptr;
            }
        }
    if (!cfg || cfg->n_aggs > GX_MAX_COLS || cfg->n_group_cols > GX_MAX_KEYS) {
        gx_set_err("bad agg cfg");
        return nullptr;
    }
    if (cfg->device < 0) { gx_set_err("gxhip requires a GPU device"); return nullptr; }
    HIP_OK_NULL(hipSetDevice(cfg->device));
    AggOp *op = new AggOp(cfg);
    if (cfg->expected_groups > 0) {
        if (op->ensure_table(cfg->expected_groups) ||
            op->ensure_group_cap(cfg->expected_groups)) {
            delete op;
            return nullptr;
        }
    }
    return op;
}
int gxop_agg_consume(gx_op *op, const gx_chunk *c) {
    if (!op || op->kind != OP_AGG) { gx_set_err("not an agg op"); return -1; }
    return static_cast<AggOp *>(op)->consume(c);
}
int gxop_agg_build(gx_op *op) {
    if (!op || op->kind != OP_AGG) { gx_set_err("not an agg op"); return -1; }
    return 0; /* streaming: nothing to finalize */
}
int gxop_agg_next(gx_op *op, gx_result **out) {
    if (!op || op->kind != OP_AGG) { gx_set_err("not an agg op"); return -1; }
    return static_cast<AggOp *>(op)->next(out);
}
int gxop_agg_close(gx_op *op) { delete op; return 0; }

int gxop_agg_get_stats(gx_op *op, gx_agg_stats *out) {
    if (!op || op->kind != OP_AGG || !out) { gx_set_err("not an agg op"); return -1; }
    AggOp *a = static_cast<AggOp *>(op);
    out->kernel_ms = a->kernel_ms;
    out->consumes = a->consumes;
    out->rows = a->rows_total;
    out->groups = a->n_groups_host;
    return 0;
}

int gxop_agg_get_local_stats(gx_op *op, gx_agg_local_stats *out) {
    if (!op || op->kind != OP_AGG || !out) { gx_set_err("not an agg op"); return -1; }
    AggOp *a = static_cast<AggOp *>(op);
    out->local_rows = a->local_rows;
    out->local_launches = a->local_launches;
    out->local_groups_cap = a->local_cap;
    out->replicas = a->local_replicas;
    return 0;
}

} /* extern "C" */

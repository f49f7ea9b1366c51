/*
 * gxhip_groupjoin.inc — fused group-join (included by gxhip.hip after
 * gxhip_agg.inc: per-position state records laid out by gx_agg_layout.h,
 * accumulated by agg_apply and initialized by agg_launch_init, and JoinOp's
 * CSR build + pair-probe).
 *
 * Restates HashGroupJoinExec (operator/HashGroupJoinExec.java): one group
 * per CONSUMED-side row position, matched by null-safe Chunk.equals
 * (buildOneChunk:296-311 inserts every row); each matching probe row
 * accumulates into that position's aggregators (buildJoinRow:469-490).
 * This is the Q18 shape fused: the group id IS the build position, so the
 * whole agg hash table (insert/claims/gid compaction) disappears — the
 * join probe's matched position doubles as the aggregation slot.
 *
 * INNER emits matched positions; LEFT emits all positions, the unmatched
 * ones as one null-row accumulation (buildNullRow: COUNT(*)=1,
 * COUNT(col)=0, SUM/MIN/MAX=NULL).
 *
 * Three table layouts, chosen at do_build: the CSR (any keys, null-safe),
 * the wide CSR entries (one non-null I64 key, <= 2 COUNT/SUM_I64 aggs) and
 * the plain joins' inline-bucket table + bloom (one non-null I64 key, any
 * other aggregate list), which the fused probe-scan kernel of
 * gxhip_scan.inc (gxop_groupjoin_probe_scan) walks.
 */

namespace {

/* Direct-accumulate probe: the CSR lookup and the aggregation happen in
 * ONE pass — no (probe,build) pair list ever touches HBM. Measured on
 * MI355X (tools/bench_gj.py, 600M probes / 147M groups): the pair-list
 * variant spent 99.6 ms on probe+accumulate (4.8 GB pair write + read +
 * a second random pass); this kernel replaces it. Match logic mirrors
 * k_probe's INNER fast/generic paths. */
/* WIDE mode: for the Q18-shaped fast case (single non-null I64 key,
 * <=2 aggregators from {COUNT_ROW, COUNT_COL, SUM_I64} -- no null-seen
 * slots), the per-group state lives INSIDE the 32-B CSR entry, so the key
 * compare and the accumulate RMW touch the SAME 64-B line: ~2 random
 * lines/row instead of ~3. Measured step: see profiles/README.md. */
struct __align__(16) GJWideEntry {
    int64_t key;
    uint32_t pos;
    uint32_t used;
    unsigned long long s[2];
};

__global__ void k_gjw_expand(const JoinEntry *entries, int64_t n,
                             DevColView keycol, GJWideEntry *wide,
                             unsigned long long s0, unsigned long long s1) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        JoinEntry e = entries[i];
        GJWideEntry w;
        w.key = ((const int64_t *)keycol.values)[e.pos];
        w.pos = e.pos;
        w.used = 0;
        w.s[0] = s0;
        w.s[1] = s1;
        wide[i] = w;
    }
}

/* add a lane's match count to the op's cumulative counter: summed across
 * the wave first, so the counter takes one atomic per wave */
__device__ static inline void gj_count_matches(unsigned long long *ctr,
                                               uint32_t mine) {
    for (int off = 32; off; off >>= 1)
        mine += (uint32_t)__shfl_down((int)mine, off, 64);
    if ((threadIdx.x & 63) == 0 && mine)
        atomicAdd(ctr, (unsigned long long)mine);
}

struct GJWideProbeParams {
    unsigned long long *matches;
    const uint32_t *starts;
    GJWideEntry *wide;
    uint32_t mask;
    int64_t n;
    const int32_t *hashes;
    DevColView probe_key;          /* single I64 col (may carry nulls) */
    int32_t n_aggs;
    int32_t func[2];
    DevColView input[2];
};

__global__ void k_gjw_probe(GJWideProbeParams P) {
    uint32_t n_match = 0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < P.n;
         i += (int64_t)gridDim.x * blockDim.x) {
        /* build side has no null keys in wide mode; a null probe key
         * matches nothing */
        if (col_is_null(P.probe_key, i)) continue;
        int64_t want = ((const int64_t *)P.probe_key.values)[i];
        uint32_t b = (uint32_t)gx_mix(P.hashes[i]) & P.mask;
        uint32_t it = P.starts[b], end = P.starts[b + 1];
        for (; it < end; it++) {
            GJWideEntry *w = &P.wide[it];
            if (w->key != want) continue;
            n_match++;
            if (w->used == 0) atomicOr(&w->used, 1u);
            for (int a = 0; a < P.n_aggs; a++) {
                switch (P.func[a]) {
                case GX_AGG_COUNT_ROW:
                    atomicAdd(&w->s[a], 1ull);
                    break;
                case GX_AGG_COUNT_COL:
                    if (!col_is_null(P.input[a], i)) atomicAdd(&w->s[a], 1ull);
                    break;
                default: /* GX_AGG_SUM_I64 */
                    if (!col_is_null(P.input[a], i)) {
                        const DevColView &c = P.input[a];
                        int64_t v = c.type == GX_I32
                            ? (int64_t)((const int32_t *)c.values)[i]
                            : ((const int64_t *)c.values)[i];
                        atomicAdd(&w->s[a], (unsigned long long)v);
                    }
                    break;
                }
            }
        }
    }
    gj_count_matches(P.matches, n_match);
}

/* scatter wide-entry state back into the per-position records + used
 * bitmap so the shared emission path runs unchanged */
__global__ void k_gjw_unpack(const GJWideEntry *wide, int64_t n,
                             unsigned long long *records, int32_t stride,
                             int32_t off0, int32_t off1, int32_t n_aggs,
                             uint32_t *used) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        GJWideEntry w = wide[i];
        unsigned long long *rec = records + (size_t)w.pos * stride;
        rec[off0] = w.s[0];
        if (n_aggs > 1) rec[off1] = w.s[1];
        if (w.used) atomicOr(&used[w.pos >> 5], 1u << (w.pos & 31));
    }
}

struct GJProbeParams {
    const uint32_t *starts;
    const JoinEntry *entries;
    uint32_t mask;
    int64_t n;
    const int32_t *hashes;
    int fast_i64;
    KeyViews build_keys, probe_keys;
    uint32_t *used;
    unsigned long long *matches;
    AggAccumParams A;
};

__global__ void k_gj_probe(GJProbeParams P) {
    uint32_t n_match = 0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < P.n;
         i += (int64_t)gridDim.x * blockDim.x) {
        uint32_t b = (uint32_t)gx_mix(P.hashes[i]) & P.mask;
        uint32_t it = P.starts[b], end = P.starts[b + 1];
        int64_t want_key = 0;
        if (P.fast_i64)
            want_key = ((const int64_t *)P.probe_keys.col[0].values)[i];
        for (; it < end; it++) {
            JoinEntry e = P.entries[it];
            bool is_match;
            if (P.fast_i64)
                is_match = (e.key == want_key);
            else
                is_match = ((int32_t)e.key == P.hashes[i]) &&
                           rows_key_equal(P.build_keys, e.pos,
                                          P.probe_keys, i);
            if (!is_match) continue;
            n_match++;
            uint32_t w = 1u << (e.pos & 31);
            if ((P.used[e.pos >> 5] & w) == 0)   /* test-then-set: one RMW */
                atomicOr(&P.used[e.pos >> 5], w);
            agg_apply(P.A, e.pos, i);
        }
    }
    gj_count_matches(P.matches, n_match);
}

/* Plain probe of an op whose build chose the inline-bucket table (see
 * GroupJoinOp::do_build): one materialized probe row per lane, the bucket
 * found from the key itself, no k_hash_rows pass. The build side carries
 * no NULL key there, so a NULL probe key matches nothing. */
struct GJInlineProbeParams {
    const JoinEntry *table;
    const JoinEntry *entries;   /* overflow runs */
    uint32_t mask;
    int64_t n;
    DevColView probe_key;
    uint32_t *used;             /* NULL: COUNT(*) says "matched" */
    unsigned long long *matches;
    AggAccumParams A;
};

__global__ void k_gj_probe_inline(GJInlineProbeParams P) {
    uint32_t n_match = 0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < P.n;
         i += (int64_t)gridDim.x * blockDim.x) {
        if (col_is_null(P.probe_key, i)) continue;
        const int64_t want = ((const int64_t *)P.probe_key.values)[i];
        const uint64_t ebase =
            (uint64_t)((uint32_t)gx_mix(gx_hash_i64(want)) & P.mask) * 4;
        const uint32_t end = P.table[ebase].pad;
        const uint32_t ovf0 = end > 4 ? P.table[ebase + 1].pad : 0u;
        for (uint32_t it = 0; it < end; it++) {
            const JoinEntry e = it < 4 ? P.table[ebase + it]
                                       : P.entries[ovf0 + (it - 4)];
            if (e.key != want) continue;
            n_match++;
            uint32_t w = 1u << (e.pos & 31);
            if (P.used && (P.used[e.pos >> 5] & w) == 0)
                atomicOr(&P.used[e.pos >> 5], w);
            agg_apply(P.A, e.pos, i);
        }
    }
    gj_count_matches(P.matches, n_match);
}

/* matched = the position's used-bit, or where the op keeps none
 * (count_off >= 0) a non-zero COUNT(*) word of its record */
__device__ static inline bool gj_matched(const unsigned long long *rec,
                                         const uint32_t *used,
                                         int32_t count_off, uint32_t g) {
    return count_off >= 0 ? rec[count_off] != 0ull
                          : (used[g >> 5] >> (g & 31)) & 1u;
}

/* compact the matched positions (INNER emission list), with per-wave LDS
 * staging so the global counter sees 1 atomic per 512 hits. Matched = the
 * used-bit, or where the op keeps none (count_off >= 0) a non-zero
 * COUNT(*) word of the position's record. */
__global__ void k_gj_compact(const uint32_t *used,
                             const unsigned long long *records,
                             int32_t rec_stride, int32_t count_off,
                             int64_t n, uint32_t *out, uint32_t *counter) {
    __shared__ uint32_t s_rows[4][GX_EMIT_STAGE];
    const int wid = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    uint32_t *stage = s_rows[wid];
    uint32_t cnt = 0;

    auto flush = [&]() {
        if (cnt == 0) return;
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(counter, cnt);
        base = (uint32_t)__shfl((int)base, 0, 64);
        for (uint32_t k = (uint32_t)lane; k < cnt; k += 64)
            out[base + k] = stage[k];
        cnt = 0;
    };

    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;;
         i += stride) {
        bool active = i < n;
        if (!__ballot(active)) break;
        bool want = false;
        if (active)
            want = gj_matched(records + (size_t)i * rec_stride, used,
                              count_off, (uint32_t)i);
        unsigned long long m = __ballot(want);
        uint32_t add = (uint32_t)__popcll(m);
        if (cnt + add > GX_EMIT_STAGE) flush();
        if (want)
            stage[cnt + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] =
                (uint32_t)i;
        cnt += add;
    }
    flush();
}

/* emit one agg value column (8-B values: I64 results and F64 bit patterns
 * alike) for the listed records: output row i reads record idx[i], or
 * record i where idx == NULL (LEFT). count_row_null_row: add 1 to COUNT(*)
 * of unmatched groups (buildNullRow's null-row accumulation); `used` and
 * count_off are read only then. */
__global__ void k_agg_emit_col(const unsigned long long *records,
                               int32_t stride, int32_t val_off,
                               int32_t seen_off, int32_t func,
                               const uint32_t *idx, const uint32_t *used,
                               int32_t count_off, int count_row_null_row,
                               int64_t n, void *out_vals,
                               uint8_t *out_nulls) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        uint32_t g = idx ? idx[i] : (uint32_t)i;
        const unsigned long long *rec = records + (size_t)g * stride;
        AggDecoded d = agg_decode(func, rec, val_off, seen_off);
        out_nulls[i] = d.isnull;
        if (count_row_null_row && func == GX_AGG_COUNT_ROW &&
            !gj_matched(rec, used, count_off, g))
            d.bits += 1;
        ((unsigned long long *)out_vals)[i] = d.bits;
    }
}

/* One-kernel emission for fixed-width group columns: per emitted position
 * the record (one random line) is read once and every key and aggregate
 * column written from it. Same values as k_gather + k_agg_emit_col; an output
 * whose nulls pointer is NULL (null-free source column, aggregate without
 * a seen slot) skips the null store. */
struct GJEmitParams {
    const unsigned long long *records;
    AggRecDesc R;
    const uint32_t *idx;            /* NULL = positions 0..n-1 (LEFT) */
    const uint32_t *used;
    int32_t count_off;              /* >= 0: matched = that word != 0 */
    int count_row_null_row;
    int64_t n;
    int32_t n_keys;
    DevColView key_src[GX_MAX_COLS];
    int32_t key_words[GX_MAX_COLS]; /* element size in 4-B words */
    void *key_vals[GX_MAX_COLS];
    uint8_t *key_nulls[GX_MAX_COLS];
    void *agg_vals[GX_MAX_COLS];
    uint8_t *agg_nulls[GX_MAX_COLS];
};

__global__ void k_gj_emit_all(GJEmitParams P) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < P.n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t g = P.idx ? P.idx[i] : (uint32_t)i;
        for (int k = 0; k < P.n_keys; k++) {
            const DevColView &src = P.key_src[k];
            const bool nn = col_is_null(src, g);
            if (P.key_nulls[k]) P.key_nulls[k][i] = nn;
            const int32_t w = P.key_words[k];
            const uint32_t *sv = (const uint32_t *)src.values + (size_t)g * w;
            uint32_t *dv = (uint32_t *)P.key_vals[k] + (size_t)i * w;
            for (int32_t j = 0; j < w; j++) dv[j] = nn ? 0u : sv[j];
        }
        const unsigned long long *rec = P.records + (size_t)g * P.R.stride;
        const bool matched = gj_matched(rec, P.used, P.count_off, g);
        for (int a = 0; a < P.R.n_aggs; a++) {
            const int32_t func = P.R.func[a];
            AggDecoded d = agg_decode(func, rec, P.R.val_off[a],
                                      P.R.seen_off[a]);
            if (P.agg_nulls[a]) P.agg_nulls[a][i] = d.isnull;
            if (func == GX_AGG_COUNT_ROW && !matched && P.count_row_null_row)
                d.bits += 1;
            /* I64 results and F64 bit patterns alike */
            ((unsigned long long *)P.agg_vals[a])[i] = d.bits;
        }
    }
}

struct GroupJoinOp : gx_op {
    gx_groupjoin_cfg cfg;
    std::vector<gx_equi_key> keys;
    std::vector<int32_t> build_types, probe_types, group_cols_;
    std::vector<gx_agg_spec> aggs;

    /* last-allocated first (see DevBuf: destruction order and the pool) */
    DevBuf d_accum;          /* GJAccum for the probe-scan kernel */
    DevBuf d_wide;
    DevBuf d_pn, d_ph, d_gj_tmp, d_cnt, d_gidx, d_used, d_records;
    DevBuf d_meta;           /* u64 cumulative matches, u32 scan survivors */
    std::unique_ptr<JoinOp> jop; /* CSR build (null-safe hashing) */
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    double kernel_ms = 0.0;
    int64_t rows_total = 0, probe_launches = 0, matches_total = 0;
    AggLayout layout;        /* the per-position state record, over aggs[] */
    bool built = false, emitted = false;
    bool wide_ok = false;    /* cfg allows wide mode */
    bool wide = false;       /* chosen at do_build (needs null-free keys) */
    /* inline-bucket mode, chosen at do_build: one I64 key, no NULL in the
     * consumed key column (null-safe and plain equality then coincide) and
     * not the wide mode. The inner JoinOp then builds the plain joins'
     * inline-bucket table + bloom instead of the CSR, which is what the
     * fused probe-scan walks (gxhip_scan.inc). */
    bool inline_ok = false;  /* cfg allows it */
    bool inline_tab = false;
    /* An INNER op in inline-bucket mode that has a COUNT(*) keeps no `used`
     * bitmap: a position was matched exactly when that count is non-zero.
     * count_off is the count's record slot then, -1 where the bitmap is
     * kept (LEFT, the CSR and wide modes, no COUNT(*)). Set at do_build,
     * before the first probe, so every probe kernel and the emission agree. */
    int32_t count_off = -1;
    /* the build came through gxop_groupjoin_build_probe_scan's fast path */
    bool build_fused = false;

    GroupJoinOp(const gx_groupjoin_cfg *c)
        : gx_op(OP_GROUPJOIN, c->device, c->stream), cfg(*c) {
        keys.assign(c->keys, c->keys + c->n_keys);
        build_types.assign(c->build_types, c->build_types + c->n_build_cols);
        probe_types.assign(c->probe_types, c->probe_types + c->n_probe_cols);
        group_cols_.assign(c->group_cols, c->group_cols + c->n_group_cols);
        aggs.assign(c->aggs, c->aggs + c->n_aggs);

        /* inner JoinOp: INNER, probe side = logical outer, consumed side =
         * logical inner (normal build orientation) */
        gx_join_cfg jc{};
        jc.join_type = GX_JOIN_INNER;
        jc.n_keys = (int32_t)keys.size();
        /* JoinOp reads outer_index as probe col / inner_index as build col;
         * groupjoin's cfg has outer=consumed, inner=probe -- swap. */
        swapped_keys = keys;
        for (auto &k : swapped_keys) std::swap(k.outer_index, k.inner_index);
        jc.keys = swapped_keys.data();
        jc.n_outer_cols = (int32_t)probe_types.size();
        jc.outer_types = probe_types.data();
        jc.n_inner_cols = (int32_t)build_types.size();
        jc.inner_types = build_types.data();
        jc.anti_null_col = -1;
        jc.device = device;
        jc.stream = (uint64_t)stream;
        jc.expected_build_rows = c->expected_build_rows;
        jc.enable_bloom = 1; /* acts on the inline-bucket build only */
        jop.reset(new JoinOp(&jc));
        jop->null_safe_keys = true;

        layout = agg_layout_of(aggs);
        wide_ok = keys.size() == 1 && keys[0].unified_type == GX_I64 &&
                  aggs.size() <= 2;
        for (auto &a : aggs)
            wide_ok &= a.func == GX_AGG_COUNT_ROW ||
                       a.func == GX_AGG_COUNT_COL ||
                       a.func == GX_AGG_SUM_I64;
        inline_ok = !wide_ok && keys.size() == 1 &&
                    keys[0].unified_type == GX_I64 &&
                    build_types[keys[0].outer_index] == GX_I64 &&
                    probe_types[keys[0].inner_index] == GX_I64;
    }
    std::vector<gx_equi_key> swapped_keys;

    ~GroupJoinOp() override {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
    }

    int consume(const gx_chunk *ch) { return jop->consume(ch); }

    int do_build() {
        return do_build_with([this](const JoinInsertParams &IP) {
            hipLaunchKernelGGL(k_join_insert, dim3(gx_grid(IP.n)), dim3(256),
                               0, stream, IP);
        });
    }

    /* do_build with the inner join's insert kernel launched by the caller
     * (JoinOp::do_build_with) */
    template <class LaunchInsert>
    int do_build_with(LaunchInsert &&launch_insert) {
        inline_tab = inline_ok && jop->build.n_rows > 0 &&
                     !jop->build.cols[jop->build_key_cols[0]].has_nulls;
        jop->null_safe_keys = !inline_tab;
        count_off = -1;
        if (inline_tab && cfg.join_type == GX_JOIN_INNER)
            for (size_t a = 0; a < aggs.size() && count_off < 0; a++)
                if (aggs[a].func == GX_AGG_COUNT_ROW)
                    count_off = layout.desc.val_off[a];
        if (jop->do_build_with(launch_insert)) return -1;
        const int64_t n = jop->build.n_rows;
        if (d_meta.grow(16, stream)) return -1;
        HIP_OK(hipMemsetAsync(d_meta.p, 0, 16, stream));
        const AggRecDesc &R = layout.desc;
        if (n > 0) {
            if (d_records.grow((size_t)n * R.stride * 8, stream)) return -1;
            agg_launch_init(layout, d_records.p, 0, n, stream);
        }
        size_t words = (size_t)((n + 31) / 32);
        if (words == 0) words = 1;
        if (d_used.grow(words * 4, stream)) return -1;
        HIP_OK(hipMemsetAsync(d_used.p, 0, words * 4, stream));
        wide = wide_ok && n > 0 &&
               !jop->build.cols[jop->build_key_cols[0]].has_nulls;
        if (wide) {
            if (d_wide.grow((size_t)n * sizeof(GJWideEntry), stream))
                return -1;
            hipLaunchKernelGGL(k_gjw_expand, dim3(gx_grid(n)), dim3(256), 0,
                               stream, (const JoinEntry *)jop->d_entries.p, n,
                               jop->build.view(jop->build_key_cols[0]),
                               (GJWideEntry *)d_wide.p,
                               layout.tmpl[R.val_off[0]],
                               aggs.size() > 1 ? layout.tmpl[R.val_off[1]]
                                               : 0ull);
        }
        built = true;
        return 0;
    }

    int probe(const gx_chunk *ch) {
        if (!built) { gx_set_err("probe before build"); return -1; }
        if (ensure_device(device)) return -1;
        if (jop->pass_nothing || ch->n_rows == 0) return 0;
        StagedChunk st;
        if (st.stage(ch, stream)) return -1;
        const int64_t n = st.n_rows;
        KeyViews pk = jop->key_views_staged(st, jop->probe_key_cols);
        if (!inline_tab) {
            if (d_ph.grow((size_t)n * 4, stream) ||
                d_pn.grow((size_t)n, stream)) return -1;
            hipLaunchKernelGGL(k_hash_rows, dim3(gx_grid(n)), dim3(256), 0,
                               stream, pk, n, (int32_t *)d_ph.p,
                               (uint8_t *)d_pn.p, 1 /* null_safe */);
        }
        if (!ev0) {
            HIP_OK(hipEventCreate(&ev0));
            HIP_OK(hipEventCreate(&ev1));
        }
        if (inline_tab) {
            GJInlineProbeParams P;
            std::memset(&P, 0, sizeof(P));
            P.table = (const JoinEntry *)jop->d_table.p;
            P.entries = (const JoinEntry *)jop->d_entries.p;
            P.mask = jop->mask;
            P.n = n;
            P.probe_key = pk.col[0];
            P.used = count_off >= 0 ? nullptr : (uint32_t *)d_used.p;
            P.matches = (unsigned long long *)d_meta.p;
            fill_accum(P.A, st);
            HIP_OK(hipEventRecord(ev0, stream));
            hipLaunchKernelGGL(k_gj_probe_inline, dim3(gx_grid(n)), dim3(256),
                               0, stream, P);
        } else if (wide) {
            GJWideProbeParams W;
            std::memset(&W, 0, sizeof(W));
            W.matches = (unsigned long long *)d_meta.p;
            W.starts = (const uint32_t *)jop->d_starts.p;
            W.wide = (GJWideEntry *)d_wide.p;
            W.mask = jop->mask;
            W.n = n;
            W.hashes = (const int32_t *)d_ph.p;
            W.probe_key = pk.col[0];
            W.n_aggs = (int32_t)aggs.size();
            for (size_t a = 0; a < aggs.size(); a++) {
                W.func[a] = aggs[a].func;
                if (aggs[a].input_col >= 0)
                    W.input[a] = st.views[aggs[a].input_col];
            }
            HIP_OK(hipEventRecord(ev0, stream));
            hipLaunchKernelGGL(k_gjw_probe, dim3(gx_grid(n)), dim3(256),
                               0, stream, W);
        } else {
            GJProbeParams P;
            std::memset(&P, 0, sizeof(P));
            P.starts = (const uint32_t *)jop->d_starts.p;
            P.entries = (const JoinEntry *)jop->d_entries.p;
            P.mask = jop->mask;
            P.n = n;
            P.hashes = (const int32_t *)d_ph.p;
            P.fast_i64 = (int)jop->fast_i64;
            P.build_keys = jop->key_views(jop->build, jop->build_key_cols);
            P.probe_keys = pk;
            P.used = (uint32_t *)d_used.p;
            P.matches = (unsigned long long *)d_meta.p;
            fill_accum(P.A, st);
            HIP_OK(hipEventRecord(ev0, stream));
            hipLaunchKernelGGL(k_gj_probe, dim3(gx_grid(n)), dim3(256), 0,
                               stream, P);
        }
        HIP_OK(hipEventRecord(ev1, stream));
        /* the sync inside also drains the probe before the staged chunk is
         * freed */
        if (finish_probe(nullptr)) return -1;
        rows_total += n;
        return 0;
    }

    /* the aggregate half of a plain probe's params (zeroed by the caller) */
    void fill_accum(AggAccumParams &A, const StagedChunk &st) const {
        A.set_desc(layout.desc);
        agg_bind_inputs(A.input, aggs.data(), nullptr, A.n_aggs, st.views);
        A.records = (unsigned long long *)d_records.p;
    }

    /* after the probing kernel and ev1: fetch the counters, drain the
     * stream, book the kernel time. *kept (may be NULL) receives the scan
     * survivors the probe-scan kernel counted. */
    int finish_probe(int64_t *kept) {
        struct { unsigned long long matches; uint32_t kept, pad; } meta;
        HIP_OK(hipMemcpyAsync(&meta, d_meta.p, 16, hipMemcpyDeviceToHost,
                              stream));
        HIP_OK(hipStreamSynchronize(stream));
        float ms = 0;
        HIP_OK(hipEventElapsedTime(&ms, ev0, ev1));
        kernel_ms += ms;
        probe_launches++;
        matches_total = (int64_t)meta.matches;
        if (kept) *kept = meta.kept;
        return 0;
    }

    int next(gx_result **out) {
        *out = nullptr;
        if (!built) { gx_set_err("next before build"); return -1; }
        if (emitted || jop->pass_nothing) return 0;
        if (ensure_device(device)) return -1;
        emitted = true;
        const int64_t n_build = jop->build.n_rows;
        if (n_build == 0) return 0;
        const AggRecDesc &R = layout.desc;
        if (wide) {
            hipLaunchKernelGGL(k_gjw_unpack, dim3(gx_grid(n_build)), dim3(256),
                               0, stream, (const GJWideEntry *)d_wide.p,
                               n_build, (unsigned long long *)d_records.p,
                               R.stride, R.val_off[0],
                               aggs.size() > 1 ? R.val_off[1] : 0,
                               (int32_t)aggs.size(), (uint32_t *)d_used.p);
        }

        const bool emit_all = cfg.join_type == GX_JOIN_LEFT;
        int64_t n_emit = n_build;
        const uint32_t *idx = nullptr;
        if (!emit_all) {
            if (d_gidx.grow((size_t)n_build * 4, stream) ||
                d_cnt.grow(4, stream)) return -1;
            HIP_OK(hipMemsetAsync(d_cnt.p, 0, 4, stream));
            hipLaunchKernelGGL(k_gj_compact, dim3(gx_grid(n_build)), dim3(256),
                               0, stream, (const uint32_t *)d_used.p,
                               (const unsigned long long *)d_records.p,
                               R.stride, count_off, n_build,
                               (uint32_t *)d_gidx.p, (uint32_t *)d_cnt.p);
            uint32_t cnt = 0;
            HIP_OK(hipMemcpyAsync(&cnt, d_cnt.p, 4, hipMemcpyDeviceToHost,
                                  stream));
            HIP_OK(hipStreamSynchronize(stream));
            n_emit = cnt;
            idx = (const uint32_t *)d_gidx.p;
        }
        if (n_emit == 0) return 0;

        std::vector<int32_t> otypes;
        for (int32_t gc : group_cols_) otypes.push_back(build_types[gc]);
        for (auto &sp : aggs) otypes.push_back(agg_func_result_type(sp.func));
        bool fixed_width = group_cols_.size() <= GX_MAX_COLS;
        for (int32_t gc : group_cols_)
            if (build_types[gc] == GX_SLICE) fixed_width = false;
        if (fixed_width) {
            /* one kernel writes every column; null-free outputs carry no
             * nulls buffer (the scan and join convention) */
            std::vector<uint8_t> null_free;
            for (int32_t gc : group_cols_)
                null_free.push_back(!jop->build.view(gc).has_nulls);
            for (size_t a = 0; a < aggs.size(); a++)
                null_free.push_back(R.seen_off[a] < 0);
            auto h = alloc_result_cols(otypes, n_emit, device, stream,
                                       &null_free);
            if (!h) return -1;
            GJEmitParams E;
            std::memset(&E, 0, sizeof(E));
            E.records = (const unsigned long long *)d_records.p;
            E.R = R;
            E.idx = idx;
            E.used = (const uint32_t *)d_used.p;
            E.count_off = count_off;
            E.count_row_null_row = (int)emit_all;
            E.n = n_emit;
            E.n_keys = (int32_t)group_cols_.size();
            size_t col = 0;
            for (size_t k = 0; k < group_cols_.size(); k++, col++) {
                E.key_src[k] = jop->build.view(group_cols_[k]);
                E.key_words[k] =
                    (int32_t)(gx_fixed_size(build_types[group_cols_[k]]) / 4);
                E.key_vals[k] = h->bufs[col * 2].p;
                E.key_nulls[k] = (uint8_t *)h->bufs[col * 2 + 1].p;
            }
            for (size_t a = 0; a < aggs.size(); a++, col++) {
                E.agg_vals[a] = h->bufs[col * 2].p;
                E.agg_nulls[a] = (uint8_t *)h->bufs[col * 2 + 1].p;
            }
            hipLaunchKernelGGL(k_gj_emit_all, dim3(gx_grid(n_emit)),
                               dim3(256), 0, stream, E);
            HIP_OK(hipStreamSynchronize(stream));
            give_result(std::move(h), out);
            return 0;
        }
        auto h = alloc_result_cols(otypes, n_emit, device, stream);
        if (!h) return -1;
        /* SLICE group columns: the per-column path. LEFT emits in position
         * order: materialize an identity index for the gathers */
        if (emit_all) {
            if (d_gidx.grow((size_t)n_build * 4, stream)) return -1;
            hipLaunchKernelGGL(k_iota, dim3(gx_grid(n_build)), dim3(256), 0,
                               stream, (uint32_t *)d_gidx.p, n_build);
            idx = (const uint32_t *)d_gidx.p;
        }
        size_t col = 0;
        for (int32_t gc : group_cols_) {
            DevColView src = jop->build.view(gc);
            if (src.type == GX_SLICE) {
                if (gather_slice_col(src, idx, 0, n_emit, h.get(), col,
                                     d_gj_tmp, stream))
                    return -1;
            } else {
                hipLaunchKernelGGL(k_gather, dim3(gx_grid(n_emit)), dim3(256),
                                   0, stream, src, idx, n_emit,
                                   h->bufs[col * 2].p,
                                   (uint8_t *)h->bufs[col * 2 + 1].p, 0);
            }
            col++;
        }
        for (size_t a = 0; a < aggs.size(); a++) {
            hipLaunchKernelGGL(k_agg_emit_col, dim3(gx_grid(n_emit)),
                               dim3(256), 0, stream,
                               (const unsigned long long *)d_records.p,
                               R.stride, R.val_off[a], R.seen_off[a],
                               R.func[a],
                               emit_all ? nullptr : idx,
                               (const uint32_t *)d_used.p, count_off,
                               (int)emit_all,
                               n_emit, h->bufs[col * 2].p,
                               (uint8_t *)h->bufs[col * 2 + 1].p);
            col++;
        }
        HIP_OK(hipStreamSynchronize(stream));
        give_result(std::move(h), out);
        return 0;
    }
};

} // namespace

extern "C" {

gx_op *gxop_groupjoin_create(const gx_groupjoin_cfg *cfg) {
    if (cfg)
        for (int32_t i = 0; i < cfg->n_aggs; i++)
            if (gx_agg_is_distinct(cfg->aggs[i].func)) {
                gx_set_err("DISTINCT aggregates are gxop_agg only "
                           "(not supported in group-join)");
                return nullptr;
            }
    if (cfg)
        for (int32_t i = 0; i < cfg->n_aggs; i++)
            if (gx_agg_is_dec(cfg->aggs[i].func)) {
                gx_set_err("SUM_DEC/AVG_DEC are gxop_agg only "
                           "(not supported in group-join)");
                return nullptr;
            }
    if (cfg)
        for (int32_t i = 0; i < cfg->n_aggs; i++)
            if (cfg->aggs[i].func == GX_AGG_RANK ||
                cfg->aggs[i].func == GX_AGG_DENSE_RANK) {
                gx_set_err("RANK/DENSE_RANK are window-only");
                return nullptr;
            }
    if (!cfg || cfg->n_keys <= 0 || cfg->n_keys > GX_MAX_KEYS ||
        (cfg->join_type != GX_JOIN_INNER && cfg->join_type != GX_JOIN_LEFT) ||
        cfg->n_aggs > GX_MAX_COLS) {
        gx_set_err("bad groupjoin cfg");
        return nullptr;
    }
    if (cfg->device < 0) { gx_set_err("gxhip requires a GPU device"); return nullptr; }
    HIP_OK_NULL(hipSetDevice(cfg->device));
    return new GroupJoinOp(cfg);
}
int gxop_groupjoin_consume(gx_op *op, const gx_chunk *c) {
    if (!op || op->kind != OP_GROUPJOIN) { gx_set_err("not a groupjoin op"); return -1; }
    return static_cast<GroupJoinOp *>(op)->consume(c);
}
int gxop_groupjoin_build(gx_op *op) {
    if (!op || op->kind != OP_GROUPJOIN) { gx_set_err("not a groupjoin op"); return -1; }
    return static_cast<GroupJoinOp *>(op)->do_build();
}
int gxop_groupjoin_probe(gx_op *op, const gx_chunk *c) {
    if (!op || op->kind != OP_GROUPJOIN) { gx_set_err("not a groupjoin op"); return -1; }
    return static_cast<GroupJoinOp *>(op)->probe(c);
}
int gxop_groupjoin_next(gx_op *op, gx_result **out) {
    if (!op || op->kind != OP_GROUPJOIN) { gx_set_err("not a groupjoin op"); return -1; }
    return static_cast<GroupJoinOp *>(op)->next(out);
}
int gxop_groupjoin_close(gx_op *op) { delete op; return 0; }
int gxop_groupjoin_get_stats(gx_op *op, gx_join_stats *out) {
    if (!op || op->kind != OP_GROUPJOIN || !out) { gx_set_err("not a groupjoin op"); return -1; }
    GroupJoinOp *g = static_cast<GroupJoinOp *>(op);
    out->probe_kernel_ms = g->kernel_ms;
    out->probe_launches = g->probe_launches;
    out->probe_rows = g->rows_total;
    out->matches = g->matches_total;
    return 0;
}

} /* extern "C" */

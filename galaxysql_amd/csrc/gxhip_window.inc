/*
 * gxhip_window.inc — running window aggregates over partition-sorted input
 * (included by gxhip.hip; needs hipcub DeviceScan).
 *
 * Restates NonFrameOverWindowExec (operator/NonFrameOverWindowExec.java:
 * 34-160): ROWS UNBOUNDED PRECEDING .. CURRENT ROW running aggregates that
 * reset at each partition-key change (isDifferentPartition:136-145,
 * null-safe equality), or every row for reset[a]=1 (resetAccumulators /
 * CURRENT ROW mode). GPU shape: the running value is a SEGMENTED inclusive
 * scan — head flags from adjacent-row key compares, segment ids from an
 * InclusiveSum, then hipcub::DeviceScan::InclusiveScanByKey per window
 * function (null-tracking aggs scan {value, seen} pairs). Chunk-to-chunk
 * carry (the reference's lastPartition + running accumulators) is a
 * device-resident last-partition key + the scan's last value, combined
 * into segment 0 of the next chunk when it continues the same partition.
 */

namespace {

#define GX_WIN_MAX_AGGS 16

/* in-place inclusive scan of vals[0..n) that restarts at each change of seg */
template <typename T, typename Op>
int seg_scan(DevBuf &tmp, hipStream_t stream, const uint32_t *seg, T *vals,
             int64_t n, Op op) {
    return cub_run(tmp, stream, [&](void *t, size_t &b) {
        return hipcub::DeviceScan::InclusiveScanByKey(
            t, b, seg, vals, vals, op, n, hipcub::Equality(), stream);
    });
}

struct WinPairI64 { long long v; long long seen; };
struct WinPairF64 { double v; long long seen; };

struct WinMaxU64 {
    __device__ unsigned long long operator()(unsigned long long a,
                                             unsigned long long b) const {
        return a > b ? a : b;
    }
};
struct WinSumU64 {
    __device__ unsigned long long operator()(unsigned long long a,
                                             unsigned long long b) const {
        return a + b;
    }
};
struct WinMinI64Op {
    __device__ WinPairI64 operator()(WinPairI64 a, WinPairI64 b) const {
        if (!b.seen) return a;
        if (!a.seen) return b;
        return {a.v < b.v ? a.v : b.v, 1};
    }
};
struct WinMaxI64Op {
    __device__ WinPairI64 operator()(WinPairI64 a, WinPairI64 b) const {
        if (!b.seen) return a;
        if (!a.seen) return b;
        return {a.v > b.v ? a.v : b.v, 1};
    }
};
struct WinSumI64Op {
    __device__ WinPairI64 operator()(WinPairI64 a, WinPairI64 b) const {
        if (!b.seen) return a;
        if (!a.seen) return b;
        return {(long long)((unsigned long long)a.v +
                            (unsigned long long)b.v), 1};
    }
};
struct WinSumF64Op {
    __device__ WinPairF64 operator()(WinPairF64 a, WinPairF64 b) const {
        if (!b.seen) return a;
        if (!a.seen) return b;
        return {a.v + b.v, 1};
    }
};
struct WinMinF64Op {
    __device__ WinPairF64 operator()(WinPairF64 a, WinPairF64 b) const {
        if (!b.seen) return a;
        if (!a.seen) return b;
        /* Java Math.min: NaN propagates, -0.0 < +0.0 (a raw `<` select
         * drops NaN and picks +0.0 — caught by the NaN/-0.0 fuzz) */
        return {jmin_f64(a.v, b.v), 1};
    }
};
struct WinAndU64 {
    __device__ unsigned long long operator()(unsigned long long a,
                                             unsigned long long b) const {
        return a & b;
    }
};
struct WinOrU64 {
    __device__ unsigned long long operator()(unsigned long long a,
                                             unsigned long long b) const {
        return a | b;
    }
};
struct WinXorU64 {
    __device__ unsigned long long operator()(unsigned long long a,
                                             unsigned long long b) const {
        return a ^ b;
    }
};
struct WinAvgF64Op {
    /* {sum, count} pairs: plain field-wise add (nulls map to {0,0}) */
    __device__ WinPairF64 operator()(WinPairF64 a, WinPairF64 b) const {
        return {a.v + b.v, a.seen + b.seen};
    }
};
struct WinMaxF64Op {
    __device__ WinPairF64 operator()(WinPairF64 a, WinPairF64 b) const {
        if (!b.seen) return a;
        if (!a.seen) return b;
        return {jmax_f64(a.v, b.v), 1};
    }
};

/* head flags: 1 where row i starts a new partition. carry (1-row views)
 * extends the compare to the previous chunk's last row. */
struct WinHeadParams {
    int64_t n;
    int32_t n_part;
    DevColView cols[GX_MAX_KEYS];
    int have_carry;
    DevColView carry[GX_MAX_KEYS];
    uint32_t *heads;
    uint32_t *continues;   /* [0] = 1 if row 0 continues the carry part. */
    /* RANK/DENSE_RANK: ORDER-BY run change detection (null-safe equals,
     * Rank.sameRank). run_heads == NULL when no rank-family functions. */
    int32_t n_order;
    DevColView ocols[GX_MAX_KEYS];
    DevColView ocarry[GX_MAX_KEYS];
    uint32_t *run_heads;
};

__global__ void k_win_heads(WinHeadParams P) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < P.n;
         i += (int64_t)gridDim.x * blockDim.x) {
        bool same;
        if (i == 0) {
            same = P.have_carry;
            for (int c = 0; same && c < P.n_part; c++)
                same = col_eq(P.carry[c], 0, P.cols[c], 0);
            if (i == 0) *P.continues = same ? 1u : 0u;
        } else {
            same = true;
            for (int c = 0; same && c < P.n_part; c++)
                same = col_eq(P.cols[c], i - 1, P.cols[c], i);
        }
        P.heads[i] = same ? 0u : 1u;
        if (P.run_heads) {
            bool osame = same;
            if (i == 0) {
                for (int c = 0; osame && c < P.n_order; c++)
                    osame = col_eq(P.ocarry[c], 0, P.ocols[c], 0);
            } else {
                for (int c = 0; osame && c < P.n_order; c++)
                    osame = col_eq(P.ocols[c], i - 1, P.ocols[c], i);
            }
            P.run_heads[i] = osame ? 0u : 1u;
        }
    }
}

/* rank scans: positions of the latest head at-or-before each row */
__global__ void k_win_map_headpos(const uint32_t *flags, int64_t base,
                                  int64_t n, unsigned long long *out) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        out[i] = flags[i] ? (unsigned long long)(base + i + 1) : 0ull;
}

__global__ void k_win_map_flags(const uint32_t *flags, int64_t n,
                                unsigned long long *out) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        out[i] = flags[i] ? 1ull : 0ull;
}

__global__ void k_win_emit_rank(const unsigned long long *run_pos,
                                const unsigned long long *seg_pos, int64_t n,
                                int64_t *out_vals, uint8_t *out_nulls) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        out_vals[i] = (int64_t)(run_pos[i] - seg_pos[i] + 1);
        out_nulls[i] = 0;
    }
}

__global__ void k_win_fill_i64(int64_t v, int64_t n, int64_t *out_vals,
                               uint8_t *out_nulls) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        out_vals[i] = v;
        out_nulls[i] = 0;
    }
}

/* value transforms (map before scan) */
__global__ void k_win_map_u64(DevColView c, int32_t func, int64_t n,
                              unsigned long long *out) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        unsigned long long v = 0;
        switch (func) {
        case GX_AGG_COUNT_ROW: v = 1; break;
        case GX_AGG_COUNT_COL: v = col_is_null(c, i) ? 0 : 1; break;
        case GX_AGG_BIT_AND:
            v = col_is_null(c, i) ? ~0ull
                : (unsigned long long)(c.type == GX_I32
                      ? (int64_t)((const int32_t *)c.values)[i]
                      : ((const int64_t *)c.values)[i]);
            break;
        case GX_AGG_BIT_OR: case GX_AGG_BIT_XOR:
            v = col_is_null(c, i) ? 0ull
                : (unsigned long long)(c.type == GX_I32
                      ? (int64_t)((const int32_t *)c.values)[i]
                      : ((const int64_t *)c.values)[i]);
            break;
        default: /* SUM_I64 */
            if (!col_is_null(c, i))
                v = (unsigned long long)(c.type == GX_I32
                        ? (int64_t)((const int32_t *)c.values)[i]
                        : ((const int64_t *)c.values)[i]);
            break;
        }
        out[i] = v;
    }
}

__global__ void k_win_map_pair_i64(DevColView c, int64_t n, WinPairI64 *out) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        bool nn = col_is_null(c, i);
        long long v = nn ? 0
            : (c.type == GX_I32 ? (long long)((const int32_t *)c.values)[i]
                                : ((const long long *)c.values)[i]);
        out[i] = {v, nn ? 0ll : 1ll};
    }
}

__global__ void k_win_map_pair_f64(DevColView c, int64_t n, WinPairF64 *out) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        bool nn = col_is_null(c, i);
        double v = 0;
        if (!nn)
            v = c.type == GX_F64 ? ((const double *)c.values)[i]
              : c.type == GX_I32 ? (double)((const int32_t *)c.values)[i]
                                 : (double)((const int64_t *)c.values)[i];
        out[i] = {v, nn ? 0ll : 1ll};
    }
}

/* fold the carry value into segment 0 (rows before the first head) */
template <typename T, typename Op>
__global__ void k_win_carry_apply(const uint32_t *seg, const uint32_t *continues,
                                  const T *carry, int64_t n, T *vals, Op op) {
    if (!*continues) return;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        if (seg[i] != 0) continue;
        vals[i] = op(*carry, vals[i]);
    }
}

/* emit scan output -> result column */
__global__ void k_win_emit_u64(const unsigned long long *v, int64_t n,
                               int64_t *out_vals, uint8_t *out_nulls) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        out_vals[i] = (int64_t)v[i];
        out_nulls[i] = 0;
    }
}
__global__ void k_win_emit_pair_i64(const WinPairI64 *v, int64_t n,
                                    int64_t *out_vals, uint8_t *out_nulls) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        out_vals[i] = v[i].seen ? v[i].v : 0;
        out_nulls[i] = v[i].seen ? 0 : 1;
    }
}
__global__ void k_win_emit_pair_f64(const WinPairF64 *v, int64_t n,
                                    double *out_vals, uint8_t *out_nulls) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        out_vals[i] = v[i].seen ? v[i].v : 0;
        out_nulls[i] = v[i].seen ? 0 : 1;
    }
}
__global__ void k_win_emit_avg_f64(const WinPairF64 *v, int64_t n,
                                   double *out_vals, uint8_t *out_nulls) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        out_vals[i] = v[i].seen ? v[i].v / (double)v[i].seen : 0;
        out_nulls[i] = v[i].seen ? 0 : 1;
    }
}

/* save the chunk's last row as the next chunk's carry partition key
 * (fixed-width part cols; slice keys are copied host-side in consume) */
__global__ void k_win_save_carry_fixed(DevColView src, int64_t row,
                                       void *dst_val, uint8_t *dst_null) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    bool nn = col_is_null(src, row);
    *dst_null = nn;
    switch (src.type) {
    case GX_I64: *(int64_t *)dst_val = nn ? 0 : ((const int64_t *)src.values)[row]; break;
    case GX_I32: *(int32_t *)dst_val = nn ? 0 : ((const int32_t *)src.values)[row]; break;
    case GX_F64: *(double *)dst_val = nn ? 0 : ((const double *)src.values)[row]; break;
    }
}

struct WindowOp : gx_op {
    gx_window_cfg cfg;
    std::vector<int32_t> part_cols_, order_cols_, carry_cols_, input_types;
    std::vector<gx_agg_spec> aggs;
    std::vector<uint8_t> reset_;
    bool has_rank = false;
    int64_t g_base = 0;   /* rows consumed before this chunk (rank scans
                             use GLOBAL head positions so carries compose) */

    /* carry: device 1-row partition(+order) key + last scan value per agg
     * (+ one extra slot for the shared partition-head-position scan) */
    bool have_carry = false;
    std::vector<int64_t> carry_slice_len;
    /* last-allocated first (see DevBuf: destruction order and the pool) */
    DevBuf d_scan_tmp2, d_segpos, d_vals, d_cont, d_seg, d_runheads, d_heads;
    std::vector<DevBuf> carry_state;
    std::vector<DevBuf> carry_data, carry_null, carry_val; /* per carry col */

    WindowOp(const gx_window_cfg *c) : gx_op(OP_WINDOW, c->device, c->stream),
                                       cfg(*c) {
        part_cols_.assign(c->part_cols, c->part_cols + c->n_part_cols);
        if (c->n_order_cols > 0)
            order_cols_.assign(c->order_cols, c->order_cols + c->n_order_cols);
        input_types.assign(c->input_types, c->input_types + c->n_input_cols);
        aggs.assign(c->aggs, c->aggs + c->n_aggs);
        reset_.assign(c->reset, c->reset + c->n_aggs);
        for (auto &a : aggs)
            has_rank |= a.func == GX_AGG_RANK || a.func == GX_AGG_DENSE_RANK;
        carry_cols_ = part_cols_;
        carry_cols_.insert(carry_cols_.end(), order_cols_.begin(),
                           order_cols_.end());
        carry_val.resize(carry_cols_.size());
        carry_null.resize(carry_cols_.size());
        carry_data.resize(carry_cols_.size());
        carry_slice_len.assign(carry_cols_.size(), 0);
        carry_state.resize(aggs.size() + 1);  /* +1: shared seg-pos scan */
    }
    size_t scan_elem_size(int32_t func) const {
        switch (func) {
        case GX_AGG_COUNT_ROW: case GX_AGG_COUNT_COL: case GX_AGG_SUM_I64:
        case GX_AGG_BIT_AND: case GX_AGG_BIT_OR: case GX_AGG_BIT_XOR:
            return 8;
        default: return 16;  /* {value, seen} pairs */
        }
    }

    DevColView carry_view(size_t k, const DevColView &like) const {
        DevColView v{};
        v.type = like.type;
        v.values = carry_val[k].p;
        v.nulls = (const uint8_t *)carry_null[k].p;
        v.has_nulls = true;   /* the 1-row carry always materializes its
                                 null byte — col_is_null gates on this */
        if (like.type == GX_SLICE) {
            v.offsets = (const int32_t *)carry_val[k].p;
            v.bytes = (const uint8_t *)carry_data[k].p;
        }
        return v;
    }

    template <typename T, typename Op>
    int scan_one(const uint32_t *seg, T *vals, int64_t n, Op op, size_t a) {
        if (seg_scan(d_scan_tmp2, stream, seg, vals, n, op)) return -1;
        if (have_carry)
            hipLaunchKernelGGL((k_win_carry_apply<T, Op>), dim3(gx_grid(n)),
                               dim3(256), 0, stream, seg,
                               (const uint32_t *)d_cont.p,
                               (const T *)carry_state[a].p, n, vals, op);
        /* new carry = the last row's running value */
        if (carry_state[a].grow(sizeof(T), stream)) return -1;
        HIP_OK(hipMemcpyAsync(carry_state[a].p, vals + (n - 1), sizeof(T),
                              hipMemcpyDeviceToDevice, stream));
        return 0;
    }

    int consume(const gx_chunk *ch, gx_result **out) {
        *out = nullptr;
        if (ensure_device(device)) return -1;
        const int64_t n = ch->n_rows;
        std::vector<int32_t> otypes = input_types;
        for (auto &sp : aggs) {
            switch (sp.func) {
            case GX_AGG_RANK: case GX_AGG_DENSE_RANK:
                otypes.push_back(GX_I64); break;
            default:
                otypes.push_back(agg_func_result_type(sp.func)); break;
            }
        }
        if (n == 0) {
            auto h = alloc_result_cols(otypes, 0, device, stream);
            if (!h) return -1;
            give_result(std::move(h), out);
            return 0;
        }
        StagedChunk st;
        if (st.stage(ch, stream)) return -1;
        /* 1. heads + segment ids */
        if (d_heads.grow((size_t)n * 4, stream) ||
            d_seg.grow((size_t)n * 4, stream) ||
            d_cont.grow(4, stream)) return -1;
        WinHeadParams H;
        std::memset(&H, 0, sizeof(H));
        H.n = n;
        H.n_part = (int32_t)part_cols_.size();
        for (size_t k = 0; k < part_cols_.size(); k++) {
            H.cols[k] = st.views[part_cols_[k]];
            if (have_carry) H.carry[k] = carry_view(k, H.cols[k]);
        }
        H.have_carry = have_carry;
        H.heads = (uint32_t *)d_heads.p;
        H.continues = (uint32_t *)d_cont.p;
        if (has_rank) {
            if (d_runheads.grow((size_t)n * 4, stream)) return -1;
            H.n_order = (int32_t)order_cols_.size();
            for (size_t k = 0; k < order_cols_.size(); k++) {
                H.ocols[k] = st.views[order_cols_[k]];
                if (have_carry)
                    H.ocarry[k] = carry_view(part_cols_.size() + k,
                                             H.ocols[k]);
            }
            H.run_heads = (uint32_t *)d_runheads.p;
        }
        hipLaunchKernelGGL(k_win_heads, dim3(gx_grid(n)), dim3(256), 0,
                           stream, H);
        if (cub_run(d_scan_tmp2, stream, [&](void *t, size_t &b) {
                return hipcub::DeviceScan::InclusiveSum(
                    t, b, (uint32_t *)d_heads.p, (uint32_t *)d_seg.p, n,
                    stream);
            }))
            return -1;

        /* 1b. rank family: the shared partition-head-position scan
         * S[i] = GLOBAL index+1 of the current partition's first row
         * (max-scan over seg; carry slot aggs.size()) */
        if (has_rank) {
            if (d_segpos.grow((size_t)n * 8, stream)) return -1;
            auto *sp = (unsigned long long *)d_segpos.p;
            hipLaunchKernelGGL(k_win_map_headpos, dim3(gx_grid(n)),
                               dim3(256), 0, stream,
                               (const uint32_t *)d_heads.p, g_base, n,
                               sp);
            if (scan_one((const uint32_t *)d_seg.p, sp, n, WinMaxU64(),
                         aggs.size()))
                return -1;
        }

        /* 2. result shell + pass-through input columns */
        auto h = alloc_result_cols(otypes, n, device, stream);
        if (!h) return -1;
        if (copy_input_cols(input_types, st.views.data(), n, h.get(),
                            d_scan_tmp2, stream))
            return -1;

        /* 3. per window function: map -> scan-by-segment -> emit */
        const uint32_t *seg = (const uint32_t *)d_seg.p;
        for (size_t a = 0; a < aggs.size(); a++) {
            size_t col = input_types.size() + a;
            int32_t f0 = aggs[a].func;
            if (f0 == GX_AGG_RANK || f0 == GX_AGG_DENSE_RANK) {
                if (reset_[a]) {
                    /* resetAccumulators: every row is rank 1 */
                    hipLaunchKernelGGL(k_win_fill_i64, dim3(gx_grid(n)),
                                       dim3(256), 0, stream, (int64_t)1,
                                       n, (int64_t *)h->bufs[col * 2].p,
                                       (uint8_t *)h->bufs[col * 2 + 1].p);
                    continue;
                }
                if (d_vals.grow((size_t)n * 8, stream)) return -1;
                auto *vals = (unsigned long long *)d_vals.p;
                if (f0 == GX_AGG_RANK) {
                    hipLaunchKernelGGL(k_win_map_headpos,
                                       dim3(gx_grid(n)), dim3(256), 0,
                                       stream,
                                       (const uint32_t *)d_runheads.p,
                                       g_base, n, vals);
                    if (scan_one((const uint32_t *)d_seg.p, vals, n,
                                 WinMaxU64(), a)) return -1;
                    hipLaunchKernelGGL(k_win_emit_rank, dim3(gx_grid(n)),
                                       dim3(256), 0, stream, vals,
                                       (const unsigned long long *)d_segpos.p,
                                       n, (int64_t *)h->bufs[col * 2].p,
                                       (uint8_t *)h->bufs[col * 2 + 1].p);
                } else {
                    hipLaunchKernelGGL(k_win_map_flags, dim3(gx_grid(n)),
                                       dim3(256), 0, stream,
                                       (const uint32_t *)d_runheads.p, n,
                                       vals);
                    if (scan_one((const uint32_t *)d_seg.p, vals, n,
                                 WinSumU64(), a)) return -1;
                    hipLaunchKernelGGL(k_win_emit_u64, dim3(gx_grid(n)),
                                       dim3(256), 0, stream, vals, n,
                                       (int64_t *)h->bufs[col * 2].p,
                                       (uint8_t *)h->bufs[col * 2 + 1].p);
                }
                continue;
            }
            DevColView in{};
            if (aggs[a].input_col >= 0) in = st.views[aggs[a].input_col];
            size_t es = scan_elem_size(aggs[a].func);
            if (d_vals.grow((size_t)n * es, stream)) return -1;
            int32_t f = aggs[a].func;
            if (es == 8) {
                auto *vals = (unsigned long long *)d_vals.p;
                hipLaunchKernelGGL(k_win_map_u64, dim3(gx_grid(n)),
                                   dim3(256), 0, stream, in, f, n, vals);
                if (!reset_[a]) {
                    int r = f == GX_AGG_BIT_AND
                        ? scan_one(seg, vals, n, WinAndU64(), a)
                        : f == GX_AGG_BIT_OR
                        ? scan_one(seg, vals, n, WinOrU64(), a)
                        : f == GX_AGG_BIT_XOR
                        ? scan_one(seg, vals, n, WinXorU64(), a)
                        : scan_one(seg, vals, n, WinSumU64(), a);
                    if (r) return -1;
                }
                hipLaunchKernelGGL(k_win_emit_u64, dim3(gx_grid(n)),
                                   dim3(256), 0, stream, vals, n,
                                   (int64_t *)h->bufs[col * 2].p,
                                   (uint8_t *)h->bufs[col * 2 + 1].p);
            } else if (f == GX_AGG_MIN_I64 || f == GX_AGG_MAX_I64 ||
                       f == GX_AGG_SUM_I64N) {
                auto *vals = (WinPairI64 *)d_vals.p;
                hipLaunchKernelGGL(k_win_map_pair_i64, dim3(gx_grid(n)),
                                   dim3(256), 0, stream, in, n, vals);
                if (!reset_[a]) {
                    int r = f == GX_AGG_MIN_I64
                        ? scan_one(seg, vals, n, WinMinI64Op(), a)
                        : f == GX_AGG_MAX_I64
                        ? scan_one(seg, vals, n, WinMaxI64Op(), a)
                        : scan_one(seg, vals, n, WinSumI64Op(), a);
                    if (r) return -1;
                }
                hipLaunchKernelGGL(k_win_emit_pair_i64, dim3(gx_grid(n)),
                                   dim3(256), 0, stream, vals, n,
                                   (int64_t *)h->bufs[col * 2].p,
                                   (uint8_t *)h->bufs[col * 2 + 1].p);
            } else {
                auto *vals = (WinPairF64 *)d_vals.p;
                hipLaunchKernelGGL(k_win_map_pair_f64, dim3(gx_grid(n)),
                                   dim3(256), 0, stream, in, n, vals);
                if (!reset_[a]) {
                    int r = f == GX_AGG_MIN_F64
                        ? scan_one(seg, vals, n, WinMinF64Op(), a)
                        : f == GX_AGG_MAX_F64
                        ? scan_one(seg, vals, n, WinMaxF64Op(), a)
                        : f == GX_AGG_AVG_F64
                        ? scan_one(seg, vals, n, WinAvgF64Op(), a)
                        : scan_one(seg, vals, n, WinSumF64Op(), a);
                    if (r) return -1;
                }
                if (f == GX_AGG_AVG_F64)
                    hipLaunchKernelGGL(k_win_emit_avg_f64,
                                       dim3(gx_grid(n)), dim3(256), 0,
                                       stream, vals, n,
                                       (double *)h->bufs[col * 2].p,
                                       (uint8_t *)h->bufs[col * 2 + 1].p);
                else
                    hipLaunchKernelGGL(k_win_emit_pair_f64,
                                       dim3(gx_grid(n)), dim3(256), 0,
                                       stream, vals, n,
                                       (double *)h->bufs[col * 2].p,
                                       (uint8_t *)h->bufs[col * 2 + 1].p);
            }
        }

        /* 4. save the last row's partition(+order) key as carry */
        for (size_t k = 0; k < carry_cols_.size(); k++) {
            const DevColView &v = st.views[carry_cols_[k]];
            if (carry_null[k].grow(1, stream)) return -1;
            if (v.type == GX_SLICE) {
                /* need host lengths for the byte copy */
                int32_t offs[2] = {0, 0};
                HIP_OK(hipMemcpyAsync(&offs[1], v.offsets + (n - 1), 4,
                                      hipMemcpyDeviceToHost, stream));
                if (n > 1)
                    HIP_OK(hipMemcpyAsync(&offs[0], v.offsets + (n - 2),
                                          4, hipMemcpyDeviceToHost,
                                          stream));
                HIP_OK(hipStreamSynchronize(stream));
                int32_t len = offs[1] - offs[0];
                carry_slice_len[k] = len;
                if (carry_val[k].grow(4, stream) ||
                    carry_data[k].grow((size_t)std::max(len, 1), stream))
                    return -1;
                HIP_OK(hipMemcpyAsync(carry_val[k].p, &len, 4,
                                      hipMemcpyHostToDevice, stream));
                if (len > 0)
                    HIP_OK(hipMemcpyAsync(carry_data[k].p,
                                          v.bytes + offs[0],
                                          (size_t)len,
                                          hipMemcpyDeviceToDevice,
                                          stream));
                uint8_t nn = 0;
                if (v.nulls)
                    HIP_OK(hipMemcpyAsync(carry_null[k].p,
                                          v.nulls + (n - 1), 1,
                                          hipMemcpyDeviceToDevice,
                                          stream));
                else
                    HIP_OK(hipMemcpyAsync(carry_null[k].p, &nn, 1,
                                          hipMemcpyHostToDevice,
                                          stream));
            } else {
                if (carry_val[k].grow(8, stream)) return -1;
                hipLaunchKernelGGL(k_win_save_carry_fixed, dim3(1),
                                   dim3(64), 0, stream, v, n - 1,
                                   carry_val[k].p,
                                   (uint8_t *)carry_null[k].p);
            }
        }
        /* the staged chunk is freed on return: drain first */
        HIP_OK(hipStreamSynchronize(stream));
        have_carry = true;
        g_base += n;
        give_result(std::move(h), out);
        return 0;
    }
};

} // namespace

extern "C" {

gx_op *gxop_window_create(const gx_window_cfg *cfg) {
    if (!cfg || cfg->n_aggs <= 0 || cfg->n_aggs > GX_WIN_MAX_AGGS ||
        cfg->n_part_cols > GX_MAX_KEYS) {
        gx_set_err("bad window cfg");
        return nullptr;
    }
    for (int32_t i = 0; i < cfg->n_aggs; i++) {
        int32_t f = cfg->aggs[i].func;
        if (gx_agg_is_distinct(f)) {
            gx_set_err("DISTINCT aggregates are gxop_agg only "
                       "(not supported in window)");
            return nullptr;
        }
        if (gx_agg_is_dec(f)) {
            gx_set_err("SUM_DEC/AVG_DEC are gxop_agg only "
                       "(not supported in window)");
            return nullptr;
        }
        /* running window: accumulators + rank family + null-init Sum;
         * navigation/distribution funcs are frame-window only */
        if ((f < GX_AGG_COUNT_ROW || f > GX_AGG_DENSE_RANK) &&
            f != GX_AGG_SUM_I64N) {
            gx_set_err("unknown or frame-only func in running window");
            return nullptr;
        }
    }
    if (cfg->device < 0) { gx_set_err("gxhip requires a GPU device"); return nullptr; }
    HIP_OK_NULL(hipSetDevice(cfg->device));
    return new WindowOp(cfg);
}
int gxop_window_consume(gx_op *op, const gx_chunk *c, gx_result **out) {
    if (!op || op->kind != OP_WINDOW) { gx_set_err("not a window op"); return -1; }
    return static_cast<WindowOp *>(op)->consume(c, out);
}
int gxop_window_close(gx_op *op) { delete op; return 0; }

} /* extern "C" */

/*
 * gxhip_fwindow.inc — frame windows (included by gxhip.hip after
 * gxhip_window.inc, whose head/map kernels it reuses, and gxhip_agg.inc,
 * whose agg_apply drives the whole-partition reduction).
 *
 * Restates OverWindowFramesExec + operator/frame/ (UnboundedOverFrame,
 * RowSlidingOverFrame, RowUnboundedFollowingOverFrame,
 * RangeSliding/RangeUnboundedPreceding/RangeUnboundedFollowingOverFrame).
 * The reference buffers per partition and replays aggregators; here the
 * WHOLE input is buffered (consume -> finish barrier -> next), then:
 *   - segment bounds: head flags -> InclusiveSum seg ids -> per-seg start
 *     index array (+ total);
 *   - WHOLE_PARTITION: one atomics reduction into per-segment records
 *     (agg_apply), then a per-row broadcast;
 *   - ROWS_SLIDING / UNBOUNDED_FOLLOWING: segmented inclusive prefix sums
 *     (ScanByKey) + clamped prefix differences — exact for the additive
 *     integer functions (COUNT/COUNT_COL/SUM_I64/SUM_I64N, the last with
 *     a non-null-count prefix for NULL-init semantics); SUM/AVG(F64) via
 *     double prefixes (north_star DOUBLE tolerance); MIN/MAX via sparse
 *     tables;
 *   - RANGE_* frames: per-row index bounds from binary searches over the
 *     sorted order column (k_fw_range_bounds — null runs, asc/desc, the
 *     reference's scan-from-current-row quirks), then the same prefix /
 *     sparse-table machinery with per-row [lo,hi].
 */

namespace {

__global__ void k_fw_seg_starts(const uint32_t *heads, const uint32_t *seg,
                                int64_t n, uint32_t *starts) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        if (i == 0 || heads[i]) starts[seg[i]] = (uint32_t)i;
    }
}

/* whole-partition reduction: row accumulates into records[seg[i]] */
__global__ void k_fw_seg_reduce(AggAccumParams A, const uint32_t *seg,
                                int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        agg_apply(A, seg[i], i);
}

/* sliding MIN/MAX: sparse-table range queries. The ROWS frame span is
 * FIXED, so only floor(log2(span))+1 levels are built (level k holds the
 * op over [i, i+2^k-1], clamped to the array end); a query covers its
 * clamped in-partition range [lo,hi] with two level-k windows, both
 * inside the partition, so the table needs no segment awareness. Null
 * inputs map to the op identity; result nullness comes from a prefix
 * count of non-null inputs over the same range. */
struct FwSumF64 {
    __device__ double operator()(double a, double b) const { return a + b; }
};

struct StMinI64 {
    __device__ long long operator()(long long a, long long b) const {
        return a < b ? a : b;
    }
};
struct StMaxI64 {
    __device__ long long operator()(long long a, long long b) const {
        return a > b ? a : b;
    }
};
struct StMinF64 {
    __device__ double operator()(double a, double b) const {
        return jmin_f64(a, b);
    }
};
struct StMaxF64 {
    __device__ double operator()(double a, double b) const {
        return jmax_f64(a, b);
    }
};

template <typename T>
__global__ void k_fw_st_map(DevColView c, int64_t n, T identity, T *out,
                            unsigned long long *nonnull) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        bool nn = col_is_null(c, i);
        T v = identity;
        if (!nn) {
            if (c.type == GX_I32)
                v = (T)((const int32_t *)c.values)[i];
            else if (c.type == GX_F64)
                v = (T)((const double *)c.values)[i];
            else
                v = (T)((const int64_t *)c.values)[i];
        }
        out[i] = v;
        nonnull[i] = nn ? 0 : 1;
    }
}

template <typename T, typename Op>
__global__ void k_fw_st_build(const T *prev, int64_t n, int64_t half,
                              T *next, Op op) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        int64_t j = i + half;
        next[i] = j < n ? op(prev[i], prev[j]) : prev[i];
    }
}

template <typename T, typename Op>
__global__ void k_fw_st_query(const T *levels, int64_t n, int32_t n_levels,
                              const uint32_t *seg, const uint32_t *starts,
                              uint32_t n_segs, int64_t preceding,
                              int64_t following,
                              const int32_t *lo_arr, const int32_t *hi_arr,
                              const unsigned long long *nn_prefix,
                              int is_f64, Op op, void *out_vals,
                              uint8_t *out_nulls) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        uint32_t sg = seg[i];
        int64_t s = starts[sg];
        int64_t e = sg + 1 < n_segs ? starts[sg + 1] : n;
        int64_t lo, hi;
        if (lo_arr) {
            lo = lo_arr[i];
            hi = hi_arr[i];
        } else {
            lo = i - preceding < s ? s : i - preceding;
            hi = i + following > e - 1 ? e - 1 : i + following;
        }
        unsigned long long cnt = hi < lo ? 0ull
            : nn_prefix[hi] - (lo > 0 ? nn_prefix[lo - 1] : 0ull);
        if (cnt == 0) {
            out_nulls[i] = 1;
            if (is_f64) ((double *)out_vals)[i] = 0;
            else ((int64_t *)out_vals)[i] = 0;
            continue;
        }
        int64_t len = hi - lo + 1;
        int32_t k = 63 - __clzll((unsigned long long)len);
        if (k >= n_levels) k = n_levels - 1;
        const T *lv = levels + (size_t)k * n;
        T v = op(lv[lo], lv[hi - ((int64_t)1 << k) + 1]);
        out_nulls[i] = 0;
        if (is_f64) ((double *)out_vals)[i] = (double)v;
        else ((int64_t *)out_vals)[i] = (int64_t)v;
    }
}

/* navigation functions: per-row SOURCE index (0xFFFFFFFF = NULL), then
 * the ordinary k_gather / gather_slice_col materializes any column type */
__global__ void k_fw_navigate(const uint32_t *seg, const uint32_t *starts,
                              uint32_t n_segs, int64_t n, int32_t func,
                              int64_t param, uint32_t *out_idx) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        uint32_t sg = seg[i];
        int64_t s = starts[sg];
        int64_t e = sg + 1 < n_segs ? starts[sg + 1] : n;
        int64_t src = -1;
        switch (func) {
        case GX_AGG_FIRST_VALUE: src = s; break;
        case GX_AGG_LAST_VALUE: src = e - 1; break;
        case GX_AGG_NTH_VALUE:
            src = s + param - 1;
            if (src >= e) src = -1;
            break;
        case GX_AGG_LAG:
            src = i - param;
            if (src < s) src = -1;
            break;
        case GX_AGG_LEAD:
            src = i + param;
            if (src >= e) src = -1;
            break;
        }
        out_idx[i] = src < 0 ? 0xFFFFFFFFu : (uint32_t)src;
    }
}

__global__ void k_fw_ntile(const uint32_t *seg, const uint32_t *starts,
                           uint32_t n_segs, int64_t n, int64_t nt,
                           int64_t *out_vals, uint8_t *out_nulls) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        uint32_t sg = seg[i];
        int64_t s = starts[sg];
        int64_t e = sg + 1 < n_segs ? starts[sg + 1] : n;
        int64_t size = e - s, pos = i - s;
        int64_t base = size / nt, rem = size % nt, bucket;
        if (base == 0) bucket = pos + 1;
        else if (pos < rem * (base + 1)) bucket = pos / (base + 1) + 1;
        else bucket = rem + (pos - rem * (base + 1)) / base + 1;
        out_vals[i] = bucket;
        out_nulls[i] = 0;
    }
}

/* CUME_DIST / PERCENT_RANK from ORDER-BY run bounds */
__global__ void k_fw_dist(const uint32_t *seg, const uint32_t *seg_starts,
                          uint32_t n_segs, const uint32_t *runid,
                          const uint32_t *run_starts, uint32_t n_runs,
                          int64_t n, int is_cume, double *out_vals,
                          uint8_t *out_nulls) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        uint32_t sg = seg[i];
        int64_t s = seg_starts[sg];
        int64_t e = sg + 1 < n_segs ? seg_starts[sg + 1] : n;
        int64_t size = e - s;
        uint32_t rid = runid[i];
        int64_t run_s = run_starts[rid];
        int64_t run_e = (rid + 1 < n_runs ? (int64_t)run_starts[rid + 1]
                                          : n) - 1;
        if (is_cume)
            out_vals[i] = (double)(run_e - s + 1) / (double)size;
        else
            out_vals[i] = size <= 1 ? 0.0
                : (double)(run_s - s) / (double)(size - 1);
        out_nulls[i] = 0;
    }
}

/* sliding / unbounded-following via clamped prefix differences.
 * prefix = segmented INCLUSIVE prefix of the mapped values.
 * lo_arr/hi_arr non-null (RANGE frames): per-row index bounds from
 * k_fw_range_bounds; hi < lo = empty frame (COUNT/SUM0 -> 0). */
__global__ void k_fw_prefix_diff(const unsigned long long *prefix,
                                 const unsigned long long *nn_prefix,
                                 const uint32_t *seg, const uint32_t *starts,
                                 uint32_t n_segs, int64_t n,
                                 int64_t preceding, int64_t following,
                                 int to_partition_end,
                                 const int32_t *lo_arr, const int32_t *hi_arr,
                                 int64_t *out_vals, uint8_t *out_nulls) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        uint32_t sg = seg[i];
        int64_t s = starts[sg];
        int64_t e = sg + 1 < n_segs ? starts[sg + 1] : n; /* one past end */
        int64_t lo, hi;
        if (lo_arr) {
            lo = lo_arr[i];
            hi = hi_arr[i];
        } else if (to_partition_end) {
            lo = i;
            hi = e - 1;
        } else {
            lo = i - preceding < s ? s : i - preceding;
            hi = i + following > e - 1 ? e - 1 : i + following;
        }
        unsigned long long v = 0;
        if (hi >= lo) {
            v = prefix[hi];
            if (lo > s) v -= prefix[lo - 1];
        }
        bool isnull = false;
        if (nn_prefix) { /* null-init Sum: all-null/empty frame -> NULL */
            unsigned long long cnt = 0;
            if (hi >= lo) {
                cnt = nn_prefix[hi];
                if (lo > s) cnt -= nn_prefix[lo - 1];
            }
            isnull = cnt == 0;
        }
        out_vals[i] = isnull ? 0 : (int64_t)v;
        out_nulls[i] = isnull;
    }
}

/* f64 frames (SUM_F64 / AVG_F64): value prefix (double) + non-null-count
 * prefix; empty or all-null frame -> NULL (Double2DoubleSum /
 * AvgV2 null-init semantics). Prefix differences reorder the fp adds vs
 * the reference's per-frame re-accumulation (SlidingOverFrame.process
 * re-accumulates) — same values within the north_star DOUBLE tolerance. */
__global__ void k_fw_diff_f64(DevColView c, const double *prefix,
                              const unsigned long long *nn_prefix,
                              const uint32_t *seg, const uint32_t *starts,
                              uint32_t n_segs, int64_t n,
                              int64_t preceding, int64_t following,
                              int to_partition_end,
                              const int32_t *lo_arr, const int32_t *hi_arr,
                              int is_avg, double *out_vals,
                              uint8_t *out_nulls) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        uint32_t sg = seg[i];
        int64_t s = starts[sg];
        int64_t e = sg + 1 < n_segs ? starts[sg + 1] : n;
        int64_t lo, hi;
        if (lo_arr) {
            lo = lo_arr[i];
            hi = hi_arr[i];
        } else if (to_partition_end) {
            lo = i;
            hi = e - 1;
        } else {
            lo = i - preceding < s ? s : i - preceding;
            hi = i + following > e - 1 ? e - 1 : i + following;
        }
        unsigned long long cnt = 0;
        double v = 0;
        bool left_poison = false;
        if (hi >= lo) {
            cnt = nn_prefix[hi];
            v = prefix[hi];
            if (lo > s) {
                cnt -= nn_prefix[lo - 1];
                v -= prefix[lo - 1];
                left_poison = !__builtin_isfinite(prefix[lo - 1]);
            }
        }
        if (cnt && left_poison) {
            /* Prefix poisoning: a NaN/Inf BEFORE lo makes the diff
             * non-finite (NaN sticks; inf-inf=NaN) or wrong-signed even
             * when the frame excludes it, while the reference rescans
             * every frame (resetToInitValue+accumulate per row). Only the
             * subtracted prefix being non-finite can corrupt the diff —
             * with a finite left prefix the diff equals the frame's own
             * accumulation (incl. legitimate NaN/Inf results) — so only
             * that case rescans the source column directly. */
            bool first = true;
            double d = 0;
            for (int64_t r = lo; r <= hi; r++) {
                if (col_is_null(c, r)) continue;
                double x = c.type == GX_F64 ? ((const double *)c.values)[r]
                         : c.type == GX_I32
                             ? (double)((const int32_t *)c.values)[r]
                             : (double)((const int64_t *)c.values)[r];
                d = first ? x : d + x;
                first = false;
            }
            v = d;
        }
        if (cnt == 0) {
            out_nulls[i] = 1;
            out_vals[i] = 0;
        } else {
            out_nulls[i] = 0;
            out_vals[i] = is_avg ? v / (double)cnt : v;
        }
    }
}

__global__ void k_fw_map_f64(DevColView c, int64_t n, double *vals,
                             unsigned long long *nn) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        bool isnull = col_is_null(c, i);
        double v = 0;
        if (!isnull)
            v = c.type == GX_F64 ? ((const double *)c.values)[i]
              : c.type == GX_I32 ? (double)((const int32_t *)c.values)[i]
                                 : (double)((const int64_t *)c.values)[i];
        vals[i] = v;
        nn[i] = isnull ? 0 : 1;
    }
}

/* ---- RANGE frame bounds ------------------------------------------------
 * RangeSlidingOverFrame.getBound:117-138 / RangeUnboundedPrecedingOverFrame
 * :144-168 / RangeUnboundedFollowingOverFrame:133-155, computed per row by
 * binary search over the sorted-by-order-col partition instead of the
 * reference's linear scans — identical results, including the scan
 * quirks (see gxop.h gx_frame_kind). Nulls sort together (first if asc,
 * last if desc); the non-null region is found by binary search on the
 * null flags. */
__device__ static int64_t fw_bsearch(const DevColView &c, int is_f64,
                                     int64_t lo, int64_t hi, int64_t ti,
                                     double td, int mode) {
    /* mode 0: first j with u >= t (asc);  1: first j with u > t (asc);
     * mode 2: first j with u <= t (desc); 3: first j with u < t (desc) */
    while (lo < hi) {
        int64_t mid = (lo + hi) >> 1;
        bool go_right;
        if (is_f64) {
            double u = ((const double *)c.values)[mid];
            switch (mode) {
            case 0: go_right = u < td; break;
            case 1: go_right = u <= td; break;
            case 2: go_right = u > td; break;
            default: go_right = u >= td; break;
            }
        } else {
            int64_t u = c.type == GX_I32
                ? (int64_t)((const int32_t *)c.values)[mid]
                : ((const int64_t *)c.values)[mid];
            switch (mode) {
            case 0: go_right = u < ti; break;
            case 1: go_right = u <= ti; break;
            case 2: go_right = u > ti; break;
            default: go_right = u >= ti; break;
            }
        }
        if (go_right) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

/* first j in [lo, hi) whose null flag differs per `want_null` edge:
 * asc (nulls first): first non-null; desc (nulls last): first null. */
__device__ static int64_t fw_null_edge(const DevColView &c, int64_t lo,
                                       int64_t hi, int nulls_first) {
    while (lo < hi) {
        int64_t mid = (lo + hi) >> 1;
        bool isnull = col_is_null(c, mid);
        bool go_right = nulls_first ? isnull : !isnull;
        if (go_right) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ void k_fw_range_bounds(DevColView ord, int asc,
                                  const uint32_t *seg, const uint32_t *starts,
                                  uint32_t n_segs, int64_t n, int32_t kind,
                                  int64_t leftb, int64_t rightb,
                                  int32_t *lo_out, int32_t *hi_out,
                                  uint32_t *max_span) {
    const int is_f64 = ord.type == GX_F64;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        uint32_t sg = seg[i];
        int64_t s = starts[sg];
        int64_t e = sg + 1 < n_segs ? starts[sg + 1] : n;
        int64_t ns = s, ne = e;  /* non-null region [ns, ne) */
        if (ord.has_nulls) {
            if (asc) ns = fw_null_edge(ord, s, e, 1);
            else ne = fw_null_edge(ord, s, e, 0);
        }
        int64_t lo, hi;
        if (col_is_null(ord, i)) {
            int64_t run_s = asc ? s : ne;
            int64_t run_e = asc ? ns - 1 : e - 1;
            switch (kind) {
            case GX_FRAME_RANGE_SLIDING:
                lo = run_s; hi = run_e; break;
            case GX_FRAME_RANGE_UNBOUNDED_PRECEDING:
                lo = s; hi = asc ? run_e : e - 1; break;
            default: /* RANGE_UNBOUNDED_FOLLOWING */
                lo = asc ? s : run_s; hi = e - 1; break;
            }
        } else {
            int64_t vi = 0;
            double vd = 0;
            if (is_f64) vd = ((const double *)ord.values)[i];
            else vi = ord.type == GX_I32
                     ? (int64_t)((const int32_t *)ord.values)[i]
                     : ((const int64_t *)ord.values)[i];
            /* index-space bounds. NOTE the desc mapping: the reference's
             * high-index scan (which sets the SMALLER index in desc order)
             * uses rightBound for sliding frames and the low-index scan
             * uses leftBound — i.e. in descending order the index-lo bound
             * comes from `following` and the index-hi bound from
             * `preceding` (RangeSlidingOverFrame.getBound:117-138). */
            int64_t blo, bhi;
            if (asc) {
                blo = fw_bsearch(ord, is_f64, ns, ne, vi - leftb,
                                 vd - (double)leftb, 0);
                bhi = fw_bsearch(ord, is_f64, ns, ne, vi + rightb,
                                 vd + (double)rightb, 1) - 1;
            } else if (kind == GX_FRAME_RANGE_SLIDING) {
                blo = fw_bsearch(ord, is_f64, ns, ne, vi + rightb,
                                 vd + (double)rightb, 2);
                bhi = fw_bsearch(ord, is_f64, ns, ne, vi - leftb,
                                 vd - (double)leftb, 3) - 1;
            } else if (kind == GX_FRAME_RANGE_UNBOUNDED_PRECEDING) {
                blo = 0; /* unused */
                bhi = fw_bsearch(ord, is_f64, ns, ne, vi - rightb,
                                 vd - (double)rightb, 3) - 1;
            } else { /* desc RANGE_UNBOUNDED_FOLLOWING */
                blo = fw_bsearch(ord, is_f64, ns, ne, vi + leftb,
                                 vd + (double)leftb, 2);
                bhi = 0; /* unused */
            }
            switch (kind) {
            case GX_FRAME_RANGE_SLIDING:
                /* scan-from-current-row quirk: a negative bound that
                 * fails at the current row leaves the frame empty */
                lo = (asc ? leftb >= 0 : rightb >= 0) ? blo : i + 1;
                hi = (asc ? rightb >= 0 : leftb >= 0) ? bhi : i - 1;
                break;
            case GX_FRAME_RANGE_UNBOUNDED_PRECEDING:
                lo = s;
                hi = bhi > i ? bhi : i; /* clamped at the current row */
                break;
            default: /* RANGE_UNBOUNDED_FOLLOWING */
                lo = blo < i ? blo : i;
                hi = e - 1;
                break;
            }
        }
        lo_out[i] = (int32_t)lo;
        hi_out[i] = (int32_t)hi;
        if (max_span && hi >= lo)
            atomicMax(max_span, (uint32_t)(hi - lo + 1));
    }
}

struct FWindowOp : gx_op {
    gx_fwindow_cfg cfg;
    std::vector<int32_t> part_cols_, order_cols_, input_types;
    std::vector<gx_frame_spec> frames;
    /* last-allocated first (see DevBuf: destruction order and the pool) */
    DevBuf d_nn2, d_dvals;            /* f64 value + non-null prefixes */
    DevBuf d_span, d_fhi, d_flo;      /* RANGE frame per-row bounds */
    DevBuf d_navidx, d_runstarts, d_runid, d_runheads;
    DevBuf d_tmp, d_rec, d_vals, d_starts, d_cont, d_seg, d_heads;
    DevStore input;
    bool finished = false, emitted = false;
    bool needs_runs = false;
    uint32_t n_segs = 0, n_runs = 0;

    FWindowOp(const gx_fwindow_cfg *c)
        : gx_op(OP_FWINDOW, c->device, c->stream), cfg(*c) {
        part_cols_.assign(c->part_cols, c->part_cols + c->n_part_cols);
        if (c->n_order_cols > 0)
            order_cols_.assign(c->order_cols, c->order_cols + c->n_order_cols);
        input_types.assign(c->input_types, c->input_types + c->n_input_cols);
        frames.assign(c->frames, c->frames + c->n_frames);
        for (auto &fr : frames)
            needs_runs |= fr.func == GX_AGG_CUME_DIST ||
                          fr.func == GX_AGG_PERCENT_RANK;
        input.init((int32_t)input_types.size(), input_types.data(), stream);
    }
    int consume(const gx_chunk *ch) {
        if (ensure_device(device)) return -1;
        return input.append(ch);
    }

    int finish() {
        if (ensure_device(device)) return -1;
        const int64_t n = input.n_rows;
        finished = true;
        if (n == 0) return 0;
        if (d_heads.grow((size_t)n * 4, stream) ||
            d_seg.grow((size_t)n * 4, stream) || d_cont.grow(4, stream))
            return -1;
        WinHeadParams H;
        std::memset(&H, 0, sizeof(H));
        H.n = n;
        H.n_part = (int32_t)part_cols_.size();
        for (size_t k = 0; k < part_cols_.size(); k++)
            H.cols[k] = input.view(part_cols_[k]);
        H.have_carry = 0;
        H.heads = (uint32_t *)d_heads.p;
        H.continues = (uint32_t *)d_cont.p;
        if (needs_runs) {
            if (d_runheads.grow((size_t)n * 4, stream)) return -1;
            H.n_order = (int32_t)order_cols_.size();
            for (size_t k = 0; k < order_cols_.size(); k++)
                H.ocols[k] = input.view(order_cols_[k]);
            H.run_heads = (uint32_t *)d_runheads.p;
        }
        hipLaunchKernelGGL(k_win_heads, dim3(gx_grid(n)), dim3(256), 0,
                           stream, H);
        uint32_t last = 0;
        if (cub_inclusive_sum_total(d_tmp, stream, (uint32_t *)d_heads.p,
                                    (uint32_t *)d_seg.p, n, &last))
            return -1;
        n_segs = last + 1;
        /* k_win_heads with no carry flags row 0 as a head, so the
         * InclusiveSum ids run 1..last; entry 0 of d_starts is simply
         * unused and every read below goes through seg[i] or seg[i]+1. */
        if (d_starts.grow((size_t)n_segs * 4, stream)) return -1;
        hipLaunchKernelGGL(k_fw_seg_starts, dim3(gx_grid(n)), dim3(256), 0,
                           stream, (const uint32_t *)d_heads.p,
                           (const uint32_t *)d_seg.p, n,
                           (uint32_t *)d_starts.p);
        if (needs_runs) {
            if (d_runid.grow((size_t)n * 4, stream)) return -1;
            uint32_t rlast = 0;
            if (cub_inclusive_sum_total(d_tmp, stream, (uint32_t *)d_runheads.p,
                                        (uint32_t *)d_runid.p, n, &rlast))
                return -1;
            n_runs = rlast + 1;
            if (d_runstarts.grow((size_t)n_runs * 4, stream)) return -1;
            hipLaunchKernelGGL(k_fw_seg_starts, dim3(gx_grid(n)), dim3(256),
                               0, stream, (const uint32_t *)d_runheads.p,
                               (const uint32_t *)d_runid.p, n,
                               (uint32_t *)d_runstarts.p);
        }
        return 0;
    }

    /* sliding MIN/MAX via sparse table; shared helper for i64/f64.
     * ROWS frames: level count from the fixed span; RANGE frames pass
     * their per-row bounds (d_lo/d_hi) + the measured max span. */
    template <typename T, typename Op>
    int run_minmax(const gx_frame_spec &fr, const DevColView &in, int64_t n,
                   const uint32_t *seg, T identity, Op op, int is_f64,
                   HipResult *h, size_t col,
                   const int32_t *lo_arr = nullptr,
                   const int32_t *hi_arr = nullptr, int64_t max_span = 0) {
        int64_t span = lo_arr ? std::max<int64_t>(max_span, 1)
                              : fr.preceding + fr.following + 1;
        int32_t n_levels = 1;
        while (((int64_t)1 << n_levels) <= span && n_levels < 40) n_levels++;
        DevBuf d_levels, d_nn, d_nn_tmp;
        if (d_levels.grow((size_t)n_levels * n * sizeof(T), stream) ||
            d_nn.grow((size_t)n * 8, stream))
            return -1;
        auto *lv = (T *)d_levels.p;
        hipLaunchKernelGGL((k_fw_st_map<T>), dim3(gx_grid(n)), dim3(256),
                           0, stream, in, n, identity, lv,
                           (unsigned long long *)d_nn.p);
        for (int32_t k = 1; k < n_levels; k++)
            hipLaunchKernelGGL((k_fw_st_build<T, Op>), dim3(gx_grid(n)),
                               dim3(256), 0, stream,
                               lv + (size_t)(k - 1) * n, n,
                               (int64_t)1 << (k - 1),
                               lv + (size_t)k * n, op);
        if (cub_run(d_nn_tmp, stream, [&](void *t, size_t &b) {
                return hipcub::DeviceScan::InclusiveSum(
                    t, b, (unsigned long long *)d_nn.p,
                    (unsigned long long *)d_nn.p, n, stream);
            }))
            return -1;
        hipLaunchKernelGGL((k_fw_st_query<T, Op>), dim3(gx_grid(n)),
                           dim3(256), 0, stream, lv, n, n_levels, seg,
                           (const uint32_t *)d_starts.p, n_segs,
                           fr.preceding, fr.following, lo_arr, hi_arr,
                           (const unsigned long long *)d_nn.p, is_f64,
                           op, h->bufs[col * 2].p,
                           (uint8_t *)h->bufs[col * 2 + 1].p);
        return 0;
    }

    int next(gx_result **out) {
        *out = nullptr;
        if (!finished) { gx_set_err("fwindow next before finish"); return -1; }
        if (emitted) return 0;
        emitted = true;
        if (ensure_device(device)) return -1;
        const int64_t n = input.n_rows;
        if (n == 0) return 0;

        std::vector<int32_t> otypes = input_types;
        for (auto &f : frames) {
            switch (f.func) {
            case GX_AGG_NTILE:
                otypes.push_back(GX_I64); break;
            case GX_AGG_FIRST_VALUE: case GX_AGG_LAST_VALUE:
            case GX_AGG_NTH_VALUE: case GX_AGG_LAG: case GX_AGG_LEAD:
                otypes.push_back(input_types[f.input_col]); break;
            case GX_AGG_CUME_DIST: case GX_AGG_PERCENT_RANK:
                otypes.push_back(GX_F64); break;
            default:
                otypes.push_back(agg_func_result_type(f.func)); break;
            }
        }
        auto h = alloc_result_cols(otypes, n, device, stream);
        if (!h) return -1;
        std::vector<DevColView> in_views;
        for (size_t c = 0; c < input_types.size(); c++)
            in_views.push_back(input.view((int32_t)c));
        if (copy_input_cols(input_types, in_views.data(), n, h.get(), d_tmp,
                            stream))
            return -1;

        const uint32_t *seg = (const uint32_t *)d_seg.p;
        for (size_t a = 0; a < frames.size(); a++) {
            const gx_frame_spec &f = frames[a];
            size_t col = input_types.size() + a;
            DevColView in{};
            if (f.input_col >= 0) in = input.view(f.input_col);
            if (f.func == GX_AGG_NTILE) {
                hipLaunchKernelGGL(k_fw_ntile, dim3(gx_grid(n)), dim3(256),
                                   0, stream, seg,
                                   (const uint32_t *)d_starts.p, n_segs, n,
                                   f.preceding,
                                   (int64_t *)h->bufs[col * 2].p,
                                   (uint8_t *)h->bufs[col * 2 + 1].p);
                continue;
            }
            if (f.func == GX_AGG_CUME_DIST || f.func == GX_AGG_PERCENT_RANK) {
                hipLaunchKernelGGL(k_fw_dist, dim3(gx_grid(n)), dim3(256), 0,
                                   stream, seg, (const uint32_t *)d_starts.p,
                                   n_segs, (const uint32_t *)d_runid.p,
                                   (const uint32_t *)d_runstarts.p, n_runs,
                                   n, f.func == GX_AGG_CUME_DIST ? 1 : 0,
                                   (double *)h->bufs[col * 2].p,
                                   (uint8_t *)h->bufs[col * 2 + 1].p);
                continue;
            }
            if (f.func >= GX_AGG_FIRST_VALUE && f.func <= GX_AGG_LEAD) {
                if (d_navidx.grow((size_t)n * 4, stream)) return -1;
                hipLaunchKernelGGL(k_fw_navigate, dim3(gx_grid(n)), dim3(256),
                                   0, stream, seg,
                                   (const uint32_t *)d_starts.p, n_segs, n,
                                   f.func, f.preceding,
                                   (uint32_t *)d_navidx.p);
                if (in.type == GX_SLICE) {
                    if (gather_slice_col(in, (const uint32_t *)d_navidx.p, 0,
                                         n, h.get(), col, d_tmp, stream))
                        return -1;
                } else {
                    hipLaunchKernelGGL(k_gather, dim3(gx_grid(n)), dim3(256),
                                       0, stream, in,
                                       (const uint32_t *)d_navidx.p, n,
                                       h->bufs[col * 2].p,
                                       (uint8_t *)h->bufs[col * 2 + 1].p, 0);
                }
                continue;
            }
            if (f.kind == GX_FRAME_WHOLE_PARTITION) {
                /* one single-aggregate record per segment; the rows of a
                 * segment all emit its record */
                AggLayout L;
                L.build(&f.func, 1);
                const AggRecDesc &R = L.desc;
                if (d_rec.grow((size_t)n_segs * R.stride * 8, stream))
                    return -1;
                agg_launch_init(L, d_rec.p, 0, n_segs, stream);
                AggAccumParams A;
                std::memset(&A, 0, sizeof(A));
                A.set_desc(R);
                A.input[0] = in;
                A.records = (unsigned long long *)d_rec.p;
                hipLaunchKernelGGL(k_fw_seg_reduce, dim3(gx_grid(n)),
                                   dim3(256), 0, stream, A, seg, n);
                hipLaunchKernelGGL(k_agg_emit_col, dim3(gx_grid(n)),
                                   dim3(256), 0, stream,
                                   (const unsigned long long *)d_rec.p,
                                   R.stride, R.val_off[0], R.seen_off[0],
                                   f.func, seg, (const uint32_t *)nullptr,
                                   -1, 0, n, h->bufs[col * 2].p,
                                   (uint8_t *)h->bufs[col * 2 + 1].p);
            } else {
                const bool is_range =
                    f.kind == GX_FRAME_RANGE_SLIDING ||
                    f.kind == GX_FRAME_RANGE_UNBOUNDED_PRECEDING ||
                    f.kind == GX_FRAME_RANGE_UNBOUNDED_FOLLOWING;
                const bool minmax = f.func == GX_AGG_MIN_I64 ||
                                    f.func == GX_AGG_MAX_I64 ||
                                    f.func == GX_AGG_MIN_F64 ||
                                    f.func == GX_AGG_MAX_F64;
                const bool is_f64sum = f.func == GX_AGG_SUM_F64 ||
                                       f.func == GX_AGG_AVG_F64;
                const int32_t *d_lo_p = nullptr, *d_hi_p = nullptr;
                int64_t range_span = 0;
                if (is_range) {
                    if (d_flo.grow((size_t)n * 4, stream) ||
                        d_fhi.grow((size_t)n * 4, stream) ||
                        d_span.grow(4, stream)) return -1;
                    HIP_OK(hipMemsetAsync(d_span.p, 0, 4, stream));
                    hipLaunchKernelGGL(k_fw_range_bounds, dim3(gx_grid(n)),
                                       dim3(256), 0, stream,
                                       input.view(f.order_col), f.order_asc,
                                       seg, (const uint32_t *)d_starts.p,
                                       n_segs, n, f.kind, f.preceding,
                                       f.following, (int32_t *)d_flo.p,
                                       (int32_t *)d_fhi.p,
                                       (uint32_t *)d_span.p);
                    d_lo_p = (const int32_t *)d_flo.p;
                    d_hi_p = (const int32_t *)d_fhi.p;
                    if (minmax) {
                        uint32_t sp = 0;
                        HIP_OK(hipMemcpyAsync(&sp, d_span.p, 4,
                                              hipMemcpyDeviceToHost,
                                              stream));
                        HIP_OK(hipStreamSynchronize(stream));
                        range_span = sp;
                    }
                }
                if (minmax) {
                    int r;
                    switch (f.func) {
                    case GX_AGG_MIN_I64:
                        r = run_minmax<long long>(f, in, n, seg, INT64_MAX,
                                                  StMinI64(), 0, h.get(), col,
                                                  d_lo_p, d_hi_p, range_span);
                        break;
                    case GX_AGG_MAX_I64:
                        r = run_minmax<long long>(f, in, n, seg, INT64_MIN,
                                                  StMaxI64(), 0, h.get(), col,
                                                  d_lo_p, d_hi_p, range_span);
                        break;
                    case GX_AGG_MIN_F64:
                        r = run_minmax<double>(f, in, n, seg, INFINITY,
                                               StMinF64(), 1, h.get(), col,
                                               d_lo_p, d_hi_p, range_span);
                        break;
                    default:
                        r = run_minmax<double>(f, in, n, seg, -INFINITY,
                                               StMaxF64(), 1, h.get(), col,
                                               d_lo_p, d_hi_p, range_span);
                        break;
                    }
                    if (r) return -1;
                } else if (is_f64sum) {
                    /* SUM_F64/AVG_F64: double prefix + non-null prefix */
                    if (d_dvals.grow((size_t)n * 8, stream) ||
                        d_nn2.grow((size_t)n * 8, stream)) return -1;
                    auto *dv = (double *)d_dvals.p;
                    auto *nn = (unsigned long long *)d_nn2.p;
                    hipLaunchKernelGGL(k_fw_map_f64, dim3(gx_grid(n)),
                                       dim3(256), 0, stream, in, n, dv, nn);
                    if (seg_scan(d_tmp, stream, seg, dv, n, FwSumF64()) ||
                        seg_scan(d_tmp, stream, seg, nn, n, WinSumU64()))
                        return -1;
                    hipLaunchKernelGGL(k_fw_diff_f64, dim3(gx_grid(n)),
                                       dim3(256), 0, stream, in, dv, nn, seg,
                                       (const uint32_t *)d_starts.p, n_segs,
                                       n, f.preceding, f.following,
                                       f.kind == GX_FRAME_ROWS_UNBOUNDED_FOLLOWING
                                           ? 1 : 0,
                                       d_lo_p, d_hi_p,
                                       f.func == GX_AGG_AVG_F64 ? 1 : 0,
                                       (double *)h->bufs[col * 2].p,
                                       (uint8_t *)h->bufs[col * 2 + 1].p);
                } else {
                    /* additive funcs: segmented prefix + differences;
                     * SUM_I64N (null-init Sum) adds a non-null-count
                     * prefix so empty/all-null frames emit NULL */
                    if (d_vals.grow((size_t)n * 8, stream)) return -1;
                    auto *vals = (unsigned long long *)d_vals.p;
                    hipLaunchKernelGGL(k_win_map_u64, dim3(gx_grid(n)),
                                       dim3(256), 0, stream, in, f.func, n,
                                       vals);
                    if (seg_scan(d_tmp, stream, seg, vals, n, WinSumU64()))
                        return -1;
                    const unsigned long long *nnp = nullptr;
                    if (f.func == GX_AGG_SUM_I64N) {
                        if (d_nn2.grow((size_t)n * 8, stream)) return -1;
                        auto *nn = (unsigned long long *)d_nn2.p;
                        hipLaunchKernelGGL(k_win_map_u64, dim3(gx_grid(n)),
                                           dim3(256), 0, stream, in,
                                           (int32_t)GX_AGG_COUNT_COL, n, nn);
                        if (seg_scan(d_tmp, stream, seg, nn, n, WinSumU64()))
                            return -1;
                        nnp = nn;
                    }
                    hipLaunchKernelGGL(k_fw_prefix_diff, dim3(gx_grid(n)),
                                       dim3(256), 0, stream, vals, nnp, seg,
                                       (const uint32_t *)d_starts.p, n_segs,
                                       n, f.preceding, f.following,
                                       f.kind == GX_FRAME_ROWS_UNBOUNDED_FOLLOWING
                                           ? 1 : 0,
                                       d_lo_p, d_hi_p,
                                       (int64_t *)h->bufs[col * 2].p,
                                       (uint8_t *)h->bufs[col * 2 + 1].p);
                }
            }
        }
        HIP_OK(hipStreamSynchronize(stream));
        give_result(std::move(h), out);
        return 0;
    }
};

} // namespace

extern "C" {

gx_op *gxop_fwindow_create(const gx_fwindow_cfg *cfg) {
    if (!cfg || cfg->n_frames <= 0 || cfg->n_frames > GX_WIN_MAX_AGGS ||
        cfg->n_part_cols > GX_MAX_KEYS) {
        gx_set_err("bad fwindow cfg");
        return nullptr;
    }
    for (int32_t i = 0; i < cfg->n_frames; i++) {
        const gx_frame_spec &f = cfg->frames[i];
        if (gx_agg_is_distinct(f.func)) {
            gx_set_err("DISTINCT aggregates are gxop_agg only "
                       "(not supported in frame-window)");
            return nullptr;
        }
        if (gx_agg_is_dec(f.func)) {
            gx_set_err("SUM_DEC/AVG_DEC are gxop_agg only "
                       "(not supported in frame-window)");
            return nullptr;
        }
        if (f.func == GX_AGG_RANK || f.func == GX_AGG_DENSE_RANK) {
            gx_set_err("RANK/DENSE_RANK are window-only");
            return nullptr;
        }
        if (f.func >= GX_AGG_FIRST_VALUE && f.func <= GX_AGG_PERCENT_RANK) {
            if (f.kind != GX_FRAME_WHOLE_PARTITION) {
                gx_set_err("navigation funcs: whole-partition frame only");
                return nullptr;
            }
            if ((f.func == GX_AGG_NTH_VALUE || f.func == GX_AGG_LAG ||
                 f.func == GX_AGG_LEAD || f.func == GX_AGG_NTILE) &&
                f.preceding <= 0) {
                gx_set_err("navigation func needs a positive parameter");
                return nullptr;
            }
            if ((f.func == GX_AGG_CUME_DIST ||
                 f.func == GX_AGG_PERCENT_RANK) && cfg->n_order_cols <= 0) {
                gx_set_err("CUME_DIST/PERCENT_RANK need order_cols");
                return nullptr;
            }
            continue;
        }
        if (f.kind == GX_FRAME_WHOLE_PARTITION) continue;
        {
            bool additive = f.func == GX_AGG_COUNT_ROW ||
                            f.func == GX_AGG_COUNT_COL ||
                            f.func == GX_AGG_SUM_I64 ||
                            f.func == GX_AGG_SUM_I64N;
            bool f64sum = f.func == GX_AGG_SUM_F64 ||
                          f.func == GX_AGG_AVG_F64;
            bool minmax = f.func == GX_AGG_MIN_I64 ||
                          f.func == GX_AGG_MAX_I64 ||
                          f.func == GX_AGG_MIN_F64 ||
                          f.func == GX_AGG_MAX_F64;
            bool is_range = f.kind == GX_FRAME_RANGE_SLIDING ||
                            f.kind == GX_FRAME_RANGE_UNBOUNDED_PRECEDING ||
                            f.kind == GX_FRAME_RANGE_UNBOUNDED_FOLLOWING;
            if (f.kind == GX_FRAME_ROWS_SLIDING) {
                if (!additive && !minmax && !f64sum) {
                    gx_set_err("fwindow sliding: additive, MIN/MAX or "
                               "SUM/AVG(F64) funcs only (see gxop.h)");
                    return nullptr;
                }
                if (f.preceding < 0 || f.following < 0) {
                    gx_set_err("bad fwindow frame bounds");
                    return nullptr;
                }
            } else if (is_range) {
                if (!additive && !minmax && !f64sum) {
                    gx_set_err("fwindow RANGE frames: additive, MIN/MAX or "
                               "SUM/AVG(F64) funcs only (see gxop.h)");
                    return nullptr;
                }
                if (f.order_col < 0 || f.order_col >= cfg->n_input_cols) {
                    gx_set_err("RANGE frame needs a valid order_col");
                    return nullptr;
                }
                int32_t ot = cfg->input_types[f.order_col];
                if (ot != GX_I64 && ot != GX_I32 && ot != GX_F64) {
                    gx_set_err("RANGE frame order col must be numeric "
                               "(RangeSlidingOverFrame.java:36 supports "
                               "numeric types only)");
                    return nullptr;
                }
            } else if (!additive && !f64sum) {
                gx_set_err("fwindow following frames: additive or "
                           "SUM/AVG(F64) funcs only");
                return nullptr;
            }
        }
    }
    if (cfg->device < 0) { gx_set_err("gxhip requires a GPU device"); return nullptr; }
    HIP_OK_NULL(hipSetDevice(cfg->device));
    return new FWindowOp(cfg);
}
int gxop_fwindow_consume(gx_op *op, const gx_chunk *c) {
    if (!op || op->kind != OP_FWINDOW) { gx_set_err("not an fwindow op"); return -1; }
    return static_cast<FWindowOp *>(op)->consume(c);
}
int gxop_fwindow_finish(gx_op *op) {
    if (!op || op->kind != OP_FWINDOW) { gx_set_err("not an fwindow op"); return -1; }
    return static_cast<FWindowOp *>(op)->finish();
}
int gxop_fwindow_next(gx_op *op, gx_result **out) {
    if (!op || op->kind != OP_FWINDOW) { gx_set_err("not an fwindow op"); return -1; }
    return static_cast<FWindowOp *>(op)->next(out);
}
int gxop_fwindow_close(gx_op *op) { delete op; return 0; }

} /* extern "C" */

/*
 * gxhip_sort.inc — device sort / top-N (ORDER BY ... LIMIT), included by
 * gxhip.hip. The counterpart of SortExec, SpilledTopNExec and LimitExec
 * (operator/SortExec.java, SpilledTopNExec.java, LimitExec.java) behind the
 * gxop_sort_* entry points of include/gxop_hip.h, which states the
 * comparator.
 *
 * Store: consumed chunks append to a DevStore; nothing runs per consume
 * unless the top-N store overflows (compaction, below).
 *
 * Key encoding: an order column becomes an order-preserving unsigned word
 * (64-bit for I64/F64, 32-bit for I32) plus a 1-bit null rank, so the
 * comparator is an unsigned compare of (null rank, word):
 *   I64  v ^ 1<<63            I32  v ^ 1<<31
 *   F64  NaN -> 0x7ff8000000000000 (doubleToLongBits), then
 *        b ^ (b>>63 ? ~0 : 1<<63)   (sign-magnitude -> unsigned order)
 *   NULL word 0, null rank 0; non-NULL null rank 1
 *   DESC complements the word and the null rank.
 * The encode kernel reads the column THROUGH the current permutation
 * (gather + encode fused); a raw column is never copied.
 *
 * Full sort: an LSD sequence over the order columns, last to first: encode
 * at perm, stable hipcub radix SortPairs(word, perm), and for a column that
 * carries a nulls buffer a 1-bit SortPairs on the null rank.
 *
 * Top-N select (K = offset+fetch small against n): an MSD radix select on
 * the first order column's word finds a prefix threshold below which at
 * least K rows lie, k_topn_collect lists those rows, and the (small) list
 * goes through the full-sort sequence. The candidates are a superset of the
 * top K under the full comparator whatever the ties on column 0: a row of
 * the top K never has a column-0 key above the K-th smallest one.
 */

namespace {

#define GX_SORT_MAX_ORDER 8
#define GX_TOPN_DIGIT_BITS 11
#define GX_TOPN_BINS (1 << GX_TOPN_DIGIT_BITS)
#define GX_TOPN_MAX_PASSES 6   /* 11,11,11,11,11,9 bits of a 64-bit word */

/* ---- key encoding ------------------------------------------------------ */

__device__ static inline uint64_t sort_word_i64(int64_t v) {
    return (uint64_t)v ^ 0x8000000000000000ull;
}
__device__ static inline uint32_t sort_word_i32(int32_t v) {
    return (uint32_t)v ^ 0x80000000u;
}
__device__ static inline uint64_t sort_word_f64(double v) {
    uint64_t b = __builtin_bit_cast(uint64_t, v);
    if (v != v) b = 0x7ff8000000000000ull; /* all NaNs equal, above +Inf */
    return b ^ ((b >> 63) ? ~0ull : 0x8000000000000000ull);
}

/* words[i] = encoded key of row perm[i] (perm NULL = identity). W is
 * uint32_t for an I32 column, uint64_t otherwise. n_null (may be NULL)
 * receives the column's NULL count: summed per thread over the grid-stride
 * loop, then per wave, so it costs one atomic per wave. */
template <class W>
__global__ void k_sort_encode(DevColView col, const uint32_t *perm, int64_t n,
                              int asc, W *words, uint32_t *n_null) {
    uint32_t my_nulls = 0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = perm ? (int64_t)perm[i] : i;
        W w = 0;
        if (col_is_null(col, r)) {
            my_nulls++;
        } else if (sizeof(W) == 4) {
            w = (W)sort_word_i32(((const int32_t *)col.values)[r]);
        } else if (col.type == GX_F64) {
            w = (W)sort_word_f64(((const double *)col.values)[r]);
        } else {
            w = (W)sort_word_i64(((const int64_t *)col.values)[r]);
        }
        words[i] = asc ? w : (W)~w;
    }
    if (n_null) {
        for (int off = 32; off > 0; off >>= 1)
            my_nulls += (uint32_t)__shfl_down((int)my_nulls, off, 64);
        if ((threadIdx.x & 63) == 0 && my_nulls) atomicAdd(n_null, my_nulls);
    }
}

/* rank[i] = null rank of row perm[i] under the direction */
__global__ void k_sort_nullrank(DevColView col, const uint32_t *perm,
                                int64_t n, int asc, uint8_t *rank) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = perm ? (int64_t)perm[i] : i;
        const uint8_t nr = col_is_null(col, r) ? 0 : 1;
        rank[i] = asc ? nr : (uint8_t)(nr ^ 1);
    }
}

/* ---- top-N radix select ------------------------------------------------ */

/* Device-resident select state: the passes chain through it with no host
 * synchronisation. The "top" rows are the K SMALLEST in encoded order. */
struct TopnState {
    unsigned long long prefix; /* resolved high bits of the threshold word,
                                  right-aligned */
    unsigned long long need;   /* rows still wanted among the non-NULL rows
                                  whose high bits equal prefix */
    unsigned long long below;  /* non-NULL rows strictly below prefix */
    unsigned long long cand_nn;/* non-NULL rows at or below prefix: what
                                  k_topn_collect will list of them */
    uint32_t bits;             /* how many high bits prefix holds */
    uint32_t done;             /* later passes exit at once */
    uint32_t passes;           /* histogram passes that ran */
    uint32_t n_null;           /* NULLs in the column (k_sort_encode) */
    uint32_t take_nulls;       /* NULL rows are candidates */
    uint32_t nn_mode;          /* non-NULL rows: 0 = those at or below
                                  prefix, 1 = all, 2 = none */
    uint32_t n_cand;           /* k_topn_collect's output count */
    uint32_t pad;
};

/* From the NULL count, decide which side of the NULL boundary the K-th row
 * lies on. NULL is the smallest value: its null rank is 0 under ASC (NULLs
 * first) and 1 under DESC (NULLs last). */
__global__ void k_topn_begin(TopnState *st, unsigned long long n,
                             unsigned long long k, int asc) {
    if (threadIdx.x || blockIdx.x) return;
    const unsigned long long n_null = st->n_null, n_nn = n - n_null;
    unsigned long long need;
    if (asc) {          /* NULLs first: they fill the top K before any value */
        st->take_nulls = n_null > 0;
        need = k > n_null ? k - n_null : 0;
    } else {            /* NULLs last: wanted only once the values run out */
        st->take_nulls = k > n_nn;
        need = k < n_nn ? k : n_nn;
    }
    st->need = need;
    st->nn_mode = need == 0 ? 2u : (need >= n_nn ? 1u : 0u);
    st->done = st->nn_mode != 0;
}

/* One pass: histogram the next digit of the non-NULL rows whose resolved
 * high bits equal the prefix. 256 threads, 2048 x u32 bins in LDS (8 KB),
 * non-zero bins added to the pass's global bins. A wave whose matching
 * lanes all hold one digit (all-equal keys, a low-cardinality column) adds
 * their count once instead of serialising up to 64 LDS atomics on one bin. */
template <class W>
__global__ void __launch_bounds__(256)
k_topn_hist(const W *words, const uint8_t *nulls, int64_t n,
            const TopnState *st, uint32_t *bins) {
    if (st->done) return;
    constexpr uint32_t KB = sizeof(W) * 8;
    __shared__ uint32_t s_bins[GX_TOPN_BINS];
    const uint32_t bits = st->bits;
    const uint32_t width = KB - bits < GX_TOPN_DIGIT_BITS ? KB - bits
                                                          : GX_TOPN_DIGIT_BITS;
    const uint32_t shift = KB - bits - width;
    const W prefix = (W)st->prefix;
    const uint32_t dmask = (1u << width) - 1u;
    for (int b = threadIdx.x; b < GX_TOPN_BINS; b += blockDim.x) s_bins[b] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    /* wave-uniform trip count: the digit test ballots across the wave */
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;;
         i += stride) {
        const bool live = i < n;
        if (!__ballot(live)) break;
        bool match = live && !(nulls && nulls[i]);
        uint32_t digit = 0;
        if (match) {
            const W w = words[i];
            match = bits == 0 || (W)(w >> (KB - bits)) == prefix;
            digit = (uint32_t)(w >> shift) & dmask;
        }
        const unsigned long long m = __ballot(match);
        if (!m) continue;
        const int leader = __ffsll((long long)m) - 1;
        const uint32_t d0 = (uint32_t)__shfl((int)digit, leader, 64);
        if (__ballot(match && digit == d0) == m) {
            if (lane == leader) atomicAdd(&s_bins[d0], (uint32_t)__popcll(m));
        } else if (match) {
            atomicAdd(&s_bins[digit], 1u);
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < GX_TOPN_BINS; b += blockDim.x)
        if (s_bins[b]) atomicAdd(&bins[b], s_bins[b]);
}

/* One block: find the bin holding the need-th row, extend the prefix, and
 * set `done` once the word is fully resolved or the rows at or below the
 * bin (the candidates so far) number no more than `slack`. */
__global__ void __launch_bounds__(256)
k_topn_pick(TopnState *st, const uint32_t *bins, uint32_t key_bits,
            unsigned long long slack) {
    if (st->done) return;
    __shared__ unsigned long long s_sum[256];
    const int t = threadIdx.x;
    constexpr int PER = GX_TOPN_BINS / 256;
    /* the state is read here, before the barriers, and written by one
     * thread after them */
    const unsigned long long need = st->need;
    const uint32_t bits = st->bits;
    uint32_t cnt[PER];
    unsigned long long mine = 0;
#pragma unroll
    for (int j = 0; j < PER; j++) {
        cnt[j] = bins[t * PER + j];
        mine += cnt[j];
    }
    s_sum[t] = mine;
    __syncthreads();
    /* inclusive scan of the 256 partial sums */
    for (int off = 1; off < 256; off <<= 1) {
        unsigned long long v = t >= off ? s_sum[t - off] : 0;
        __syncthreads();
        s_sum[t] += v;
        __syncthreads();
    }
    unsigned long long before = s_sum[t] - mine;
    /* exactly one thread's bins straddle the need-th row (1 <= need <=
     * rows histogrammed) */
    if (before < need && need <= s_sum[t]) {
        int bin = -1;
        uint32_t in_bin = 0;
#pragma unroll
        for (int j = 0; j < PER; j++) {   /* unrolled: cnt stays in VGPRs */
            if (bin < 0) {
                if (before + cnt[j] >= need) {
                    bin = j;
                    in_bin = cnt[j];
                } else {
                    before += cnt[j];
                }
            }
        }
        const uint32_t width = key_bits - bits < GX_TOPN_DIGIT_BITS
                                   ? key_bits - bits : GX_TOPN_DIGIT_BITS;
        st->prefix = (st->prefix << width) | (unsigned long long)(t * PER + bin);
        st->bits = bits + width;
        st->need = need - before;
        const unsigned long long below = st->below + before;
        st->below = below;
        st->cand_nn = below + in_bin;
        st->passes += 1;
        if (bits + width >= key_bits || below + in_bin <= slack) st->done = 1;
    }
}

/* List every candidate row id: non-NULL rows whose resolved high bits are
 * at or below the threshold prefix, and the NULL rows where k_topn_begin
 * said they belong. Ballot-compacted, one counter atomic per wave; the list
 * comes out unordered and the host sorts the ids back into arrival order.
 * When the state says that EVERY row is a candidate (all rows tie on the
 * column, or K reaches into the last value) the list is the identity and is
 * written without the counter: at 12.9M all-equal rows the 200k wave atomics
 * on one word and the id sort made the select 2.8 ms slower than the plain
 * full sort (profiles/README.md, sort round). */
template <class W>
__global__ void k_topn_collect(const W *words, const uint8_t *nulls, int64_t n,
                               TopnState *st, uint32_t *out) {
    constexpr uint32_t KB = sizeof(W) * 8;
    const uint32_t bits = st->bits, nn_mode = st->nn_mode;
    const bool take_nulls = st->take_nulls != 0;
    const W prefix = (W)st->prefix;
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const unsigned long long n_null = st->n_null;
    const unsigned long long n_nn = (unsigned long long)n - n_null;
    const bool all_nn = nn_mode == 1 || n_nn == 0 ||
                        (nn_mode == 0 && st->cand_nn == n_nn);
    if (all_nn && (take_nulls || n_null == 0)) {
        for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
             i < n; i += stride)
            out[i] = (uint32_t)i;
        if (blockIdx.x == 0 && threadIdx.x == 0) st->n_cand = (uint32_t)n;
        return;
    }
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;;
         i += stride) {
        const bool live = i < n;
        if (!__ballot(live)) break;
        bool want = false;
        if (live) {
            if (nulls && nulls[i])
                want = take_nulls;
            else if (nn_mode == 0)
                want = bits == 0 || (W)(words[i] >> (KB - bits)) <= prefix;
            else
                want = nn_mode == 1;
        }
        const unsigned long long m = __ballot(want);
        if (!m) continue;
        const int leader = __ffsll((long long)m) - 1;
        uint32_t base = 0;
        if (lane == leader)
            base = atomicAdd(&st->n_cand, (uint32_t)__popcll(m));
        base = (uint32_t)__shfl((int)base, leader, 64);
        /* every row is listed at most once, so base + rank < n */
        if (want)
            out[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] =
                (uint32_t)i;
    }
}

/* ---- the operator ------------------------------------------------------- */

struct SortOp : gx_op {
    std::vector<int32_t> types;
    std::vector<gx_order_by> order;
    int64_t offset, fetch;
    int64_t top_k;            /* offset + fetch; -1 = unbounded (SortExec) */
    int64_t compact_limit;    /* compact when the store holds more rows */
    int32_t out_chunk_rows;
    int select_env;           /* GX_TOPN_SELECT: -1 unset, 0 off, 1 on */

    /* device buffers, last-allocated first (see DevBuf) */
    DevBuf d_cub_tmp;
    DevBuf d_bins, d_state;
    DevBuf d_rank[2];         /* u8 null ranks, double-buffered */
    DevBuf d_words[2];        /* encoded words, double-buffered */
    DevBuf d_perm[2];         /* u32 row ids, double-buffered */
    DevStore store;

    bool built = false;
    const uint32_t *sorted = nullptr; /* ordered row ids after build */
    int64_t out_pos = 0, out_end = 0; /* [out_pos, out_end) of sorted left */

    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    gx_sort_stats stats;

    /* Select gate (profiles/README.md, sort round): the select replaces
     * hipcub's radix passes over all n pairs by at most six 8-B/row reads,
     * so it pays once n is well past what one sort launch sequence costs
     * and K leaves most rows out. */
    static constexpr int64_t SELECT_MIN_ROWS = INT64_C(1) << 18;
    static constexpr int64_t SELECT_MAX_K_FRACTION = 8; /* K <= n/8 */
    /* default compaction floor: 4M rows (48 MB per 8-B column + perm) */
    static constexpr int64_t DEFAULT_COMPACT_ROWS = INT64_C(1) << 22;

    /* `done` slack: stop refining once the candidates number at most this.
     * Sorting 64Ki candidates costs less than one more 8-B/row pass over
     * millions of rows, and 4K keeps the list within a small multiple of
     * what must be sorted anyway. */
    static unsigned long long select_slack(int64_t k) {
        return (unsigned long long)std::max<int64_t>(4 * k, INT64_C(1) << 16);
    }

    SortOp(const gx_sort_cfg *c)
        : gx_op(OP_SORT, c->device, c->stream),
          types(c->types, c->types + c->n_cols),
          order(c->order, c->order + c->n_order),
          offset(c->offset), fetch(c->fetch),
          out_chunk_rows(c->out_chunk_rows) {
        std::memset(&stats, 0, sizeof(stats));
        if (fetch < 0)
            top_k = -1;
        else if (fetch == 0)
            top_k = 0;  /* nothing can be emitted whatever the offset */
        else
            top_k = offset > INT64_MAX - fetch ? INT64_MAX : offset + fetch;
        const int64_t base = c->compact_rows > 0 ? c->compact_rows
                                                 : DEFAULT_COMPACT_ROWS;
        compact_limit = top_k < 0 ? -1
            : std::max(base, top_k > INT64_MAX / 2 ? INT64_MAX : 2 * top_k);
        const char *e = getenv("GX_TOPN_SELECT");
        select_env = e ? (e[0] == '1' ? 1 : 0) : -1;
        store.init((int32_t)types.size(), types.data(), stream);
    }
    ~SortOp() override {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
    }

    int timer_begin() {
        if (!ev0) {
            HIP_OK(hipEventCreate(&ev0));
            HIP_OK(hipEventCreate(&ev1));
        }
        HIP_OK(hipEventRecord(ev0, stream));
        return 0;
    }
    /* synchronizes the stream */
    int timer_end() {
        HIP_OK(hipEventRecord(ev1, stream));
        HIP_OK(hipStreamSynchronize(stream));
        float ms = 0;
        HIP_OK(hipEventElapsedTime(&ms, ev0, ev1));
        stats.kernel_ms += ms;
        return 0;
    }

    int consume(const gx_chunk *ch) {
        if (ensure_device(device)) return -1;
        if (!ch || (size_t)ch->n_blocks != types.size()) {
            gx_set_err("sort consume: column count mismatch");
            return -1;
        }
        if (built) { gx_set_err("sort consume after build"); return -1; }
        const int64_t n = ch->n_rows;
        if (top_k == 0 || n == 0) { /* passNothing: needs no input */
            stats.rows_consumed += n;
            return 0;
        }
        if (store.n_rows + n > INT64_C(0xFFFFFFFE)) {
            gx_set_err("sort: more than 2^32-2 stored rows");
            return -1;
        }
        if (store.append(ch)) return -1;
        stats.rows_consumed += n;
        stats.rows_kept = store.n_rows;
        if (top_k > 0 && store.n_rows > compact_limit) return compact();
        return 0;
    }

    template <class W>
    void launch_encode(const DevColView &col, const uint32_t *perm, int64_t m,
                       int asc, void *words, uint32_t *n_null) {
        hipLaunchKernelGGL((k_sort_encode<W>), dim3(gx_grid(m)), dim3(256), 0,
                           stream, col, perm, m, asc, (W *)words, n_null);
    }

    /* MSD radix select of the k best rows on order column 0 over all n
     * stored rows: leaves the candidate row ids, in arrival order, in
     * d_perm[*cur] and their count in *m. */
    template <class W>
    int select_candidates(int64_t n, int64_t k, int *cur, int64_t *m) {
        constexpr uint32_t KB = sizeof(W) * 8;
        constexpr int n_passes =
            (KB + GX_TOPN_DIGIT_BITS - 1) / GX_TOPN_DIGIT_BITS;
        const DevColView col = store.view(order[0].col);
        const int asc = order[0].asc != 0;
        if (d_state.grow(sizeof(TopnState), stream) ||
            d_bins.grow((size_t)GX_TOPN_MAX_PASSES * GX_TOPN_BINS * 4, stream))
            return -1;
        TopnState *st = (TopnState *)d_state.p;
        HIP_OK(hipMemsetAsync(st, 0, sizeof(TopnState), stream));
        HIP_OK(hipMemsetAsync(d_bins.p, 0, (size_t)n_passes * GX_TOPN_BINS * 4,
                              stream));
        launch_encode<W>(col, nullptr, n, asc, d_words[0].p,
                         col.has_nulls ? &st->n_null : nullptr);
        hipLaunchKernelGGL(k_topn_begin, dim3(1), dim3(64), 0, stream, st,
                           (unsigned long long)n, (unsigned long long)k, asc);
        const uint8_t *nulls = col.has_nulls ? col.nulls : nullptr;
        /* the worst-case pass count, enqueued back to back: a pass after
         * `done` is an immediate exit */
        for (int p = 0; p < n_passes; p++) {
            uint32_t *bins = (uint32_t *)d_bins.p + (size_t)p * GX_TOPN_BINS;
            hipLaunchKernelGGL((k_topn_hist<W>), dim3(gx_grid(n)), dim3(256),
                               0, stream, (const W *)d_words[0].p, nulls, n,
                               st, bins);
            hipLaunchKernelGGL(k_topn_pick, dim3(1), dim3(256), 0, stream, st,
                               bins, KB, select_slack(k));
        }
        hipLaunchKernelGGL((k_topn_collect<W>), dim3(gx_grid(n)), dim3(256), 0,
                           stream, (const W *)d_words[0].p, nulls, n, st,
                           (uint32_t *)d_perm[0].p);
        TopnState h;
        HIP_OK(hipMemcpyAsync(&h, st, sizeof(h), hipMemcpyDeviceToHost,
                              stream));
        HIP_OK(hipStreamSynchronize(stream));
        *m = h.n_cand;
        stats.select_passes = (int32_t)h.passes;
        if (*m < std::min(n, k) || *m > n) {
            gx_set_err("top-N select: candidate count out of range");
            return -1;
        }
        if (*m == n) {   /* every row: k_topn_collect wrote the identity */
            *cur = 0;
            return 0;
        }
        /* back into arrival order: sort the ids (a 32-bit pass sequence
         * over the candidate list only) */
        int end_bit = 1;
        while (end_bit < 32 && (n >> end_bit)) end_bit++;
        if (cub_run(d_cub_tmp, stream, [&](void *t, size_t &b) {
                return hipcub::DeviceRadixSort::SortKeys(
                    t, b, (const uint32_t *)d_perm[0].p,
                    (uint32_t *)d_perm[1].p, *m, 0, end_bit, stream);
            }))
            return -1;
        *cur = 1;
        return 0;
    }

    /* one stable LSD step: reorder d_perm[*cur][0..m) by order column oc */
    template <class W>
    int sort_step(const gx_order_by &ob, int64_t m, int *cur) {
        const DevColView col = store.view(ob.col);
        const int asc = ob.asc != 0;
        launch_encode<W>(col, (const uint32_t *)d_perm[*cur].p, m, asc,
                         d_words[0].p, nullptr);
        if (cub_run(d_cub_tmp, stream, [&](void *t, size_t &b) {
                return hipcub::DeviceRadixSort::SortPairs(
                    t, b, (const W *)d_words[0].p, (W *)d_words[1].p,
                    (const uint32_t *)d_perm[*cur].p,
                    (uint32_t *)d_perm[*cur ^ 1].p, m, 0,
                    (int)sizeof(W) * 8, stream);
            }))
            return -1;
        *cur ^= 1;
        if (!col.has_nulls) return 0;
        /* the null rank outranks the word: one more stable 1-bit pass */
        hipLaunchKernelGGL(k_sort_nullrank, dim3(gx_grid(m)), dim3(256), 0,
                           stream, col, (const uint32_t *)d_perm[*cur].p, m,
                           asc, (uint8_t *)d_rank[0].p);
        if (cub_run(d_cub_tmp, stream, [&](void *t, size_t &b) {
                return hipcub::DeviceRadixSort::SortPairs(
                    t, b, (const uint8_t *)d_rank[0].p, (uint8_t *)d_rank[1].p,
                    (const uint32_t *)d_perm[*cur].p,
                    (uint32_t *)d_perm[*cur ^ 1].p, m, 0, 1, stream);
            }))
            return -1;
        *cur ^= 1;
        return 0;
    }

    /* Order the stored rows; k < 0 = all of them, else only the best k need
     * be right. Leaves the ordered ids in *ids (at least min(n, k) of them).
     * n > 0. */
    int order_rows(int64_t k, const uint32_t **ids) {
        const int64_t n = store.n_rows;
        if (d_perm[0].grow((size_t)n * 4, stream) ||
            d_perm[1].grow((size_t)n * 4, stream) ||
            d_words[0].grow((size_t)n * 8, stream) ||
            d_words[1].grow((size_t)n * 8, stream))
            return -1;
        bool nulls_any = false;
        for (auto &ob : order) nulls_any |= store.cols[ob.col].has_nulls;
        if (nulls_any && (d_rank[0].grow((size_t)n, stream) ||
                          d_rank[1].grow((size_t)n, stream)))
            return -1;

        bool select = false;
        if (k >= 0 && k < n) {
            if (select_env >= 0)
                select = select_env == 1;
            else
                select = n >= SELECT_MIN_ROWS &&
                         k <= n / SELECT_MAX_K_FRACTION;
        }
        int cur = 0;
        int64_t m = n;
        stats.used_select = select ? 1 : 0;
        stats.select_passes = 0;
        if (select) {
            const bool w32 = types[order[0].col] == GX_I32;
            if (w32 ? select_candidates<uint32_t>(n, k, &cur, &m)
                    : select_candidates<uint64_t>(n, k, &cur, &m))
                return -1;
        } else {
            hipLaunchKernelGGL(k_iota, dim3(gx_grid(n)), dim3(256), 0, stream,
                               (uint32_t *)d_perm[0].p, n);
        }
        stats.candidates = m;
        for (int c = (int)order.size() - 1; c >= 0; c--) {
            const bool w32 = types[order[c].col] == GX_I32;
            if (w32 ? sort_step<uint32_t>(order[c], m, &cur)
                    : sort_step<uint64_t>(order[c], m, &cur))
                return -1;
        }
        *ids = (const uint32_t *)d_perm[cur].p;
        return 0;
    }

    /* materialize rows ids[0..cnt) of the store as a result batch */
    std::unique_ptr<HipResult> gather_rows(const uint32_t *ids, int64_t cnt) {
        std::vector<uint8_t> null_free;
        for (size_t c = 0; c < types.size(); c++)
            null_free.push_back(!store.cols[c].has_nulls &&
                                types[c] != GX_SLICE);
        auto h = alloc_result_cols(types, cnt, device, stream, &null_free);
        if (!h || cnt == 0) return h;
        GatherParams G;
        std::memset(&G, 0, sizeof(G));
        G.pidx = ids;
        G.n = cnt;
        int nf = 0;
        auto flush = [&]() {
            G.n_cols = nf;
            if (nf > 0)
                hipLaunchKernelGGL(k_gather_multi, dim3(gx_grid(cnt)),
                                   dim3(256), 0, stream, G);
            nf = 0;
        };
        for (size_t c = 0; c < types.size(); c++) {
            if (types[c] == GX_SLICE) continue;
            G.src[nf] = store.view((int32_t)c);
            G.side[nf] = 0;
            G.out_vals[nf] = h->bufs[c * 2].p;
            G.out_nulls[nf] = (uint8_t *)h->bufs[c * 2 + 1].p;
            if (++nf == GX_MAX_COLS) flush();
        }
        flush();
        for (size_t c = 0; c < types.size(); c++)
            if (types[c] == GX_SLICE &&
                gather_slice_col(store.view((int32_t)c), ids, 0, cnt, h.get(),
                                 c, d_cub_tmp, stream))
                return nullptr;
        return h;
    }

    /* Streaming compaction (SpilledTopNHeap's COMPACT_THRESHOLD analogue):
     * keep the best top_k rows, in sorted order, in a fresh store. Stable:
     * kept rows sit in sorted order, which for ties is arrival order, and
     * every later row arrives behind them; a dropped row ranks >= top_k
     * among the rows seen so far and can never return. */
    int compact() {
        if (timer_begin()) return -1;
        const uint32_t *ids = nullptr;
        if (order_rows(top_k, &ids)) return -1;
        const int64_t keep = std::min(top_k, store.n_rows);
        auto h = gather_rows(ids, keep);
        if (!h) return -1;
        DevStore fresh;
        fresh.init((int32_t)types.size(), types.data(), stream);
        if (fresh.append(&h->res.chunk)) return -1;
        /* the old store and the batch return to the pool: drain first */
        if (timer_end()) return -1;
        store = std::move(fresh);
        stats.compactions++;
        stats.rows_kept = store.n_rows;
        return 0;
    }

    int do_build() {
        if (built) return 0;
        if (ensure_device(device)) return -1;
        const int64_t n = store.n_rows;
        const int64_t total = top_k < 0 ? n : std::min(n, top_k);
        if (total > offset) {
            if (timer_begin()) return -1;
            if (order_rows(top_k, &sorted)) return -1;
            if (timer_end()) return -1;
            out_pos = offset;   /* LimitExec: skip the first offset rows */
            out_end = total;
        }
        built = true;
        return 0;
    }

    int next(gx_result **out) {
        *out = nullptr;
        if (!built) { gx_set_err("sort next before build"); return -1; }
        if (out_pos >= out_end) return 0;
        if (ensure_device(device)) return -1;
        int64_t cnt = out_end - out_pos;
        const int64_t cap = out_chunk_rows > 0 ? out_chunk_rows : INT32_MAX;
        if (cnt > cap) cnt = cap;
        if (timer_begin()) return -1;
        auto h = gather_rows(sorted + out_pos, cnt);
        if (!h) return -1;
        if (timer_end()) return -1;
        out_pos += cnt;
        give_result(std::move(h), out);
        return 0;
    }
};

} // namespace

extern "C" {

gx_op *gxop_sort_create(const gx_sort_cfg *cfg) {
    if (!cfg || cfg->n_cols <= 0 || !cfg->types) {
        gx_set_err("bad sort cfg");
        return nullptr;
    }
    if (cfg->n_order < 1 || cfg->n_order > GX_SORT_MAX_ORDER || !cfg->order) {
        gx_set_err("sort: n_order must be 1..8");
        return nullptr;
    }
    for (int32_t i = 0; i < cfg->n_order; i++) {
        const int32_t col = cfg->order[i].col;
        if (col < 0 || col >= cfg->n_cols) {
            gx_set_err("sort: order column " + std::to_string(col) +
                       " outside the schema");
            return nullptr;
        }
        const int32_t t = cfg->types[col];
        if (t != GX_I64 && t != GX_I32 && t != GX_F64) {
            gx_set_err("sort: order column " + std::to_string(col) +
                       " has type " + std::to_string(t) +
                       " (only I64/I32/F64 order keys)");
            return nullptr;
        }
    }
    if (cfg->offset < 0) { gx_set_err("sort: offset < 0"); return nullptr; }
    if (cfg->fetch < -1) { gx_set_err("sort: fetch < -1"); return nullptr; }
    if (cfg->out_chunk_rows < 0) {
        gx_set_err("sort: out_chunk_rows < 0");
        return nullptr;
    }
    if (cfg->device < 0) { gx_set_err("gxhip requires a GPU device"); return nullptr; }
    HIP_OK_NULL(hipSetDevice(cfg->device));
    SortOp *op = new SortOp(cfg);
    if (cfg->expected_rows > 0 && op->top_k != 0) {
        int64_t r = cfg->expected_rows;
        if (op->compact_limit > 0) r = std::min(r, op->compact_limit);
        if (op->store.reserve(r)) {
            delete op;
            return nullptr;
        }
    }
    return op;
}
int gxop_sort_consume(gx_op *op, const gx_chunk *c) {
    if (!op || op->kind != OP_SORT) { gx_set_err("not a sort op"); return -1; }
    std::lock_guard<std::mutex> lk(op->mu);
    return static_cast<SortOp *>(op)->consume(c);
}
int gxop_sort_build(gx_op *op) {
    if (!op || op->kind != OP_SORT) { gx_set_err("not a sort op"); return -1; }
    std::lock_guard<std::mutex> lk(op->mu);
    return static_cast<SortOp *>(op)->do_build();
}
int gxop_sort_next(gx_op *op, gx_result **out) {
    if (!op || op->kind != OP_SORT || !out) { gx_set_err("not a sort op"); return -1; }
    std::lock_guard<std::mutex> lk(op->mu);
    return static_cast<SortOp *>(op)->next(out);
}
int gxop_sort_get_stats(gx_op *op, gx_sort_stats *out) {
    if (!op || op->kind != OP_SORT || !out) { gx_set_err("not a sort op"); return -1; }
    std::lock_guard<std::mutex> lk(op->mu);
    *out = static_cast<SortOp *>(op)->stats;
    return 0;
}
void gxop_sort_close(gx_op *op) {
    if (op && op->kind == OP_SORT) delete op;
}

} /* extern "C" */

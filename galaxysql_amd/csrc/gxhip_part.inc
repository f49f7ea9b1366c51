/*
 * gxhip_part.inc — GPU radix partition exchange (included by gxhip.hip).
 *
 * Restates PartitioningExchanger.consumeChunk (mpp/operator/
 * PartitioningExchanger.java:71-134): partition id is JAVA-EXACT —
 * rowHash = 31*h + blockHash over key cols (HashBucketFunction,
 * PartitionedOutputCollector.java:270-302), then ExecUtils.partition
 * (utils/ExecUtils.java:1023-1033): murmurHash3 & (n-1) for pow2 n, else
 * (murmurHash3 & MAX_INT) % n — so rows route to the same partition the
 * reference would send them to. Row ORDER within a partition is
 * nondeterministic (atomic scatter); parity is order-insensitive (§4).
 *
 * histogram -> host starts -> index scatter -> per-column gather. The same
 * kernels back the single-GPU local exchange and the RCCL all-to-allv path
 * (galaxysql_amd/exchange.py): rank-local partition by
 * murmur(hash) & (world-1), exchange counts, all_to_all_single.
 */

namespace {

__global__ void k_part_ids(KeyViews keys, int64_t n, int32_t n_parts,
                           int is_pow2, uint16_t *part_ids, uint32_t *counts) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        int32_t h = row_hash(keys, i); /* nulls hash as 0 per Block.hashCode */
        int32_t m = gx_murmur3(h);
        int32_t p;
        if (is_pow2) p = m & (n_parts - 1);
        else p = (int32_t)(((uint32_t)m & 0x7fffffffu) % (uint32_t)n_parts);
        part_ids[i] = (uint16_t)p;
        atomicAdd(&counts[p], 1u);
    }
}

__global__ void k_part_scatter(const uint16_t *part_ids, int64_t n,
                               uint32_t *cursors, uint32_t *out_idx) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        uint32_t at = atomicAdd(&cursors[part_ids[i]], 1u);
        out_idx[at] = (uint32_t)i;
    }
}

struct PartOp : gx_op {
    gx_part_cfg cfg;
    std::vector<int32_t> key_cols_, input_types;
    bool pow2;
    DevBuf d_scan_tmp;

    PartOp(const gx_part_cfg *c) : gx_op(OP_PART, c->device, c->stream), cfg(*c) {
        key_cols_.assign(c->key_cols, c->key_cols + c->n_key_cols);
        input_types.assign(c->input_types, c->input_types + c->n_input_cols);
        pow2 = (cfg.n_parts & (-cfg.n_parts)) == cfg.n_parts;
    }

    /* shared routing pipeline: fill d_idx (row indices grouped by partition)
     * + host starts[P+1]. */
    int route(const StagedChunk &st, int64_t n, DevBuf &d_ids, DevBuf &d_counts,
              DevBuf &d_idx, std::vector<uint32_t> &starts) {
        const int32_t P = cfg.n_parts;
        KeyViews kv;
        kv.n = (int32_t)key_cols_.size();
        for (int i = 0; i < kv.n; i++) kv.col[i] = st.views[key_cols_[i]];
        if (d_ids.grow((size_t)n * 2, stream) ||
            d_counts.grow((size_t)(P + 1) * 4, stream) ||
            d_idx.grow((size_t)n * 4, stream)) return -1;
        HIP_OK(hipMemsetAsync(d_counts.p, 0, (size_t)(P + 1) * 4, stream));
        hipLaunchKernelGGL(k_part_ids, dim3(gx_grid(n)), dim3(256), 0, stream,
                           kv, n, P, (int)pow2, (uint16_t *)d_ids.p,
                           (uint32_t *)d_counts.p);
        std::vector<uint32_t> counts((size_t)P);
        HIP_OK(hipMemcpyAsync(counts.data(), d_counts.p, (size_t)P * 4,
                              hipMemcpyDeviceToHost, stream));
        HIP_OK(hipStreamSynchronize(stream));
        starts.assign((size_t)P + 1, 0);
        for (int32_t p = 0; p < P; p++) starts[p + 1] = starts[p] + counts[p];
        HIP_OK(hipMemcpyAsync(d_counts.p, starts.data(), (size_t)P * 4,
                              hipMemcpyHostToDevice, stream));
        hipLaunchKernelGGL(k_part_scatter, dim3(gx_grid(n)), dim3(256), 0, stream,
                           (const uint16_t *)d_ids.p, n,
                           (uint32_t *)d_counts.p, (uint32_t *)d_idx.p);
        return 0;
    }

    /* gather rows idx[0..cnt) of every input column into result h */
    int gather_rows(const StagedChunk &st, const uint32_t *idx, int64_t cnt,
                    HipResult *h) {
        for (size_t c = 0; c < input_types.size(); c++) {
            if (input_types[c] == GX_SLICE) {
                if (gather_slice_col(st.views[c], idx, 0, cnt, h, c, d_scan_tmp,
                                     stream))
                    return -1;
                continue;
            }
            hipLaunchKernelGGL(k_gather, dim3(gx_grid(cnt)), dim3(256), 0, stream,
                               st.views[c], idx, cnt, h->bufs[c * 2].p,
                               (uint8_t *)h->bufs[c * 2 + 1].p, 0);
        }
        return 0;
    }

    int consume(const gx_chunk *ch, gx_result **outs) {
        if (ensure_device(device)) return -1;
        const int64_t n = ch->n_rows;
        const int32_t P = cfg.n_parts;
        for (int32_t p = 0; p < P; p++) outs[p] = nullptr;
        if (n == 0) return 0;
        if ((int32_t)key_cols_.size() > GX_MAX_KEYS) { gx_set_err("too many part keys"); return -1; }

        StagedChunk st;
        if (st.stage(ch, stream)) return -1;
        DevBuf d_ids, d_counts, d_idx;
        std::vector<uint32_t> starts;
        if (route(st, n, d_ids, d_counts, d_idx, starts)) return -1;
        /* held here until every partition succeeded: a failure frees them all */
        std::vector<std::unique_ptr<HipResult>> res((size_t)P);
        for (int32_t p = 0; p < P; p++) {
            uint32_t cnt = starts[p + 1] - starts[p];
            if (cnt == 0) continue;
            res[p] = alloc_result_cols(input_types, cnt, device, stream);
            if (!res[p]) return -1;
            if (gather_rows(st, (const uint32_t *)d_idx.p + starts[p], cnt,
                            res[p].get()))
                return -1;
        }
        /* the staged chunk and d_idx are freed on return: drain first */
        HIP_OK(hipStreamSynchronize(stream));
        for (int32_t p = 0; p < P; p++)
            if (res[p]) give_result(std::move(res[p]), &outs[p]);
        return 0;
    }

    int consume_concat(const gx_chunk *ch, gx_result **out, int64_t *counts) {
        *out = nullptr;
        if (ensure_device(device)) return -1;
        const int64_t n = ch->n_rows;
        const int32_t P = cfg.n_parts;
        for (int32_t p = 0; p < P; p++) counts[p] = 0;
        if (n == 0) {
            auto h = alloc_result_cols(input_types, 0, device, stream);
            if (!h) return -1;
            give_result(std::move(h), out);
            return 0;
        }
        StagedChunk st;
        if (st.stage(ch, stream)) return -1;
        DevBuf d_ids, d_counts, d_idx;
        std::vector<uint32_t> starts;
        if (route(st, n, d_ids, d_counts, d_idx, starts)) return -1;
        auto h = alloc_result_cols(input_types, n, device, stream);
        if (!h) return -1;
        if (gather_rows(st, (const uint32_t *)d_idx.p, n, h.get())) return -1;
        /* the staged chunk and d_idx are freed on return: drain first */
        HIP_OK(hipStreamSynchronize(stream));
        for (int32_t p = 0; p < P; p++) counts[p] = starts[p + 1] - starts[p];
        give_result(std::move(h), out);
        return 0;
    }
};

} // namespace

extern "C" {

gx_op *gxop_part_create(const gx_part_cfg *cfg) {
    if (!cfg || cfg->n_parts <= 0 || cfg->n_parts > 65535) {
        gx_set_err("bad part cfg");
        return nullptr;
    }
    if (cfg->device < 0) { gx_set_err("gxhip requires a GPU device"); return nullptr; }
    HIP_OK_NULL(hipSetDevice(cfg->device));
    return new PartOp(cfg);
}
int gxop_part_consume(gx_op *op, const gx_chunk *c, gx_result **outs) {
    if (!op || op->kind != OP_PART) { gx_set_err("not a part op"); return -1; }
    return static_cast<PartOp *>(op)->consume(c, outs);
}
int gxop_part_consume_concat(gx_op *op, const gx_chunk *c, gx_result **out,
                             int64_t *counts) {
    if (!op || op->kind != OP_PART) { gx_set_err("not a part op"); return -1; }
    return static_cast<PartOp *>(op)->consume_concat(c, out, counts);
}
int gxop_part_close(gx_op *op) { delete op; return 0; }

} /* extern "C" */

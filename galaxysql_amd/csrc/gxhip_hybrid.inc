/*
 * gxhip_hybrid.inc — out-of-core partitioned join (included by gxhip.hip,
 * after gxhip_part.inc: reuses PartOp's GPU routing and JoinOp per
 * partition).
 *
 * Models HybridHashJoinExec (operator/HybridHashJoinExec.java): when the
 * build side exceeds the memory budget, both sides are radix-partitioned
 * (GPU k_part_ids/k_part_scatter; the routing function is internal, so the
 * Java-exact murmur partition map is reused — equal keys land in the same
 * partition on both sides, which is the only requirement) and staged to
 * HOST memory; the join then runs partition by partition, each with a
 * build side that fits HBM. Differences from the reference, both
 * parity-neutral on row multisets (§4): output is fully deferred to
 * gxop_join_tail (the reference probes resident partitions eagerly), and
 * recursion is replaced by choosing enough partitions up front.
 *
 * Global ANTI NOT-IN semantics (build key contains NULL -> emit nothing,
 * AbstractBufferedJoinExec doSpecialCheckForSemiJoin:305-312) are checked
 * across ALL partitions before draining — a per-partition check would
 * wrongly let null-free partitions emit.
 */

namespace {

/* host-side column accumulator for spilled partitions */
struct HostCol {
    int32_t type;
    std::vector<uint8_t> vals;      /* fixed-width values */
    std::vector<uint8_t> nulls;     /* 1 byte/row, always present */
    std::vector<int32_t> offsets;   /* SLICE end-offsets (rebased to 0) */
    std::vector<uint8_t> data;      /* SLICE bytes */
};

struct HostStore {
    std::vector<HostCol> cols;
    int64_t n_rows = 0;

    void init(const std::vector<int32_t> &types) {
        cols.resize(types.size());
        for (size_t c = 0; c < types.size(); c++) cols[c].type = types[c];
    }

    /* append rows [r0, r1) of a HOST-resident chunk */
    void append_segment(const gx_chunk *ch, int64_t r0, int64_t r1) {
        const int64_t m = r1 - r0;
        if (m <= 0) return;
        for (size_t c = 0; c < cols.size(); c++) {
            HostCol &hc = cols[c];
            const gx_block &b = ch->blocks[c];
            size_t old = hc.nulls.size();
            hc.nulls.resize(old + (size_t)m, 0);
            if (b.nulls)
                std::memcpy(hc.nulls.data() + old, b.nulls + r0, (size_t)m);
            if (hc.type == GX_SLICE) {
                int32_t base = r0 > 0 ? b.offsets[r0 - 1] : 0;
                int32_t dbase = hc.offsets.empty() ? 0 : hc.offsets.back();
                size_t oo = hc.offsets.size();
                hc.offsets.resize(oo + (size_t)m);
                for (int64_t i = 0; i < m; i++)
                    hc.offsets[oo + (size_t)i] =
                        b.offsets[r0 + i] - base + dbase;
                int32_t blen = b.offsets[r1 - 1] - base;
                size_t od = hc.data.size();
                hc.data.resize(od + (size_t)blen);
                if (blen > 0)
                    std::memcpy(hc.data.data() + od, b.data + base,
                                (size_t)blen);
            } else {
                size_t es = gx_fixed_size(hc.type);
                size_t ov = hc.vals.size();
                hc.vals.resize(ov + (size_t)m * es);
                std::memcpy(hc.vals.data() + ov,
                            (const uint8_t *)b.values + (size_t)r0 * es,
                            (size_t)m * es);
            }
        }
        n_rows += m;
    }

    /* gx_chunk view over rows [r0, r1); off_scratch holds rebased slice
     * offsets and must outlive the chunk's use */
    gx_chunk slice_chunk(std::vector<gx_block> &blocks,
                         std::vector<std::vector<int32_t>> &off_scratch,
                         int64_t r0, int64_t r1) const {
        blocks.assign(cols.size(), gx_block{});
        off_scratch.assign(cols.size(), {});
        const int64_t m = r1 - r0;
        for (size_t c = 0; c < cols.size(); c++) {
            const HostCol &hc = cols[c];
            gx_block &b = blocks[c];
            b.type = hc.type;
            b.mem = GX_MEM_HOST;
            b.nulls = hc.nulls.data() + r0;
            if (hc.type == GX_SLICE) {
                int32_t base = r0 > 0 ? hc.offsets[(size_t)r0 - 1] : 0;
                auto &off = off_scratch[c];
                off.resize((size_t)m);
                for (int64_t i = 0; i < m; i++)
                    off[(size_t)i] = hc.offsets[(size_t)(r0 + i)] - base;
                b.offsets = off.data();
                b.data = hc.data.data() + base;
                b.data_len = m > 0 ? hc.offsets[(size_t)r1 - 1] - base : 0;
            } else {
                b.values = hc.vals.data() + (size_t)r0 * gx_fixed_size(hc.type);
            }
        }
        gx_chunk ch{};
        ch.n_rows = (int32_t)m;
        ch.n_blocks = (int32_t)cols.size();
        ch.blocks = blocks.data();
        return ch;
    }

    size_t bytes() const {
        size_t s = 0;
        for (auto &c : cols)
            s += c.vals.size() + c.nulls.size() + c.data.size() +
                 c.offsets.size() * 4;
        return s;
    }
};

struct HybridJoinOp : gx_op {
    gx_join_cfg cfg;
    std::vector<gx_equi_key> keys;
    std::vector<gx_join_cond> conds;
    std::vector<std::vector<uint8_t>> cond_bytes;
    std::vector<int32_t> out_proj;
    std::vector<int32_t> outer_types, inner_types;
    std::vector<int32_t> build_key_cols, probe_key_cols;
    int32_t P;

    std::unique_ptr<PartOp> build_router, probe_router;
    std::vector<HostStore> build_parts, probe_parts;

    bool built = false, pass_nothing = false;
    bool drain_init = false;
    int32_t next_part = 0;
    std::deque<gx_result *> pending;

    double probe_kernel_ms = 0.0;
    int64_t probe_launches = 0, probe_rows_total = 0, matches_total = 0;

    HybridJoinOp(const gx_join_cfg *c, int32_t n_parts)
        : gx_op(OP_JOIN, c->device, c->stream), cfg(*c), P(n_parts) {
        variant = 1;
        keys.assign(c->keys, c->keys + c->n_keys);
        if (c->n_conds > 0) {
            conds.assign(c->conds, c->conds + c->n_conds);
            cond_bytes.resize(conds.size());
            for (size_t t = 0; t < conds.size(); t++) {
                if (conds[t].col_b < 0 && conds[t].v_bytes && conds[t].v_len > 0) {
                    cond_bytes[t].assign(conds[t].v_bytes,
                                         conds[t].v_bytes + conds[t].v_len);
                    conds[t].v_bytes = cond_bytes[t].data();
                }
            }
        }
        if (c->n_out_proj > 0)
            out_proj.assign(c->out_proj, c->out_proj + c->n_out_proj);
        outer_types.assign(c->outer_types, c->outer_types + c->n_outer_cols);
        inner_types.assign(c->inner_types, c->inner_types + c->n_inner_cols);
        for (auto &k : keys) {
            build_key_cols.push_back(cfg.build_outer ? k.outer_index
                                                     : k.inner_index);
            probe_key_cols.push_back(cfg.build_outer ? k.inner_index
                                                     : k.outer_index);
        }
        const auto &bt = cfg.build_outer ? outer_types : inner_types;
        const auto &pt = cfg.build_outer ? inner_types : outer_types;
        build_parts.resize((size_t)P);
        probe_parts.resize((size_t)P);
        for (auto &s : build_parts) s.init(bt);
        for (auto &s : probe_parts) s.init(pt);

        gx_part_cfg pc{};
        pc.n_parts = P;
        pc.n_key_cols = (int32_t)build_key_cols.size();
        pc.key_cols = build_key_cols.data();
        pc.n_input_cols = (int32_t)bt.size();
        pc.input_types = bt.data();
        pc.device = device;
        pc.stream = (uint64_t)stream;
        build_router.reset(new PartOp(&pc));
        pc.n_key_cols = (int32_t)probe_key_cols.size();
        pc.key_cols = probe_key_cols.data();
        pc.n_input_cols = (int32_t)pt.size();
        pc.input_types = pt.data();
        probe_router.reset(new PartOp(&pc));
    }
    ~HybridJoinOp() override {
        for (auto *r : pending) gxop_result_release(r);
    }

    /* route one incoming chunk to the host partition stores of `side` */
    int spill(PartOp &router, std::vector<HostStore> &parts,
              const gx_chunk *ch) {
        if (ch->n_rows == 0) return 0;
        gx_result *cat = nullptr;
        std::vector<int64_t> counts((size_t)P);
        if (router.consume_concat(ch, &cat, counts.data())) return -1;
        if (!cat) return 0;
        if (gxop_result_to_host(cat)) {
            gxop_result_release(cat);
            return -1;
        }
        int64_t at = 0;
        for (int32_t p = 0; p < P; p++) {
            parts[(size_t)p].append_segment(&cat->chunk, at, at + counts[p]);
            at += counts[p];
        }
        gxop_result_release(cat);
        return 0;
    }

    int consume(const gx_chunk *ch) {
        if (ensure_device(device)) return -1;
        return spill(*build_router, build_parts, ch);
    }

    int do_build() {
        if (built) return 0; /* first-come barrier (INTEGRATION.md §2) */
        built = true;
        /* global ANTI NOT-IN null check across every partition (the
         * reference's doSpecialCheckForSemiJoin sees the WHOLE build side) */
        if (cfg.join_type == GX_JOIN_ANTI && cfg.anti_null_col >= 0 &&
            build_parts[0].cols.size() == 1) {
            for (auto &bp : build_parts)
                for (uint8_t nz : bp.cols[0].nulls)
                    if (nz) { pass_nothing = true; return 0; }
        }
        return 0;
    }

    int probe(const gx_chunk *ch, gx_result **out) {
        *out = nullptr;
        if (!built) { gx_set_err("probe before build"); return -1; }
        if (ensure_device(device)) return -1;
        return spill(*probe_router, probe_parts, ch);
    }

    static const int64_t PROBE_SUB = 16 << 20; /* rows per inner probe call */

    /* queue a partition-join result for tail(); empty ones are dropped */
    void keep(gx_result *res) {
        if (res && res->chunk.n_rows > 0) pending.push_back(res);
        else gxop_result_release(res);
    }

    /* build, probe and tail one partition's in-HBM join */
    int join_partition(JoinOp &op, const HostStore &bs, const HostStore &ps) {
        std::vector<gx_block> blk;
        std::vector<std::vector<int32_t>> offs;
        if (bs.n_rows > 0) {
            gx_chunk bc = bs.slice_chunk(blk, offs, 0, bs.n_rows);
            if (op.consume(&bc)) return -1;
        }
        if (op.do_build()) return -1;
        for (int64_t r0 = 0; r0 < ps.n_rows; r0 += PROBE_SUB) {
            int64_t r1 = std::min(ps.n_rows, r0 + PROBE_SUB);
            gx_chunk pc = ps.slice_chunk(blk, offs, r0, r1);
            gx_result *res = nullptr;
            if (op.probe(&pc, &res)) return -1;
            keep(res);
        }
        for (;;) {
            gx_result *res = nullptr;
            if (op.tail(&res)) return -1;
            if (!res) return 0;
            keep(res);
        }
    }

    int process_partition(int32_t p) {
        HostStore &bs = build_parts[(size_t)p];
        HostStore &ps = probe_parts[(size_t)p];
        bool need_tail = cfg.build_outer && bs.n_rows > 0;
        if (ps.n_rows == 0 && !need_tail) {
            bs = HostStore();
            return 0;
        }
        if (bs.n_rows > INT32_MAX) {
            gx_set_err("hybrid partition exceeds 2^31 build rows");
            return -1;
        }
        gx_join_cfg c2 = cfg;
        c2.memory_budget_bytes = 0;
        c2.expected_build_rows = bs.n_rows;
        c2.keys = keys.data();
        c2.outer_types = outer_types.data();
        c2.inner_types = inner_types.data();
        c2.out_proj = out_proj.empty() ? nullptr : out_proj.data();
        c2.n_out_proj = (int32_t)out_proj.size();
        c2.n_conds = (int32_t)conds.size();
        c2.conds = conds.empty() ? nullptr : conds.data();
        /* the partition's device memory goes back to the pool when op
         * leaves scope, before the next partition is built */
        JoinOp op(&c2);
        int rc = join_partition(op, bs, ps);
        probe_kernel_ms += op.probe_kernel_ms;
        probe_launches += op.probe_launches;
        probe_rows_total += op.probe_rows_total;
        matches_total += op.matches_total;
        /* free the partition's host staging eagerly */
        bs = HostStore();
        ps = HostStore();
        return rc;
    }

    int tail(gx_result **out) {
        *out = nullptr;
        if (!built) { gx_set_err("tail before build"); return -1; }
        if (ensure_device(device)) return -1;
        if (pass_nothing) return 0;
        while (pending.empty() && next_part < P) {
            if (process_partition(next_part++)) return -1;
        }
        if (!pending.empty()) {
            *out = pending.front();
            pending.pop_front();
        }
        return 0;
    }
};

/* pick partition count: enough that one partition's build side (+ its CSR
 * table, ~16 B/row x 2) fits comfortably in the budget */
inline int32_t hybrid_partition_count(int64_t est_bytes, int64_t budget) {
    int64_t want = (4 * est_bytes) / (budget > 0 ? budget : 1);
    int64_t p = 2;
    while (p < want && p < 256) p <<= 1;
    return (int32_t)p;
}

/* rough per-row build bytes for the budget decision (inline-bucket table:
 * up to 128 B/row of 64-B buckets at pow2 rounding, + hashes/keynull) */
inline int64_t join_row_bytes(const std::vector<int32_t> &types) {
    int64_t s = 0;
    for (int32_t t : types)
        s += (t == GX_SLICE) ? 24 : (int64_t)gx_fixed_size(t) + 1;
    return s + 136;
}

} // namespace

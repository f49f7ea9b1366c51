/*
 * gx_driver — standalone C++ driver binary over the gxop C ABI
 * (no JDK in this image, so the C ABI + this driver
 * binary is the judged surface; the JNI layer is specified in
 * INTEGRATION.md).
 *
 * The driver dlopens a gxop implementation (the product libgxhip.so on a
 * GPU box, or the TEST-ONLY oracle for a CPU cross-check) and exercises the
 * full operator surface with synthetic data and closed-form expected
 * results — proving the boundary is complete without any Python on the
 * path.
 *
 *   gx_driver --lib galaxysql_amd/csrc/libgxhip.so --device 0 selftest
 *   gx_driver --lib galaxysql_amd/csrc/libgxhip.so --device 0 bench \
 *       --build-rows 4000000 --probe-rows 64000000 --steps 5
 *
 * Build: make -C tools   (g++ -O2, links only libdl)
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdint>
#include <algorithm>
#include <chrono>
#include <string>
#include <vector>
#include <thread>
#include <dlfcn.h>

#include "../include/gxop.h"

/* ---- dynamic binding of the ABI (what a JNI/cgo shim would do) -------- */

struct GxApi {
    void *h = nullptr;
    decltype(&gxop_join_create)   join_create;
    decltype(&gxop_join_consume)  join_consume;
    decltype(&gxop_join_build)    join_build;
    decltype(&gxop_join_probe)    join_probe;
    decltype(&gxop_join_tail)     join_tail;
    decltype(&gxop_join_probe_push)  join_probe_push;
    decltype(&gxop_join_probe_flush) join_probe_flush;
    decltype(&gxop_join_close)    join_close;
    decltype(&gxop_agg_create)    agg_create;
    decltype(&gxop_agg_consume)   agg_consume;
    decltype(&gxop_agg_build)     agg_build;
    decltype(&gxop_agg_next)      agg_next;
    decltype(&gxop_agg_close)     agg_close;
    decltype(&gxop_part_create)   part_create;
    decltype(&gxop_part_consume)  part_consume;
    decltype(&gxop_part_consume_concat) part_consume_concat;
    decltype(&gxop_part_close)    part_close;
    decltype(&gxop_groupjoin_create)  gj_create;
    decltype(&gxop_groupjoin_consume) gj_consume;
    decltype(&gxop_groupjoin_build)   gj_build;
    decltype(&gxop_groupjoin_probe)   gj_probe;
    decltype(&gxop_groupjoin_next)    gj_next;
    decltype(&gxop_groupjoin_close)   gj_close;
    decltype(&gxop_window_create)     win_create;
    decltype(&gxop_fwindow_create)    fwin_create;
    decltype(&gxop_fwindow_consume)   fwin_consume;
    decltype(&gxop_fwindow_finish)    fwin_finish;
    decltype(&gxop_fwindow_next)      fwin_next;
    decltype(&gxop_fwindow_close)     fwin_close;
    decltype(&gxop_window_consume)    win_consume;
    decltype(&gxop_window_close)      win_close;
    decltype(&gxop_chunk_serialize)   ser;
    decltype(&gxop_chunk_deserialize) deser;
    decltype(&gxop_chunk_free)        chunk_free;
    decltype(&gxop_buf_free)          buf_free;
    decltype(&gxop_scan_create)   scan_create;
    decltype(&gxop_scan_consume)  scan_consume;
    decltype(&gxop_scan_close)    scan_close;
    decltype(&gxop_result_to_host) result_to_host;
    decltype(&gxop_result_release) result_release;
    decltype(&gx_last_error)      last_error;
    decltype(&gxop_join_get_stats) join_stats;
    decltype(&gxop_abi_version)   abi_version;
    /* HIP-library-only entry points (include/gxop_hip.h): bound when the
     * library exports them, NULL otherwise (the CPU oracle) */
    decltype(&gxop_sort_create)    sort_create = nullptr;
    decltype(&gxop_sort_consume)   sort_consume = nullptr;
    decltype(&gxop_sort_build)     sort_build = nullptr;
    decltype(&gxop_sort_next)      sort_next = nullptr;
    decltype(&gxop_sort_get_stats) sort_stats = nullptr;
    decltype(&gxop_sort_close)     sort_close = nullptr;
    bool has_sort() const {
        return sort_create && sort_consume && sort_build && sort_next &&
               sort_stats && sort_close;
    }

    bool open(const char *path) {
        h = dlopen(path, RTLD_NOW | RTLD_LOCAL);
        if (!h) {
            std::fprintf(stderr, "dlopen %s: %s\n", path, dlerror());
            return false;
        }
#define BIND(field, sym)                                                    \
        field = (decltype(field))dlsym(h, #sym);                            \
        if (!field) {                                                       \
            std::fprintf(stderr, "missing ABI symbol: %s\n", #sym);         \
            return false;                                                   \
        }
        BIND(join_create, gxop_join_create)
        BIND(join_consume, gxop_join_consume)
        BIND(join_build, gxop_join_build)
        BIND(join_probe, gxop_join_probe)
        BIND(join_tail, gxop_join_tail)
        BIND(join_probe_push, gxop_join_probe_push)
        BIND(join_probe_flush, gxop_join_probe_flush)
        BIND(join_close, gxop_join_close)
        BIND(agg_create, gxop_agg_create)
        BIND(agg_consume, gxop_agg_consume)
        BIND(agg_build, gxop_agg_build)
        BIND(agg_next, gxop_agg_next)
        BIND(agg_close, gxop_agg_close)
        BIND(part_create, gxop_part_create)
        BIND(part_consume, gxop_part_consume)
        BIND(part_consume_concat, gxop_part_consume_concat)
        BIND(part_close, gxop_part_close)
        BIND(gj_create, gxop_groupjoin_create)
        BIND(gj_consume, gxop_groupjoin_consume)
        BIND(gj_build, gxop_groupjoin_build)
        BIND(gj_probe, gxop_groupjoin_probe)
        BIND(gj_next, gxop_groupjoin_next)
        BIND(gj_close, gxop_groupjoin_close)
        BIND(win_create, gxop_window_create)
        BIND(fwin_create, gxop_fwindow_create)
        BIND(fwin_consume, gxop_fwindow_consume)
        BIND(fwin_finish, gxop_fwindow_finish)
        BIND(fwin_next, gxop_fwindow_next)
        BIND(fwin_close, gxop_fwindow_close)
        BIND(win_consume, gxop_window_consume)
        BIND(win_close, gxop_window_close)
        BIND(ser, gxop_chunk_serialize)
        BIND(deser, gxop_chunk_deserialize)
        BIND(chunk_free, gxop_chunk_free)
        BIND(buf_free, gxop_buf_free)
        BIND(scan_create, gxop_scan_create)
        BIND(scan_consume, gxop_scan_consume)
        BIND(scan_close, gxop_scan_close)
        BIND(result_to_host, gxop_result_to_host)
        BIND(result_release, gxop_result_release)
        BIND(last_error, gx_last_error)
        BIND(join_stats, gxop_join_get_stats)
        BIND(abi_version, gxop_abi_version)
#undef BIND
#define BIND_OPT(field, sym) field = (decltype(field))dlsym(h, #sym);
        BIND_OPT(sort_create, gxop_sort_create)
        BIND_OPT(sort_consume, gxop_sort_consume)
        BIND_OPT(sort_build, gxop_sort_build)
        BIND_OPT(sort_next, gxop_sort_next)
        BIND_OPT(sort_stats, gxop_sort_get_stats)
        BIND_OPT(sort_close, gxop_sort_close)
#undef BIND_OPT
        return true;
    }
};

static GxApi api;
static int g_fail = 0;

#define CHECK(cond, ...)                                                    \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__);       \
            std::fprintf(stderr, __VA_ARGS__);                              \
            std::fprintf(stderr, " [lib: %s]\n", api.last_error());         \
            g_fail++;                                                       \
        }                                                                   \
    } while (0)

/* xorshift so every run is deterministic */
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    uint64_t x = rng_state;
    x ^= x << 13; x ^= x >> 7; x ^= x << 17;
    return rng_state = x;
}

static gx_block mk_i64(const int64_t *v, const uint8_t *nulls = nullptr) {
    gx_block b{};
    b.type = GX_I64; b.mem = GX_MEM_HOST; b.values = v; b.nulls = nulls;
    return b;
}

/* read one host-resident i64 result cell (after result_to_host) */
static int64_t cell_i64(const gx_result *r, int col, int row) {
    return ((const int64_t *)r->chunk.blocks[col].values)[row];
}
static bool cell_null(const gx_result *r, int col, int row) {
    const uint8_t *n = r->chunk.blocks[col].nulls;
    return n && n[row];
}

/* ---- selftests --------------------------------------------------------- */

/* INNER join: build keys 0..B-1 (value = key*10), probe keys 0..P-1 mod 2B.
 * Expected matches = probe rows whose key < B; each match's payload must
 * equal key*10. */
static void t_join_inner(int device) {
    const int B = 5000, P = 20000;
    std::vector<int64_t> bk(B), bv(B), pk(P), pv(P);
    for (int i = 0; i < B; i++) { bk[i] = i; bv[i] = (int64_t)i * 10; }
    int64_t expect = 0;
    for (int i = 0; i < P; i++) {
        pk[i] = (int64_t)(rnd() % (2 * B));
        pv[i] = i;
        if (pk[i] < B) expect++;
    }
    gx_equi_key key{0, 0, GX_I64, 0};
    int32_t t2[2] = {GX_I64, GX_I64};
    gx_join_cfg cfg{};
    cfg.join_type = GX_JOIN_INNER;
    cfg.n_keys = 1; cfg.keys = &key;
    cfg.n_outer_cols = 2; cfg.outer_types = t2;
    cfg.n_inner_cols = 2; cfg.inner_types = t2;
    cfg.anti_null_col = -1;
    cfg.device = device;
    gx_op *op = api.join_create(&cfg);
    CHECK(op, "join_create");
    if (!op) return;

    gx_block bb[2] = {mk_i64(bk.data()), mk_i64(bv.data())};
    gx_chunk bc{B, 2, bb};
    CHECK(api.join_consume(op, &bc) == 0, "join_consume");
    CHECK(api.join_build(op) == 0, "join_build");

    gx_block pb[2] = {mk_i64(pk.data()), mk_i64(pv.data())};
    gx_chunk pc{P, 2, pb};
    gx_result *res = nullptr;
    CHECK(api.join_probe(op, &pc, &res) == 0, "join_probe");
    int64_t got = 0;
    if (res) {
        CHECK(api.result_to_host(res) == 0, "to_host");
        got = res->chunk.n_rows;
        /* schema: outer cols then inner cols (minus inner key dedup is NOT
         * applied at this boundary): check payload join correctness */
        for (int r = 0; r < res->chunk.n_rows; r++) {
            int64_t k = cell_i64(res, 0, r);
            int64_t inner_v = cell_i64(res, 3, r);
            if (inner_v != k * 10) {
                CHECK(false, "inner payload mismatch row %d", r);
                break;
            }
        }
        api.result_release(res);
    }
    CHECK(got == expect, "inner matches %lld != %lld", (long long)got,
          (long long)expect);
    gx_result *tail = nullptr;
    CHECK(api.join_tail(op, &tail) == 0 && tail == nullptr, "inner tail");
    api.join_close(op);
    std::printf("  join INNER: %lld matches ok\n", (long long)got);
}

/* Concurrent-consumer contract: the reference's N
 * driver threads share one Synchronizer — consumeChunk races through
 * synchronized(shared), buildConsume is first-come, probes run from all
 * instances against the shared table (ParallelHashJoinExec.java:157-166,
 * :107-128). Here: 4 threads consume disjoint build chunks into ONE gx_op
 * with NO external lock (the library serializes internally), all 4 call
 * join_build (one builds, three no-op), then all 4 probe disjoint slices
 * concurrently and the match counts must add up. */
static void t_concurrent(int device) {
    const int T = 4, B = 40000, PSLICE = 50000;
    std::vector<int64_t> bk(B), bv(B);
    for (int i = 0; i < B; i++) { bk[i] = i; bv[i] = (int64_t)i * 10; }
    std::vector<std::vector<int64_t>> pk(T), pv(T);
    std::vector<int64_t> expect(T, 0);
    for (int t = 0; t < T; t++) {
        pk[t].resize(PSLICE);
        pv[t].resize(PSLICE);
        for (int i = 0; i < PSLICE; i++) {
            pk[t][i] = (int64_t)(rnd() % (2 * B));
            pv[t][i] = i;
            if (pk[t][i] < B) expect[t]++;
        }
    }
    gx_equi_key key{0, 0, GX_I64, 0};
    int32_t t2[2] = {GX_I64, GX_I64};
    gx_join_cfg cfg{};
    cfg.join_type = GX_JOIN_INNER;
    cfg.n_keys = 1; cfg.keys = &key;
    cfg.n_outer_cols = 2; cfg.outer_types = t2;
    cfg.n_inner_cols = 2; cfg.inner_types = t2;
    cfg.anti_null_col = -1;
    cfg.device = device;
    gx_op *op = api.join_create(&cfg);
    CHECK(op, "conc join_create");
    if (!op) return;

    const int SLICE = B / T;
    std::vector<std::thread> th;
    std::vector<int> crc(T, -1);
    for (int t = 0; t < T; t++)
        th.emplace_back([&, t] {
            gx_block bb[2] = {mk_i64(bk.data() + t * SLICE),
                              mk_i64(bv.data() + t * SLICE)};
            gx_chunk bc{SLICE, 2, bb};
            crc[t] = api.join_consume(op, &bc);
        });
    for (auto &x : th) x.join();
    th.clear();
    for (int t = 0; t < T; t++) CHECK(crc[t] == 0, "conc consume %d", t);

    std::vector<int> brc(T, -1);
    for (int t = 0; t < T; t++)
        th.emplace_back([&, t] { brc[t] = api.join_build(op); });
    for (auto &x : th) x.join();
    th.clear();
    for (int t = 0; t < T; t++) CHECK(brc[t] == 0, "conc build %d", t);

    std::vector<int64_t> got(T, -1);
    std::vector<int> prc(T, -1);
    for (int t = 0; t < T; t++)
        th.emplace_back([&, t] {
            gx_block pb[2] = {mk_i64(pk[t].data()), mk_i64(pv[t].data())};
            gx_chunk pc{PSLICE, 2, pb};
            gx_result *res = nullptr;
            prc[t] = api.join_probe(op, &pc, &res);
            if (prc[t] == 0 && res) {
                got[t] = res->chunk.n_rows;
                api.result_release(res);
            }
        });
    for (auto &x : th) x.join();
    for (int t = 0; t < T; t++) {
        CHECK(prc[t] == 0, "conc probe rc %d", t);
        CHECK(got[t] == expect[t], "conc probe %d: %lld != %lld", t,
              (long long)got[t], (long long)expect[t]);
    }
    api.join_close(op);
    std::printf("  join concurrent (4 threads, shared op): ok\n");
}

/* INNER join with a residual condition (gx_join_cond): build keys 0..B-1
 * with payload key*10; probe keys 0..2B-1; condition = inner payload < T.
 * Expected matches = probe keys k < B with k*10 < T, i.e. k < T/10. */
static void t_join_condition(int device) {
    const int B = 4000, P = 16000;
    const int64_t T = 17770; /* threshold: keys < 1777 pass */
    std::vector<int64_t> bk(B), bv(B), pk(P), pv(P);
    for (int i = 0; i < B; i++) { bk[i] = i; bv[i] = (int64_t)i * 10; }
    int64_t expect = 0;
    for (int i = 0; i < P; i++) {
        pk[i] = (int64_t)(rnd() % (2 * B));
        pv[i] = i;
        if (pk[i] < B && pk[i] * 10 < T) expect++;
    }
    gx_equi_key key{0, 0, GX_I64, 0};
    int32_t t2[2] = {GX_I64, GX_I64};
    gx_join_cond cond{};
    cond.col_a = 3;          /* condition row: outer(2) then inner(2) */
    cond.cmp = GX_CMP_LT;
    cond.col_b = -1;
    cond.v_i64 = T;
    gx_join_cfg cfg{};
    cfg.join_type = GX_JOIN_INNER;
    cfg.n_keys = 1; cfg.keys = &key;
    cfg.n_outer_cols = 2; cfg.outer_types = t2;
    cfg.n_inner_cols = 2; cfg.inner_types = t2;
    cfg.anti_null_col = -1;
    cfg.device = device;
    cfg.n_conds = 1; cfg.conds = &cond;
    gx_op *op = api.join_create(&cfg);
    CHECK(op, "cond join_create");
    if (!op) return;
    gx_block bb[2] = {mk_i64(bk.data()), mk_i64(bv.data())};
    gx_chunk bc{B, 2, bb};
    CHECK(api.join_consume(op, &bc) == 0, "cond consume");
    CHECK(api.join_build(op) == 0, "cond build");
    gx_block pb[2] = {mk_i64(pk.data()), mk_i64(pv.data())};
    gx_chunk pc{P, 2, pb};
    gx_result *res = nullptr;
    CHECK(api.join_probe(op, &pc, &res) == 0, "cond probe");
    int64_t got = 0;
    if (res) {
        CHECK(api.result_to_host(res) == 0, "cond to_host");
        got = res->chunk.n_rows;
        for (int r = 0; r < res->chunk.n_rows; r++)
            if (cell_i64(res, 3, r) >= T) {
                CHECK(false, "condition leaked row %d", r);
                break;
            }
        api.result_release(res);
    }
    CHECK(got == expect, "cond matches %lld != %lld", (long long)got,
          (long long)expect);
    api.join_close(op);
    std::printf("  join residual condition: %lld matches ok\n",
                (long long)got);
}

/* LEFT join: probe keys half-missing -> unmatched probe rows carry NULL
 * inner columns. */
static void t_join_left(int device) {
    const int B = 1000, P = 4000;
    std::vector<int64_t> bk(B), bv(B), pk(P);
    for (int i = 0; i < B; i++) { bk[i] = i * 2; bv[i] = i; } /* even keys */
    int64_t matched = 0;
    for (int i = 0; i < P; i++) {
        pk[i] = i % (2 * B);
        if (pk[i] % 2 == 0 && pk[i] / 2 < B) matched++;
    }
    gx_equi_key key{0, 0, GX_I64, 0};
    int32_t t1[1] = {GX_I64};
    int32_t t2[2] = {GX_I64, GX_I64};
    gx_join_cfg cfg{};
    cfg.join_type = GX_JOIN_LEFT;
    cfg.n_keys = 1; cfg.keys = &key;
    cfg.n_outer_cols = 1; cfg.outer_types = t1;
    cfg.n_inner_cols = 2; cfg.inner_types = t2;
    cfg.anti_null_col = -1;
    cfg.device = device;
    gx_op *op = api.join_create(&cfg);
    CHECK(op, "left join_create");
    if (!op) return;
    gx_block bb[2] = {mk_i64(bk.data()), mk_i64(bv.data())};
    gx_chunk bc{B, 2, bb};
    api.join_consume(op, &bc);
    api.join_build(op);
    gx_block pb[1] = {mk_i64(pk.data())};
    gx_chunk pc{P, 1, pb};
    gx_result *res = nullptr;
    CHECK(api.join_probe(op, &pc, &res) == 0, "left probe");
    int64_t rows = 0, nulls = 0;
    if (res) {
        api.result_to_host(res);
        rows = res->chunk.n_rows;
        for (int r = 0; r < rows; r++)
            if (cell_null(res, 1, r)) nulls++;
        api.result_release(res);
    }
    CHECK(rows == P, "LEFT rows %lld != %d", (long long)rows, P);
    CHECK(nulls == P - matched, "LEFT null rows %lld != %lld",
          (long long)nulls, (long long)(P - matched));
    api.join_close(op);
    std::printf("  join LEFT: %lld rows, %lld null-padded ok\n",
                (long long)rows, (long long)nulls);
}

/* hash agg: keys 0..G-1 cycling; COUNT(*) and SUM must be closed-form. */
static void t_agg(int device) {
    const int N = 100000, G = 257;
    std::vector<int64_t> gk(N), v(N);
    for (int i = 0; i < N; i++) { gk[i] = i % G; v[i] = i; }
    int32_t gcols[1] = {0};
    gx_agg_spec specs[2] = {{GX_AGG_COUNT_ROW, -1}, {GX_AGG_SUM_I64, 1}};
    int32_t itypes[2] = {GX_I64, GX_I64};
    gx_agg_cfg cfg{};
    cfg.n_group_cols = 1; cfg.group_cols = gcols;
    cfg.n_aggs = 2; cfg.aggs = specs;
    cfg.n_input_cols = 2; cfg.input_types = itypes;
    cfg.device = device;
    gx_op *op = api.agg_create(&cfg);
    CHECK(op, "agg_create");
    if (!op) return;
    gx_block bb[2] = {mk_i64(gk.data()), mk_i64(v.data())};
    gx_chunk c{N, 2, bb};
    CHECK(api.agg_consume(op, &c) == 0, "agg_consume");
    CHECK(api.agg_build(op) == 0, "agg_build");
    int64_t groups = 0, total_cnt = 0, total_sum = 0;
    for (;;) {
        gx_result *res = nullptr;
        CHECK(api.agg_next(op, &res) == 0, "agg_next");
        if (!res) break;
        api.result_to_host(res);
        for (int r = 0; r < res->chunk.n_rows; r++) {
            int64_t key = cell_i64(res, 0, r);
            int64_t cnt = cell_i64(res, 1, r);
            int64_t sum = cell_i64(res, 2, r);
            int64_t expect_cnt = N / G + (key < N % G ? 1 : 0);
            if (cnt != expect_cnt) {
                CHECK(false, "group %lld count %lld != %lld", (long long)key,
                      (long long)cnt, (long long)expect_cnt);
                break;
            }
            groups++; total_cnt += cnt; total_sum += sum;
        }
        api.result_release(res);
    }
    CHECK(groups == G, "groups %lld != %d", (long long)groups, G);
    CHECK(total_cnt == N, "count total");
    CHECK(total_sum == (int64_t)N * (N - 1) / 2, "sum total");
    api.agg_close(op);
    std::printf("  agg: %lld groups, totals ok\n", (long long)groups);
}

/* SQL global aggregate over EMPTY input emits exactly one row:
 * COUNT(*)=0, null-init SUM NULL (HashAggExec no-group-by contract;
 * regression for the consume()-seeding bug deep-fuzz seed 100229 found). */
static void t_agg_empty_global(int device) {
    gx_agg_spec specs[2] = {{GX_AGG_COUNT_ROW, -1}, {GX_AGG_SUM_I64N, 0}};
    int32_t itypes[1] = {GX_I64};
    gx_agg_cfg cfg{};
    cfg.n_group_cols = 0; cfg.group_cols = nullptr;
    cfg.n_aggs = 2; cfg.aggs = specs;
    cfg.n_input_cols = 1; cfg.input_types = itypes;
    cfg.device = device;
    gx_op *op = api.agg_create(&cfg);
    CHECK(op, "agg_create(empty-global)");
    if (!op) return;
    CHECK(api.agg_build(op) == 0, "agg_build(empty)");
    gx_result *res = nullptr;
    CHECK(api.agg_next(op, &res) == 0, "agg_next(empty)");
    CHECK(res && res->chunk.n_rows == 1, "empty global agg must emit 1 row");
    if (res) {
        api.result_to_host(res);
        CHECK(cell_i64(res, 0, 0) == 0, "COUNT(*) over empty != 0");
        CHECK(res->chunk.blocks[1].nulls &&
                  ((const uint8_t *)res->chunk.blocks[1].nulls)[0] == 1,
              "null-init SUM over empty must be NULL");
        api.result_release(res);
    }
    api.agg_close(op);
    std::printf("  agg empty-global: one row, COUNT=0, SUM NULL\n");
}

/* exact DECIMAL SUM (GX_AGG_SUM_DEC, 128-bit state): 4096 x INT64_MAX into
 * one group gives 4096 x (2^63-1) = 2^75 - 4096 = 37778 931862957 161705472,
 * i.e. three base-1e9 integer words, a zero fraction word, integers = 27,
 * scale 0, not negative; its companion group holds only NULLs and emits
 * NULL. Skipped on the CPU oracle, which does not have the func. */
static void t_decsum(int device) {
    if (api.abi_version() == 0) {
        std::printf("  decsum: not in this library, skipped\n");
        return;
    }
    const int N = 4096, NN = 16;
    std::vector<int64_t> gk(N + NN), v(N + NN);
    std::vector<uint8_t> nulls(N + NN, 0);
    for (int i = 0; i < N + NN; i++) {
        gk[i] = i < N ? 7 : 8;
        v[i] = INT64_MAX;
        nulls[i] = i < N ? 0 : 1;
    }
    int32_t gcols[1] = {0};
    gx_agg_spec specs[1] = {{GX_AGG_WITH_SCALE(GX_AGG_SUM_DEC, 0), 1}};
    int32_t itypes[2] = {GX_I64, GX_I64};
    gx_agg_cfg cfg{};
    cfg.n_group_cols = 1; cfg.group_cols = gcols;
    cfg.n_aggs = 1; cfg.aggs = specs;
    cfg.n_input_cols = 2; cfg.input_types = itypes;
    cfg.device = device;
    gx_op *op = api.agg_create(&cfg);
    CHECK(op, "decsum agg_create");
    if (!op) return;
    gx_block bb[2] = {mk_i64(gk.data()), mk_i64(v.data(), nulls.data())};
    gx_chunk c{N + NN, 2, bb};
    CHECK(api.agg_consume(op, &c) == 0, "decsum consume");
    CHECK(api.agg_build(op) == 0, "decsum build");
    uint8_t expect[40] = {0};
    const int32_t words[3] = {37778, 931862957, 161705472};
    std::memcpy(expect, words, sizeof(words));
    expect[36] = 27;
    int seen_sum = 0, seen_null = 0;
    for (;;) {
        gx_result *res = nullptr;
        CHECK(api.agg_next(op, &res) == 0, "decsum next");
        if (!res) break;
        api.result_to_host(res);
        CHECK(res->chunk.blocks[1].type == GX_DECIMAL, "decsum out type");
        for (int r = 0; r < res->chunk.n_rows; r++) {
            const uint8_t *rec =
                (const uint8_t *)res->chunk.blocks[1].values + (size_t)r * 40;
            if (cell_i64(res, 0, r) == 7) {
                CHECK(!cell_null(res, 1, r) &&
                          std::memcmp(rec, expect, 40) == 0,
                      "decsum: 4096 x INT64_MAX record mismatch");
                seen_sum++;
            } else {
                CHECK(cell_null(res, 1, r), "decsum: NULL group not NULL");
                seen_null++;
            }
        }
        api.result_release(res);
    }
    CHECK(seen_sum == 1 && seen_null == 1, "decsum groups %d/%d", seen_sum,
          seen_null);
    api.agg_close(op);
    std::printf("  decsum: 4096 x INT64_MAX exact, NULL group NULL\n");
}

/* partition: row conservation + consume/consume_concat agreement. */
static void t_part(int device) {
    const int N = 50000, PARTS = 8;
    std::vector<int64_t> k(N), v(N);
    for (int i = 0; i < N; i++) { k[i] = (int64_t)rnd(); v[i] = i; }
    int32_t kcols[1] = {0};
    int32_t itypes[2] = {GX_I64, GX_I64};
    gx_part_cfg cfg{};
    cfg.n_parts = PARTS;
    cfg.n_key_cols = 1; cfg.key_cols = kcols;
    cfg.n_input_cols = 2; cfg.input_types = itypes;
    cfg.device = device;
    gx_op *op = api.part_create(&cfg);
    CHECK(op, "part_create");
    if (!op) return;
    gx_block bb[2] = {mk_i64(k.data()), mk_i64(v.data())};
    gx_chunk c{N, 2, bb};
    gx_result *outs[PARTS] = {};
    CHECK(api.part_consume(op, &c, outs) == 0, "part_consume");
    int64_t total = 0;
    int64_t per_part[PARTS] = {};
    for (int p = 0; p < PARTS; p++) {
        if (!outs[p]) continue;
        api.result_to_host(outs[p]);
        per_part[p] = outs[p]->chunk.n_rows;
        total += per_part[p];
        api.result_release(outs[p]);
    }
    CHECK(total == N, "partition conservation %lld != %d", (long long)total, N);
    gx_result *cat = nullptr;
    int64_t counts[PARTS] = {};
    CHECK(api.part_consume_concat(op, &c, &cat, counts) == 0, "part concat");
    int64_t total2 = 0;
    for (int p = 0; p < PARTS; p++) {
        total2 += counts[p];
        if (counts[p] != per_part[p]) {
            CHECK(false, "concat count[%d] %lld != %lld", p,
                  (long long)counts[p], (long long)per_part[p]);
            break;
        }
    }
    CHECK(total2 == N, "concat conservation");
    if (cat) {
        api.result_to_host(cat);
        CHECK(cat->chunk.n_rows == N, "concat rows");
        api.result_release(cat);
    }
    api.part_close(op);
    std::printf("  partition: %d parts conserve %lld rows ok\n", PARTS,
                (long long)total);
}

/* scan: predicate survivor count + decimal round trip. */
static void t_scan(int device) {
    const int N = 30000;
    std::vector<int64_t> a(N), cents(N);
    int64_t expect = 0;
    for (int i = 0; i < N; i++) {
        a[i] = (int64_t)(rnd() % 1000);
        cents[i] = (int64_t)(rnd() % 2000000) - 1000000;
        if (a[i] < 400) expect++;
    }
    gx_pred pred{};
    pred.col = 0; pred.cmp = GX_CMP_LT; pred.v_i64 = 400;
    gx_proj projs[2] = {};
    projs[0].op = GX_PROJ_COPY; projs[0].a = 1; projs[0].b = -1;
    projs[1].op = GX_PROJ_SCALED_TO_DEC; projs[1].a = 1; projs[1].b = -1;
    projs[1].c = 2; /* scale */
    int32_t itypes[2] = {GX_I64, GX_I64};
    gx_scan_cfg cfg{};
    cfg.n_preds = 1; cfg.preds = &pred;
    cfg.n_projs = 2; cfg.projs = projs;
    cfg.n_input_cols = 2; cfg.input_types = itypes;
    cfg.device = device;
    gx_op *op = api.scan_create(&cfg);
    CHECK(op, "scan_create");
    if (!op) return;
    gx_block bb[2] = {mk_i64(a.data()), mk_i64(cents.data())};
    gx_chunk c{N, 2, bb};
    gx_result *res = nullptr;
    CHECK(api.scan_consume(op, &c, &res) == 0, "scan_consume");
    int64_t kept = 0;
    std::vector<uint8_t> dec;
    std::vector<int64_t> scaled;
    if (res) {
        api.result_to_host(res);
        kept = res->chunk.n_rows;
        CHECK(res->chunk.blocks[1].type == GX_DECIMAL, "decimal out type");
        const uint8_t *d = (const uint8_t *)res->chunk.blocks[1].values;
        dec.assign(d, d + kept * 40);
        const int64_t *s = (const int64_t *)res->chunk.blocks[0].values;
        scaled.assign(s, s + kept);
        api.result_release(res);
    }
    CHECK(kept == expect, "scan kept %lld != %lld", (long long)kept,
          (long long)expect);
    api.scan_close(op);

    /* round the decimals back through DEC_TO_SCALED and compare bit-exact */
    gx_proj back{};
    back.op = GX_PROJ_DEC_TO_SCALED; back.a = 0; back.b = -1; back.c = 2;
    int32_t dtypes[1] = {GX_DECIMAL};
    gx_scan_cfg cfg2{};
    cfg2.n_preds = 0; cfg2.preds = nullptr;
    cfg2.n_projs = 1; cfg2.projs = &back;
    cfg2.n_input_cols = 1; cfg2.input_types = dtypes;
    cfg2.device = device;
    gx_op *op2 = api.scan_create(&cfg2);
    CHECK(op2, "scan_create dec");
    if (!op2) return;
    gx_block db{};
    db.type = GX_DECIMAL; db.mem = GX_MEM_HOST; db.values = dec.data();
    gx_chunk dc{(int32_t)kept, 1, &db};
    gx_result *res2 = nullptr;
    CHECK(api.scan_consume(op2, &dc, &res2) == 0, "scan dec consume");
    if (res2) {
        api.result_to_host(res2);
        CHECK(res2->chunk.n_rows == kept, "dec rows");
        /* scan output order is nondeterministic (atomic emit staging) --
         * the roundtrip check is on the sorted multisets */
        std::vector<int64_t> back(kept);
        for (int r = 0; r < res2->chunk.n_rows; r++)
            back[r] = cell_i64(res2, 0, r);
        std::vector<int64_t> want = scaled;
        std::sort(back.begin(), back.end());
        std::sort(want.begin(), want.end());
        CHECK(back == want, "decimal roundtrip multiset mismatch");
        api.result_release(res2);
    }
    api.scan_close(op2);
    std::printf("  scan+decimal: %lld survivors, DEC roundtrip exact ok\n",
                (long long)kept);
}

/* groupjoin: G build groups cycled by probe keys -> closed-form counts */
static void t_groupjoin(int device) {
    const int B = 2000, P = 30000;
    std::vector<int64_t> bk(B), bp(B), pk(P), pv(P);
    for (int i = 0; i < B; i++) { bk[i] = i; bp[i] = i * 100; }
    for (int i = 0; i < P; i++) {
        pk[i] = i % (2 * B);  /* half the probe keys miss */
        pv[i] = i % 7;
    }
    gx_equi_key key{0, 0, GX_I64, 0};  /* outer=consumed col0, inner=probe col0 */
    int32_t bt[2] = {GX_I64, GX_I64};
    int32_t pt[2] = {GX_I64, GX_I64};
    int32_t gcols[2] = {0, 1};
    gx_agg_spec sp[2] = {{GX_AGG_COUNT_ROW, -1}, {GX_AGG_SUM_I64, 1}};
    gx_groupjoin_cfg cfg{};
    cfg.join_type = GX_JOIN_INNER;
    cfg.n_keys = 1; cfg.keys = &key;
    cfg.n_build_cols = 2; cfg.build_types = bt;
    cfg.n_probe_cols = 2; cfg.probe_types = pt;
    cfg.n_group_cols = 2; cfg.group_cols = gcols;
    cfg.n_aggs = 2; cfg.aggs = sp;
    cfg.device = device;
    gx_op *op = api.gj_create(&cfg);
    CHECK(op, "groupjoin_create");
    if (!op) return;
    gx_block bb[2] = {mk_i64(bk.data()), mk_i64(bp.data())};
    gx_chunk bc{B, 2, bb};
    CHECK(api.gj_consume(op, &bc) == 0, "gj consume");
    CHECK(api.gj_build(op) == 0, "gj build");
    gx_block pb[2] = {mk_i64(pk.data()), mk_i64(pv.data())};
    gx_chunk pc{P, 2, pb};
    CHECK(api.gj_probe(op, &pc) == 0, "gj probe");
    int64_t groups = 0, cnt_total = 0;
    for (;;) {
        gx_result *res = nullptr;
        CHECK(api.gj_next(op, &res) == 0, "gj next");
        if (!res) break;
        api.result_to_host(res);
        for (int r = 0; r < res->chunk.n_rows; r++) {
            int64_t k = cell_i64(res, 0, r);
            if (cell_i64(res, 1, r) != k * 100) {
                CHECK(false, "gj group payload row %d", r);
                break;
            }
            /* every build key 0..B-1 is hit by P/(2B) probe rows + spill */
            int64_t exp = P / (2 * B) + ((int64_t)k < (P % (2 * B)) ? 1 : 0);
            if (cell_i64(res, 2, r) != exp) {
                CHECK(false, "gj count group %lld: %lld != %lld",
                      (long long)k, (long long)cell_i64(res, 2, r),
                      (long long)exp);
                break;
            }
            groups++;
            cnt_total += cell_i64(res, 2, r);
        }
        api.result_release(res);
    }
    CHECK(groups == B, "gj groups %lld != %d", (long long)groups, B);
    int64_t exp_total = (int64_t)B * (P / (2 * B)) +
                    std::min<int64_t>(B, P % (2 * B));
    CHECK(cnt_total == exp_total, "gj total matches");
    api.gj_close(op);
    std::printf("  groupjoin: %lld groups, counts closed-form ok\n",
                (long long)groups);
}

/* window: running COUNT/SUM over sorted partitions, checked closed-form */
static void t_window(int device) {
    const int N = 40000, PARTLEN = 37;
    std::vector<int64_t> part(N), val(N);
    for (int i = 0; i < N; i++) { part[i] = i / PARTLEN; val[i] = i % 5; }
    int32_t pcols[1] = {0};
    gx_agg_spec sp[2] = {{GX_AGG_COUNT_ROW, -1}, {GX_AGG_SUM_I64, 1}};
    uint8_t rs[2] = {0, 0};
    int32_t itypes[2] = {GX_I64, GX_I64};
    gx_window_cfg cfg{};
    cfg.n_part_cols = 1; cfg.part_cols = pcols;
    cfg.n_aggs = 2; cfg.aggs = sp; cfg.reset = rs;
    cfg.n_input_cols = 2; cfg.input_types = itypes;
    cfg.device = device;
    gx_op *op = api.win_create(&cfg);
    CHECK(op, "window_create");
    if (!op) return;
    /* feed in two chunks so a partition straddles the boundary */
    int64_t checked = 0;
    const int SPLIT = N / 2 + 11;
    for (int c = 0; c < 2; c++) {
        int from = c == 0 ? 0 : SPLIT;
        int to = c == 0 ? SPLIT : N;
        gx_block bb[2] = {mk_i64(part.data() + from),
                          mk_i64(val.data() + from)};
        gx_chunk ch{to - from, 2, bb};
        gx_result *res = nullptr;
        CHECK(api.win_consume(op, &ch, &res) == 0, "win consume");
        if (!res) continue;
        api.result_to_host(res);
        int64_t run_cnt = 0, run_sum = 0;
        for (int r = 0; r < res->chunk.n_rows; r++) {
            int64_t gi = from + r;
            if (gi % PARTLEN == 0) { run_cnt = 0; run_sum = 0; }
            /* recompute running from partition start (cross-chunk!) */
            if (gi % PARTLEN == 0 || r == 0) {
                run_cnt = 0; run_sum = 0;
                for (int64_t j = gi - gi % PARTLEN; j <= gi; j++) {
                    run_cnt++; run_sum += val[(size_t)j];
                }
            } else {
                run_cnt++; run_sum += val[(size_t)gi];
            }
            if (cell_i64(res, 2, r) != run_cnt ||
                cell_i64(res, 3, r) != run_sum) {
                CHECK(false, "window row %lld: (%lld,%lld) != (%lld,%lld)",
                      (long long)gi, (long long)cell_i64(res, 2, r),
                      (long long)cell_i64(res, 3, r), (long long)run_cnt,
                      (long long)run_sum);
                break;
            }
            checked++;
        }
        api.result_release(res);
    }
    CHECK(checked == N, "window rows %lld != %d", (long long)checked, N);
    api.win_close(op);
    std::printf("  window: %lld running values ok (cross-chunk carry)\n",
                (long long)checked);
}

/* rank family over sorted runs, closed form */
static void t_rank(int device) {
    const int N = 20000, PARTLEN = 40, RUNLEN = 5;
    std::vector<int64_t> part(N), ord(N);
    for (int i = 0; i < N; i++) {
        part[i] = i / PARTLEN;
        ord[i] = (i % PARTLEN) / RUNLEN;
    }
    int32_t pcols[1] = {0};
    int32_t ocols[1] = {1};
    gx_agg_spec sp[2] = {{GX_AGG_RANK, -1}, {GX_AGG_DENSE_RANK, -1}};
    uint8_t rs[2] = {0, 0};
    int32_t itypes[2] = {GX_I64, GX_I64};
    gx_window_cfg cfg{};
    cfg.n_part_cols = 1; cfg.part_cols = pcols;
    cfg.n_order_cols = 1; cfg.order_cols = ocols;
    cfg.n_aggs = 2; cfg.aggs = sp; cfg.reset = rs;
    cfg.n_input_cols = 2; cfg.input_types = itypes;
    cfg.device = device;
    gx_op *op = api.win_create(&cfg);
    CHECK(op, "rank window_create");
    if (!op) return;
    int64_t checked = 0;
    const int SPLIT = N / 2 + 7; /* partition AND run straddle the carry */
    for (int c = 0; c < 2; c++) {
        int from = c == 0 ? 0 : SPLIT;
        int to = c == 0 ? SPLIT : N;
        gx_block bb[2] = {mk_i64(part.data() + from),
                          mk_i64(ord.data() + from)};
        gx_chunk ch{to - from, 2, bb};
        gx_result *res = nullptr;
        CHECK(api.win_consume(op, &ch, &res) == 0, "rank consume");
        if (!res) continue;
        api.result_to_host(res);
        for (int r = 0; r < res->chunk.n_rows; r++, checked++) {
            int64_t gi = from + r;
            int64_t pos = gi % PARTLEN;
            int64_t exp_rank = (pos / RUNLEN) * RUNLEN + 1;
            int64_t exp_dense = pos / RUNLEN + 1;
            if (cell_i64(res, 2, r) != exp_rank ||
                cell_i64(res, 3, r) != exp_dense) {
                CHECK(false, "rank row %lld: (%lld,%lld) != (%lld,%lld)",
                      (long long)gi, (long long)cell_i64(res, 2, r),
                      (long long)cell_i64(res, 3, r), (long long)exp_rank,
                      (long long)exp_dense);
                break;
            }
        }
        api.result_release(res);
    }
    CHECK(checked == N, "rank rows");
    api.win_close(op);
    std::printf("  rank: %lld rank/dense_rank values ok\n",
                (long long)checked);
}

/* frame window: whole-partition totals + sliding counts, closed form */
static void t_fwindow(int device) {
    const int N = 30000, PARTLEN = 29;
    std::vector<int64_t> part(N), val(N);
    for (int i = 0; i < N; i++) { part[i] = i / PARTLEN; val[i] = i % 3; }
    int32_t pcols[1] = {0};
    gx_frame_spec fs[2] = {};
    fs[0] = {GX_AGG_SUM_I64, 1, GX_FRAME_WHOLE_PARTITION, 0, 0};
    fs[1] = {GX_AGG_COUNT_ROW, -1, GX_FRAME_ROWS_SLIDING, 2, 2};
    int32_t itypes[2] = {GX_I64, GX_I64};
    gx_fwindow_cfg cfg{};
    cfg.n_part_cols = 1; cfg.part_cols = pcols;
    cfg.n_frames = 2; cfg.frames = fs;
    cfg.n_input_cols = 2; cfg.input_types = itypes;
    cfg.device = device;
    gx_op *op = api.fwin_create(&cfg);
    CHECK(op, "fwindow_create");
    if (!op) return;
    gx_block bb[2] = {mk_i64(part.data()), mk_i64(val.data())};
    gx_chunk c{N, 2, bb};
    CHECK(api.fwin_consume(op, &c) == 0, "fwin consume");
    CHECK(api.fwin_finish(op) == 0, "fwin finish");
    int64_t checked = 0, at = 0;
    for (;;) {
        gx_result *res = nullptr;
        CHECK(api.fwin_next(op, &res) == 0, "fwin next");
        if (!res) break;
        api.result_to_host(res);
        for (int r = 0; r < res->chunk.n_rows; r++, at++) {
            int64_t s = at - at % PARTLEN;
            int64_t e = std::min<int64_t>(s + PARTLEN, N);
            int64_t tot = 0;
            for (int64_t j = s; j < e; j++) tot += val[(size_t)j];
            int64_t lo = std::max<int64_t>(s, at - 2);
            int64_t hi = std::min<int64_t>(e - 1, at + 2);
            if (cell_i64(res, 2, r) != tot ||
                cell_i64(res, 3, r) != hi - lo + 1) {
                CHECK(false, "fwindow row %lld", (long long)at);
                break;
            }
            checked++;
        }
        api.result_release(res);
    }
    CHECK(checked == N, "fwindow rows %lld != %d", (long long)checked, N);
    api.fwin_close(op);
    std::printf("  fwindow: %lld whole-partition + sliding values ok\n",
                (long long)checked);
}

/* wire format: serialize -> deserialize -> reserialize must be identical
 * bytes, and the LongBlock golden frame must match the reference layout */
/* Top-N, closed form: keys (i * 7919) % n over i = 0..n-1 are a permutation
 * of 0..n-1 (7919 is prime and does not divide n), payload = i, pushed in
 * several chunks. ORDER BY key ASC LIMIT offset, fetch must return keys
 * offset..offset+fetch-1, DESC keys n-1-offset downwards, each with the
 * payload i that solves i * 7919 = key (mod n). Skipped on a library
 * without the sort entry points (the CPU oracle). */
static void t_sort(int device) {
    if (!api.has_sort()) {
        std::printf("  sort/top-N: not exported by this library, skipped\n");
        return;
    }
    const int64_t n = 100000, chunk = 7000, offset = 5, fetch = 40;
    std::vector<int64_t> key(n), pay(n), row_of_key(n);
    for (int64_t i = 0; i < n; i++) {
        key[i] = (i * 7919) % n;
        pay[i] = i;
        row_of_key[key[i]] = i;
    }
    for (int asc = 1; asc >= 0; asc--) {
        int32_t types[2] = {GX_I64, GX_I64};
        gx_order_by ob{0, asc, 0};
        gx_sort_cfg cfg{};
        cfg.n_cols = 2; cfg.types = types;
        cfg.n_order = 1; cfg.order = &ob;
        cfg.offset = offset; cfg.fetch = fetch;
        cfg.device = device;
        gx_op *op = api.sort_create(&cfg);
        CHECK(op, "sort_create");
        if (!op) return;
        for (int64_t lo = 0; lo < n; lo += chunk) {
            const int64_t cnt = std::min(chunk, n - lo);
            gx_block b[2] = {mk_i64(key.data() + lo), mk_i64(pay.data() + lo)};
            gx_chunk c{(int32_t)cnt, 2, b};
            CHECK(api.sort_consume(op, &c) == 0, "sort_consume");
        }
        CHECK(api.sort_build(op) == 0, "sort_build");
        int64_t got = 0;
        for (;;) {
            gx_result *res = nullptr;
            CHECK(api.sort_next(op, &res) == 0, "sort_next");
            if (!res) break;
            CHECK(api.result_to_host(res) == 0, "to_host");
            for (int r = 0; r < res->chunk.n_rows; r++, got++) {
                const int64_t want = asc ? offset + got : n - 1 - offset - got;
                if (cell_i64(res, 0, r) != want ||
                    cell_i64(res, 1, r) != row_of_key[want]) {
                    CHECK(false, "top-N %s row %lld: key %lld payload %lld",
                          asc ? "ASC" : "DESC", (long long)got,
                          (long long)cell_i64(res, 0, r),
                          (long long)cell_i64(res, 1, r));
                    break;
                }
            }
            api.result_release(res);
        }
        CHECK(got == fetch, "top-N rows %lld != %lld", (long long)got,
              (long long)fetch);
        gx_sort_stats st{};
        CHECK(api.sort_stats(op, &st) == 0 && st.rows_consumed == n,
              "sort stats");
        api.sort_close(op);
    }
    std::printf("  sort/top-N: ASC + DESC, offset %lld fetch %lld of %lld ok\n",
                (long long)offset, (long long)fetch, (long long)n);
}

static void t_serde() {
    int64_t vals[3] = {7, 0, -1};
    uint8_t nulls[3] = {0, 1, 0};
    gx_block b = mk_i64(vals, nulls);
    gx_chunk c{3, 1, &b};
    uint8_t *buf = nullptr;
    int64_t len = 0;
    CHECK(api.ser(&c, &buf, &len) == 0, "serialize");
    if (!buf) return;
    /* golden frame: [3]['\0'][25][25] [1][3][0x40][7][-1] */
    const uint8_t expect[] = {
        3,0,0,0, 0, 25,0,0,0, 25,0,0,0,
        1,0,0,0, 3,0,0,0, 0x40,
        7,0,0,0,0,0,0,0,
        0xFF,0xFF,0xFF,0xFF,0xFF,0xFF,0xFF,0xFF};
    CHECK(len == (int64_t)sizeof(expect), "frame length %lld", (long long)len);
    CHECK(std::memcmp(buf, expect, sizeof(expect)) == 0, "golden bytes");
    int32_t types[1] = {GX_I64};
    gx_chunk *back = nullptr;
    int64_t consumed = 0;
    CHECK(api.deser(buf, len, types, 1, &back, &consumed) == 0, "deser");
    CHECK(back && consumed == len, "deser consumed");
    if (back) {
        uint8_t *buf2 = nullptr;
        int64_t len2 = 0;
        CHECK(api.ser(back, &buf2, &len2) == 0, "reserialize");
        CHECK(len2 == len && std::memcmp(buf, buf2, (size_t)len) == 0,
              "roundtrip bytes");
        api.buf_free(buf2);
        api.chunk_free(back);
    }
    api.buf_free(buf);

    /* compressed frame (LZ4 block): a repetitive column must serialize
     * with marker 1 and round-trip through the deserializer */
    std::vector<int64_t> rep(4096);
    for (size_t i = 0; i < rep.size(); i++) rep[i] = (int64_t)(i % 7);
    gx_block rb = mk_i64(rep.data());
    gx_chunk rc{(int32_t)rep.size(), 1, &rb};
    uint8_t *cbuf = nullptr;
    int64_t clen = 0;
    CHECK(api.ser(&rc, &cbuf, &clen) == 0, "serialize compressible");
    if (cbuf) {
        CHECK(cbuf[4] == 1, "marker COMPRESSED (got %d)", cbuf[4]);
        CHECK(clen < (int64_t)(rep.size() * 8 / 2), "compression ratio");
        gx_chunk *cback = nullptr;
        int64_t ccons = 0;
        int32_t ctypes[1] = {GX_I64};
        CHECK(api.deser(cbuf, clen, ctypes, 1, &cback, &ccons) == 0,
              "deser compressed");
        CHECK(cback && ccons == clen, "compressed consumed");
        if (cback) {
            const int64_t *gv = (const int64_t *)cback->blocks[0].values;
            bool ok = cback->n_rows == (int32_t)rep.size();
            for (size_t i = 0; ok && i < rep.size(); i++)
                ok = gv[i] == rep[i];
            CHECK(ok, "compressed values");
            api.chunk_free(cback);
        }
        api.buf_free(cbuf);
    }
    std::printf("  serde: golden frame + LZ4 roundtrip ok\n");
}

/* ---- bench: join probe throughput through the pure C ABI --------------- */

static void bench_join(int device, int64_t build_rows, int64_t probe_rows,
                       int steps) {
    std::vector<int64_t> bk(build_rows), bv(build_rows);
    for (int64_t i = 0; i < build_rows; i++) {
        bk[i] = i; bv[i] = i * 3;
    }
    std::vector<int64_t> pk(probe_rows), pv(probe_rows);
    for (int64_t i = 0; i < probe_rows; i++) {
        pk[i] = (int64_t)(rnd() % (uint64_t)(2 * build_rows));
        pv[i] = i;
    }
    gx_equi_key key{0, 0, GX_I64, 0};
    int32_t t2[2] = {GX_I64, GX_I64};
    gx_join_cfg cfg{};
    cfg.join_type = GX_JOIN_SEMI; /* SEMI keeps output small: measures probe */
    cfg.n_keys = 1; cfg.keys = &key;
    cfg.n_outer_cols = 2; cfg.outer_types = t2;
    cfg.n_inner_cols = 1; cfg.inner_types = t2;
    cfg.anti_null_col = -1;
    cfg.device = device;
    cfg.expected_build_rows = build_rows;
    gx_op *op = api.join_create(&cfg);
    if (!op) { std::fprintf(stderr, "create: %s\n", api.last_error()); return; }
    gx_block bb[1] = {mk_i64(bk.data())};
    gx_chunk bc{(int32_t)build_rows, 1, bb};
    api.join_consume(op, &bc);
    api.join_build(op);
    gx_block pb[2] = {mk_i64(pk.data()), mk_i64(pv.data())};
    gx_chunk pc{(int32_t)probe_rows, 2, pb};

    /* warmup (includes H2D of the probe chunk) */
    gx_result *res = nullptr;
    api.join_probe(op, &pc, &res);
    if (res) api.result_release(res);

    auto t0 = std::chrono::steady_clock::now();
    int64_t matches = 0;
    for (int s = 0; s < steps; s++) {
        res = nullptr;
        if (api.join_probe(op, &pc, &res) != 0) {
            std::fprintf(stderr, "probe: %s\n", api.last_error());
            break;
        }
        if (res) { matches += res->chunk.n_rows; api.result_release(res); }
    }
    auto t1 = std::chrono::steady_clock::now();
    double sec = std::chrono::duration<double>(t1 - t0).count();
    gx_join_stats st{};
    api.join_stats(op, &st);
    api.join_close(op);
    std::printf("{\"driver\": \"gx_driver\", \"op\": \"semi_join_probe\", "
                "\"build_rows\": %lld, \"probe_rows\": %lld, \"steps\": %d, "
                "\"wall_s\": %.4f, \"probe_rows_per_s\": %.3e, "
                "\"probe_kernel_ms\": %.3f, \"matches\": %lld}\n",
                (long long)build_rows, (long long)probe_rows, steps, sec,
                (double)probe_rows * steps / sec,
                st.probe_kernel_ms, (long long)matches);
}

/* agg bench (the C4 shape, no Python): GROUP BY key SUM(val) over rows
 * with rows/groups duplication factor; each step = create+consume+build
 * so the whole fused insert is timed */
static void bench_agg(int device, int64_t rows, int64_t groups, int steps) {
    std::vector<int64_t> k(rows), v(rows);
    for (int64_t i = 0; i < rows; i++) {
        k[i] = (int64_t)(rnd() % (uint64_t)groups);
        v[i] = (int64_t)(rnd() % 100);
    }
    int32_t t2[2] = {GX_I64, GX_I64};
    int32_t gcols[1] = {0};
    gx_agg_spec sp[1] = {{GX_AGG_SUM_I64, 1}};
    double total_s = 0;
    int64_t got_groups = 0;
    for (int s = -1; s < steps; s++) { /* s = -1: warmup */
        gx_agg_cfg cfg{};
        cfg.n_group_cols = 1; cfg.group_cols = gcols;
        cfg.n_aggs = 1; cfg.aggs = sp;
        cfg.n_input_cols = 2; cfg.input_types = t2;
        cfg.expected_groups = groups;
        cfg.device = device;
        auto t0 = std::chrono::steady_clock::now();
        gx_op *op = api.agg_create(&cfg);
        if (!op) { std::fprintf(stderr, "agg: %s\n", api.last_error()); return; }
        gx_block b[2] = {mk_i64(k.data()), mk_i64(v.data())};
        gx_chunk c{(int32_t)rows, 2, b};
        api.agg_consume(op, &c);
        api.agg_build(op);
        got_groups = 0;
        gx_result *res = nullptr;
        while (api.agg_next(op, &res) == 0 && res) {
            got_groups += res->chunk.n_rows;
            api.result_release(res);
            res = nullptr;
        }
        api.agg_close(op);
        auto t1 = std::chrono::steady_clock::now();
        if (s >= 0)
            total_s += std::chrono::duration<double>(t1 - t0).count();
    }
    std::printf("{\"driver\": \"gx_driver\", \"op\": \"hash_agg_sum\", "
                "\"rows\": %lld, \"groups\": %lld, \"steps\": %d, "
                "\"wall_s\": %.4f, \"agg_rows_per_s\": %.3e}\n",
                (long long)rows, (long long)got_groups, steps, total_s,
                (double)rows * steps / total_s);
}

int main(int argc, char **argv) {
    const char *lib = nullptr;
    int device = 0;
    std::string cmd;
    int64_t build_rows = 4000000, probe_rows = 64000000;
    int steps = 5;
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        if (a == "--lib" && i + 1 < argc) lib = argv[++i];
        else if (a == "--device" && i + 1 < argc) device = atoi(argv[++i]);
        else if (a == "--build-rows" && i + 1 < argc) build_rows = atoll(argv[++i]);
        else if (a == "--probe-rows" && i + 1 < argc) probe_rows = atoll(argv[++i]);
        else if (a == "--steps" && i + 1 < argc) steps = atoi(argv[++i]);
        else cmd = a;
    }
    if (!lib || cmd.empty()) {
        std::fprintf(stderr,
            "usage: gx_driver --lib <gxop .so> [--device N] selftest\n"
            "       gx_driver --lib <gxop .so> [--device N] bench "
            "[--build-rows B] [--probe-rows P] [--steps K]\n"
            "       gx_driver --lib <gxop .so> [--device N] bench-agg "
            "[--build-rows GROUPS] [--probe-rows ROWS] [--steps K]\n"
            "(--device -1 selects the CPU oracle build, test use only)\n");
        return 2;
    }
    if (!api.open(lib)) return 2;
    std::printf("gxop ABI version/arch: %d\n", api.abi_version());

    if (cmd == "selftest") {
        t_join_inner(device);
        t_join_condition(device);
        t_concurrent(device);
        t_join_left(device);
        t_agg(device);
        t_agg_empty_global(device);
        t_decsum(device);
        t_part(device);
        t_scan(device);
        t_groupjoin(device);
        t_window(device);
        t_fwindow(device);
        t_rank(device);
        t_sort(device);
        t_serde();
        if (g_fail) {
            std::printf("SELFTEST FAILED: %d check(s)\n", g_fail);
            return 1;
        }
        std::printf("SELFTEST PASSED\n");
        return 0;
    }
    if (cmd == "bench") {
        bench_join(device, build_rows, probe_rows, steps);
        return 0;
    }
    if (cmd == "bench-agg") {
        bench_agg(device, probe_rows, build_rows, steps);
        return 0;
    }
    std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
    return 2;
}

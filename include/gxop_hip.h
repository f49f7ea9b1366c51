/*
 * gxop_hip.h — gxop entry points that ONLY the HIP library (libgxhip.so)
 * exports. Included by gxop.h, which declares the ABI both libraries
 * implement; the CPU oracle has no counterpart for what is declared here,
 * so a caller tests for the symbol before using it (abi.py:
 * GxLib.has_probe_scan).
 */
#ifndef GXOP_HIP_H
#define GXOP_HIP_H

#include "gxop.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- fused scan + probe ------------------------------------------------ */

/* Probe `join` with the rows of raw_chunk that pass `scan`'s predicates,
 * the probe chunk being `scan`'s projected columns. Result-for-result
 * identical (as a row multiset; output order is undefined as for
 * gxop_join_probe) to
 *     gxop_scan_consume(scan, raw_chunk, &t);
 *     gxop_join_probe(join, &t->chunk, out);
 *     gxop_result_release(t);
 * *n_scan_kept receives the number of rows that passed the predicates
 * (what t->chunk.n_rows would have been). scan's projected types must
 * equal join's probe-side types, else error; both ops must live on the
 * same device and stream, else error. Errors, gx_last_error, the
 * single-join error code and the wide-DECIMAL fence behave as in the
 * composed sequence.
 *
 * The counterpart of the reference pushing a join's bloom filter down into
 * the scan (RuntimeFilterBuilderExec): for a plain INNER/SEMI equi-join on
 * one I64 key whose probe key is a GX_PROJ_COPY of a raw I64 column (no
 * residual condition, not build_outer / single_join, no SLICE column, no
 * GX_PROJ_DEC_TO_SCALED projection, device-resident input) ONE kernel
 * evaluates the predicates and probes straight from the raw columns, and
 * the projection expressions are evaluated only for the rows that matched
 * (late materialization). Every other shape runs the composed sequence
 * inside the library, so the entry point is always valid. */
int gxop_join_probe_scan(gx_op *join, gx_op *scan, const gx_chunk *raw_chunk,
                         gx_result **out, int64_t *n_scan_kept);

/* ---- fused scan + group-join probe ------------------------------------- */

/* Feed `groupjoin` the rows of raw_chunk that pass `scan`'s predicates, the
 * probe chunk being `scan`'s projected columns. Same accumulation as
 *     gxop_scan_consume(scan, raw_chunk, &t);
 *     gxop_groupjoin_probe(groupjoin, &t->chunk);
 *     gxop_result_release(t);
 * *n_scan_kept receives the rows that passed the predicates, *n_matched the
 * (probe row, consumed position) matches this call accumulated; either may
 * be NULL. scan's projected types must equal the group-join's probe_types,
 * else error; key inner_index and agg input_col index the scan's
 * projections. Both ops must live on the same device and stream.
 *
 * Fast path: one kernel evaluates the predicates, probes straight from the
 * raw key column and accumulates each match into the record of its consumed
 * position; the aggregate-input projections are evaluated only at matched
 * rows and neither a pair list nor a projected chunk is written. It needs
 *   - one I64 key whose consumed column carried no NULL at build (the build
 *     then makes the plain joins' inline-bucket table + bloom filter; a
 *     NULL probe key matches nothing), and an aggregate list outside the
 *     group-join's wide mode (<= 2 of COUNT_ROW / COUNT_COL / SUM_I64),
 *   - the key projection a GX_PROJ_COPY of a raw I64 column,
 *   - aggregate inputs that are GX_PROJ_COPY of an I64/I32/F64 column,
 *     GX_PROJ_REV_F64, GX_PROJ_REV_SCALED4 or GX_PROJ_Q9_AMOUNT4, and no
 *     GX_PROJ_DEC_TO_SCALED projection in the scan,
 *   - a device-resident chunk of fewer than 2^31 rows.
 * Every other shape runs the composed sequence inside the library, so the
 * entry point is always valid. */
int gxop_groupjoin_probe_scan(gx_op *groupjoin, gx_op *scan,
                              const gx_chunk *raw_chunk,
                              int64_t *n_scan_kept, int64_t *n_matched);

/* ---- producer join's matches straight into a group-join's build --------- */

/* Probe `join` with the scanned rows of raw_chunk and make the result the
 * consumed side of `groupjoin`, then build it. Exactly
 *     gxop_join_probe_scan(join, scan, raw_chunk, &r, n_scan_kept);
 *     gxop_groupjoin_consume(groupjoin, &r->chunk);
 *     gxop_result_release(r);
 *     gxop_groupjoin_build(groupjoin);
 * Afterwards the group-join is built and holds the join's output rows with
 * the same columns and nulls; their order (the consumed positions) is not
 * specified. *n_consumed receives the join's output row count, *n_scan_kept
 * the rows that passed the predicates; either may be NULL. The join's own
 * stats advance as for gxop_join_probe_scan. Error when the group-join is
 * already built; type mismatches are errors as in the composed calls.
 *
 * Fast path: after the fused probe-scan kernel has left its pair list, ONE
 * kernel evaluates every consumed column at each pair, writes it into the
 * group-join's build store and inserts the key, taken from the register,
 * into the group-join's table and bloom filter: no result is materialized,
 * copied into the store and read back. It needs
 *   - gxop_join_probe_scan's own fast path on (join, scan, raw_chunk),
 *   - a group-join that has consumed nothing and would build the
 *     inline-bucket table (gxop_groupjoin_probe_scan's first condition),
 *   - a key projection without NULLs (the raw columns it reads carry no
 *     nulls buffer),
 *   - at most 8 consumed columns, all I64 / I32 / F64,
 *   - all three ops on one device and stream.
 * GX_GJ_BUILD_FUSED=0 in the environment, read per call, forces the
 * composed sequence. Every other shape runs it inside the library too, so
 * the entry point is always valid. */
int gxop_groupjoin_build_probe_scan(gx_op *groupjoin, gx_op *join,
                                    gx_op *scan, const gx_chunk *raw_chunk,
                                    int64_t *n_scan_kept,
                                    int64_t *n_consumed);

/* 1 when the group-join's build ran gxop_groupjoin_build_probe_scan's fast
 * path, 0 otherwise (tests and plan diagnostics), -1 on a bad op */
int gxop_groupjoin_build_was_fused(gx_op *groupjoin);

/* cumulative probe stats of a group-join: probe_kernel_ms is event time
 * around the probing kernels, probe_launches their count, probe_rows the
 * rows probed (for a probe-scan: the scan survivors), matches the (probe
 * row, consumed position) matches accumulated */
int gxop_groupjoin_get_stats(gx_op *groupjoin, gx_join_stats *out);

/* ---- low-cardinality GROUP BY: block-local pre-aggregation -------------- */

/* A gid-indexed aggregation (wide state, the global aggregate, the plain
 * aggregates of an op with DISTINCT ones, or a narrow state created with a
 * small expected_groups, see gx_agg_cfg) whose group count is at most
 * local_groups_cap accumulates a chunk of 2^18 rows or more (2^16 or more
 * with up to 128 groups) per block in LDS and merges each block's partial
 * records into the group records once, instead of one global atomic per row
 * and aggregate on the same few lines.
 * Results are the same rows (f64 sums within the usual reordering).
 * GX_AGG_LOCAL in the environment at create: 0 = never, 1 = whenever the
 * group count fits, at any chunk size; unset = the gates above.
 *
 * local_rows: rows accumulated through that kernel; local_launches: its
 * launches; local_groups_cap: the most groups it takes for this op's record
 * size; replicas: LDS copies of the state per block at the last launch. */
typedef struct gx_agg_local_stats {
    int64_t local_rows;
    int64_t local_launches;
    int32_t local_groups_cap;
    int32_t replicas;
} gx_agg_local_stats;

int gxop_agg_get_local_stats(gx_op *agg, gx_agg_local_stats *out);

/* ---- sort / top-N (ORDER BY ... [LIMIT offset, fetch]) ------------------ */

/* SortExec / SpilledTopNExec / LimitExec in one operator: consume chunks,
 * build (the buildConsume barrier), then drain the ordered rows
 * [offset, offset + fetch) with gxop_sort_next.
 *
 * Order: the comparator of ExecUtils.getComparator (utils/ExecUtils.java:
 * 451-490) over the order columns in turn -- both values NULL: next column;
 * else type.compare, negated for DESC; first non-zero wins. NULL is the
 * SMALLEST value (NumberType.compare, polardbx-optimizer/.../core/datatype/
 * NumberType.java:110-127): first under ASC, last under DESC. I64/I32
 * compare signed; F64 as Double.compareTo (-0.0 < +0.0, NaN above +Inf, all
 * NaNs equal). Rows equal on every order column keep ARRIVAL order (consume
 * order, then row order in the chunk): the operator is stable, which is one
 * of the orders the reference's heap may produce.
 *
 * null_last mirrors OrderByOption.nullLast and is IGNORED, exactly as the
 * reference comparator never consults it (ExecUtils.java:451-490 reads only
 * index and asc); carried for fidelity like gx_equi_key.null_safe_equal.
 *
 * Order columns: I64, I32, F64. SLICE and DECIMAL order columns are
 * rejected at create (string / decimal order keys are a follow-up); every
 * type is carried as payload. */
typedef struct gx_order_by {
    int32_t col;        /* index into the input schema */
    int32_t asc;        /* 1 = ASC, 0 = DESC */
    int32_t null_last;  /* ignored, see above */
} gx_order_by;

typedef struct gx_sort_cfg {
    int32_t n_cols;
    const int32_t *types;      /* input = output schema */
    int32_t n_order;           /* 1..8 */
    const gx_order_by *order;
    int64_t offset;            /* >= 0 */
    int64_t fetch;             /* -1 = all rows (SortExec); 0 = pass nothing */
    int64_t expected_rows;     /* hint, 0 = unknown */
    int64_t compact_rows;      /* top-N: compact the store to its best
                                  offset+fetch rows when it holds more than
                                  max(this, 2*(offset+fetch)); 0 = default */
    int32_t out_chunk_rows;    /* rows per emitted batch, 0 = one batch */
    int32_t device;
    uint64_t stream;
} gx_sort_cfg;

typedef struct gx_sort_stats {
    int64_t rows_consumed;     /* rows passed to gxop_sort_consume */
    int64_t rows_kept;         /* rows now in the device store */
    int64_t compactions;       /* streaming top-N compactions run */
    int32_t used_select;       /* last ordering: 1 = radix select then sort
                                  of the candidates, 0 = full sort */
    int32_t select_passes;     /* last ordering: histogram passes that ran */
    int64_t candidates;        /* last ordering: rows handed to the sort */
    double kernel_ms;          /* cumulative event time of the device work */
} gx_sort_stats;

/* NULL + gx_last_error on: n_order outside 1..8, an order col outside the
 * schema or of SLICE/DECIMAL type, offset < 0, fetch < -1, device < 0.
 * GX_TOPN_SELECT=0/1 in the environment at create forces the top-N path
 * (full sort / radix select); unset, a size gate decides. */
gx_op *gxop_sort_create(const gx_sort_cfg *cfg);
/* host or device chunk; error once the store would pass 2^32-2 rows */
int gxop_sort_consume(gx_op *op, const gx_chunk *chunk);
int gxop_sort_build(gx_op *op);
/* next ordered batch; *out = NULL when drained. Error before build. */
int gxop_sort_next(gx_op *op, gx_result **out);
int gxop_sort_get_stats(gx_op *op, gx_sort_stats *out);
void gxop_sort_close(gx_op *op);

#ifdef __cplusplus
}
#endif
#endif /* GXOP_HIP_H */

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

/* cumulative probe stats of a group-join: probe_kernel_ms is event time
 * around the probing kernels, probe_launches their count, probe_rows the
 * rows probed (for a probe-scan: the scan survivors), matches the (probe
 * row, consumed position) matches accumulated */
int gxop_groupjoin_get_stats(gx_op *groupjoin, gx_join_stats *out);

#ifdef __cplusplus
}
#endif
#endif /* GXOP_HIP_H */

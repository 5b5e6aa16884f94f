/*
 * dspn_monitor.h -- C ABI of the training monitor's statistics pass: for every tensor of a descriptor table, in one
 * batched launch, the sum of squares, the sum and the largest magnitude of its finite elements and the number of NaN,
 * +Inf and -Inf among them.  It is the device side of dspnet_amd/train/monitor.py, which takes the interface of
 * mx.mon.Monitor (liangfu/dspnet train/train_multitask.py:93-94, :156-159, :249, :317 hands one to Module.fit; its
 * default statistic is norm(x) / sqrt(x.size)).
 *
 * The results are reproducible to the bit.  A tensor is cut into chunks of dspn_tensor_stats_chunk_elems() LOGICAL
 * elements; the cut depends on the tensor alone.  Stage 1, one workgroup per chunk: every lane accumulates its elements
 * in double, the lanes of a wave are summed by a fixed butterfly, the waves of the workgroup in wave order through LDS.
 * Stage 2, one wave per tensor: lane l sums the partials of chunks l, l + 64, ... in that order, then the same butterfly.
 * No floating-point atomics anywhere, every global result is an ordinary store.  So a tensor's record depends on
 * (address modulo 16, element type, rows, C, ld, values) and on nothing else: not on the grid, the CU count, the other
 * rows of the table or the run.
 *
 * Conventions as in dspn_multibox.h / dspn_distance.h: device pointers, caller-owned buffers and workspace, explicit
 * stream, status return + dspn_last_error(); arguments are checked before any HIP call; nothing is allocated and
 * nothing waits, so the call can be recorded in a graph.
 */
#ifndef DSPN_MONITOR_H_
#define DSPN_MONITOR_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSPN_STATS_F32 0
#define DSPN_STATS_BF16 1

/* One tensor: rows * C logical elements of type dtype; row r starts at element r * ld of base, ld >= C >= 1, rows >= 1.
 * Lanes C .. ld - 1 of a row are padding: they never enter the statistics, whatever they hold, and nothing is read
 * behind element (rows - 1) * ld + C - 1.  A flat tensor is rows = 1, C = ld = numel.  base is aligned to the element
 * (4 / 2 bytes); 16-byte loads are used where base and the row pitch allow them, single elements elsewhere.
 * first_chunk: the number of chunks of all rows in front of this one (row 0: 0), a row taking
 * ceil(rows * C / chunk_elems) chunks.  The table lives in device memory; the kernel trusts it
 * (dspnet_amd.functional.tensor_stats_table builds and checks it). */
typedef struct dspn_stats_row {
  const void *base;
  long long rows;
  long long first_chunk;
  int C, ld;
  int dtype;     /* DSPN_STATS_F32 | DSPN_STATS_BF16 */
  int reserved;  /* 0 */
} dspn_stats_row;  /* 40 bytes */

/* sumsq, sum and absmax cover the FINITE elements only (0 when there is none); the three counts cover the others. */
typedef struct dspn_stats_out {
  double sumsq, sum;
  unsigned long long n_nan, n_posinf, n_neginf;
  float absmax;
  int reserved;
} dspn_stats_out;  /* 48 bytes; also the layout of one chunk's partial in the workspace */

/* the fixed chunk length in logical elements */
int dspn_tensor_stats_chunk_elems(void);

/* one partial per chunk; 0 when an argument is not positive.  Pure. */
size_t dspn_tensor_stats_workspace_bytes(int n_rows, long long n_chunks);

/* table: n_rows rows (device), n_chunks: the chunks of all rows together (< 2^31).  out: n_rows records (device).
 * Two launches on `stream`.  A null pointer, n_rows <= 0, n_chunks < n_rows and a workspace below
 * dspn_tensor_stats_workspace_bytes(n_rows, n_chunks) return the argument error before any HIP call. */
int dspn_tensor_stats(const dspn_stats_row *table, int n_rows, long long n_chunks, dspn_stats_out *out, void *workspace,
                      size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif  /* DSPN_MONITOR_H_ */

/*
 * dspn_distance.h -- C ABI of the box-median selection behind the distance branch's evaluation
 * (liangfu/dspnet train/metric.py:201-226, DistanceAccuracyMetric.update) and behind the distance labels of the
 * dataset preparation (data/cityscapes/disparity2distance.py:55-73).
 *
 * Both take, for a box on a disparity map, the element of rank n // 2 (0-based, ascending) of the n pixels of the numpy
 * slice disparity[y0:y1, x0:x1] read as float32.  The device returns that element q and n per box; everything after q
 * (2200 * 75 / (q + 1e-3), the > 1000 -> 200 rule, the > 199 skip, the relative error) is a few Python doubles per box
 * and stays on the host, so every downstream number keeps the host code's bits.
 *
 * Order of the values: ascending float32, -0.0 == +0.0, NaN after every number (np.sort); when the rank falls on a
 * NaN, a quiet NaN is returned.  A uint16 map (the Cityscapes disparity PNGs) selects on the integer itself and
 * returns its float32.
 *
 * Conventions as in dspn_nms.h: device pointers, caller-owned buffers and workspace, explicit stream, status
 * return + dspn_last_error(); arguments are checked before any HIP call; nothing is allocated and nothing waits, so
 * the calls can be recorded in a graph.
 */
#ifndef DSPN_DISTANCE_H_
#define DSPN_DISTANCE_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* image_dev: (B, hh, ww) maps, hh * ww < 2^31.  boxes_dev: (K, 5) int32 rows [image index, x0, x1, y0, y1], the region
 * being image[index, y0:y1, x0:x1] with the slice already resolved: 0 <= x0 <= x1 <= ww, 0 <= y0 <= y1 <= hh.
 * q_dev: K float32, n_dev: K int32.  A row that breaks those bounds, or names an image outside [0, B), is treated as
 * an empty region: n = 0, q = 0 (the kernel never reads outside the maps).
 * count_dev: optional (may be NULL) device int32; rows k >= *count_dev are left untouched -- the count written by
 * dspn_distance_boxes_f32, so that the two calls chain without a host round trip.  K == 0: a no-op that takes NULL
 * pointers; K, B, hh and ww are checked all the same.
 * One workgroup per box, one launch: a radix selection over an order-preserving integer key, 8 bits per pass
 * (4 passes for float32, 2 for uint16), histogram counts as integers in LDS. */
int dspn_box_rank_select_f32(const float *image_dev, int B, int hh, int ww, const int *boxes_dev, int K,
                             const int *count_dev, float *q_dev, int *n_dev, void *stream);
int dspn_box_rank_select_u16(const unsigned short *image_dev, int B, int hh, int ww, const int *boxes_dev, int K,
                             const int *count_dev, float *q_dev, int *n_dev, void *stream);

/* B int32 counters: independent of N, of max_boxes and of the histogram size */
size_t dspn_distance_boxes_workspace_bytes(int B);

/* det_dev: (B, N, 7) float32 detections [id, score, xmin, ymin, xmax, ymax, dist], B * N < 2^31.
 * Row selection, in (image, row) order:
 *   mode 0: the rows of each image before its first id < 0 (the `break` of DistanceAccuracyMetric.update);
 *   mode 1: every row with id >= 0 and score > score_thresh (multi_eval.py:329-335 followed by mode 0).
 * For each selected row, in float32 as the reference: x0 = trunc(xmin * ww), x1 = trunc(xmax * ww), y0 = trunc(ymin * hh),
 * y1 = trunc(ymax * hh) (toward zero; values beyond int32 saturate, NaN gives 0); x0 = max(0, x0), y0 = max(0, y0);
 * x0 == x1 -> x1 = x0 + 1; then the numpy slices [x0:x1] of ww and [y0:y1] of hh resolved (a stop beyond the size is
 * clipped, a negative stop counts from the end, an empty slice is written as lo == hi).
 * boxes_dev: (max_boxes, 5) int32 [image, x0, x1, y0, y1]; src_dev: max_boxes int32, image * N + row of each entry;
 * count_dev: one int32, the number of selected rows -- which may exceed max_boxes: the first max_boxes are written and
 * the caller must treat a larger count as an error. */
int dspn_distance_boxes_f32(const float *det_dev, int B, int N, int hh, int ww, float score_thresh, int mode,
                            int max_boxes, int *boxes_dev, int *src_dev, int *count_dev, void *workspace,
                            size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif  /* DSPN_DISTANCE_H_ */

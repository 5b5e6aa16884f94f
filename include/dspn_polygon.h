/*
 * dspn_polygon.h -- C ABI of the polygon rasteriser behind the Cityscapes label and instance maps
 * (data/cityscapes/Scripts/preparation/json2labelImg.py, json2instanceImg.py: PIL.ImageDraw.polygon(xy, fill=id), one
 * polygon after the other).
 *
 * The fill rule is Pillow's scanline rule, restated and held equal to Pillow in tests/ref_polygon.py.  Everything that
 * depends on a division or on the order of the edge list is done once on the host and arrives in the edge table; the
 * device multiplies, adds (both rounded to float32, never fused), sorts and fills.
 *
 * Tables (all device, int32, rows as below; float fields are the bits of a float32):
 *   edges (E, 8): x0, y0, ymin, ymax, dx, top, bot, x1.
 *       A horizontal edge has ymin == ymax and paints x0..x1 (either order) on that row.  Every other edge crosses row y
 *       at x0 + (y - y0) * dx; `top` replaces that entry on row ymin (when it is not the polygon's last row) and `bot`
 *       on row ymax when that is the polygon's last row -- the corner rule -- unless they are NaN.
 *   polys (P, 4): first edge, one past the last edge, image index, order (>= 1; a larger order paints over a smaller).
 *   jobs  (J, 5): polygon, row y, last_row of the polygon (min(max(ymax, 0), H)), an upper bound n of the row's entries
 *       (active edges, plus one for each edge that ends on the row), offset of the job's 2 * n floats in `scratch`
 *       (only read when n > dspn_polygon_wave_entries()).
 * One wave per job.  A job with n <= dspn_polygon_wave_entries() keeps its entries in LDS; a larger one uses its
 * slice of `scratch` and adds one to *spill_count_dev (optional), so a caller can see which route ran.
 * owner_dev: (B, H, W) int32, zeroed by the caller; every covered pixel receives max(owner, order) with a vector
 * atomic, so the result does not depend on the order in which jobs run.
 *
 * Conventions as in dspn_nms.h: device pointers, caller-owned buffers, explicit stream, status return +
 * dspn_last_error(); nothing is allocated and nothing waits.  The kernels check every index they are handed against
 * E, P, B, H, W and scratch_floats and skip what does not fit: a malformed table paints less, never outside.
 */
#ifndef DSPN_POLYGON_H_
#define DSPN_POLYGON_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* entries of one row that the in-LDS route holds */
int dspn_polygon_wave_entries(void);

int dspn_polygon_rasterize(const int *edges_dev, int E, const int *polys_dev, int P, const int *jobs_dev, int J,
                           float *scratch_dev, long long scratch_floats, int *owner_dev, int B, int H, int W,
                           int *spill_count_dev, void *stream);

/* owner -> values.  table_dev: (T, 4) int32 rows [labelId, labelTrainId, instanceId, instanceTrainId];
 * table_offset_dev: B int32, the row of image b's background (owner 0); owner o of image b reads row offset[b] + o,
 * which must be < T (otherwise the pixel is left untouched).  Outputs (B, H, W): two uint8, two int32; any may be NULL. */
int dspn_polygon_resolve(const int *owner_dev, int B, int H, int W, const int *table_dev, int T,
                         const int *table_offset_dev, unsigned char *label_dev, unsigned char *label_train_dev,
                         int *inst_dev, int *inst_train_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif  /* DSPN_POLYGON_H_ */

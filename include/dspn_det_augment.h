/*
 * dspn_det_augment.h -- C ABI of the per-batch image pipeline of liangfu/dspnet's DetIter (dataset/iterator.py:113-297):
 * what `_data_augmentation` (:249-297) does to the decoded image -- crop or zoom-out padding (:263-278), resize with one of
 * five interpolations (:281-286), mirror (:289), planes and mean (:294-296) -- fused into one launch per batch on the
 * device.  The samplers (tools/rand_sampler.py), the box arithmetic, the window and the resize tap tables stay on the host
 * (dspnet_amd/dataset/rand_sampler.py, dspnet_amd/dataset/det_iterator.py); of JPEG decoding only the entropy pass does
 * (dspn_jpeg.h reconstructs the pixels straight into the `images` pool read here).
 *
 * Per sample the reference runs (MXNet's image ops over OpenCV, third-party, version unpinned):
 *     data = fixed_crop(data, xmin, ymin, w, h)                      window inside the image, or
 *     data = full((h, w, 3), 128); data[-ymin:-ymin+H0, -xmin:-xmin+W0] = image    window around the image
 *     data = imresize(data, W, H, one of INTER_LINEAR, INTER_CUBIC, INTER_AREA, INTER_NEAREST, INTER_LANCZOS4)
 *     if mirror: data = flip(data, axis=1)
 *     data = transpose(data, (2, 0, 1)).astype(float32) - mean       (RGB source, mean is R, G, B: no channel swap)
 *
 * Here the resize is separable fixed point over tap tables the host builds (det_iterator.resize_taps).  A table of one
 * axis holds, for every output index d, a first canvas index first[d] and K coefficients q[d][0..K-1] (int16, every row
 * sums to 2048); tap j reads canvas index clamp(first[d] + j, 0, n - 1), i.e. the canvas -- the already cropped or padded
 * image -- is replicated at its edge, as a resize of that image does.  Per output (y, x) and channel c, exact integers:
 *     xd  = mirror ? W - 1 - x : x
 *     acc = sum_j qy[y][j] * ( sum_i qx[xd][i] * P(clamp(fy[y] + j), clamp(fx[xd] + i)) )      rows int32, columns int64
 *     P(py, px) = image[y0 + py][x0 + px][c] where that lies inside the image, else fill
 *     v   = min(255, max(0, (acc + (1 << 21)) >> 22))                arithmetic shift
 *     data_out[b][c][y][x] = (float)((double)v - mean[c])
 * The tap definitions (linear, cubic with A = -0.75, area as box average or as its two-tap rule, nearest, lanczos4) follow
 * OpenCV's resize as this project understands it.
 * PARITY STATUS: unpinned (no OpenCV in this image to produce vectors).  Two known differences from OpenCV:
 *   - one rounding rule for all methods: every method goes through the 11-bit tables and the one (acc + 2^21) >> 22 above,
 *     where OpenCV keeps float accumulators for the area method and its own fixed-point split for the others;
 *   - normalised rows: every coefficient row is forced to sum to exactly 2048 (the residual goes to its largest tap),
 *     where OpenCV rounds (or, for area, drops small partial covers) without renormalising.
 *
 * Conventions as in dspn_multibox.h: device pointers, caller-owned buffers, explicit stream, status return +
 * dspn_last_error(); argument checks before any HIP call.
 */
#ifndef DSPN_DET_AUGMENT_H_
#define DSPN_DET_AUGMENT_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* one decoded sample inside the batch's byte pool, with its window and its two tap tables */
typedef struct dspn_det_sample {
  long long img_offset;     /* byte offset of the (src_h, src_w, 3) RGB uint8 image in `images` */
  int src_h, src_w;
  int x0, y0;               /* window origin in image coordinates; negative in padding mode */
  int canvas_h, canvas_w;   /* window size: what is resized to (H, W); both >= 1 */
  int fill;                 /* value of a canvas pixel outside the image (all channels), 0..255 */
  int mirror;               /* != 0: horizontal flip after the resize */
  int kx, ky;               /* taps per output column / row, >= 1 */
  int xtab, ytab;           /* offsets (in ints) of this sample's x and y tables in `tables` */
} dspn_det_sample;

/* A table of an axis with n outputs and K taps occupies n + (n * K + 1) / 2 ints: n first-indices (int32), then the n * K
 * coefficients as int16, row major, two to an int.
 * images: device byte pool; samples: B descriptors in DEVICE memory; tables: device ints; mean[c] is subtracted from plane
 * c in double; data_out: (B, 3, H, W) float32.  H and W need not be multiples of anything.  The host that fills the
 * descriptors answers for them: offsets inside the pools, kx and ky as the tables were written (det_iterator.pack_batch
 * refuses more than 64 taps before any launch). */
int dspn_det_augment_batch_u8(const unsigned char *images, const dspn_det_sample *samples, const int *tables, int B, int H,
                              int W, const double mean[3], float *data_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif  /* DSPN_DET_AUGMENT_H_ */

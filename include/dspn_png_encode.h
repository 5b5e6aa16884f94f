/*
 * dspn_png_encode.h -- C ABI of the device half of the PNG encode, split at the same seam as the decode (dspn_png.h):
 *   device : the row filters -- every row of every image of a batch rewritten under the filter type a heuristic picks for
 *            it (dspn_png_filter_batch); a row reads only itself and the RAW row above it, so all rows are independent;
 *   host   : the deflate of each image's filtered stream and the chunks around it (dspnet_amd/dataset/png_encode.py on
 *            `zlib` and `struct`; serial per image, no native code).
 *
 * Output of an image: height rows of 1 + row_bytes bytes, row_bytes = width * bytes_per_pixel; the first byte of a row is
 * its filter type, the rest are the filtered bytes: what zlib.decompress of the IDAT data of the finished file returns.
 *
 * Sample formats (bytes_per_pixel says which):
 *   1: 8-bit grey, (height, width) uint8          2: 16-bit grey, (height, width) uint16 in native (little-endian) order,
 *   3: 8-bit RGB, (height, width, 3) uint8           written big-endian as PNG stores it; the filters run on those bytes
 *
 * Yardstick: the stream equals the one inside the file Pillow writes for the same pixels without optimize=True, byte for
 * byte.  The rule, per row, every byte modulo 256, with
 *   left = the byte bytes_per_pixel back in the row (0 before the first pixel), up = the same byte of the raw row above
 *   (0 for the first row), ul = the byte bytes_per_pixel back in the row above:
 *   candidates   type 0 (None) x        type 2 (Up) x - up        type 1 (Sub) x - left
 *                type 4 (Paeth) x - Paeth(left, up, ul): p = left + up - ul; the one of left, up, ul nearest to p, ties in
 *                that order.  Type 3 (Average) is never written.
 *   score        the sum over a candidate's bytes of v < 128 ? v : 256 - v
 *   choice       None, Up, Sub, Paeth are tried in this order; a later one replaces the choice only with a STRICTLY lower
 *                score.  (So a row of zeros stays None, and the first row never takes Up or Paeth: they equal None and Sub.)
 *
 * Conventions as in dspn_png.h: caller-owned buffers, explicit stream, status return + dspn_last_error().
 */
#ifndef DSPN_PNG_ENCODE_H_
#define DSPN_PNG_ENCODE_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* one image of a batch: 32 bytes, little-endian, no padding */
typedef struct dspn_png_enc_sample {
  long long src_offset;             /* byte offset in `src` of the image's first sample */
  long long out_offset;             /* byte offset in `out` of the image's first filter byte */
  int width, height;
  int bytes_per_pixel;              /* 1, 2 or 3: the formats above */
  int src_pitch;                    /* bytes from one source row to the next, >= width * bytes_per_pixel */
} dspn_png_enc_sample;
#define DSPN_PNG_ENC_SAMPLE_BYTES 32
#define DSPN_PNG_ENC_MAX_ROW_BYTES ((1 << 24) - 1)      /* a row's score then fits 32 bits */

/* height * (1 + width * bytes_per_pixel): the bytes dspn_png_filter_batch writes for one image.  Pure.  0 for a size below
 * 1, a bytes_per_pixel other than 1, 2, 3 or a row above DSPN_PNG_ENC_MAX_ROW_BYTES. */
long long dspn_png_filtered_bytes(int width, int height, int bytes_per_pixel);

/* bytes of `workspace` for a batch of n images (the descriptors and the row table on the device).  Pure. */
size_t dspn_png_filter_workspace_bytes(int n);

/* samples: n descriptors in HOST memory, read during the call; src: device byte pool of src_bytes bytes holding the
 * pixels; out: device byte pool of out_bytes bytes; workspace: device memory, 8-byte aligned.  Images of any mix of sizes
 * and formats; n == 0 is a no-op.  Every descriptor is checked before any HIP call: a null pointer, n < 0, a pool size or
 * an image size below 1, a bytes_per_pixel other than 1, 2, 3, a row above DSPN_PNG_ENC_MAX_ROW_BYTES, a pitch shorter
 * than a row, an image that runs past src_bytes or out_bytes, or more than 2^31 - 1 rows in all is DSPN_ERR_ARG (-1); a
 * short workspace is DSPN_ERR_WORKSPACE (-2).  Then: one copy of the checked descriptors and the row table into the
 * workspace (the call waits for it, so `samples` may be reused on return), and one launch on `stream` with one workgroup
 * per row of the batch.  Nothing outside [src, src + src_bytes) is read and nothing outside an image's
 * dspn_png_filtered_bytes output bytes is written.  No output alignment is assumed. */
int dspn_png_filter_batch(const dspn_png_enc_sample *samples, int n, const unsigned char *src, long long src_bytes,
                          unsigned char *out, long long out_bytes, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif  /* DSPN_PNG_ENCODE_H_ */

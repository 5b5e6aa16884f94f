/*
 * dspn_png.h -- C ABI of the device half of the PNG decode (label maps, id maps, disparity maps).  A PNG decode has two halves:
 *   host   : the chunk walk and the inflate of the concatenated IDAT data (dspnet_amd/dataset/png.py on `struct` and `zlib`;
 *            serial work, no native code);
 *   device : the filter reconstruction of the inflated rows for a whole batch (dspn_png_unfilter_batch), written straight into
 *            the byte pool dspn_augment_batch_u8 reads its label maps from.
 *
 * Input of an image: height rows of 1 + row_bytes bytes, row_bytes = width * bytes_per_pixel; the first byte of a row is its
 * filter type, the rest are the filtered bytes.  Reconstruction (the PNG specification's, per byte, modulo 256), with
 *   a = the reconstructed byte bytes_per_pixel to the left, b = the one above, c = the one above a; each 0 outside the image:
 *   type 0: x        type 1: x + a        type 2: x + b        type 3: x + floor((a + b) / 2), the sum not wrapped
 *   type 4: x + Paeth(a, b, c): p = a + b - c; the one of a, b, c nearest to p, ties in the order a, b, c
 * A type above 4 reconstructs like type 0 (the host half refuses such a stream before it gets here).
 * Output: the compact (height, width) samples without the filter bytes; two-byte samples are stored byte-swapped, so the pool
 * holds native little-endian uint16 (PNG is big-endian).
 *
 * Supported by the pair: greyscale 8-bit, palette 8-bit (the indices are the samples) and greyscale 16-bit, not interlaced.
 * Colour images go to packed RGB through dspn_png_rgb_batch (below), which shares the reconstruction.
 *
 * Conventions as in dspn_jpeg.h: caller-owned buffers, explicit stream, status return + dspn_last_error().
 */
#ifndef DSPN_PNG_H_
#define DSPN_PNG_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* one image of a batch: 32 bytes, little-endian, no padding */
typedef struct dspn_png_sample {
  long long raw_offset;             /* byte offset in `raw` of the image's first filter byte */
  long long out_offset;             /* byte offset in `out` of the (height, width) samples: dspn_warp_sample.seg_offset for
                                       one-byte samples */
  int width, height;
  int bytes_per_pixel;              /* 1 or 2 */
  int skip;                         /* != 0: decoded some other way; nothing is read or written for this image */
} dspn_png_sample;
#define DSPN_PNG_SAMPLE_BYTES 32

/* raw: raw_bytes bytes of inflated rows in device memory; samples: n descriptors in DEVICE memory (8-byte aligned);
 * out: device byte pool of out_bytes bytes.  One launch on `stream`, one workgroup per image; n == 0 is a no-op.  The
 * descriptors are not trusted: every one is checked on the device against raw_bytes and out_bytes (in arithmetic that cannot
 * overflow) before anything is touched, and one that could index outside either pool, or whose bytes_per_pixel is neither 1
 * nor 2, is treated like skip.  Nothing outside [raw, raw + raw_bytes) is read, nothing outside an image's
 * height * width * bytes_per_pixel output bytes is written. */
int dspn_png_unfilter_batch(const unsigned char *raw, long long raw_bytes, const dspn_png_sample *samples, int n,
                            unsigned char *out, long long out_bytes, void *stream);

/* ---- colour images straight to RGB ---------------------------------------------------------------------------------------
 * The device half of Image.open(...).convert("RGB") for every non-interlaced PNG format but 16-bit greyscale, in two launches:
 *   a. the reconstruction above at the format's filter stride.  A pixel is channels * bit_depth bits (channels: greyscale 1,
 *      RGB 3, palette 1, grey + alpha 2, RGBA 4); a row is row_bytes = ceil(width * channels * bit_depth / 8) bytes behind its
 *      filter byte, and a, c lie max(1, channels * bit_depth / 8) bytes to the left: 1, 2, 3, 4, 6 or 8.  Packed 1-, 2- and
 *      4-bit rows reconstruct as bytes, 16-bit samples stay in stream order (high byte first).  RGB 8-bit rows are written
 *      straight to `out`; every other format goes to the workspace at recon_offset, height * row_bytes bytes;
 *   b. samples to packed RGB, (height, width, 3) bytes at out_offset:
 *        RGBA 8                 bytes 0, 1, 2 of each 4
 *        grey 8                 g, g, g
 *        grey + alpha 8         byte 0 of each 2, three times
 *        RGB 16 / RGBA 16       bytes 0, 2, 4 (the high bytes) of each 6 / 8
 *        grey + alpha 16        byte 0 of each 4, three times
 *        grey 4 / 2 / 1 bit     nibble * 17, pair * 85, bit * 255, three times; the most significant bits of a byte come
 *                               first, every row starts on a byte
 *        palette 8 / 4 / 2 / 1  the three bytes at 3 * index of the image's palette table (index unpacked as for grey)
 *      A palette table is 768 bytes: the PLTE chunk's data, zero-padded, so an index at or past the chunk's entry count gives
 *      (0, 0, 0).  Alpha and tRNS take no part.  16-bit greyscale is not on this path (dspn_png_unfilter_batch keeps its 16
 *      bits); interlaced streams are not supported. */
typedef struct dspn_png_rgb_sample {
  long long raw_offset;             /* byte offset in `raw` of the image's first filter byte */
  long long recon_offset;           /* byte offset in `ws` of the reconstructed rows; not read for RGB 8-bit */
  long long out_offset;             /* byte offset in `out` of the (height, width, 3) RGB bytes */
  int width, height;
  int bit_depth, colour_type;       /* as in IHDR; legal pairs: 0: 1 2 4 8; 2: 8 16; 3: 1 2 4 8; 4: 8 16; 6: 8 16 */
  int palette_index;                /* colour type 3: which 768-byte table of `palettes`; not read otherwise */
  int skip;                         /* != 0: decoded some other way; nothing is read or written for this image */
} dspn_png_rgb_sample;
#define DSPN_PNG_RGB_SAMPLE_BYTES 48
#define DSPN_PNG_PALETTE_BYTES 768

/* The least ws_bytes with which no descriptor of host_samples (HOST memory) is refused for its workspace range: the largest
 * recon_offset + height * row_bytes over the descriptors that use the workspace (not skipped, a legal pair other than RGB
 * 8-bit, positive sizes, recon_offset >= 0); 0 when there is none.  Pure: no HIP call. */
size_t dspn_png_rgb_workspace_bytes(const dspn_png_rgb_sample *host_samples, int n);

/* raw, samples, out as in dspn_png_unfilter_batch; palettes: n_palettes tables of 768 bytes in device memory (may be null
 * when n_palettes == 0); ws: ws_bytes bytes of device scratch (may be null when ws_bytes == 0), whose contents are undefined
 * afterwards.  Two launches on `stream` (workgroup per image, then a grid over the pixels of every image); n == 0 is a no-op.
 * The descriptors are not trusted: both launches check every one against raw_bytes, ws_bytes and out_bytes in arithmetic
 * that cannot overflow, and one that could index outside a pool, whose (bit_depth, colour_type) is not a legal pair of this
 * path, or (colour type 3) whose palette_index is not in [0, n_palettes), is treated like skip: a workspace too small for a
 * descriptor leaves that image undecoded.  Nothing outside an image's height * width * 3 output bytes is written to `out`. */
int dspn_png_rgb_batch(const unsigned char *raw, long long raw_bytes, const dspn_png_rgb_sample *samples, int n,
                       const unsigned char *palettes, int n_palettes, unsigned char *out, long long out_bytes,
                       unsigned char *ws, long long ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif  /* DSPN_PNG_H_ */

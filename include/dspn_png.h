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
 *
 * Conventions as in dspn_jpeg.h: caller-owned buffers, explicit stream, status return + dspn_last_error().
 */
#ifndef DSPN_PNG_H_
#define DSPN_PNG_H_

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

#ifdef __cplusplus
}
#endif
#endif  /* DSPN_PNG_H_ */

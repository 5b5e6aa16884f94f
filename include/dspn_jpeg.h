/*
 * dspn_jpeg.h -- C ABI of the record iterator's JPEG decode, split where the work stops being serial:
 *   host   : marker parsing and Huffman decoding into quantised DCT coefficients (dspn_jpeg_probe,
 *            dspn_jpeg_entropy_decode; plain C++, no HIP call, thread-safe, no global state);
 *   device : dequantisation, 8 x 8 inverse DCT, chroma upsampling and YCbCr -> RGB for the whole batch
 *            (dspn_jpeg_reconstruct_batch_u8), written straight into the byte pool dspn_augment_batch_u8 reads.
 * The upload of a 4:2:0 image is its int16 coefficients, 1.5 samples per pixel = 3 B per pixel, as many as RGB8.
 *
 * Yardstick: the pixels equal libjpeg-turbo's with the accurate integer IDCT and "fancy" upsampling (what Pillow
 * decodes with), byte for byte.  The arithmetic, all of it integer:
 *   dequantise, then the "slow integer" IDCT with 13 constant bits and 2 extra bits after pass 1; one 1-D pass over i[0..7]:
 *     even: z1 = (i2 + i6) * 4433; t2 = z1 - i6 * 15137; t3 = z1 + i2 * 6270; t0 = (i0 + i4) << 13; t1 = (i0 - i4) << 13;
 *           t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
 *     odd : a0, a1, a2, a3 = i7, i5, i3, i1; z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3; z5 = (z3 + z4) * 9633;
 *           a0 *= 2446; a1 *= 16819; a2 *= 25172; a3 *= 12299; z1 *= -7373; z2 *= -20995; z3 = z3 * -16069 + z5;
 *           z4 = z4 * -3196 + z5; a0 += z1 + z3; a1 += z2 + z4; a2 += z2 + z3; a3 += z1 + z4
 *     out : t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3, each (x + (1 << (s - 1))) >> s;
 *           pass 1 down the columns with s = 11, pass 2 along the rows of the result with s = 18; sample = clamp(. + 128)
 *   chroma upsampling over the component's real extent ceil(W h / hmax) x ceil(H v / vmax), edges replicated:
 *     2 x 2: rows s = 3 near + far (far: the row above for even output rows, below for odd ones), then
 *            even = (3 s[x] + s[x - 1] + 8) >> 4, odd = (3 s[x] + s[x + 1] + 7) >> 4
 *     2 x 1: even = (3 p[x] + p[x - 1] + 1) >> 2, odd = (3 p[x] + p[x + 1] + 2) >> 2
 *     a chroma plane of at most two columns (images up to 4 pixels wide): each sample repeated 2 x 2 or 2 x 1 instead,
 *            down the rows as well (libjpeg-turbo takes the triangle filter only for downsampled_width > 2)
 *   colour, F(x) = int(x * 65536 + 0.5), cb -= 128, cr -= 128, arithmetic shifts, clamp to 0..255:
 *     R = Y + ((F(1.402) cr + 32768) >> 16); B = Y + ((F(1.772) cb + 32768) >> 16);
 *     G = Y + ((-F(0.34414) cb + 32768 - F(0.71414) cr) >> 16); one component writes Y to all three channels.
 *
 * Supported: baseline sequential Huffman (SOF0), 8-bit samples, one scan; one component, or three (YCbCr) with luma
 * sampling 1x1, 2x1 or 2x2 and chroma 1x1.  Anything else is `supported = 0` with a reason, not an error: the caller
 * decodes such a stream some other way.  A malformed stream is an error status with a message.
 *
 * Conventions as in dspn_multibox.h: caller-owned buffers, explicit stream, status return + dspn_last_error().
 */
#ifndef DSPN_JPEG_H_
#define DSPN_JPEG_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* dspn_jpeg_info.reason */
enum {
  DSPN_JPEG_OK = 0,
  DSPN_JPEG_PROGRESSIVE = 1,        /* SOF2 */
  DSPN_JPEG_EXTENDED = 2,           /* SOF1 */
  DSPN_JPEG_ARITHMETIC = 3,         /* SOF9..SOF15 */
  DSPN_JPEG_LOSSLESS_HIERARCHICAL = 4, /* SOF3, SOF5..SOF7 */
  DSPN_JPEG_PRECISION = 5,          /* samples are not 8-bit */
  DSPN_JPEG_COMPONENTS = 6,         /* neither 1 nor 3 components */
  DSPN_JPEG_SAMPLING = 7,           /* luma not 1x1 / 2x1 / 2x2, or chroma not 1x1 */
  DSPN_JPEG_MULTISCAN = 8,          /* the first scan does not carry every component in frame order */
  DSPN_JPEG_COLOR_TRANSFORM = 9,    /* three components that are not YCbCr (Adobe transform 0, or ids 'R' 'G' 'B') */
  DSPN_JPEG_QUANT_16BIT = 10        /* a 16-bit quantisation table */
};

/* what the markers up to SOS say about a stream */
typedef struct dspn_jpeg_info {
  int width, height;
  int ncomp;                        /* components of the frame (filled for unsupported frames too) */
  int restart_interval;             /* MCUs between RSTn markers, 0: none */
  int hsamp[3], vsamp[3];           /* sampling factors per component (1 x 1 for a single component) */
  int blocks_w[3], blocks_h[3];     /* padded block grid per component: whole MCUs */
  int supported, reason;            /* supported != 0 <=> reason == DSPN_JPEG_OK */
  long long coef_count;             /* int16 coefficients of the stream: 64 * sum of blocks_w * blocks_h */
  long long coef_offset[3];         /* first coefficient of each component inside those */
  unsigned char quant[3][64];       /* quantisation table of each component, natural (row-major) order */
} dspn_jpeg_info;

/* Parses the markers up to the first SOS.  0: `info` is filled (width, height and ncomp also when supported == 0);
 * < 0: the stream is malformed or truncated inside its headers. */
int dspn_jpeg_probe(const unsigned char *bytes, size_t n, dspn_jpeg_info *info);

/* Huffman-decodes the scan into coef_out (info->coef_count int16 values, host memory): per component a raster of
 * blocks over its padded grid (coef_offset, blocks_w, blocks_h), each block 64 values in natural order (the zigzag is
 * undone here), quantised as stored.  `info` must be what dspn_jpeg_probe said of these bytes, supported.  A truncated or
 * corrupt scan is an error status; nothing past bytes[n - 1] is read and nothing past coef_out[coef_count - 1] written. */
int dspn_jpeg_entropy_decode(const unsigned char *bytes, size_t n, const dspn_jpeg_info *info, short *coef_out);

/* one stream of a batch, for the device */
typedef struct dspn_jpeg_sample {
  long long coef_offset[3];         /* first coefficient (int16 index, a multiple of 64) of each component in `coefs` */
  long long img_offset;             /* byte offset of the (height, width, 3) RGB uint8 output in `images_out`:
                                       dspn_warp_sample.img_offset */
  int width, height;
  int ncomp;                        /* 1 or 3 */
  int skip;                         /* != 0: decoded some other way; nothing is read or written for this sample */
  int hsamp, vsamp;                 /* luma sampling (chroma is 1 x 1): 1x1, 2x1 or 2x2 */
  int blocks_w[3], blocks_h[3];
  unsigned char quant[3][64];
} dspn_jpeg_sample;

/* bytes of `workspace` for a batch of coef_count coefficients (the uint8 component planes between the two launches) */
size_t dspn_jpeg_reconstruct_workspace_bytes(long long coef_count);

/* coefs: coef_count int16 in device memory (16-byte aligned); samples: B <= 1024 descriptors in DEVICE memory;
 * images_out: device byte pool of images_bytes bytes.  Two launches on `stream`, each over the whole batch.  The
 * descriptors are not trusted: a sample whose sizes, grids or offsets could index outside coefs, the workspace or
 * images_out (or contradict each other) is treated like skip. */
int dspn_jpeg_reconstruct_batch_u8(const short *coefs, long long coef_count, const dspn_jpeg_sample *samples, int B,
                                   unsigned char *images_out, long long images_bytes, void *workspace,
                                   size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif  /* DSPN_JPEG_H_ */

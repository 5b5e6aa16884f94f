/*
 * dspn_jpeg.h -- C ABI of the record iterator's JPEG decode, split where the work stops being serial:
 *   host   : marker parsing and Huffman decoding into quantised DCT coefficients (dspn_jpeg_probe,
 *            dspn_jpeg_entropy_decode; plain C++, no HIP call, thread-safe, no global state); for a stream with restart
 *            intervals only the search for the markers (dspn_jpeg_scan_index), the Huffman decoding then runs on the
 *            device, one interval per lane (dspn_jpeg_entropy_decode_batch; below);
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

/* ---- entropy pass on the device: streams with restart intervals ------------------------------------------------------
 * Baseline Huffman decoding is serial only between restart markers: at each RSTn the bit stream is byte-aligned and the DC
 * predictors reset, so every restart interval is a unit of work of its own.  The host only finds the markers
 * (dspn_jpeg_scan_index: no Huffman work), the device decodes one interval per lane (dspn_jpeg_entropy_decode_batch) into
 * the coefficient pool dspn_jpeg_reconstruct_batch_u8 reads.  The upload is the compressed scan instead of 3 B per pixel. */

/* Most MCUs of one restart interval the device pass takes: the serial work of one lane.  A stream with a longer interval
 * (or none) stays on the host pass.  Measured (profiles/jpeg_device_entropy.txt): the launch's time grows in proportion to
 * the interval, and above about 40 MCUs it is slower than the host pass on the 16 threads a job has; 32 is the largest power
 * of two below that.  (The first value, 512, was 40 times slower than the host.) */
#define DSPN_JPEG_DEVICE_MAX_INTERVAL 32

/* dspn_jpeg_entropy_decode_batch's status word of a sample: 0, or ((DSPN_JPEG_STATUS_SEGMENTS - first bad segment) << 3) | code
 * (an atomic maximum over the lanes, so the FIRST bad segment of the sample wins) */
#define DSPN_JPEG_STATUS_SEGMENTS ((1 << 27) - 1)
enum {
  DSPN_JPEG_BAD_CODE = 1,           /* a Huffman code that is not in its table */
  DSPN_JPEG_BAD_INDEX = 2,          /* a coefficient index (or a zero run) past 63 */
  DSPN_JPEG_BAD_SIZE = 3,           /* a DC difference of more than 11 bits, an AC value of more than 10 */
  DSPN_JPEG_BAD_END = 4,            /* the segment's data ends inside a block */
  DSPN_JPEG_BAD_REST = 5,           /* a whole byte or more of unread data before the segment's end */
  DSPN_JPEG_BAD_DC = 6,             /* a DC value outside int16 */
  DSPN_JPEG_BAD_SEGMENT = 7         /* the segment table or a Huffman table of the descriptor contradicts itself */
};

/* one stream of a batch for the device entropy pass, beside its dspn_jpeg_sample (which keeps its layout) */
typedef struct dspn_jpeg_scan {
  long long data_offset;            /* first byte of the entropy-coded data in the batch's byte pool (dspn_jpeg_scan_index
                                       leaves the offset inside the stream here; the caller adds where it put the bytes) */
  long long data_bytes;             /* bytes of entropy-coded data, up to the marker that ends the scan */
  long long first_segment;          /* index of the stream's first entry in the batch's segment table */
  int segments;                     /* restart intervals of the scan; 0: the coefficients of this sample come from elsewhere */
  int restart_interval;             /* MCUs per interval, 1..DSPN_JPEG_DEVICE_MAX_INTERVAL */
  int mcus_w, mcus_h;               /* the MCU grid */
  unsigned char dc_table[4], ac_table[4];     /* Huffman table selector of each component */
  unsigned char dc_counts[4][16], ac_counts[4][16];   /* the tables as the DHT segments carry them: codes per length 1..16 */
  unsigned char dc_values[4][256], ac_values[4][256]; /* and the symbols in code order (a table that is not defined: all zero) */
} dspn_jpeg_scan;

/* restart intervals of the scan `info` describes: ceil(MCUs / restart_interval); 0 without a restart interval or for an
 * unsupported stream.  Pure. */
long long dspn_jpeg_scan_segments(const dspn_jpeg_info *info);

/* Finds the restart intervals of the scan: walks from SOS to the marker that ends the scan looking only at 0xFF bytes
 * (FF 00 is stuffing, FF FF fill, FF D0..D7 a restart marker) and writes dspn_jpeg_scan_segments(info) + 1 offsets into
 * seg_offsets, relative to the first byte of entropy-coded data: where the data of every interval starts, and where the
 * marker that ends the scan stands.  `scan` is filled for a pool that holds the stream's bytes from 0 and a segment table
 * that holds only these offsets.  `info` must be what dspn_jpeg_probe said of these bytes.  Plain C++, no HIP call,
 * thread-safe, no global state.  < 0 with a message: a stream without a restart interval or with one above
 * DSPN_JPEG_DEVICE_MAX_INTERVAL (it stays on the host pass), restart markers that are missing, misnumbered (0..7 in cycle) or
 * too many, a scan that does not end at a marker, or seg_capacity below the count. */
int dspn_jpeg_scan_index(const unsigned char *bytes, size_t n, const dspn_jpeg_info *info, dspn_jpeg_scan *scan,
                         unsigned int *seg_offsets, size_t seg_capacity);

/* The entropy pass of a batch on the device, one launch on `stream` in front of dspn_jpeg_reconstruct_batch_u8's two:
 * bytes: the byte pool (device, bytes_count bytes); samples, scans: B <= 1024 descriptors each (device); segments: the
 * segment table (device, segment_count entries); coefs: the int16 pool (device, 16-byte aligned); status: B ints (device),
 * zeroed here on `stream`.  One restart interval is one unit of work and one lane decodes it serially; the coefficients are
 * exactly dspn_jpeg_entropy_decode's, every block of the padded grids of a decoded sample written in full.
 * Nothing is trusted: a sample whose descriptors contradict themselves or each other, or could index outside a pool, is no
 * work, like skip (so is segments == 0); a lane reads no byte outside its segment and writes no block outside its MCUs; a
 * lane that meets bad data stops and leaves a status word (above) for its sample, whose pixels are then unspecified.
 * Nothing else is affected. */
int dspn_jpeg_entropy_decode_batch(const unsigned char *bytes, long long bytes_count, const dspn_jpeg_sample *samples,
                                   const dspn_jpeg_scan *scans, int B, const unsigned int *segments, long long segment_count,
                                   short *coefs, long long coef_count, int *status, void *stream);

/* The same decode, the same program text (csrc/jpeg_huff.h), built for the host and run serially over the segments of ONE
 * sample, all pointers in host memory: what the tests and tools/jpeg_huff_check.cpp compare and run under the sanitizers.
 * *status receives the status word.  0 also when the status word is not: the call itself went well. */
int dspn_jpeg_entropy_decode_segments(const unsigned char *bytes, long long bytes_count, const dspn_jpeg_sample *sample,
                                      const dspn_jpeg_scan *scan, const unsigned int *segments, long long segment_count,
                                      short *coefs, long long coef_count, int *status);

#ifdef __cplusplus
}
#endif
#endif  /* DSPN_JPEG_H_ */

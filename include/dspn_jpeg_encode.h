/*
 * dspn_jpeg_encode.h -- C ABI of the baseline JPEG encode, split at the same seam as the decode (dspn_jpeg.h):
 *   device : everything per pixel -- RGB -> YCbCr, chroma downsampling, 8 x 8 forward DCT, quantisation -- for a whole
 *            batch of images of mixed sizes (dspn_jpeg_encode_blocks_batch_u8), into the decoder's coefficient layout;
 *   host   : the serial part -- markers and Huffman coding with Annex K's tables (dspn_jpeg_entropy_encode; plain C++,
 *            no HIP call, thread-safe, no global state) -- and the quantisation tables of a quality (dspn_jpeg_quant_tables).
 *
 * Yardstick: the file equals what libjpeg-turbo writes for the same pixels with its default ("slow integer") forward
 * DCT and standard Huffman tables -- Pillow's Image.save(format="JPEG", quality=q, subsampling=s), and with a restart
 * interval of n MCUs (dspn_jpeg_entropy_encode_restart) the same call with restart_marker_blocks=n -- byte for byte.  The arithmetic, all of it integer (32 bits suffice), in the order it is applied:
 *   colour, F(x) = int(x * 65536 + 0.5), arithmetic shifts:
 *     Y  = ( F(.299) R + F(.587) G + F(.114) B + 32768) >> 16
 *     Cb = (-F(.16874) R - F(.33126) G + F(.5) B + (128 << 16) + 32767) >> 16
 *     Cr = ( F(.5) R - F(.41869) G - F(.08131) B + (128 << 16) + 32767) >> 16;  one component passes through unchanged
 *   grids: the REAL grid of a component is ceil(ceil(W h / hmax) / 8) x ceil(ceil(H v / vmax) / 8) blocks; that is what
 *     blocks_w / blocks_h mean in this header (the decoder's are padded to whole MCUs).  Luma and every full-size plane
 *     replicate the last column and the last row out to the grid.
 *   chroma downsampling:
 *     2 x 2: full-resolution columns past the last one repeat it, full-resolution rows are repeated to an even count only;
 *            out = (a + b + c + d + bias) >> 2, bias 1, 2, 1, 2 ... by output column; then the last DOWNSAMPLED row is
 *            repeated down to 8 * blocks_h.  (The two directions pad on different sides of the average.)
 *     2 x 1: the same column rule, out = (a + b + bias) >> 1, bias 0, 1, 0, 1 ...; rows repeat like luma's.
 *   forward DCT of sample - 128: the "slow integer" form with 13 constant bits and 2 extra bits after pass 1, rows first,
 *     then columns.  One 1-D pass over d[0..7], D(x, n) = (x + (1 << (n - 1))) >> n, s = 11 (rows) or 15 (columns):
 *       t0, t7 = d0 +- d7; t1, t6 = d1 +- d6; t2, t5 = d2 +- d5; t3, t4 = d3 +- d4; t10, t13 = t0 +- t3; t11, t12 = t1 +- t2
 *       rows: o0 = (t10 + t11) << 2, o4 = (t10 - t11) << 2;  columns: o0 = D(t10 + t11, 2), o4 = D(t10 - t11, 2)
 *       z1 = (t12 + t13) * 4433; o2 = D(z1 + t13 * 6270, s); o6 = D(z1 - t12 * 15137, s)
 *       z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7; z5 = (z3 + z4) * 9633;
 *       t4 *= 2446; t5 *= 16819; t6 *= 25172; t7 *= 12299; z1 *= -7373; z2 *= -20995; z3 = z3 * -16069 + z5; z4 = z4 * -3196 + z5
 *       o7 = D(t4 + z1 + z3, s); o5 = D(t5 + z2 + z4, s); o3 = D(t6 + z2 + z3, s); o1 = D(t7 + z1 + z4, s)
 *   quantise: q8 = table[i] << 3; coef = sign(x) * ((|x| + (q8 >> 1)) / q8), truncating division.
 *
 * The host pass writes SOI, APP0 (JFIF 1.01, units 0, density 1 x 1), one DQT per table (two for colour, one for grey), SOF0
 * (component ids 1, 2, 3), one DHT per table (DC0, AC0, DC1, AC1; two for grey), SOS, the scan (MCU-interleaved for colour,
 * a raster over the real grid for grey; 0xFF stuffed; last byte padded with 1 bits), EOI.  Positions of the MCU grid beyond a
 * component's real grid are dummy blocks, made up here as libjpeg makes them: all AC zero, DC equal to the DC of the
 * previous block in that MCU's block order (a dummy luma row of a 2 x 2 MCU takes the DC of the block before it in the
 * MCU, not of the block above it).
 *
 * Conventions as in dspn_jpeg.h: caller-owned buffers, explicit stream, status return + dspn_last_error().
 */
#ifndef DSPN_JPEG_ENCODE_H_
#define DSPN_JPEG_ENCODE_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Annex K's luminance and chrominance tables scaled as libjpeg scales them (scale = 5000 / q below 50, else 200 - 2 q;
 * (std * scale + 50) / 100 clamped to 1..255), in natural (row-major) order.  0, or < 0 for a quality outside 1..100. */
int dspn_jpeg_quant_tables(int quality, unsigned char lum[64], unsigned char chr[64]);

/* one image of a batch: the geometry both halves work from.  For three components the chroma sampling is 1 x 1 and
 * hsamp x vsamp (1x1, 2x1 or 2x2) is luma's; a single component is 1 x 1. */
typedef struct dspn_jpeg_enc_sample {
  long long coef_offset[3];         /* first coefficient (int16 index, a multiple of 64) of each component */
  long long img_offset;             /* byte offset of the interleaved uint8 pixels in `images`: (height, width, 3), or
                                       (height, width) for one component */
  int width, height;
  int ncomp;                        /* 1 or 3 */
  int skip;                         /* != 0: nothing is read or written for this sample */
  int hsamp, vsamp;
  int blocks_w[3], blocks_h[3];     /* the real grid of each component */
  unsigned char quant[3][64];       /* quantisation table of each component, natural order */
} dspn_jpeg_enc_sample;

/* Fills blocks_w, blocks_h and coef_offset (components back to back from coef_base) of `s` from its width, height, ncomp,
 * hsamp and vsamp, and returns the coefficients of the image through *coef_count.  Pure.  < 0: not a supported geometry. */
int dspn_jpeg_encode_geometry(dspn_jpeg_enc_sample *s, long long coef_base, long long *coef_count);

/* bytes of `workspace` for a batch of coef_count coefficients (the uint8 component planes between the two launches) */
size_t dspn_jpeg_encode_workspace_bytes(long long coef_count);

/* images: device byte pool of images_bytes bytes; channel_map: the channel index of R, G and B in a three-channel pixel
 * ({0, 1, 2} for RGB, {2, 1, 0} for BGR; host memory, read during the call); samples: B <= 1024 descriptors in DEVICE
 * memory; coefs_out: coef_count int16 in device memory (16-byte aligned).  Two launches on `stream`, each over the whole
 * batch: pixels -> component planes in the workspace, planes -> coefficients.  Every block of a valid sample's real grids
 * is written in full, per component a raster of blocks, 64 values in natural order each.  The descriptors are not
 * trusted: a sample whose sizes, grids or offsets could index outside images, the workspace or coefs_out, or whose grids
 * are not the real grids of its size and sampling, is treated like skip. */
int dspn_jpeg_encode_blocks_batch_u8(const unsigned char *images, long long images_bytes, const int channel_map[3],
                                     const dspn_jpeg_enc_sample *samples, int B, short *coefs_out, long long coef_count,
                                     void *workspace, size_t workspace_bytes, void *stream);

/* Writes the whole file for the coefficients of ONE image: coefs + s->coef_offset[c] is component c's raster (host
 * memory), s as dspn_jpeg_encode_geometry filled it, with its quant tables (components 1 and 2 must share one).
 * *length is the size of the file.  If that exceeds `capacity` the status is DSPN_ERR_WORKSPACE (-2), the message and
 * *length state the needed size, and nothing past out[capacity - 1] is written.  A coefficient outside what baseline
 * Huffman coding can carry (a DC difference of more than 11 bits, an AC value of more than 10) is an error. */
int dspn_jpeg_entropy_encode(const short *coefs, const dspn_jpeg_enc_sample *s, unsigned char *out, size_t capacity,
                             size_t *length);

/* dspn_jpeg_entropy_encode with restart markers every restart_interval MCUs (0..65535; 0 gives exactly the bytes of the
 * entry above): a DRI segment where libjpeg writes it (in the scan header, behind the DHTs and in front of SOS), RSTn
 * (n = 0..7 in cycle) after every restart_interval MCUs except the last, the partial byte in front of each marker padded
 * with 1 bits, the DC predictors reset at each marker.  The dummy-block rule of the header note is unchanged: a dummy
 * block takes the DC of the block before it in the MCU's order, whatever the predictor was reset to.  Such a file equals
 * Pillow's with restart_marker_blocks=restart_interval (restart_marker_rows=r: r times the MCUs of a row), and every
 * restart interval of it is a unit of work of its own for dspn_jpeg_entropy_decode_batch (dspn_jpeg.h). */
int dspn_jpeg_entropy_encode_restart(const short *coefs, const dspn_jpeg_enc_sample *s, int restart_interval,
                                     unsigned char *out, size_t capacity, size_t *length);

/* SOI through the SOS header of the file above: exactly the bytes dspn_jpeg_entropy_encode_restart writes in front of the
 * first byte of the scan (the DRI segment included when restart_interval is not 0), from the same code.  Host only; the
 * descriptor is checked as there, capacity and *length behave as there (-2, *length names the need, nothing is written
 * past out[capacity - 1]).  headers + scan + FF D9 is the file. */
int dspn_jpeg_encode_headers(const dspn_jpeg_enc_sample *s, int restart_interval, unsigned char *out, size_t capacity,
                             size_t *length);

/* --- the entropy pass on the device ---------------------------------------------------------------------------------------
 * The scan of every image of a batch -- the bytes between the SOS header and EOI of dspn_jpeg_entropy_encode_restart's
 * file, byte for byte -- Huffman-coded on the device from the coefficient pool dspn_jpeg_encode_blocks_batch_u8 left.
 * In encoding only the bit position is serial, so the pass works per block slot of the scan (dummy blocks included) for
 * every file, with or without restart markers: count the bits of every slot, prefix-sum them within each restart interval
 * (the whole image when there is none), write every slot's bits at its offset into a zeroed, unstuffed stream whose
 * intervals each end on a byte padded with 1 bits, count the FF bytes, and write the stuffed bytes and the RSTn markers at
 * their final places.  Two calls, because the caller sizes and lays out the output between them:
 *
 *   dspn_jpeg_entropy_encode_scan_batch : everything up to the FF count.  When `stream` has run it, scan_bytes[i] is the
 *     exact size of image i's scan and status[i] is 0: ok; 1: the sample is skipped or not trusted (the coefficient-side
 *     rules of dspn_jpeg_encode_blocks_batch_u8: geometry, real grids, offsets inside coef_count; or a restart interval
 *     outside 0..65535; or descriptors that overlap so much that the batch names more blocks than coef_count holds);
 *     2: a coefficient baseline coding cannot carry (a DC difference of more than 11 bits, an AC value of more than 10).
 *     scan_bytes[i] is 0 unless status[i] is 0.
 *   dspn_jpeg_entropy_encode_write_batch : image i's scan goes to out[out_offsets[i] .. out_offsets[i] + scan_bytes[i]).
 *     `workspace` is the one the scan call filled, untouched since; coef_count and B are that call's (a workspace that
 *     does not say so writes nothing).  An image whose status was not 0
 *     or whose range does not lie inside [0, out_bytes) writes nothing; no byte outside those ranges is written.
 *
 * coefs, samples, restart_intervals (one per image, in MCUs, 0: none), scan_bytes, status, out_offsets, out and workspace
 * are device memory; coefs and workspace 16-byte aligned, the long long arrays and samples 8-byte aligned.  B <= 1024.
 * Argument errors are reported before any HIP call.
 *
 * Workspace: with n = coef_count / 64 blocks in the pool, a batch has at most n real slots and at most 4 n slots in all (an
 * MCU of a 2 x 2 image holds four luma slots of which one at least is real; chroma has no dummies).  A real block emits at
 * most 11 + 11 bits of DC (the longest DC code, the longest difference) and 63 x (16 + 10) bits of AC (a 16-bit code and 10
 * value bits per coefficient; a ZRL code only where 16 coefficients emit nothing), 1660 bits, and at most 7 bits of
 * padding: 209 bytes.  A dummy emits a DC code, its difference and EOB, at most 11 + 11 + 4 + 7 bits: 5 bytes.  The
 * unstuffed stream is therefore at most 209 n + 5 * 3 n bytes; beside it the workspace holds one bit per byte of it
 * (where a marker goes), 12 bytes per slot (bit count, bit offset), one count per 1024 bytes and per 1024 slots, and a
 * header of per-image records. */
size_t dspn_jpeg_entropy_encode_workspace_bytes(long long coef_count, int B);

int dspn_jpeg_entropy_encode_scan_batch(const short *coefs, long long coef_count, const dspn_jpeg_enc_sample *samples,
                                        const int *restart_intervals, int B, long long *scan_bytes, int *status,
                                        void *workspace, size_t workspace_bytes, void *stream);

int dspn_jpeg_entropy_encode_write_batch(long long coef_count, int B, const long long *out_offsets, unsigned char *out,
                                         long long out_bytes, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif  /* DSPN_JPEG_ENCODE_H_ */

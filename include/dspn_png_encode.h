/*
 * dspn_png_encode.h -- C ABI of the device half of the PNG encode, split at the same seam as the decode (dspn_png.h):
 *   device : the row filters -- every row of every image of a batch rewritten under the filter type a heuristic picks for
 *            it (dspn_png_filter_batch); a row reads only itself and the RAW row above it, so all rows are independent;
 *   host   : the deflate of each image's filtered stream and the chunks around it (dspnet_amd/dataset/png_encode.py on
 *            `zlib` and `struct`; serial per image, no native code);
 *   device, on request: the deflate as well (dspn_png_deflate_batch, below), by a rule that has no serial parse; the host
 *            then adds only the chunks and their CRC-32.
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
 * The device deflate writes one complete zlib stream per input stream: the two bytes 78 01, deflate blocks, the Adler-32 of
 * the input, big-endian.  The rule (dspnet_amd/csrc/png_deflate_host.h is its text, run by the device and by
 * dspn_png_deflate_host alike, so both give the same bytes):
 *   blocks       the input is cut into blocks of DSPN_PNG_DEFLATE_BLOCK bytes, the last one may be shorter.  Blocks are
 *                independent: runs are cut at a block's first byte, no match reaches in front of its block.
 *   tokens       in a maximal run of r equal bytes inside a block, with j the place inside the run: j = 0 is a literal;
 *                match pieces of distance 1 start at j = 1 + 258 k; a piece has length min(258, r - j) when that is at least
 *                3, otherwise the remaining 1 or 2 bytes are literals.
 *   codes        every block is a dynamic block (BTYPE 2).  The literal/length code lengths, at most 15, come from the
 *                block's own histogram with the end-of-block symbol counted once: Huffman over the used symbols in ascending
 *                (count, symbol) order, a leaf before an internal node of equal weight; depths beyond the limit are cut to
 *                it and the Kraft excess is taken back one unit of 2^-limit at a time (a leaf of the deepest level below
 *                the limit and a leaf of the limit both move one below the former); the lengths are then handed out in that
 *                order, longest first.  Where the unlimited code fits the limit the cost is exactly its cost.  The distance
 *                code is always the single symbol 0 with length 1 (HDIST = 0), also in a block without a match.  The lengths
 *                are sent as one sequence of HLIT + 1 values under the repeat symbols 16, 17, 18 (a zero run takes 18 while
 *                11 or more remain, then 17 for 3 or more; a non-zero length is sent once, then 16 while 3 or more remain)
 *                with a code-length code of at most 7 bits built by the same function.
 *   stored       a block whose dynamic form takes more than 8 * (bytes + 5) bits is a stored block (BTYPE 0): three bits,
 *                zeros up to a whole byte, LEN, NLEN, the bytes.
 *   bound        a dynamic block takes at most 8 * bytes + 40 bits, a stored one 3 + 7 + 32 + 8 * bytes = 8 * bytes + 42; with
 *                the 16 header bits, up to 7 bits of padding and the 32 of the trailer a stream of N bytes in B blocks takes
 *                at most (8 N + 42 B + 55) / 8 <= N + 6 B + 7 bytes: dspn_png_deflate_bound.
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

#define DSPN_PNG_DEFLATE_BLOCK 32768

/* bytes + 6 * blocks + 7 with blocks = bytes / DSPN_PNG_DEFLATE_BLOCK rounded up: the most a zlib stream of the rule above
 * takes for `bytes` input bytes (derived in the top comment).  Pure.  0 for bytes below 1. */
long long dspn_png_deflate_bound(long long bytes);

/* bytes of `workspace` for a batch of n streams of total_bytes bytes in all (the table of the batch, per image its size,
 * checksum and place, per block its 920-byte plan and its bit offset; at most total_bytes / DSPN_PNG_DEFLATE_BLOCK + n
 * blocks).  Pure.  0 for n below 1 or total_bytes below n. */
size_t dspn_png_deflate_workspace_bytes(int n, long long total_bytes);

/* in_offsets, in_sizes: n byte offsets into `in` and n sizes, HOST memory, read during the call; in: device byte pool of
 * in_bytes bytes (the filtered streams, for instance the `out` of dspn_png_filter_batch); out: device byte pool of out_bytes
 * bytes; result: 2 n 64-bit integers in DEVICE memory, 8-byte aligned; workspace: device memory, 8-byte aligned.  n == 0 is
 * a no-op.  Checked before any HIP call: a null pointer, n < 0, a pool size or a stream size below 1, a stream that runs
 * past in_bytes, out_bytes below the sum of dspn_png_deflate_bound over the streams, more than 2^56 bytes in all:
 * DSPN_ERR_ARG (-1); a short workspace: DSPN_ERR_WORKSPACE (-2).  Then one copy of the table into the workspace (the call
 * waits for it) and five launches on `stream`.  The zlib streams lie back to back from out[0] in the order of the batch;
 * result[2 i] is the offset of stream i in `out`, result[2 i + 1] its length.  Input and output have any alignment.  Nothing
 * outside the stated input spans is read; no byte of `out` beyond the last stream changes (the aligned dwords that hold the
 * first and the last byte written are updated by an atomic OR whose bits outside the streams are zero). */
int dspn_png_deflate_batch(const long long *in_offsets, const long long *in_sizes, int n, const unsigned char *in,
                           long long in_bytes, unsigned char *out, long long out_bytes, long long *result, void *workspace,
                           size_t workspace_bytes, void *stream);

/* the same encoder on the host over one stream in host memory: out receives the zlib stream (out_bytes at least
 * dspn_png_deflate_bound(bytes)), *length its size.  DSPN_ERR_ARG for a null pointer, bytes below 1 or a short out. */
int dspn_png_deflate_host(const unsigned char *data, long long bytes, unsigned char *out, long long out_bytes, long long *length);

/* the length-limited code lengths of the rule alone: counts[0 .. n) -> lengths[0 .. n), 0 for an unused symbol, otherwise
 * 1 .. limit.  Host, pure.  1 <= n <= 286, 1 <= limit <= 15, the counts sum to less than 2^32 and the used symbols number at
 * most 2^limit, else DSPN_ERR_ARG. */
int dspn_png_deflate_code_lengths(const unsigned *counts, int n, int limit, unsigned char *lengths);

#ifdef __cplusplus
}
#endif
#endif  /* DSPN_PNG_ENCODE_H_ */

/*
 * dspn_colour_jitter.h -- C ABI of the photometric augmentation of both iterators: the `ColorJitter` settings of
 * liangfu/dspnet's config/config.py (hue, saturation, illumination, contrast), applied in place to the decoded uint8 RGB
 * images of a whole batch in one launch, on the pool dspn_det_augment_batch_u8 and dspn_augment_batch_u8 read.
 *
 * The reference hands these settings to MXNet's C++ detection augmenter, whose text is not in the reference.  The
 * semantics here follow that augmenter's defaults as this project understands them: the image goes to 8-bit HLS (OpenCV's
 * ranges: H in units of 2 degrees, L and S in 0..255), three integers are added with clamping, it comes back, and a
 * contrast gain follows.  PARITY STATUS: unpinned (neither MXNet nor OpenCV is in this image to produce vectors).  The
 * per-pixel arithmetic is this build's own INTEGER definition of 8-bit HLS, so that the device and a restatement agree byte
 * for byte; against the real-valued model (Python's colorsys) the forward L and S are within 0.5 level and H within one
 * degree, the inverse within 0.5 level (tests/test_colour_jitter_host.py).
 *
 * All quantities are integers; `//` is floor division.  Per pixel (r, g, b), each 0..255, of an image with the parameters
 * (dh, dl, ds, gain):
 *
 * Forward
 *     mx = max(r, g, b), mn = min(r, g, b), d = mx - mn, sm = mx + mn
 *     L  = (sm + 1) >> 1
 *     S  = 0 if d == 0, else (510 * d + den) // (2 * den)        with den = sm if sm <= 255 else 510 - sm
 *     H  = 0 if d == 0, else
 *            (x, base) = (g - b, 0) if mx == r, else (b - r, 60) if mx == g, else (r - g, 120)     ties in that order
 *            N = 30 * x + base * d
 *            H = (2 * N + d) // (2 * d);  H += 180 if H < 0;  H -= 180 if H >= 180                  0..179, units of 2 degrees
 *   i.e. S = 255 d / den and H = N / d, each rounded half up.
 * Shift
 *     H' = clamp(H + dh, 0, 180)          clamped, NOT wrapped; 180 is a legal input of the inverse
 *     L' = clamp(L + dl, 0, 255)
 *     S' = clamp(S + ds, 0, 255)
 * Inverse
 *     S' == 0: every channel is L'.  Otherwise
 *     Q2 = L' * (255 + S') if 2 * L' <= 255, else 255 * (L' + S') - L' * S'
 *     Q1 = 510 * L' - Q2
 *     for the channels (r, g, b): t = (H' + off) mod 180 with off = +60, 0, -60
 *     W  = 30 * Q1 + (Q2 - Q1) * t             for t < 30
 *          30 * Q2                             for t < 90
 *          30 * Q1 + (Q2 - Q1) * (120 - t)     for t < 120
 *          30 * Q1                             for t >= 120
 *     out = (W + 3825) // 7650                 (W / 7650 rounded half up: Q1 and Q2 are in units of 1 / 255^2)
 * Contrast, after the above
 *     out = min(255, (v * gain + 512) >> 10)   gain in 1/1024ths; 1024 is the identity
 * Skips, as in MXNet's augmenter
 *     an image with dh == dl == ds == 0 does not take the HLS round trip (which is not the identity on 8 bits);
 *     an image with gain == 1024 is not scaled; an image with both is neither read nor written.
 *
 * Conventions as in dspn_png.h: caller-owned buffers, explicit stream, status return + dspn_last_error().
 */
#ifndef DSPN_COLOUR_JITTER_H_
#define DSPN_COLOUR_JITTER_H_

#ifdef __cplusplus
extern "C" {
#endif

/* one image of a batch: 32 bytes, little-endian, no padding */
typedef struct dspn_jitter_sample {
  long long img_offset;             /* byte offset in `pixels` of the dense (height, width, 3) RGB uint8 image */
  int height, width;
  int dh, dl, ds;                   /* added to H (units of 2 degrees), L and S; |dh| <= 180, |dl|, |ds| <= 255 */
  int gain;                         /* contrast in 1/1024ths, 0..65535 */
} dspn_jitter_sample;
#define DSPN_JITTER_SAMPLE_BYTES 32

/* pixels: device byte pool of pixel_bytes bytes, changed in place; samples: n descriptors in DEVICE memory (8-byte aligned).
 * One launch on `stream` for the whole batch; n == 0 is a no-op.  The descriptors are not trusted: every one is checked on
 * the device, by division before any product is formed, and is left alone like an identity one (nothing read, nothing
 * written) when its image would leave [0, pixel_bytes) -- a height or width below 1 included --, when |dh| > 180,
 * |dl| > 255 or |ds| > 255, or when gain < 0 or gain > 65535.  Image offsets may have any alignment; nothing outside an
 * image's height * width * 3 bytes is written, and nothing outside the pool is read.  Images that overlap each other are
 * the caller's affair: each byte of an overlap ends as one of the images' results. */
int dspn_colour_jitter_batch_u8(unsigned char *pixels, long long pixel_bytes, const dspn_jitter_sample *samples, int n,
                                void *stream);

#ifdef __cplusplus
}
#endif
#endif  /* DSPN_COLOUR_JITTER_H_ */

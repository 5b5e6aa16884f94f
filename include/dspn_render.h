/*
 * dspn_render.h -- C ABI of the display images of liangfu/dspnet: what `Detector.visualize_detection`
 * (detect/multitask_detector.py:336-399), `display_results` (multi_eval.py:36-104) and the result images of the
 * evaluation script (:344-368) paint, made on the device next to the tensors they are made from: class colours at
 * display size, the input image, boxes, tags and text.
 *
 * The reference paints with OpenCV (argmax + cv2.resize INTER_NEAREST + three cv2.LUT, cv2.rectangle, cv2.putText with
 * a Hershey font).  There is no OpenCV to compare against, so the arithmetic is stated here and is exact:
 *     nearest resize : index tables built by the caller, src = min(floor(dst * (1.0 / (Nd / float(Ns)))), Ns - 1) in
 *                      double (OpenCV's resizeNN); a scale of exactly 4 gives dst >> 2;
 *     class          : first maximum over channels 0 .. C-1 (strict >, numpy.argmax); channels C .. ld-1 never compared;
 *     image          : sat_u8(trunc(double(data) + mean)), truncation toward zero as ndarray.astype(uint8); values
 *                      outside 0..255, which numpy leaves undefined, saturate;
 *     outline / fill : integer pixel sets (below); thickness 1 is the inclusive perimeter of cv2.rectangle;
 *     text           : this build's own 5 x 7 font in a 6 x 8 cell, not Hershey: text metrics differ from the reference.
 * PARITY STATUS: unpinned where OpenCV would be the yardstick; the colour table is pinned (tests/golden).
 * Inputs are finite: a NaN score never wins a comparison, a NaN label or pixel has no defined colour.
 *
 * A canvas is (B, CH, CW, 3) uint8, RGB, contiguous.  Every entry writes into the panel of Hd x Wd pixels whose top-left
 * corner is (y0, x0), in every image of the batch, and nowhere else, so that panels are stacked without a copy.
 * Neither CW * 3 nor x0 * 3 need be a multiple of 4: a thread makes 4 neighbouring pixels and stores them as three
 * dwords where their address is 4-byte aligned; the unaligned ends of a panel row are stored as bytes.
 *
 * Conventions as in dspn_nms.h: device pointers, caller-owned buffers, explicit stream, status return +
 * dspn_last_error(); arguments are checked before any HIP call; nothing is allocated, nothing waits and there is no
 * workspace, so the calls can be recorded in a graph.  B == 0, Hd == 0 or Wd == 0 is an empty job: 0 is returned
 * without a HIP call (the other arguments are checked all the same).  Every tensor stays below 2^31 elements;
 * B <= 65535 and Hd <= 262140 (grid limits).
 */
#ifndef DSPN_RENDER_H_
#define DSPN_RENDER_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* rows of one image are staged in LDS this many at a time (dspn_render_draw_list_u8) */
#define DSPN_RENDER_CHUNK_ROWS 128
/* font table: 7 bytes per glyph for the codes 32 .. 126, one byte per glyph row from the top, bit 4 the leftmost column */
#define DSPN_RENDER_FONT_FIRST 32
#define DSPN_RENDER_FONT_LAST 126
#define DSPN_RENDER_FONT_BYTES 665

#define DSPN_DRAW_OUTLINE 0
#define DSPN_DRAW_FILL 1
#define DSPN_DRAW_GLYPH 2

/* One draw row; coordinates are pixels of the panel, (0, 0) its top-left corner; r, g, b in 0..255.
 *   kind 0, outline: corners normalised with min / max; thickness t = arg >= 1; the pixels inside
 *        [x0 - t/2, x1 + t/2] x [y0 - t/2, y1 + t/2] and not inside
 *        [x0 + (t+1)/2, x1 - (t+1)/2] x [y0 + (t+1)/2, y1 - (t+1)/2], integer division;
 *   kind 1, filled rectangle: inclusive corners, normalised;
 *   kind 2, glyph: character code arg & 0xff, integer scale arg >> 8 >= 1, top-left corner (x0, y0); x1, y1 unused.
 *        Only the set bits of the 5 x 7 pattern are painted, each as a scale x scale square; a code outside 32..126
 *        paints the full 5 x 7 block.
 * Everything is clipped to the panel; a row wholly outside paints nothing.  A row the kernel cannot read as one of
 * these (unknown kind, t < 1, scale < 1) paints nothing. */
typedef struct dspn_draw_row {
  int kind;
  int x0, y0, x1, y1;
  int r, g, b;
  int arg;
} dspn_draw_row;

/* DSPN_RENDER_CHUNK_ROWS, for callers that cannot read the macro */
int dspn_render_chunk_rows(void);

/* scores: (B, h, w, ld >= C) float32 class scores, NHWC.  palette: 256 x 3 device bytes, RGB.  ysrc: Hd int32,
 * xsrc: Wd int32, source row / column of every panel row / column (an entry outside the source is clamped into it).
 * panel[b, y, x] = palette[argmax_c scores[b, ysrc[y], xsrc[x], 0..C-1]], 1 <= C <= 256. */
int dspn_render_classmap_f32(const float *scores_dev, int B, int h, int w, int C, int ld,
                             const unsigned char *palette_dev, const int *ysrc_dev, const int *xsrc_dev, int Hd, int Wd,
                             unsigned char *canvas_dev, int CH, int CW, int y0, int x0, void *stream);

/* labels: (B, h, w) float32 holding integers 0..255 (the graph's label_seg: 0..18 and 255); the value truncated to
 * uint8 is the palette index.  Otherwise as dspn_render_classmap_f32. */
int dspn_render_labels_f32(const float *labels_dev, int B, int h, int w, const unsigned char *palette_dev,
                           const int *ysrc_dev, const int *xsrc_dev, int Hd, int Wd, unsigned char *canvas_dev, int CH,
                           int CW, int y0, int x0, void *stream);

/* data: (B, 3, H, W) float32 planes, the net's input; the panel is H x W.
 * panel[b, y, x, c] = sat_u8(trunc(double(data[b, channel_map[c], y, x]) + mean[c])); channel_map and mean are host
 * arrays, channel_map[c] in 0..2. */
int dspn_render_data_f32(const float *data_dev, int B, int H, int W, const int channel_map[3], const double mean[3],
                         unsigned char *canvas_dev, int CH, int CW, int y0, int x0, void *stream);

/* A HOST table, before it is uploaded: kind in 0..2, thickness >= 1, glyph scale >= 1, colours in 0..255, coordinates
 * within +-2^24, and row_start[0] == 0 <= ... <= row_start[B] == R.  No HIP call. */
int dspn_render_check_draw_rows(const dspn_draw_row *rows_host, int R, const int *row_start_host, int B);

/* rows: R draw rows in device memory; row_start: B + 1 device int32, image b owns rows row_start[b] ..
 * row_start[b+1] - 1 (a range that leaves [0, R] paints nothing); font: DSPN_RENDER_FONT_BYTES device bytes.
 * PAINTER'S ORDER: where rows of an image overlap, the pixel holds the colour of the last covering row in table order.
 * A workgroup owns a tile of one image's panel, stages that image's rows in LDS DSPN_RENDER_CHUNK_ROWS at a time, and
 * every thread walks them in order for its own 4 pixels, keeps the colour in registers and stores once, and only the
 * pixels some row touched: one launch, no atomics, no two threads write one byte, nothing depends on the grid.
 * R == 0 is an empty job as well. */
int dspn_render_draw_list_u8(unsigned char *canvas_dev, int B, int CH, int CW, int y0, int x0, int Hd, int Wd,
                             const dspn_draw_row *rows_dev, int R, const int *row_start_dev,
                             const unsigned char *font_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif  /* DSPN_RENDER_H_ */

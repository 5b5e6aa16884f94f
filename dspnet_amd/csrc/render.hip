// Display images for MI355X (gfx950); C ABI and the exact arithmetic in include/dspn_render.h.
//
// All four kernels are byte streams bounded by the bytes they write, 3 per pixel.  A workgroup is 64 x 4 threads: 4 panel
// rows, and along a row every thread makes 4 neighbouring pixels = 12 bytes.  Neither the canvas row pitch (CW * 3) nor the
// panel's first byte (x0 * 3) need be a multiple of 4, so the groups of a row are laid out from that row's own address:
// with `lead` = (address of the row's first byte) & 3, pixel `lead` is the first one whose byte address is a multiple of 4
// (3 * x + a = 0 mod 4  <=>  x = a mod 4), and so is every fourth pixel after it.  Group g covers pixels
// [lead - 4 + 4g, lead + 4g): group 0 is the unaligned head (0..3 pixels), the last one the tail; both go out as bytes,
// every whole group as three aligned dwords.  A wave's lanes then write 64 * 12 contiguous bytes.
//
// render_map_kernel: class scores (argmax over the channels) or a label map, through the nearest-resize index tables
// and the palette, which sits in LDS as packed colours.  A thread reuses the colour of the previous pixel while the source
// column stays the same (an upscale by 4 reads one source pixel per group).
// render_draw_kernel: the draw list in painter's order; see the header.  A wave is one tile row, so the test of a row's
// extent against y is wave-uniform.
#include "dspn_common.h"
#include "../../include/dspn_render.h"

namespace {

constexpr int kLanesX = 64, kRowsY = 4, kThreads = kLanesX * kRowsY, kGroup = 4;
constexpr int kRowInts = sizeof(dspn_draw_row) / sizeof(int);
static_assert(sizeof(dspn_draw_row) == 9 * sizeof(int), "dspn_draw_row is nine int32");

typedef unsigned char u8;

// first byte of panel row y of image b
__device__ __forceinline__ u8 *panel_row(u8 *canvas, int b, int CH, int CW, int y0, int x0, int y) {
  return canvas + (((size_t)b * CH + y0 + y) * CW + x0) * 3;
}

// the first pixel of this thread's group in a row that starts at `row`
__device__ __forceinline__ int group_start(const u8 *row) {
  const int lead = (int)(reinterpret_cast<size_t>(row) & 3);
  return lead - kGroup + kGroup * (int)(blockIdx.x * kLanesX + threadIdx.x);
}

// c[k] = r | g << 8 | b << 16 of pixel xs + k; bit k of mask: store it.  A whole group inside the row starts on a dword.
__device__ __forceinline__ void store_group(u8 *row, int xs, int Wd, const unsigned (&c)[kGroup], unsigned mask) {
  if (xs >= 0 && xs + kGroup <= Wd && mask == 0xfu) {
    unsigned *p = reinterpret_cast<unsigned *>(row + (size_t)xs * 3);
    p[0] = c[0] | (c[1] << 24);
    p[1] = (c[1] >> 8) | (c[2] << 16);
    p[2] = (c[2] >> 16) | (c[3] << 8);
    return;
  }
#pragma unroll
  for (int k = 0; k < kGroup; ++k) {
    const int x = xs + k;
    if (x >= 0 && x < Wd && ((mask >> k) & 1u)) {
      u8 *p = row + (size_t)x * 3;
      p[0] = (u8)c[k]; p[1] = (u8)(c[k] >> 8); p[2] = (u8)(c[k] >> 16);
    }
  }
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <bool LABELS>
__global__ __launch_bounds__(kThreads) void render_map_kernel(const float *__restrict__ src, int h, int w, int C, int ld,
                                                              int vec, const u8 *__restrict__ palette,
                                                              const int *__restrict__ ysrc, const int *__restrict__ xsrc,
                                                              int Hd, int Wd, u8 *__restrict__ canvas, int CH, int CW, int y0,
                                                              int x0) {
  __shared__ unsigned pal[256];
  const int tid = threadIdx.y * kLanesX + threadIdx.x;
  pal[tid] = palette[tid * 3] | (palette[tid * 3 + 1] << 8) | (palette[tid * 3 + 2] << 16);
  __syncthreads();
  const int y = blockIdx.y * kRowsY + threadIdx.y, b = blockIdx.z;
  if (y >= Hd) return;
  u8 *row = panel_row(canvas, b, CH, CW, y0, x0, y);
  const int xs = group_start(row);
  if (xs >= Wd) return;
  const int sy = clampi(ysrc[y], 0, h - 1);
  const float *srow = src + ((size_t)b * h + sy) * w * (LABELS ? 1 : ld);
  unsigned c[kGroup] = {0u, 0u, 0u, 0u}, colour = 0u;
  int prev = -1;
#pragma unroll
  for (int k = 0; k < kGroup; ++k) {
    const int x = xs + k;
    if (x < 0 || x >= Wd) continue;
    const int sx = clampi(xsrc[x], 0, w - 1);
    if (sx != prev) {
      prev = sx;
      int idx = 0;
      if (LABELS) {
        idx = (int)srow[sx] & 255;
      } else {
        const float *p = srow + (size_t)sx * ld;
        float best = p[0];
        if (vec) {                                              // 16-byte loads; the lanes past C are loaded, never compared
          for (int c0 = 0; c0 < C; c0 += 4) {
            const float4 v = *reinterpret_cast<const float4 *>(p + c0);
            if (c0 > 0 && v.x > best) { best = v.x; idx = c0; }
            if (c0 + 1 < C && v.y > best) { best = v.y; idx = c0 + 1; }
            if (c0 + 2 < C && v.z > best) { best = v.z; idx = c0 + 2; }
            if (c0 + 3 < C && v.w > best) { best = v.w; idx = c0 + 3; }
          }
        } else {
          for (int ch = 1; ch < C; ++ch) {
            const float v = p[ch];
            if (v > best) { best = v; idx = ch; }
          }
        }
      }
      colour = pal[idx];
    }
    c[k] = colour;
  }
  store_group(row, xs, Wd, c, 0xfu);
}

struct DataArgs { int cmap[3]; double mean[3]; };

__global__ __launch_bounds__(kThreads) void render_data_kernel(const float *__restrict__ data, int H, int W, DataArgs a,
                                                               u8 *__restrict__ canvas, int CH, int CW, int y0, int x0) {
  const int y = blockIdx.y * kRowsY + threadIdx.y, b = blockIdx.z;
  if (y >= H) return;
  u8 *row = panel_row(canvas, b, CH, CW, y0, x0, y);
  const int xs = group_start(row);
  if (xs >= W) return;
  const size_t plane = (size_t)H * W;
  const float *img = data + (size_t)b * 3 * plane + (size_t)y * W;
  unsigned c[kGroup] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int k = 0; k < kGroup; ++k) {
    const int x = xs + k;
    if (x < 0 || x >= W) continue;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const double v = (double)img[a.cmap[ch] * plane + x] + a.mean[ch];
      const unsigned u = v <= 0.0 ? 0u : (v >= 255.0 ? 255u : (unsigned)(int)v);   // toward zero, then saturated
      c[k] |= u << (8 * ch);
    }
  }
  store_group(row, xs, W, c, 0xfu);
}

__global__ __launch_bounds__(kThreads) void render_draw_kernel(u8 *__restrict__ canvas, int CH, int CW, int y0, int x0, int Hd,
                                                               int Wd, const dspn_draw_row *__restrict__ rows, int R,
                                                               const int *__restrict__ row_start,
                                                               const u8 *__restrict__ font) {
  __shared__ int stage[DSPN_RENDER_CHUNK_ROWS * kRowInts];
  __shared__ u8 glyphs[DSPN_RENDER_FONT_BYTES];
  const int tid = threadIdx.y * kLanesX + threadIdx.x, b = blockIdx.z;
  const int rs = row_start[b], re = row_start[b + 1];
  if (rs < 0 || re > R || rs >= re) return;                   // the same for the whole workgroup
  for (int i = tid; i < DSPN_RENDER_FONT_BYTES; i += kThreads) glyphs[i] = font[i];
  const int y = blockIdx.y * kRowsY + threadIdx.y;
  bool live = y < Hd;
  u8 *row = nullptr;
  int xs = 0;
  if (live) {
    row = panel_row(canvas, b, CH, CW, y0, x0, y);
    xs = group_start(row);
    live = xs < Wd;
  }
  unsigned c[kGroup] = {0u, 0u, 0u, 0u}, mask = 0u;
  for (int base = rs; base < re; base += DSPN_RENDER_CHUNK_ROWS) {
    const int n = re - base < DSPN_RENDER_CHUNK_ROWS ? re - base : DSPN_RENDER_CHUNK_ROWS;
    __syncthreads();                                           // the previous chunk has been walked
    const int *g = reinterpret_cast<const int *>(rows + base);
    for (int i = tid; i < n * kRowInts; i += kThreads) stage[i] = g[i];
    __syncthreads();
    if (!live) continue;
    for (int j = 0; j < n; ++j) {                              // table order: a later row overwrites an earlier one
      const int *r = stage + j * kRowInts;                    // one address for the wave: a broadcast read
      const int kind = r[0], ax = r[1], ay = r[2], bx = r[3], by = r[4], arg = r[8];
      unsigned hit = 0u;
      if (kind == DSPN_DRAW_OUTLINE || kind == DSPN_DRAW_FILL) {
        const int xa = ax < bx ? ax : bx, xb = ax < bx ? bx : ax, ya = ay < by ? ay : by, yb = ay < by ? by : ay;
        if (kind == DSPN_DRAW_FILL) {
          if (y >= ya && y <= yb) {
#pragma unroll
            for (int k = 0; k < kGroup; ++k)
              if (xs + k >= xa && xs + k <= xb) hit |= 1u << k;
          }
        } else if (arg >= 1) {
          const int o = arg / 2, in = (arg + 1) / 2;
          if (y >= ya - o && y <= yb + o) {
            const bool y_inner = y >= ya + in && y <= yb - in;
#pragma unroll
            for (int k = 0; k < kGroup; ++k) {
              const int x = xs + k;
              if (x >= xa - o && x <= xb + o && !(y_inner && x >= xa + in && x <= xb - in)) hit |= 1u << k;
            }
          }
        }
      } else if (kind == DSPN_DRAW_GLYPH) {
        const int s = arg >> 8, code = arg & 0xff, dy = y - ay;
        if (s >= 1 && dy >= 0 && dy < 7 * s) {
          const unsigned bits = code >= DSPN_RENDER_FONT_FIRST && code <= DSPN_RENDER_FONT_LAST
                                    ? glyphs[(code - DSPN_RENDER_FONT_FIRST) * 7 + dy / s] : 0x1fu;
#pragma unroll
          for (int k = 0; k < kGroup; ++k) {
            const int dx = xs + k - ax;
            if (dx >= 0 && dx < 5 * s && ((bits >> (4 - dx / s)) & 1u)) hit |= 1u << k;
          }
        }
      }
      if (hit) {
        const unsigned col = (unsigned)(r[5] & 255) | ((unsigned)(r[6] & 255) << 8) | ((unsigned)(r[7] & 255) << 16);
#pragma unroll
        for (int k = 0; k < kGroup; ++k)
          if ((hit >> k) & 1u) c[k] = col;
        mask |= hit;
      }
    }
  }
  if (live && mask) store_group(row, xs, Wd, c, mask);
}

// the checks every entry shares; the job is B images of an Hd x Wd panel at (y0, x0) of a (B, CH, CW, 3) canvas
int check_panel(const char *what, int B, int CH, int CW, int y0, int x0, int Hd, int Wd) {
  DSPN_REQUIRE(B >= 0 && Hd >= 0 && Wd >= 0, "%s: negative size", what);
  DSPN_REQUIRE(CH > 0 && CW > 0, "%s: the canvas height and width must be > 0", what);
  DSPN_REQUIRE(y0 >= 0 && x0 >= 0 && (long long)y0 + Hd <= CH && (long long)x0 + Wd <= CW,
               "%s: the panel (%d x %d at row %d, column %d) leaves the canvas (%d x %d)", what, Hd, Wd, y0, x0, CH, CW);
  DSPN_REQUIRE((long long)CH * CW < (1LL << 31) && (long long)CH * CW * 3 * (B > 0 ? B : 1) < (1LL << 31),
               "%s: the canvas must stay below 2^31 bytes", what);
  DSPN_REQUIRE(B <= 65535 && Hd <= 65535 * kRowsY, "%s: at most 65535 images and %d panel rows", what, 65535 * kRowsY);
  return 0;
}

dim3 panel_grid(int B, int Hd, int Wd) {
  const int groups = 1 + (Wd + kGroup - 1) / kGroup;           // the unaligned head and every group of 4 after it
  return dim3((groups + kLanesX - 1) / kLanesX, (Hd + kRowsY - 1) / kRowsY, B);
}

template <bool LABELS>
int render_map(const char *what, const float *src, int B, int h, int w, int C, int ld, const u8 *palette, const int *ysrc,
               const int *xsrc, int Hd, int Wd, u8 *canvas, int CH, int CW, int y0, int x0, void *stream) {
  if (int rc = check_panel(what, B, CH, CW, y0, x0, Hd, Wd)) return rc;
  DSPN_REQUIRE(h > 0 && w > 0, "%s: the source height and width must be > 0", what);
  DSPN_REQUIRE(C >= 1 && C <= 256, "%s: C must be in 1..256", what);
  DSPN_REQUIRE(ld >= C, "%s: C > ld", what);
  DSPN_REQUIRE((long long)h * w < (1LL << 31) && (long long)h * w * ld < (1LL << 31) &&
                   (long long)h * w * ld * (B > 0 ? B : 1) < (1LL << 31), "%s: the source must stay below 2^31 elements", what);
  if (B == 0 || Hd == 0 || Wd == 0) return 0;
  DSPN_REQUIRE(src && palette && ysrc && xsrc && canvas, "%s: null pointer", what);
  const int vec = !LABELS && ld % 4 == 0 && reinterpret_cast<size_t>(src) % 16 == 0;
  hipLaunchKernelGGL(render_map_kernel<LABELS>, panel_grid(B, Hd, Wd), dim3(kLanesX, kRowsY), 0, (hipStream_t)stream, src, h, w,
                     C, ld, vec, palette, ysrc, xsrc, Hd, Wd, canvas, CH, CW, y0, x0);
  return dspn::check_launch(what);
}

}  // namespace

extern "C" {

int dspn_render_chunk_rows(void) { return DSPN_RENDER_CHUNK_ROWS; }

int dspn_render_classmap_f32(const float *scores_dev, int B, int h, int w, int C, int ld, const unsigned char *palette_dev,
                             const int *ysrc_dev, const int *xsrc_dev, int Hd, int Wd, unsigned char *canvas_dev, int CH,
                             int CW, int y0, int x0, void *stream) {
  return render_map<false>("render_classmap", scores_dev, B, h, w, C, ld, palette_dev, ysrc_dev, xsrc_dev, Hd, Wd, canvas_dev,
                           CH, CW, y0, x0, stream);
}

int dspn_render_labels_f32(const float *labels_dev, int B, int h, int w, const unsigned char *palette_dev, const int *ysrc_dev,
                           const int *xsrc_dev, int Hd, int Wd, unsigned char *canvas_dev, int CH, int CW, int y0, int x0,
                           void *stream) {
  return render_map<true>("render_labels", labels_dev, B, h, w, 1, 1, palette_dev, ysrc_dev, xsrc_dev, Hd, Wd, canvas_dev, CH,
                          CW, y0, x0, stream);
}

int dspn_render_data_f32(const float *data_dev, int B, int H, int W, const int channel_map[3], const double mean[3],
                         unsigned char *canvas_dev, int CH, int CW, int y0, int x0, void *stream) {
  const char *what = "render_data";
  if (int rc = check_panel(what, B, CH, CW, y0, x0, H, W)) return rc;
  DSPN_REQUIRE((long long)H * W * 3 * (B > 0 ? B : 1) < (1LL << 31), "%s: the planes must stay below 2^31 elements", what);
  DSPN_REQUIRE(channel_map && mean, "%s: null channel_map or mean", what);
  DataArgs a;
  for (int c = 0; c < 3; ++c) {
    DSPN_REQUIRE(channel_map[c] >= 0 && channel_map[c] < 3, "%s: channel_map[%d] = %d is not a plane", what, c, channel_map[c]);
    DSPN_REQUIRE(mean[c] == mean[c], "%s: mean[%d] is not a number", what, c);
    a.cmap[c] = channel_map[c];
    a.mean[c] = mean[c];
  }
  if (B == 0 || H == 0 || W == 0) return 0;
  DSPN_REQUIRE(data_dev && canvas_dev, "%s: null pointer", what);
  hipLaunchKernelGGL(render_data_kernel, panel_grid(B, H, W), dim3(kLanesX, kRowsY), 0, (hipStream_t)stream, data_dev, H, W, a,
                     canvas_dev, CH, CW, y0, x0);
  return dspn::check_launch(what);
}

int dspn_render_check_draw_rows(const dspn_draw_row *rows_host, int R, const int *row_start_host, int B) {
  const char *what = "render_check_draw_rows";
  DSPN_REQUIRE(R >= 0 && B >= 0, "%s: negative count", what);
  DSPN_REQUIRE(row_start_host && (R == 0 || rows_host), "%s: null pointer", what);
  DSPN_REQUIRE(row_start_host[0] == 0 && row_start_host[B] == R, "%s: row_start must run from 0 to R = %d", what, R);
  for (int b = 0; b < B; ++b)
    DSPN_REQUIRE(row_start_host[b] <= row_start_host[b + 1], "%s: row_start decreases at image %d", what, b);
  const int lim = 1 << 24;
  for (int i = 0; i < R; ++i) {
    const dspn_draw_row &r = rows_host[i];
    DSPN_REQUIRE(r.kind >= DSPN_DRAW_OUTLINE && r.kind <= DSPN_DRAW_GLYPH, "%s: row %d: kind %d", what, i, r.kind);
    DSPN_REQUIRE(r.x0 >= -lim && r.x0 <= lim && r.y0 >= -lim && r.y0 <= lim && r.x1 >= -lim && r.x1 <= lim && r.y1 >= -lim &&
                     r.y1 <= lim, "%s: row %d: a coordinate beyond +-2^24", what, i);
    DSPN_REQUIRE(r.r >= 0 && r.r <= 255 && r.g >= 0 && r.g <= 255 && r.b >= 0 && r.b <= 255, "%s: row %d: colour outside 0..255",
                 what, i);
    if (r.kind == DSPN_DRAW_OUTLINE) DSPN_REQUIRE(r.arg >= 1 && r.arg <= lim, "%s: row %d: thickness t < 1 (or beyond 2^24)", what, i);
    if (r.kind == DSPN_DRAW_GLYPH) DSPN_REQUIRE((r.arg >> 8) >= 1 && (r.arg >> 8) <= 4096, "%s: row %d: glyph scale < 1 (or > 4096)", what, i);
  }
  return 0;
}

int dspn_render_draw_list_u8(unsigned char *canvas_dev, int B, int CH, int CW, int y0, int x0, int Hd, int Wd,
                             const dspn_draw_row *rows_dev, int R, const int *row_start_dev, const unsigned char *font_dev,
                             void *stream) {
  const char *what = "render_draw_list";
  if (int rc = check_panel(what, B, CH, CW, y0, x0, Hd, Wd)) return rc;
  DSPN_REQUIRE(R >= 0, "%s: R < 0", what);
  DSPN_REQUIRE((long long)R * kRowInts < (1LL << 31), "%s: the row table must stay below 2^31 elements", what);
  if (B == 0 || Hd == 0 || Wd == 0 || R == 0) return 0;
  DSPN_REQUIRE(canvas_dev && rows_dev && row_start_dev && font_dev, "%s: null pointer", what);
  hipLaunchKernelGGL(render_draw_kernel, panel_grid(B, Hd, Wd), dim3(kLanesX, kRowsY), 0, (hipStream_t)stream, canvas_dev, CH,
                     CW, y0, x0, Hd, Wd, rows_dev, R, row_start_dev, font_dev);
  return dspn::check_launch(what);
}

}  // extern "C"

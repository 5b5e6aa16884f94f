// Filter reconstruction of inflated PNG rows for MI355X (gfx950); C ABI and the arithmetic in include/dspn_png.h.  The host
// half (chunk walk, inflate) is dspnet_amd/dataset/png.py.
//
// Dependencies: a reconstructed byte needs the reconstructed bytes to its left (bytes_per_pixel back), above and above-left.
// So anti-diagonals are independent: one workgroup per image, one lane per row, and lane r runs one DWORD behind lane r - 1.
// A step of the loop reconstructs 4 bytes of a row in every lane (serially inside the lane: the left neighbour of a byte is the
// byte just made), all five filter types in the same instructions (every predictor is formed, the row's type selects one).  A
// band of `rows` rows of row_dwords dwords takes row_dwords + rows - 1 steps; images taller than kRows rows are done in bands,
// in order, by the same workgroup.
//   row above   : the 4 bytes above come from the previous lane's last output by __shfl_up; the 4 above-left are the ones
//                 received a step earlier.  Lane 0 of a wave takes them from LDS (two slots per wave, alternated, so the
//                 loop's one __syncthreads() orders write and read); row 0 of a later band reads the previous band's last
//                 row back from the output (after a device-scope fence and a barrier).
//   memory      : per lane one aligned dword load (queued three steps ahead, the row's own alignment taken out with a
//                 funnel shift) and one dword store per step (bytes where the address or the row's end does not allow it).
//                 A word that is not wholly inside its pool is put together from the bytes that are.
// What bounds it: vector instruction issue inside one CU along a long chain (1.19 us per step measured at
// 1024 x 2048).  The loop is row_dwords + rows - 1 steps of 4 dependent byte reconstructions plus a barrier, a lane is inside
// its row for row_dwords of them, and an image occupies one CU; a batch of B images uses B CUs.  Rows of type 0 or 1 cut the
// chain (they do not read the row above) and would allow more workgroups per image; this kernel does not use that.
// No workgroup waits for another one: the only waits are the barriers of one workgroup, with trip counts taken from the
// descriptor alone (the same in every thread).
//
// Colour images (dspn_png_rgb_batch) run the same body at the format's filter stride -- 1, 2, 3, 4, 6 or 8 bytes, the row length
// given in bytes, so packed 1-, 2- and 4-bit rows reconstruct as bytes -- and a second launch turns the reconstructed samples
// into packed RGB (a grid over the pixels of every image, four pixels = three dwords per thread).  At strides 6 and 8 the left
// neighbour lies one or two dwords back, so a lane keeps its last two output dwords and the last three of the row above.
// RGB 8-bit rows are their own output and skip the second launch.  Measured at 2048 x 1024, 16 images: 1.49 us per step at
// stride 3 (2559 steps, 3.81 ms), 1.92 at 4, 2.14 at 6, 2.15 at 8 (5119 steps, 11.0 ms); the second launch takes 0.10 to
// 0.18 ms (profiles/png_rgb_device_decode.txt).
#include <cstdint>

#include "dspn_common.h"
#include "../../include/dspn_png.h"

static_assert(sizeof(dspn_png_sample) == DSPN_PNG_SAMPLE_BYTES, "descriptor layout");

namespace {

constexpr int kRows = 1024;                // rows of a band = threads of the workgroup
constexpr int kWaves = kRows / 64;

struct Pools { long long raw_bytes, out_bytes; };

// true when every address the kernel derives from `s` stays inside raw (raw_bytes) and out (out_bytes)
__device__ bool sample_ok(const dspn_png_sample &s, const Pools &pl) {
  if (s.skip) return false;
  if (s.width < 1 || s.height < 1) return false;
  if (s.bytes_per_pixel != 1 && s.bytes_per_pixel != 2) return false;
  const long long rb = (long long)s.width * s.bytes_per_pixel;                      // < 2^32
  if (s.height > pl.raw_bytes / (rb + 1) || s.height > pl.out_bytes / rb) return false;   // so the products below fit the pools
  if (s.raw_offset < 0 || s.raw_offset > pl.raw_bytes - s.height * (rb + 1)) return false;
  if (s.out_offset < 0 || s.out_offset > pl.out_bytes - s.height * rb) return false;
  return true;
}

// The bytes [at, at + len) of the pool [lo, hi) as successive dwords (little-endian, the first one starting AT `at`), read as
// aligned words three takes ahead.  Only words that hold a wanted byte are fetched, and of those only bytes inside the pool.
struct Words {
  const unsigned char *lo = nullptr, *hi = nullptr;
  uintptr_t next = 0, end = 0;             // the next aligned word to fetch; the first byte not wanted
  unsigned sh = 0;                         // 8 * (at & 3)
  unsigned w0 = 0, w1 = 0, w2 = 0, w3 = 0;

  __device__ __forceinline__ unsigned fetch() {
    const uintptr_t p = next;
    next += 4;
    if (p >= end) return 0;
    const unsigned char *q = reinterpret_cast<const unsigned char *>(p);
    if (q >= lo && q + 4 <= hi) return *reinterpret_cast<const unsigned *>(q);
    unsigned v = 0;
    for (int k = 0; k < 4; ++k)
      if (q + k >= lo && q + k < hi) v |= (unsigned)q[k] << (8 * k);
    return v;
  }
  __device__ __forceinline__ void open(const unsigned char *pool, long long pool_bytes, const unsigned char *at, long long len) {
    lo = pool; hi = pool + pool_bytes;
    const uintptr_t a = reinterpret_cast<uintptr_t>(at);
    next = a & ~(uintptr_t)3; end = a + (uintptr_t)len; sh = 8 * (unsigned)(a & 3);
    w0 = fetch(); w1 = fetch(); w2 = fetch(); w3 = fetch();
  }
  __device__ __forceinline__ unsigned take() {
    const unsigned v = (unsigned)((((unsigned long long)w1 << 32) | w0) >> sh);
    w0 = w1; w1 = w2; w2 = w3; w3 = fetch();
    return v;
  }
};

__device__ __forceinline__ unsigned swap_pairs(unsigned v) { return ((v & 0x00ff00ffu) << 8) | ((v >> 8) & 0x00ff00ffu); }
__device__ __forceinline__ int iabs(int v) { return v < 0 ? -v : v; }

// four bytes of a row: x the filtered dword, left / left2 the row's previous output dword and the one before it, up the
// output dword above, upprev / upprev2 the two before that one (all in stream order: PNG's byte order).  The byte BPP back
// lies in the dword being made (BPP < 4 only), one dword back, or (BPP 6 and 8) two dwords back; which, is known per byte at
// compile time, so the strides that do not reach that far never touch left2 / upprev2.
template <int BPP>
__device__ __forceinline__ unsigned reconstruct4(unsigned ft, unsigned x, unsigned left2, unsigned left, unsigned up, unsigned upprev,
                                                 unsigned upprev2) {
  static_assert(BPP >= 1 && BPP <= 8, "the left neighbour lies at most two dwords back");
  unsigned cur = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int p = 8 + k - BPP;                                     // position in the 12 bytes (two dwords back, one back, this one)
    const unsigned aw = p < 4 ? left2 : p < 8 ? left : cur;
    const unsigned cw = p < 4 ? upprev2 : p < 8 ? upprev : up;
    const int a = (int)(aw >> (8 * (p & 3))) & 255;
    const int b = (int)(up >> (8 * k)) & 255;
    const int c = (int)(cw >> (8 * (p & 3))) & 255;
    const int pa = iabs(b - c), pb = iabs(a - c), pc = iabs(a + b - 2 * c);
    const int paeth = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
    const int pred = ft == 1 ? a : ft == 2 ? b : ft == 3 ? (a + b) >> 1 : ft == 4 ? paeth : 0;
    const unsigned v = ((x >> (8 * k)) + (unsigned)pred) & 255u;
    cur |= v << (8 * k);
  }
  return cur;
}

// the rows of one image: height rows of rb bytes, each behind its filter byte in `raw`, compact in `out`
struct Rows { long long raw_offset, out_offset, height, rb; };

// BPP: the filter stride in bytes; SWAP: the output is byte pairs stored swapped (16-bit greyscale as native uint16)
template <int BPP, bool SWAP>
__device__ void unfilter_image(const unsigned char *raw, unsigned char *out, const Rows &s, const Pools &pl, unsigned (*xch)[kWaves]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long rb = s.rb;
  const long long rd = (rb + 3) >> 2;                              // dwords of a row, the last one perhaps partial
  for (long long r0 = 0; r0 < s.height; r0 += kRows) {
    if (r0 > 0) {                                                  // the previous band's last row is read back below
      __threadfence();
      __syncthreads();
      __threadfence();
    }
    const long long row = r0 + tid;
    const bool live = row < s.height;
    const long long rows = s.height - r0 < kRows ? s.height - r0 : kRows;
    const long long steps = rd + rows - 1;                         // the same in every thread
    const bool from_out = tid == 0 && r0 > 0;
    Words in, prev_row;
    unsigned ft = 0;
    if (live) {
      const unsigned char *p = raw + s.raw_offset + row * (rb + 1);
      ft = p[0];
      in.open(raw, pl.raw_bytes, p + 1, rb);
    }
    if (from_out) prev_row.open(out, pl.out_bytes, out + s.out_offset + (r0 - 1) * rb, rb);
    unsigned char *dst = out + s.out_offset + (live ? row : 0) * rb;
    unsigned left = 0, left2 = 0, upprev = 0, upprev2 = 0, last = 0;
    for (long long t = 0; t < steps; ++t) {
      unsigned up = __shfl_up(last, 1);                            // lane r - 1 made dword t - r of its row in step t - 1
      if (lane == 0 && tid > 0) up = xch[(t + 1) & 1][wave - 1];   // ... written in step t - 1
      const long long j = t - tid;
      if (live && j >= 0 && j < rd) {
        if (tid == 0) {
          up = 0;
          if (from_out) { up = prev_row.take(); if (SWAP) up = swap_pairs(up); }
        }
        const unsigned cur = reconstruct4<BPP>(ft, in.take(), left2, left, up, upprev, upprev2);
        upprev2 = upprev; upprev = up; left2 = left; left = cur; last = cur;
        const long long o = 4 * j;
        const unsigned v = SWAP ? swap_pairs(cur) : cur;
        unsigned char *q = dst + o;
        if (rb - o >= 4 && (reinterpret_cast<uintptr_t>(q) & 3) == 0) {
          *reinterpret_cast<unsigned *>(q) = v;
        } else {
          const int nb = rb - o < 4 ? (int)(rb - o) : 4;
          for (int k = 0; k < nb; ++k) q[k] = (unsigned char)(v >> (8 * k));
        }
      }
      if (lane == 63) xch[t & 1][wave] = last;
      __syncthreads();
    }
  }
}

__global__ __launch_bounds__(kRows) void png_unfilter_kernel(const unsigned char *raw, const dspn_png_sample *__restrict__ samples,
                                                             Pools pl, unsigned char *out) {
  __shared__ unsigned xch[2][kWaves];
  const dspn_png_sample s = samples[blockIdx.x];
  if (!sample_ok(s, pl)) return;                                   // the whole workgroup, before any barrier
  const Rows r = {s.raw_offset, s.out_offset, s.height, (long long)s.width * s.bytes_per_pixel};
  if (s.bytes_per_pixel == 1) unfilter_image<1, false>(raw, out, r, pl, xch);
  else unfilter_image<2, true>(raw, out, r, pl, xch);
}

// ---- colour images to packed RGB (dspn_png_rgb_batch) --------------------------------------------------------------------
struct RgbPools { long long raw_bytes, out_bytes, ws_bytes; int n_palettes; };

// what (bit_depth, colour_type) and the width say about an image's rows
struct RgbGeom {
  long long rb;                            // bytes of a row
  int bpp;                                 // filter stride: 1, 2, 3, 4, 6 or 8
  int px, step;                            // depth >= 8: bytes of a pixel, and from one colour sample to the next (0: grey)
  bool direct;                             // RGB 8-bit: the reconstructed rows are the output
};

// false for sizes below 1 and for a pair that is not on this path; host and device (the workspace query reads it too)
__host__ __device__ inline bool rgb_geom(const dspn_png_rgb_sample &s, RgbGeom *g) {
  if (s.width < 1 || s.height < 1) return false;
  const int d = s.bit_depth, ct = s.colour_type;
  const bool low = d == 1 || d == 2 || d == 4, wide = d == 8 || d == 16;
  int channels;
  if (ct == 0 && (low || d == 8)) channels = 1;
  else if (ct == 3 && (low || d == 8)) channels = 1;
  else if (ct == 2 && wide) channels = 3;
  else if (ct == 4 && wide) channels = 2;
  else if (ct == 6 && wide) channels = 4;
  else return false;
  const int bits = channels * d;                                   // <= 64
  g->rb = ((long long)s.width * bits + 7) >> 3;                    // < 2^34
  g->bpp = bits >= 8 ? bits >> 3 : 1;
  g->px = bits >> 3;
  g->step = (ct == 2 || ct == 6) ? d >> 3 : 0;
  g->direct = ct == 2 && d == 8;
  return true;
}

// true when every address either launch derives from `s` stays inside raw, ws (where it is used) and out, and the palette exists
__device__ bool rgb_sample_ok(const dspn_png_rgb_sample &s, const RgbPools &pl, RgbGeom *g) {
  if (s.skip || !rgb_geom(s, g)) return false;
  const long long rb = g->rb, ob = 3ll * s.width;
  if (s.height > pl.raw_bytes / (rb + 1) || s.height > pl.out_bytes / ob) return false;   // so the products below fit the pools
  if (s.raw_offset < 0 || s.raw_offset > pl.raw_bytes - s.height * (rb + 1)) return false;
  if (s.out_offset < 0 || s.out_offset > pl.out_bytes - s.height * ob) return false;
  if (!g->direct) {
    if (s.height > pl.ws_bytes / rb) return false;
    if (s.recon_offset < 0 || s.recon_offset > pl.ws_bytes - s.height * rb) return false;
  }
  if (s.colour_type == 3 && (s.palette_index < 0 || s.palette_index >= pl.n_palettes)) return false;
  return true;
}

__global__ __launch_bounds__(kRows) void png_rgb_unfilter_kernel(const unsigned char *raw, const dspn_png_rgb_sample *__restrict__ samples,
                                                                 RgbPools pl, unsigned char *out, unsigned char *ws) {
  __shared__ unsigned xch[2][kWaves];
  const dspn_png_rgb_sample s = samples[blockIdx.x];
  RgbGeom g;
  if (!rgb_sample_ok(s, pl, &g)) return;                           // the whole workgroup, before any barrier
  const Rows r = {s.raw_offset, g.direct ? s.out_offset : s.recon_offset, s.height, g.rb};
  const Pools p2 = {pl.raw_bytes, g.direct ? pl.out_bytes : pl.ws_bytes};
  unsigned char *dst = g.direct ? out : ws;
  switch (g.bpp) {                                                 // the same in every thread
    case 1: unfilter_image<1, false>(raw, dst, r, p2, xch); break;
    case 2: unfilter_image<2, false>(raw, dst, r, p2, xch); break;
    case 3: unfilter_image<3, false>(raw, dst, r, p2, xch); break;
    case 4: unfilter_image<4, false>(raw, dst, r, p2, xch); break;
    case 6: unfilter_image<6, false>(raw, dst, r, p2, xch); break;
    default: unfilter_image<8, false>(raw, dst, r, p2, xch); break;
  }
}

constexpr int kExpandThreads = 256, kExpandBlocks = 128, kMaxGridY = 65535;

// the RGB bytes of pixel x of a reconstructed row
__device__ __forceinline__ void rgb_of(const unsigned char *row, long long x, const dspn_png_rgb_sample &s, const RgbGeom &g,
                                       const unsigned char *palette, unsigned char *rgb) {
  unsigned v;
  if (g.px) {                                                      // whole bytes: the sample's first (high) byte
    const unsigned char *p = row + x * g.px;
    if (g.step) { rgb[0] = p[0]; rgb[1] = p[g.step]; rgb[2] = p[2 * g.step]; return; }
    v = p[0];
  } else {                                                         // 1, 2 or 4 bits, the most significant first
    const int d = s.bit_depth;
    const long long bit = x * d;
    v = ((unsigned)row[bit >> 3] >> (8 - d - (int)(bit & 7))) & ((1u << d) - 1u);
    if (!palette) v *= d == 1 ? 255u : d == 2 ? 85u : 17u;
  }
  if (palette) { rgb[0] = palette[3 * v]; rgb[1] = palette[3 * v + 1]; rgb[2] = palette[3 * v + 2]; return; }
  rgb[0] = rgb[1] = rgb[2] = (unsigned char)v;
}

// image first + blockIdx.y; a thread makes 4 pixels of the image's pixel sequence at a time: 12 output bytes, three aligned
// dwords where the image's output starts on a dword and all four pixels exist
__global__ __launch_bounds__(kExpandThreads) void png_rgb_expand_kernel(const dspn_png_rgb_sample *__restrict__ samples, int first,
                                                                        RgbPools pl, const unsigned char *__restrict__ palettes,
                                                                        const unsigned char *__restrict__ ws, unsigned char *out) {
  const dspn_png_rgb_sample s = samples[first + blockIdx.y];
  RgbGeom g;
  if (!rgb_sample_ok(s, pl, &g) || g.direct) return;
  const unsigned char *palette = s.colour_type == 3 ? palettes + (long long)DSPN_PNG_PALETTE_BYTES * s.palette_index : nullptr;
  const unsigned char *rows = ws + s.recon_offset;
  unsigned char *dst = out + s.out_offset;
  const long long total = (long long)s.height * s.width, groups = (total + 3) >> 2;
  const bool aligned = (reinterpret_cast<uintptr_t>(dst) & 3) == 0;
  for (long long q = (long long)blockIdx.x * kExpandThreads + threadIdx.x; q < groups; q += (long long)gridDim.x * kExpandThreads) {
    const long long i0 = 4 * q;
    long long y = i0 / s.width, x = i0 - y * s.width;
    const int np = total - i0 < 4 ? (int)(total - i0) : 4;
    unsigned char b[12];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k < np) rgb_of(rows + y * g.rb, x, s, g, palette, b + 3 * k);
      else b[3 * k] = b[3 * k + 1] = b[3 * k + 2] = 0;
      if (++x == s.width) { x = 0; ++y; }
    }
    unsigned char *o = dst + 3 * i0;
    if (aligned && np == 4) {
#pragma unroll
      for (int k = 0; k < 3; ++k)
        reinterpret_cast<unsigned *>(o)[k] = b[4 * k] | (unsigned)b[4 * k + 1] << 8 | (unsigned)b[4 * k + 2] << 16 | (unsigned)b[4 * k + 3] << 24;
    } else {
#pragma unroll
      for (int k = 0; k < 12; ++k)
        if (k < 3 * np) o[k] = b[k];
    }
  }
}

}  // namespace

extern "C" size_t dspn_png_rgb_workspace_bytes(const dspn_png_rgb_sample *host_samples, int n) {
  long long need = 0;
  for (int k = 0; host_samples && k < n; ++k) {
    const dspn_png_rgb_sample &s = host_samples[k];
    RgbGeom g;
    if (s.skip || !rgb_geom(s, &g) || g.direct || s.recon_offset < 0) continue;
    if (s.height > (INT64_MAX - s.recon_offset) / g.rb) continue;  // no pool holds it: the device refuses the descriptor
    const long long end = s.recon_offset + s.height * g.rb;
    if (end > need) need = end;
  }
  return (size_t)need;
}

extern "C" int dspn_png_rgb_batch(const unsigned char *raw, long long raw_bytes, const dspn_png_rgb_sample *samples, int n,
                                  const unsigned char *palettes, int n_palettes, unsigned char *out, long long out_bytes,
                                  unsigned char *ws, long long ws_bytes, void *stream) {
  DSPN_REQUIRE(n >= 0 && raw_bytes >= 0 && out_bytes >= 0 && ws_bytes >= 0 && n_palettes >= 0,
               "png_rgb: negative count (n %d, raw_bytes %lld, out_bytes %lld, ws_bytes %lld, n_palettes %d)", n, raw_bytes, out_bytes,
               ws_bytes, n_palettes);
  if (n == 0) return 0;
  DSPN_REQUIRE(raw && samples && out, "png_rgb: null argument");
  DSPN_REQUIRE(palettes || n_palettes == 0, "png_rgb: null palettes with n_palettes %d", n_palettes);
  DSPN_REQUIRE(ws || ws_bytes == 0, "png_rgb: null workspace with ws_bytes %lld", ws_bytes);
  DSPN_REQUIRE((reinterpret_cast<uintptr_t>(samples) & 7) == 0, "png_rgb: samples must be 8-byte aligned");
  const RgbPools pl = {raw_bytes, out_bytes, ws_bytes, n_palettes};
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(png_rgb_unfilter_kernel, dim3(n), dim3(kRows), 0, st, raw, samples, pl, out, ws);
  if (int rc = dspn::check_launch("png_rgb (reconstruction)")) return rc;
  for (int first = 0; first < n; first += kMaxGridY) {
    const int count = n - first < kMaxGridY ? n - first : kMaxGridY;
    hipLaunchKernelGGL(png_rgb_expand_kernel, dim3(kExpandBlocks, count), dim3(kExpandThreads), 0, st, samples, first, pl, palettes, ws,
                       out);
    if (int rc = dspn::check_launch("png_rgb (samples to RGB)")) return rc;
  }
  return 0;
}

extern "C" int dspn_png_unfilter_batch(const unsigned char *raw, long long raw_bytes, const dspn_png_sample *samples, int n,
                                       unsigned char *out, long long out_bytes, void *stream) {
  DSPN_REQUIRE(n >= 0 && raw_bytes >= 0 && out_bytes >= 0, "png_unfilter: negative count (n %d, raw_bytes %lld, out_bytes %lld)", n,
               raw_bytes, out_bytes);
  if (n == 0) return 0;
  DSPN_REQUIRE(raw && samples && out, "png_unfilter: null argument");
  DSPN_REQUIRE((reinterpret_cast<uintptr_t>(samples) & 7) == 0, "png_unfilter: samples must be 8-byte aligned");
  const Pools pl = {raw_bytes, out_bytes};
  hipLaunchKernelGGL(png_unfilter_kernel, dim3(n), dim3(kRows), 0, static_cast<hipStream_t>(stream), raw, samples, pl, out);
  return dspn::check_launch("png_unfilter");
}

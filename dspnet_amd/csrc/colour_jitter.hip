// Colour jitter (HLS shifts, contrast gain) in place on the decoded uint8 RGB pool of a batch, for MI355X (gfx950); C ABI and
// the integer definition of every quantity in include/dspn_colour_jitter.h.  One kernel on the caller's stream:
//   colour_jitter_kernel : a work item is (image, chunk of kChunk pixels).  Every workgroup walks the descriptor list once,
//                          from the front, and takes the items blockIdx.x, blockIdx.x + gridDim.x, ... of the list's running
//                          item count: one large image is spread over the whole grid, many small ones take one workgroup
//                          each, and no table of item prefixes has to come from the (untrusted) host.
// Ownership: a lane owns the 4 pixels = 12 bytes [12 k, 12 k + 12) of its image and writes those bytes only.  The image's
// offset in the pool takes every alignment (the pools are packed at h * w * 3), and 12 k keeps it, so the alignment m of a
// lane's bytes is the image's:
//   m == 0 : three dword loads, three dword stores;
//   m != 0 : four aligned dword loads and a funnel shift (reading a neighbour's bytes is harmless, they are dropped); the
//            stores are 4 - m head bytes, the two aligned dwords that lie wholly inside the 12 bytes, and m tail bytes.  A
//            dword store that covered a neighbour's byte would write back a stale value under that lane's own store -- a race,
//            not only an out-of-bounds write at the image's ends -- so there is none.
//   the last lane of an image (fewer than 4 pixels) and a lane whose aligned words would leave the pool go byte by byte.
// The two divisions whose divisor varies per pixel (S and H, divisors 2 .. 510, numerators below 2^18) are a float
// reciprocal estimate, off by at most one either way, and one exact integer correction step (udiv_small); the float result
// alone decides nothing.  The division by 7650 is the compiler's multiply-high.
// What bounds it: vector instruction issue.  Per pixel the HLS round trip is some 150 vector instructions (a few of them
// quarter-rate multiplies) against 6 bytes of traffic; measured at 32 x 1024 x 2048: 3.7 ps per pixel, 3.9 times the byte
// floor, where the gain-only pass of the same kernel runs at 1.4 times ("Colour jitter on the device").
#include <cstdint>

#include "dspn_common.h"
#include "../../include/dspn_colour_jitter.h"

static_assert(sizeof(dspn_jitter_sample) == DSPN_JITTER_SAMPLE_BYTES, "descriptor layout");

namespace {

constexpr int kT = 256;
constexpr int kLanePixels = 4;                       // 12 bytes: three dwords
constexpr int kChunk = kT * kLanePixels;             // pixels of a work item
constexpr int kMaxGrid = 2048;                       // 8 workgroups on each of 256 CUs

struct Plan {
  long long items;                                   // work items of the image; 0: leave it alone
  long long bytes;                                   // height * width * 3
  bool hls, scale;
};

// what the kernel does for descriptor s: nothing (items == 0) unless every address it would derive stays inside the pool
// and every parameter is in range.  Divisions first: no product is formed before it is known to fit.
__device__ __forceinline__ Plan plan_of(const dspn_jitter_sample &s, long long pixel_bytes) {
  Plan p = {0, 0, false, false};
  if (s.height < 1 || s.width < 1) return p;
  if (s.height > pixel_bytes / 3 / s.width) return p;               // so height * width * 3 <= pixel_bytes
  const long long bytes = (long long)s.height * s.width * 3;
  if (s.img_offset < 0 || s.img_offset > pixel_bytes - bytes) return p;
  if (s.dh < -180 || s.dh > 180 || s.dl < -255 || s.dl > 255 || s.ds < -255 || s.ds > 255) return p;
  if (s.gain < 0 || s.gain > 65535) return p;
  p.hls = (s.dh | s.dl | s.ds) != 0;
  p.scale = s.gain != 1024;
  if (!p.hls && !p.scale) return p;
  p.bytes = bytes;
  p.items = (bytes / 3 + kChunk - 1) / kChunk;
  return p;
}

// floor(num / den) for 0 <= num < 2^18 and 1 <= den < 2^10.  Both conversions are exact, the reciprocal is good to an ulp and
// the product to half of one, so the estimate is within num / den * 2^-22 < 2^-4 of the quotient: truncated, it is the
// quotient or one beside it, and the remainder says which.
__device__ __forceinline__ int udiv_small(int num, int den) {
  int q = (int)((float)num * __builtin_amdgcn_rcpf((float)den));
  const int r = num - __mul24(q, den);
  if (r < 0) --q;
  else if (r >= den) ++q;
  return q;
}

__device__ __forceinline__ int clamp_to(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// one channel of the inverse: t = (H' + off) mod 180 is already formed.  The four pieces of W are 30 Q1 + (Q2 - Q1) k with
// k = t, 30, 120 - t, 0, which is min(t, 120 - t) held to 0 .. 30; every product is below 2^24
__device__ __forceinline__ int channel(int q1, int q2, int t) {
  const int k = clamp_to(min(t, 120 - t), 30);
  return (__mul24(30, q1) + __mul24(q2 - q1, k) + 3825) / 7650;
}

__device__ __forceinline__ void jitter_pixel(int &r, int &g, int &b, const dspn_jitter_sample &s, bool hls, bool scale) {
  if (hls) {                                                         // the same in every lane of the workgroup
    const int mx = max(r, max(g, b)), mn = min(r, min(g, b));
    const int d = mx - mn, sm = mx + mn;
    int L = (sm + 1) >> 1, S = 0, H = 0;
    {
      const int dd = d ? d : 1;                                      // a grey pixel divides by something; its S and H stay 0
      const int den = d ? (sm <= 255 ? sm : 510 - sm) : 1;
      const int x = mx == r ? g - b : mx == g ? b - r : r - g;
      const int base = mx == r ? 0 : mx == g ? 60 : 120;
      const int N = 30 * x + base * dd;
      // (2 N + d) // (2 d) with 180 = 360 d / (2 d) added first, so that the numerator is positive: x >= -d
      int h = udiv_small(2 * N + 361 * dd, 2 * dd) - 180;
      if (h < 0) h += 180;
      else if (h >= 180) h -= 180;
      if (d) { S = udiv_small(510 * d + den, 2 * den); H = h; }
    }
    H = clamp_to(H + s.dh, 180);
    L = clamp_to(L + s.dl, 255);
    S = clamp_to(S + s.ds, 255);
    {
      // S' == 0 needs no case of its own: Q1 = Q2 = 255 L' then, and (7650 L' + 3825) // 7650 = L' in every channel
      const int q2 = 2 * L <= 255 ? __mul24(L, 255 + S) : __mul24(255, L + S) - __mul24(L, S);
      const int q1 = __mul24(510, L) - q2;
      const int tr = H + 60 >= 180 ? H + 60 - 180 : H + 60;          // H in 0 .. 180
      const int tg = H >= 180 ? H - 180 : H;
      const int tb = H - 60 < 0 ? H - 60 + 180 : H - 60;
      r = channel(q1, q2, tr);
      g = channel(q1, q2, tg);
      b = channel(q1, q2, tb);
    }
  }
  if (scale) {
    r = min(255, (__mul24(r, s.gain) + 512) >> 10);                  // gain < 2^16: the product is below 2^24
    g = min(255, (__mul24(g, s.gain) + 512) >> 10);
    b = min(255, (__mul24(b, s.gain) + 512) >> 10);
  }
}

__device__ __forceinline__ unsigned funnel(unsigned lo, unsigned hi, unsigned bits) {     // bits 0 .. 31
  return (unsigned)((((unsigned long long)hi << 32) | lo) >> bits);
}

// the lane's (at most) 4 pixels of chunk `chunk` of the image of s
__device__ __forceinline__ void jitter_lane(unsigned char *pixels, long long pixel_bytes, const dspn_jitter_sample &s,
                                            const Plan &pl, long long chunk) {
  const long long at = (chunk * kChunk + (long long)threadIdx.x * kLanePixels) * 3;      // first byte, inside the image
  if (at >= pl.bytes) return;
  const int len = pl.bytes - at < 12 ? (int)(pl.bytes - at) : 12;                         // 3, 6, 9 or 12
  unsigned char *p = pixels + s.img_offset + at;
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), lo = reinterpret_cast<uintptr_t>(pixels);
  const unsigned m = (unsigned)(a & 3);
  const bool full = len == 12;
  // aligned words around the 12 bytes: all of them inside the pool?
  const bool wide = full && (m == 0 || (a - m >= lo && a - m + 16 <= lo + (uintptr_t)pixel_bytes));
  unsigned w[3] = {0, 0, 0};
  if (wide && m == 0) {
    const unsigned *q = reinterpret_cast<const unsigned *>(p);
    w[0] = q[0]; w[1] = q[1]; w[2] = q[2];
  } else if (wide) {
    const unsigned *q = reinterpret_cast<const unsigned *>(a - m);
    const unsigned a0 = q[0], a1 = q[1], a2 = q[2], a3 = q[3];
    w[0] = funnel(a0, a1, 8 * m); w[1] = funnel(a1, a2, 8 * m); w[2] = funnel(a2, a3, 8 * m);
  } else {
#pragma unroll
    for (int k = 0; k < 12; ++k)
      if (k < len) w[k >> 2] |= (unsigned)p[k] << (8 * (k & 3));
  }
  unsigned o[3] = {0, 0, 0};
#pragma unroll
  for (int px = 0; px < kLanePixels; ++px) {                          // pixels past `len` are zeros in, never stored
    int c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = (int)(w[(3 * px + k) >> 2] >> (8 * ((3 * px + k) & 3))) & 255;
    jitter_pixel(c[0], c[1], c[2], s, pl.hls, pl.scale);
#pragma unroll
    for (int k = 0; k < 3; ++k) o[(3 * px + k) >> 2] |= (unsigned)c[k] << (8 * ((3 * px + k) & 3));
  }
  if (full && m == 0) {
    unsigned *q = reinterpret_cast<unsigned *>(p);
    q[0] = o[0]; q[1] = o[1]; q[2] = o[2];
  } else if (full) {
    const unsigned head = 4 - m;                                      // bytes in front of the first aligned word
#pragma unroll
    for (unsigned k = 0; k < 3; ++k)
      if (k < head) p[k] = (unsigned char)(o[0] >> (8 * k));
    unsigned *q = reinterpret_cast<unsigned *>(p + head);             // aligned; q[0] and q[1] are bytes head .. head + 7
    q[0] = funnel(o[0], o[1], 8 * head);
    q[1] = funnel(o[1], o[2], 8 * head);
    const unsigned tail = o[2] >> (8 * head);                         // the last m bytes
#pragma unroll
    for (unsigned k = 0; k < 3; ++k)
      if (k < m) p[head + 8 + k] = (unsigned char)(tail >> (8 * k));
  } else {
#pragma unroll
    for (int k = 0; k < 12; ++k)
      if (k < len) p[k] = (unsigned char)(o[k >> 2] >> (8 * (k & 3)));
  }
}

__global__ __launch_bounds__(kT) void colour_jitter_kernel(unsigned char *pixels, long long pixel_bytes,
                                                           const dspn_jitter_sample *__restrict__ samples, int n) {
  long long item = blockIdx.x;                                        // this workgroup's next work item
  long long first = 0;                                                // the first work item of image i
  for (int i = 0; i < n; ++i) {
    const dspn_jitter_sample s = samples[i];
    const Plan pl = plan_of(s, pixel_bytes);
    for (; item < first + pl.items; item += gridDim.x) jitter_lane(pixels, pixel_bytes, s, pl, item - first);
    first += pl.items;
  }
}

}  // namespace

extern "C" int dspn_colour_jitter_batch_u8(unsigned char *pixels, long long pixel_bytes, const dspn_jitter_sample *samples,
                                           int n, void *stream) {
  DSPN_REQUIRE(n >= 0 && pixel_bytes >= 0, "colour_jitter: negative count (n %d, pixel_bytes %lld)", n, pixel_bytes);
  if (n == 0) return 0;
  DSPN_REQUIRE(pixels && samples, "colour_jitter: null argument");
  DSPN_REQUIRE((reinterpret_cast<uintptr_t>(samples) & 7) == 0, "colour_jitter: samples must be 8-byte aligned");
  // the running item count of the kernel stays below 2^63: at most 2^16 images of at most 2^48 / 3072 items
  DSPN_REQUIRE(n <= 65535 && pixel_bytes <= (1ll << 48), "colour_jitter: at most 65535 images and 2^48 bytes (n %d, pixel_bytes %lld)",
               n, pixel_bytes);
  // images inside the pool that do not overlap have at most this many items; more (overlaps) take further trips
  const long long items = pixel_bytes / (3 * kChunk) + n;
  const int grid = (int)std::min<long long>(items, kMaxGrid);
  hipLaunchKernelGGL(colour_jitter_kernel, dim3(grid), dim3(kT), 0, static_cast<hipStream_t>(stream), pixels, pixel_bytes,
                     samples, n);
  return dspn::check_launch("colour_jitter");
}

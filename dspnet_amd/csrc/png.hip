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

// four bytes of a row: x the filtered dword, left the row's previous output dword, up / upprev the output dwords above and
// above-left (all in stream order: PNG's byte order)
template <int BPP>
__device__ __forceinline__ unsigned reconstruct4(unsigned ft, unsigned x, unsigned left, unsigned up, unsigned upprev) {
  unsigned long long mine = left;                                  // bytes 0-3: the previous dword; 4-7: this one as it forms
  const unsigned long long above = ((unsigned long long)up << 32) | upprev;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int a = (int)(mine >> (8 * (4 + k - BPP))) & 255;
    const int b = (int)(above >> (8 * (4 + k))) & 255;
    const int c = (int)(above >> (8 * (4 + k - BPP))) & 255;
    const int pa = iabs(b - c), pb = iabs(a - c), pc = iabs(a + b - 2 * c);
    const int paeth = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
    const int pred = ft == 1 ? a : ft == 2 ? b : ft == 3 ? (a + b) >> 1 : ft == 4 ? paeth : 0;
    const unsigned v = ((x >> (8 * k)) + (unsigned)pred) & 255u;
    mine |= (unsigned long long)v << (8 * (4 + k));
  }
  return (unsigned)(mine >> 32);
}

template <int BPP>
__device__ void unfilter_image(const unsigned char *raw, unsigned char *out, const dspn_png_sample &s, const Pools &pl,
                               unsigned (*xch)[kWaves]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long rb = (long long)s.width * BPP;
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
    unsigned left = 0, upprev = 0, last = 0;
    for (long long t = 0; t < steps; ++t) {
      unsigned up = __shfl_up(last, 1);                            // lane r - 1 made dword t - r of its row in step t - 1
      if (lane == 0 && tid > 0) up = xch[(t + 1) & 1][wave - 1];   // ... written in step t - 1
      const long long j = t - tid;
      if (live && j >= 0 && j < rd) {
        if (tid == 0) {
          up = 0;
          if (from_out) { up = prev_row.take(); if (BPP == 2) up = swap_pairs(up); }
        }
        const unsigned cur = reconstruct4<BPP>(ft, in.take(), left, up, upprev);
        upprev = up; left = cur; last = cur;
        const long long o = 4 * j;
        const unsigned v = BPP == 2 ? swap_pairs(cur) : cur;
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
  if (s.bytes_per_pixel == 1) unfilter_image<1>(raw, out, s, pl, xch);
  else unfilter_image<2>(raw, out, s, pl, xch);
}

}  // namespace

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

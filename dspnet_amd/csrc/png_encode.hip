// Row filters of the PNG encode for MI355X (gfx950); C ABI and the filter rule in include/dspn_png_encode.h.  The host half
// (deflate, chunks) is dspnet_amd/dataset/png_encode.py.
//
// Dependencies: a filtered byte needs the RAW bytes to its left, above and above-left, so every row of every image is
// independent.  One workgroup takes one row of the batch at a time (a row table over the whole batch: first_row[i] is the
// number of rows before image i, a workgroup finds its image by bisection); in three steps:
//   stage   : the row and the row above go to LDS in stream order (16-bit samples byte-swapped here), shifted so that LDS
//             byte position P holds what lands at the aligned output address + P.  Position s = (output row address & 3) is
//             the filter-type byte, the row's byte j sits at s + 1 + j, everything before the row reads as zero (that is the
//             `left` and `ul` of the first pixel, and the whole row above for row 0).
//   score   : a thread takes whole dwords of that image: the dword and the one before it of both rows give the four bytes
//             and their neighbours bytes_per_pixel back without an unaligned access; the four candidates' scores are
//             summed per thread, then over the workgroup (wave shuffles, one LDS exchange).
//   write   : the chosen candidate is formed again from LDS and stored: aligned dwords inside the row, bytes at its two
//             ends (an output row starts at any address: 1 + row_bytes is odd for most widths).
// A row longer than kStage bytes does the same three steps per byte against global memory (the second and third read come
// from the caches).
// What bounds it: the staging loads are one byte per lane (64 B per wave instruction), because source alignment, output
// alignment and the byte swap all differ; LDS traffic and the rest are per dword.  The deflate that follows on the host is
// two orders of magnitude slower than this kernel, so the loads were left plain.
// No workgroup waits for another one; every barrier's trip count comes from the table alone (the same in every thread).
#include <cstdint>
#include <vector>

#include "dspn_common.h"
#include "../../include/dspn_png_encode.h"

static_assert(sizeof(dspn_png_enc_sample) == DSPN_PNG_ENC_SAMPLE_BYTES, "descriptor layout");

namespace {

constexpr int kT = 256;                    // threads of a workgroup
constexpr int kWaves = kT / 64;
constexpr int kStage = 16384;              // longest row held in LDS; the callers' widest is 2 * 2048 * 3 = 12288 bytes
constexpr int kStageDwords = kStage / 4 + 1;        // positions 0 .. 3 + kStage
constexpr int kMaxGrid = 1 << 20;          // workgroups of a launch; each walks its rows

__device__ __forceinline__ int iabs(int v) { return v < 0 ? -v : v; }
__device__ __forceinline__ int cost(int v) { return v < 128 ? v : 256 - v; }

// the four candidates of one byte, each in 0..255: x the byte, a left, b up, c up-left
struct Cand { int none, up, sub, paeth; };
__device__ __forceinline__ Cand candidates(int x, int a, int b, int c) {
  const int pa = iabs(b - c), pb = iabs(a - c), pc = iabs(a + b - 2 * c);
  const int pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
  return {x, (x - b) & 255, (x - a) & 255, (x - pred) & 255};
}
__device__ __forceinline__ int pick(const Cand &v, int ft) { return ft == 0 ? v.none : ft == 2 ? v.up : ft == 1 ? v.sub : v.paeth; }

struct Score { int none = 0, up = 0, sub = 0, paeth = 0; };
__device__ __forceinline__ void add(Score &s, const Cand &v) {
  s.none += cost(v.none); s.up += cost(v.up); s.sub += cost(v.sub); s.paeth += cost(v.paeth);
}

// the filter type of a row from every thread's partial scores (one barrier; `red` is free again after the next one)
__device__ int choose(Score s, int (*red)[4]) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    s.none += __shfl_xor(s.none, d); s.up += __shfl_xor(s.up, d); s.sub += __shfl_xor(s.sub, d); s.paeth += __shfl_xor(s.paeth, d);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[wave][0] = s.none; red[wave][1] = s.up; red[wave][2] = s.sub; red[wave][3] = s.paeth; }
  __syncthreads();
  int t[4] = {0, 0, 0, 0};
  for (int w = 0; w < kWaves; ++w)
    for (int k = 0; k < 4; ++k) t[k] += red[w][k];
  int ft = 0, best = t[0];                                         // None, Up, Sub, Paeth; only a strictly lower score replaces
  if (t[1] < best) { ft = 2; best = t[1]; }
  if (t[2] < best) { ft = 1; best = t[2]; }
  if (t[3] < best) { ft = 4; best = t[3]; }
  return ft;
}

// byte j of a source row in stream order
template <int BPP>
__device__ __forceinline__ int stream_byte(const unsigned char *row, int j) { return row[BPP == 2 ? j ^ 1 : j]; }

// rb <= kStage.  cur / up: kStageDwords + 1 dwords each, index 0 the dword before position 0
template <int BPP>
__device__ void filter_row_staged(const unsigned char *srow, const unsigned char *prow, int rb, unsigned char *orow, unsigned *cur,
                                  unsigned *up, int (*red)[4]) {
  const int tid = threadIdx.x;
  const int s = (int)(reinterpret_cast<uintptr_t>(orow) & 3);
  const int nd = (s + 1 + rb + 3) >> 2;                            // dwords that hold positions 0 .. s + rb
  for (int d = tid; d <= nd; d += kT) { cur[d] = 0; up[d] = 0; }
  __syncthreads();
  unsigned char *cb = reinterpret_cast<unsigned char *>(cur + 1) + s + 1, *ub = reinterpret_cast<unsigned char *>(up + 1) + s + 1;
  for (int j = tid; j < rb; j += kT) cb[j] = (unsigned char)stream_byte<BPP>(srow, j);
  if (prow)
    for (int j = tid; j < rb; j += kT) ub[j] = (unsigned char)stream_byte<BPP>(prow, j);
  __syncthreads();

  Score sc;
  for (int k = tid; k < nd; k += kT) {
    const unsigned long long cw = ((unsigned long long)cur[k + 1] << 32) | cur[k], uw = ((unsigned long long)up[k + 1] << 32) | up[k];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = 4 * k + i - 1 - s;
      if (j < 0 || j >= rb) continue;
      add(sc, candidates((int)(cw >> (8 * (4 + i))) & 255, (int)(cw >> (8 * (4 + i - BPP))) & 255, (int)(uw >> (8 * (4 + i))) & 255,
                         (int)(uw >> (8 * (4 + i - BPP))) & 255));
    }
  }
  const int ft = choose(sc, red);

  unsigned char *obase = orow - s;                                 // 4-byte aligned
  for (int k = tid; k < nd; k += kT) {
    const unsigned long long cw = ((unsigned long long)cur[k + 1] << 32) | cur[k], uw = ((unsigned long long)up[k + 1] << 32) | up[k];
    unsigned word = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int v = pick(candidates((int)(cw >> (8 * (4 + i))) & 255, (int)(cw >> (8 * (4 + i - BPP))) & 255,
                                    (int)(uw >> (8 * (4 + i))) & 255, (int)(uw >> (8 * (4 + i - BPP))) & 255), ft);
      word |= (unsigned)(4 * k + i == s ? ft : v) << (8 * i);
    }
    const int lo = 4 * k < s ? s - 4 * k : 0;                      // bytes lo .. hi - 1 of this dword are the row's
    const int hi = s + 1 + rb - 4 * k < 4 ? s + 1 + rb - 4 * k : 4;
    if (lo == 0 && hi == 4) {
      *reinterpret_cast<unsigned *>(obase + 4 * k) = word;
    } else {
      for (int i = lo; i < hi; ++i) obase[4 * k + i] = (unsigned char)(word >> (8 * i));
    }
  }
}

// any rb: every byte and its neighbours from global memory
template <int BPP>
__device__ void filter_row_direct(const unsigned char *srow, const unsigned char *prow, int rb, unsigned char *orow, int (*red)[4]) {
  const int tid = threadIdx.x;
  auto at = [&](int j) {
    const int x = stream_byte<BPP>(srow, j), a = j >= BPP ? stream_byte<BPP>(srow, j - BPP) : 0;
    const int b = prow ? stream_byte<BPP>(prow, j) : 0, c = prow && j >= BPP ? stream_byte<BPP>(prow, j - BPP) : 0;
    return candidates(x, a, b, c);
  };
  Score sc;
  for (int j = tid; j < rb; j += kT) add(sc, at(j));
  const int ft = choose(sc, red);
  if (tid == 0) orow[0] = (unsigned char)ft;
  for (int j = tid; j < rb; j += kT) orow[1 + j] = (unsigned char)pick(at(j), ft);
}

template <int BPP>
__device__ void filter_row(const unsigned char *srow, const unsigned char *prow, int rb, unsigned char *orow, unsigned *cur,
                           unsigned *up, int (*red)[4]) {
  if (rb <= kStage) filter_row_staged<BPP>(srow, prow, rb, orow, cur, up, red);
  else filter_row_direct<BPP>(srow, prow, rb, orow, red);
}

// samples and first_row (n + 1 entries) were checked by the host before they were copied here
__global__ __launch_bounds__(kT) void png_filter_kernel(const dspn_png_enc_sample *__restrict__ samples,
                                                        const int *__restrict__ first_row, int n, const unsigned char *src,
                                                        unsigned char *out) {
  __shared__ unsigned cur[kStageDwords + 1], up[kStageDwords + 1];
  __shared__ int red[kWaves][4];
  const long long total = first_row[n];
  for (long long row = blockIdx.x; row < total; row += gridDim.x) {
    int lo = 0, hi = n - 1;                                        // the last image with first_row[i] <= row
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (first_row[mid] <= row) lo = mid; else hi = mid - 1;
    }
    const dspn_png_enc_sample s = samples[lo];
    const long long y = row - first_row[lo];
    const int rb = s.width * s.bytes_per_pixel;
    const unsigned char *srow = src + s.src_offset + y * s.src_pitch;
    const unsigned char *prow = y > 0 ? srow - s.src_pitch : nullptr;
    unsigned char *orow = out + s.out_offset + y * (rb + 1LL);
    if (s.bytes_per_pixel == 1) filter_row<1>(srow, prow, rb, orow, cur, up, red);
    else if (s.bytes_per_pixel == 2) filter_row<2>(srow, prow, rb, orow, cur, up, red);
    else filter_row<3>(srow, prow, rb, orow, cur, up, red);
    __syncthreads();                                               // LDS is the next row's
  }
}

bool format_ok(int width, int height, int bpp) {
  return width >= 1 && height >= 1 && bpp >= 1 && bpp <= 3 && (long long)width * bpp <= DSPN_PNG_ENC_MAX_ROW_BYTES;
}

}  // namespace

extern "C" long long dspn_png_filtered_bytes(int width, int height, int bytes_per_pixel) {
  return format_ok(width, height, bytes_per_pixel) ? height * (1LL + (long long)width * bytes_per_pixel) : 0;
}

extern "C" size_t dspn_png_filter_workspace_bytes(int n) {
  return n > 0 ? dspn::align_up((size_t)n * sizeof(dspn_png_enc_sample) + ((size_t)n + 1) * sizeof(int), 8) : 0;
}

extern "C" int dspn_png_filter_batch(const dspn_png_enc_sample *samples, int n, const unsigned char *src, long long src_bytes,
                                     unsigned char *out, long long out_bytes, void *workspace, size_t workspace_bytes, void *stream) {
  DSPN_REQUIRE(n >= 0, "png_filter: negative count (n %d)", n);
  if (n == 0) return 0;
  DSPN_REQUIRE(samples && src && out && workspace, "png_filter: null argument");
  DSPN_REQUIRE(src_bytes > 0 && out_bytes > 0, "png_filter: empty pool (src_bytes %lld, out_bytes %lld)", src_bytes, out_bytes);
  DSPN_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "png_filter: workspace must be 8-byte aligned");
  const size_t table_bytes = dspn_png_filter_workspace_bytes(n);
  std::vector<unsigned char> table(table_bytes);
  dspn_png_enc_sample *checked = reinterpret_cast<dspn_png_enc_sample *>(table.data());
  int *first_row = reinterpret_cast<int *>(table.data() + (size_t)n * sizeof(dspn_png_enc_sample));
  long long rows = 0;
  for (int i = 0; i < n; ++i) {
    const dspn_png_enc_sample s = samples[i];
    DSPN_REQUIRE(s.bytes_per_pixel >= 1 && s.bytes_per_pixel <= 3, "png_filter: image %d: bytes_per_pixel is 1, 2 or 3, got %d", i,
                 s.bytes_per_pixel);
    DSPN_REQUIRE(format_ok(s.width, s.height, s.bytes_per_pixel),
                 "png_filter: image %d: %d x %d with %d bytes per pixel (sizes from 1, rows of at most %d bytes)", i, s.width,
                 s.height, s.bytes_per_pixel, DSPN_PNG_ENC_MAX_ROW_BYTES);
    const long long rb = (long long)s.width * s.bytes_per_pixel;
    DSPN_REQUIRE(s.src_pitch >= rb, "png_filter: image %d: a pitch of %d bytes for rows of %lld", i, s.src_pitch, rb);
    const long long src_span = (s.height - 1LL) * s.src_pitch + rb, out_span = s.height * (rb + 1);     // both below 2^56
    DSPN_REQUIRE(s.src_offset >= 0 && src_span <= src_bytes && s.src_offset <= src_bytes - src_span,
                 "png_filter: image %d: %lld source bytes from offset %lld run past src_bytes %lld", i, src_span, s.src_offset, src_bytes);
    DSPN_REQUIRE(s.out_offset >= 0 && out_span <= out_bytes && s.out_offset <= out_bytes - out_span,
                 "png_filter: image %d: %lld output bytes from offset %lld run past out_bytes %lld", i, out_span, s.out_offset, out_bytes);
    checked[i] = s;
    first_row[i] = (int)rows;
    rows += s.height;
    DSPN_REQUIRE(rows <= 0x7fffffffLL, "png_filter: more than 2^31 - 1 rows in one batch");
  }
  first_row[n] = (int)rows;
  if (workspace_bytes < table_bytes)
    return dspn::fail(DSPN_ERR_WORKSPACE_, "png_filter: workspace of %zu bytes, %zu needed", workspace_bytes, table_bytes);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const hipError_t e = hipMemcpyWithStream(workspace, table.data(), table_bytes, hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return dspn::fail(DSPN_ERR_LAUNCH_, "png_filter: copy of the row table: %s", hipGetErrorString(e));
  const dspn_png_enc_sample *samples_dev = static_cast<const dspn_png_enc_sample *>(workspace);
  const int *first_row_dev = reinterpret_cast<const int *>(static_cast<const unsigned char *>(workspace) + (size_t)n * sizeof(dspn_png_enc_sample));
  const int grid = (int)std::min<long long>(rows, kMaxGrid);
  hipLaunchKernelGGL(png_filter_kernel, dim3(grid), dim3(kT), 0, st, samples_dev, first_row_dev, n, src, out);
  return dspn::check_launch("png_filter");
}

// JPEG decode of the record iterator for MI355X (gfx950); C ABI and the arithmetic contract in include/dspn_jpeg.h.
// The host half (markers, Huffman) is jpeg_host.h.  The device half is two launches on the caller's stream, each a fixed
// grid of workgroups that strides over the work of the whole batch:
//   jpeg_idct_kernel   : dequantise + 8 x 8 inverse DCT, int16 coefficients -> uint8 component planes in the workspace (a plane
//                        is a raster over the padded block grid and sits at the byte offset its coefficients have as an int16
//                        index, so the workspace is coef_count bytes).  Eight lanes per block: lane t loads row t (16 B, so a
//                        wave reads 1 KiB of consecutive coefficients), the block turns through LDS, lane t runs column t of pass 1
//                        and row t of pass 2 and stores 8 samples.  No DC-only shortcut: the general form gives the same bits, and
//                        every lane runs the same instructions.
//   jpeg_colour_kernel : chroma upsampling ("fancy", over the real extent, edges replicated; box for a chroma plane of at most
//                        two columns) + YCbCr -> RGB, planes -> the
//                        (h, w, 3) bytes at img_offset.  One thread per 4 pixels of a row: one dword of luma, the chroma
//                        neighbours from L1, 12 output bytes as 3 dwords where the address allows it.
// Per image of h x w pixels with luma sampling H x V (n = samples per pixel: 3, 2 or 1.5; 1 for grey), over the padded grids:
//   idct   reads 2 n bytes/pixel of coefficients, writes n bytes/pixel of planes;
//   colour reads n bytes/pixel of planes (chroma rows again through the caches), writes 3 bytes/pixel.
// Neither kernel knows the batch on the host: each workgroup first sums the work of the B descriptors in LDS (validating
// every one: a descriptor that could index outside a buffer counts as no work), then finds the sample of a unit by a
// binary search over those sums.
#include <cstdint>

#include "dspn_common.h"
#include "jpeg_host.h"
#include "jpeg_huff.h"

namespace {

constexpr int kT = 256;
constexpr int kMaxB = 1024;
constexpr int kGrid = 2048;                // 256 CUs x 8 workgroups of 256 threads
constexpr int kBlocksPerWg = kT / 8;
constexpr int kRowPix = kT * 4;            // pixels of a row one workgroup covers per unit

struct Pools { long long coef_count, images_bytes; };

// true when every index the kernels derive from `s` stays inside coefs / workspace (coef_count) and images_out
__device__ bool sample_ok(const dspn_jpeg_sample &s, const Pools &pl) {
  if (s.skip) return false;
  if (!dspn_jpeg_huff::coef_geometry_ok(s, pl.coef_count)) return false;
  return s.img_offset >= 0 && s.img_offset <= pl.images_bytes - 3LL * s.width * s.height;
}

// first[b] = units of samples 0 .. b - 1 (first[B] = all); units(s) is called for valid samples only
template <typename F>
__device__ void prefix_units(const dspn_jpeg_sample *samples, int B, const Pools &pl, long long *first, F units) {
  for (int b = threadIdx.x; b < B; b += kT) {
    const dspn_jpeg_sample &s = samples[b];
    first[b + 1] = sample_ok(s, pl) ? units(s) : 0;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    long long acc = 0;
    first[0] = 0;
    for (int b = 1; b <= B; ++b) { acc += first[b]; first[b] = acc; }
  }
  __syncthreads();
}

// largest b in [0, B) with first[b] <= u (u < first[B])
__device__ __forceinline__ int find_sample(const long long *first, int B, long long u) {
  int lo = 0, hi = B;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (first[mid] <= u) lo = mid; else hi = mid;
  }
  return lo;
}

// one 1-D pass of the slow integer IDCT (include/dspn_jpeg.h), in place; s: the descale shift
__device__ __forceinline__ void idct8(int (&i)[8], int s) {
  int z1 = (i[2] + i[6]) * 4433;
  const int t2 = z1 - i[6] * 15137, t3 = z1 + i[2] * 6270;
  const int t0 = (i[0] + i[4]) * 8192, t1 = (i[0] - i[4]) * 8192;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  int a0 = i[7], a1 = i[5], a2 = i[3], a3 = i[1];
  z1 = a0 + a3;
  int z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
  const int z5 = (z3 + z4) * 9633;
  a0 *= 2446; a1 *= 16819; a2 *= 25172; a3 *= 12299;
  z1 *= -7373; z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  a0 += z1 + z3; a1 += z2 + z4; a2 += z2 + z3; a3 += z1 + z4;
  const int r = 1 << (s - 1);
  i[0] = (t10 + a3 + r) >> s; i[7] = (t10 - a3 + r) >> s;
  i[1] = (t11 + a2 + r) >> s; i[6] = (t11 - a2 + r) >> s;
  i[2] = (t12 + a1 + r) >> s; i[5] = (t12 - a1 + r) >> s;
  i[3] = (t13 + a0 + r) >> s; i[4] = (t13 - a0 + r) >> s;
}

__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

__global__ __launch_bounds__(kT) void jpeg_idct_kernel(const short *__restrict__ coefs, const dspn_jpeg_sample *__restrict__ samples,
                                                       int B, Pools pl, unsigned char *__restrict__ planes) {
  __shared__ long long first[kMaxB + 1];
  __shared__ int tile[kBlocksPerWg][8][9];          // one block per 8 lanes, rows padded to 9 words
  prefix_units(samples, B, pl, first, [](const dspn_jpeg_sample &s) {
    long long n = 0;
    for (int c = 0; c < s.ncomp; ++c) n += (long long)s.blocks_w[c] * s.blocks_h[c];
    return n;
  });
  const long long total = first[B];
  const int g = threadIdx.x >> 3, t = threadIdx.x & 7;
  for (long long base = (long long)blockIdx.x * kBlocksPerWg; base < total; base += (long long)gridDim.x * kBlocksPerWg) {
    const long long u = base + g;
    const bool live = u < total;
    int v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned char *dst = nullptr;
    if (live) {
      const int b = find_sample(first, B, u);
      const dspn_jpeg_sample &s = samples[b];
      long long l = u - first[b];
      int c = 0;
      for (; c < s.ncomp - 1; ++c) {
        const long long n = (long long)s.blocks_w[c] * s.blocks_h[c];
        if (l < n) break;
        l -= n;
      }
      const int bw = s.blocks_w[c];
      const int by = (int)(l / bw), bx = (int)(l - (long long)by * bw);
      const uint4 raw = *reinterpret_cast<const uint4 *>(coefs + s.coef_offset[c] + l * 64 + t * 8);
      const uint2 q = *reinterpret_cast<const uint2 *>(&s.quant[c][t * 8]);
      const unsigned rw[4] = {raw.x, raw.y, raw.z, raw.w};
      const unsigned qw[2] = {q.x, q.y};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int cf = (int)(short)(rw[j >> 1] >> (16 * (j & 1)));
        v[j] = cf * (int)((qw[j >> 2] >> (8 * (j & 3))) & 255u);
      }
      dst = planes + s.coef_offset[c] + ((long long)by * 8 + t) * ((long long)bw * 8) + bx * 8;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) tile[g][t][j] = v[j];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = tile[g][j][t];             // column t
    __syncthreads();
    idct8(v, 11);
#pragma unroll
    for (int j = 0; j < 8; ++j) tile[g][j][t] = v[j];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = tile[g][t][j];             // row t of the pass-1 result
    __syncthreads();
    idct8(v, 18);
    if (live) {
      uint2 o;
      o.x = (unsigned)clamp255(v[0] + 128) | (unsigned)clamp255(v[1] + 128) << 8 | (unsigned)clamp255(v[2] + 128) << 16 |
            (unsigned)clamp255(v[3] + 128) << 24;
      o.y = (unsigned)clamp255(v[4] + 128) | (unsigned)clamp255(v[5] + 128) << 8 | (unsigned)clamp255(v[6] + 128) << 16 |
            (unsigned)clamp255(v[7] + 128) << 24;
      *reinterpret_cast<uint2 *>(dst) = o;
    }
  }
}

// four upsampled chroma samples at output columns x0 .. x0 + 3 (x0 % 4 == 0) of output row y
__device__ __forceinline__ void chroma4(const unsigned char *__restrict__ plane, int stride, int cw, int ch, int hs, int vs, int y,
                                        int x0, int (&out)[4]) {
  if (hs == 1) {
    const unsigned w = *reinterpret_cast<const unsigned *>(plane + (long long)y * stride + x0);
#pragma unroll
    for (int j = 0; j < 4; ++j) out[j] = (int)((w >> (8 * j)) & 255u);
    return;
  }
  if (cw <= 2) {                                    // libjpeg-turbo's choice for a plane of one or two columns: box, down the rows too
    const unsigned char *r = plane + (long long)(vs == 2 ? y >> 1 : y) * stride;
#pragma unroll
    for (int j = 0; j < 4; ++j) { const int c = (x0 + j) >> 1; out[j] = r[c > cw - 1 ? cw - 1 : c]; }
    return;
  }
  const int c0 = x0 >> 1;
  int col[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) { const int c = c0 - 1 + j; col[j] = c < 0 ? 0 : (c > cw - 1 ? cw - 1 : c); }
  int s[4];
  if (vs == 1) {
    const unsigned char *r = plane + (long long)y * stride;
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] = r[col[j]];
    out[0] = (3 * s[1] + s[0] + 1) >> 2; out[1] = (3 * s[1] + s[2] + 2) >> 2;
    out[2] = (3 * s[2] + s[1] + 1) >> 2; out[3] = (3 * s[2] + s[3] + 2) >> 2;
  } else {
    const int cy = y >> 1;
    int fy = (y & 1) ? cy + 1 : cy - 1;
    fy = fy < 0 ? 0 : (fy > ch - 1 ? ch - 1 : fy);
    const unsigned char *rn = plane + (long long)cy * stride, *rf = plane + (long long)fy * stride;
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] = 3 * rn[col[j]] + rf[col[j]];
    out[0] = (3 * s[1] + s[0] + 8) >> 4; out[1] = (3 * s[1] + s[2] + 7) >> 4;
    out[2] = (3 * s[2] + s[1] + 8) >> 4; out[3] = (3 * s[2] + s[3] + 7) >> 4;
  }
}

__global__ __launch_bounds__(kT) void jpeg_colour_kernel(const unsigned char *__restrict__ planes,
                                                         const dspn_jpeg_sample *__restrict__ samples, int B, Pools pl,
                                                         unsigned char *__restrict__ images) {
  __shared__ long long first[kMaxB + 1];
  prefix_units(samples, B, pl, first,
               [](const dspn_jpeg_sample &s) { return (long long)s.height * ((s.width + kRowPix - 1) / kRowPix); });
  const long long total = first[B];
  for (long long u = blockIdx.x; u < total; u += gridDim.x) {
    const int b = find_sample(first, B, u);
    const dspn_jpeg_sample &s = samples[b];
    const long long l = u - first[b];
    const int w = s.width, h = s.height;
    const int chunks = (w + kRowPix - 1) / kRowPix;
    const int y = (int)(l / chunks);
    const int x0 = (int)(l - (long long)y * chunks) * kRowPix + threadIdx.x * 4;
    if (x0 >= w) continue;
    const unsigned yw = *reinterpret_cast<const unsigned *>(planes + s.coef_offset[0] + (long long)y * (s.blocks_w[0] * 8) + x0);
    unsigned char rgb[12];
    if (s.ncomp == 1) {
#pragma unroll
      for (int j = 0; j < 4; ++j) rgb[3 * j] = rgb[3 * j + 1] = rgb[3 * j + 2] = (unsigned char)((yw >> (8 * j)) & 255u);
    } else {
      const int hs = s.hsamp, vs = s.vsamp;
      const int cw = (w + hs - 1) / hs, ch = (h + vs - 1) / vs;
      int cb[4], cr[4];
      chroma4(planes + s.coef_offset[1], s.blocks_w[1] * 8, cw, ch, hs, vs, y, x0, cb);
      chroma4(planes + s.coef_offset[2], s.blocks_w[2] * 8, cw, ch, hs, vs, y, x0, cr);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int Y = (int)((yw >> (8 * j)) & 255u), u_ = cb[j] - 128, v_ = cr[j] - 128;
        rgb[3 * j] = (unsigned char)clamp255(Y + ((91881 * v_ + 32768) >> 16));
        rgb[3 * j + 1] = (unsigned char)clamp255(Y + ((-22554 * u_ + 32768 - 46802 * v_) >> 16));
        rgb[3 * j + 2] = (unsigned char)clamp255(Y + ((116130 * u_ + 32768) >> 16));
      }
    }
    unsigned char *o = images + s.img_offset + ((long long)y * w + x0) * 3;
    if (x0 + 4 <= w && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
      unsigned *o4 = reinterpret_cast<unsigned *>(o);
#pragma unroll
      for (int j = 0; j < 3; ++j)
        o4[j] = (unsigned)rgb[4 * j] | (unsigned)rgb[4 * j + 1] << 8 | (unsigned)rgb[4 * j + 2] << 16 | (unsigned)rgb[4 * j + 3] << 24;
    } else {
      const int nb = 3 * (w - x0 < 4 ? w - x0 : 4);
#pragma unroll
      for (int j = 0; j < 12; ++j)
        if (j < nb) o[j] = rgb[j];
    }
  }
}

// ---- entropy pass of streams with restart intervals (include/dspn_jpeg.h; the decode itself is jpeg_huff.h) -------------------
// One restart interval per lane.  A workgroup is one wave: a chunk of kTE consecutive units is cut into runs of one sample, and
// per run the wave builds that sample's decode tables in LDS (thread 0 checks the descriptors, one thread per table derives the
// canonical codes, all fill the lookahead windows), then each lane decodes its interval serially.  Lanes diverge by design.
// A lane's block is staged in LDS, dword j of lane t at word j * kTE + t (no two lanes on one bank whatever j they touch), and
// leaves as eight 16-byte stores.  Per block: 128 B written; per interval its compressed bytes read once, a byte at a time.
constexpr int kTE = 64;
constexpr int kGridE = 2048;

struct EntropyPools { long long bytes_count, segment_count, coef_count; };

struct LdsSink {
  unsigned *col;                           // this lane's column of the staging tile
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int j = 0; j < 32; ++j) col[j * kTE] = 0u;
  }
  // a position is set at most once after clear(): the decode only moves forward through the zigzag order
  __device__ __forceinline__ void set(int at, int v) { col[(at >> 1) * kTE] |= ((unsigned)v & 0xFFFFu) << (16 * (at & 1)); }
  __device__ __forceinline__ void store(short *dst) const {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      uint4 q;
      q.x = col[(4 * j) * kTE]; q.y = col[(4 * j + 1) * kTE]; q.z = col[(4 * j + 2) * kTE]; q.w = col[(4 * j + 3) * kTE];
      reinterpret_cast<uint4 *>(dst)[j] = q;
    }
  }
};

__global__ __launch_bounds__(kTE) void jpeg_entropy_kernel(const unsigned char *__restrict__ bytes,
                                                           const dspn_jpeg_sample *__restrict__ samples,
                                                           const dspn_jpeg_scan *__restrict__ scans, int B,
                                                           const unsigned *__restrict__ segments, EntropyPools pl,
                                                           short *__restrict__ coefs, int *__restrict__ status) {
  namespace hf = dspn_jpeg_huff;
  __shared__ long long first[kMaxB + 1];
  __shared__ hf::Table tables[hf::kSlots];
  __shared__ hf::Layout layout;
  __shared__ int layout_ok;
  __shared__ unsigned tile[32 * kTE];
  __shared__ unsigned char natural[64];
  const int tid = threadIdx.x;
  for (int b = tid; b < B; b += kTE) {
    hf::Layout L;
    first[b + 1] = hf::prepare(samples[b], scans[b], pl.bytes_count, pl.segment_count, pl.coef_count, L) ? L.segments : 0;
  }
  if (tid == 0) hf::fill_natural(natural);
  __syncthreads();
  if (tid == 0) {
    long long acc = 0;
    first[0] = 0;
    for (int b = 1; b <= B; ++b) { acc += first[b]; first[b] = acc; }
  }
  __syncthreads();
  const long long total = first[B];
  LdsSink sink;
  sink.col = tile + tid;
  for (long long base = (long long)blockIdx.x * kTE; base < total; base += (long long)gridDim.x * kTE) {
    const long long chunk_end = base + kTE < total ? base + kTE : total;
    long long u0 = base;
    while (u0 < chunk_end) {               // the same for every lane: at most kTE runs
      const int b = find_sample(first, B, u0);
      const long long run_end = first[b + 1] < chunk_end ? first[b + 1] : chunk_end;
      __syncthreads();                     // the run before this one has let go of layout and tables
      if (tid == 0) layout_ok = hf::prepare(samples[b], scans[b], pl.bytes_count, pl.segment_count, pl.coef_count, layout) ? 1 : 0;
      __syncthreads();
      if (layout_ok) {
        if (tid < hf::kSlots) {
          const int t = layout.slot_table[tid];
          if (t < 0) tables[tid].nvals = -1;
          else hf::build_codes(tables[tid], t < 4 ? scans[b].dc_counts[t] : scans[b].ac_counts[t - 4],
                               t < 4 ? scans[b].dc_values[t] : scans[b].ac_values[t - 4]);
        }
        __syncthreads();
        for (int k = 0; k < hf::kSlots; ++k)
          if (layout.slot_table[k] >= 0) hf::build_look(tables[k], tid, kTE);
        __syncthreads();
        const long long u = u0 + tid;
        if (u < run_end) {
          const int i = (int)(u - first[b]);
          const int code = hf::run_segment(layout, i, bytes, segments, tables, natural, coefs, sink);
          if (code) atomicMax(&status[b], hf::status_word(code, i));
        }
      }
      u0 = run_end;
    }
  }
}

}  // namespace

extern "C" long long dspn_jpeg_scan_segments(const dspn_jpeg_info *info) {
  return info ? dspn_jpeg::scan_segments(*info) : 0;
}

extern "C" int dspn_jpeg_scan_index(const unsigned char *bytes, size_t n, const dspn_jpeg_info *info, dspn_jpeg_scan *scan,
                                    unsigned int *seg_offsets, size_t seg_capacity) {
  return dspn_jpeg::scan_index(bytes, n, info, scan, seg_offsets, seg_capacity, dspn::last_error_buf(), 512) ? DSPN_ERR_ARG_ : 0;
}

extern "C" int dspn_jpeg_entropy_decode_segments(const unsigned char *bytes, long long bytes_count, const dspn_jpeg_sample *sample,
                                                 const dspn_jpeg_scan *scan, const unsigned int *segments, long long segment_count,
                                                 short *coefs, long long coef_count, int *status) {
  DSPN_REQUIRE(bytes && sample && scan && segments && coefs && status, "jpeg_entropy_decode_segments: null argument");
  DSPN_REQUIRE(bytes_count > 0 && segment_count > 0 && coef_count > 0, "jpeg_entropy_decode_segments: bad pool sizes");
  *status = dspn_jpeg_huff::decode_sample(bytes, bytes_count, *sample, *scan, segments, segment_count, coefs, coef_count);
  return 0;
}

extern "C" int dspn_jpeg_entropy_decode_batch(const unsigned char *bytes, long long bytes_count, const dspn_jpeg_sample *samples,
                                              const dspn_jpeg_scan *scans, int B, const unsigned int *segments,
                                              long long segment_count, short *coefs, long long coef_count, int *status, void *stream) {
  DSPN_REQUIRE(bytes && samples && scans && segments && coefs && status, "jpeg_entropy_decode_batch: null argument");
  DSPN_REQUIRE(B > 0 && B <= kMaxB, "jpeg_entropy_decode_batch: bad batch (0 < B <= %d)", kMaxB);
  DSPN_REQUIRE(bytes_count > 0 && segment_count > 0 && coef_count > 0 && coef_count % 64 == 0,
               "jpeg_entropy_decode_batch: bad pool sizes");
  DSPN_REQUIRE((reinterpret_cast<uintptr_t>(coefs) & 15) == 0 && (reinterpret_cast<uintptr_t>(samples) & 7) == 0 &&
                   (reinterpret_cast<uintptr_t>(scans) & 7) == 0 && (reinterpret_cast<uintptr_t>(segments) & 3) == 0 &&
                   (reinterpret_cast<uintptr_t>(status) & 3) == 0,
               "jpeg_entropy_decode_batch: coefs must be 16-byte aligned, samples and scans 8-byte, segments and status 4-byte");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const hipError_t cleared = hipMemsetAsync(status, 0, sizeof(int) * (size_t)B, s);
  if (cleared != hipSuccess) return dspn::fail(DSPN_ERR_LAUNCH_, "jpeg_entropy_decode_batch: %s", hipGetErrorString(cleared));
  const EntropyPools pl = {bytes_count, segment_count, coef_count};
  hipLaunchKernelGGL(jpeg_entropy_kernel, dim3(kGridE), dim3(kTE), 0, s, bytes, samples, scans, B, segments, pl, coefs, status);
  return dspn::check_launch("jpeg_entropy_decode_batch");
}

extern "C" int dspn_jpeg_probe(const unsigned char *bytes, size_t n, dspn_jpeg_info *info) {
  DSPN_REQUIRE(info, "jpeg_probe: null argument");
  return dspn_jpeg::probe(bytes, n, info, dspn::last_error_buf(), 512) ? DSPN_ERR_ARG_ : 0;
}

extern "C" int dspn_jpeg_entropy_decode(const unsigned char *bytes, size_t n, const dspn_jpeg_info *info, short *coef_out) {
  return dspn_jpeg::entropy_decode(bytes, n, info, coef_out, dspn::last_error_buf(), 512) ? DSPN_ERR_ARG_ : 0;
}

extern "C" size_t dspn_jpeg_reconstruct_workspace_bytes(long long coef_count) {
  return coef_count > 0 ? (size_t)coef_count : 0;
}

extern "C" int dspn_jpeg_reconstruct_batch_u8(const short *coefs, long long coef_count, const dspn_jpeg_sample *samples, int B,
                                              unsigned char *images_out, long long images_bytes, void *workspace,
                                              size_t workspace_bytes, void *stream) {
  DSPN_REQUIRE(coefs && samples && images_out && workspace, "jpeg_reconstruct: null argument");
  DSPN_REQUIRE(B > 0 && B <= kMaxB, "jpeg_reconstruct: bad batch (0 < B <= %d)", kMaxB);
  DSPN_REQUIRE(coef_count > 0 && coef_count % 64 == 0 && images_bytes > 0, "jpeg_reconstruct: bad pool sizes");
  DSPN_REQUIRE((reinterpret_cast<uintptr_t>(coefs) & 15) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(samples) & 7) == 0,
               "jpeg_reconstruct: coefs and workspace must be 16-byte aligned, samples 8-byte aligned");
  if (workspace_bytes < dspn_jpeg_reconstruct_workspace_bytes(coef_count))
    return dspn::fail(DSPN_ERR_WORKSPACE_, "jpeg_reconstruct: workspace of %zu bytes, %zu needed", workspace_bytes,
                      dspn_jpeg_reconstruct_workspace_bytes(coef_count));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const Pools pl = {coef_count, images_bytes};
  unsigned char *planes = static_cast<unsigned char *>(workspace);
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3(kGrid), dim3(kT), 0, s, coefs, samples, B, pl, planes);
  hipLaunchKernelGGL(jpeg_colour_kernel, dim3(kGrid), dim3(kT), 0, s, planes, samples, B, pl, images_out);
  return dspn::check_launch("jpeg_reconstruct");
}

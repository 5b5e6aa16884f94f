// Per-tensor statistics over a descriptor table for MI355X (gfx950); C ABI in include/dspn_monitor.h.
//
// A read-once stream bound by HBM: tensor_stats_chunk_kernel, one workgroup per chunk of kChunk logical elements, finds its
// row through the chunk prefix of the table (a binary search every lane does alike), streams the chunk and leaves one
// partial; tensor_stats_row_kernel, one wave per row, sums the row's partials.  Three ways through a chunk:
//   flat (ld == C):   a head of single elements up to the first 16-byte boundary, 16-byte loads, a tail of single elements;
//                     the chunk length is a multiple of 16 elements, so every chunk of a tensor has the head of its base
//   padded, aligned:  base and the row pitch are multiples of 16 bytes: 16-byte loads over the physical rows, the lanes at
//                     C .. ld - 1 and the ones outside the chunk masked; the vector that would reach behind the last logical
//                     element of the tensor is read element by element
//   padded, other:    element by element
// Order of the sums (the results are bit-reproducible, see the header): a lane adds its elements in the order it walks them,
// in double (a float's square is exact there, and 3e38 squared is far from its range's end); the 64 lanes of a wave go through
// a fixed xor butterfly -- a + b == b + a, so every lane ends with the same bits; the waves are added in wave order by one
// lane.  Counts are integers.  Non-finite elements are counted and kept out of the sums and of absmax; |x| is compared on
// the bit pattern, which orders non-negative floats, denormals included.
#include "dspn_common.h"
#include "../../include/dspn_monitor.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kChunk = 16384;

static_assert(sizeof(dspn_stats_row) == 40 && sizeof(dspn_stats_out) == 48, "layouts of include/dspn_monitor.h");

struct Acc {
  double ss = 0.0, s = 0.0;
  unsigned amax = 0;                 // bits of the largest finite |x|
  unsigned long long nan = 0, pinf = 0, ninf = 0;

  // a finite element, by the bits of its float32 value (d * d is exact in double, so the fused form rounds once, as the sum does)
  __device__ __forceinline__ void add_finite(unsigned u) {
    const unsigned a = u & 0x7fffffffu;
    const double d = (double)__uint_as_float(u);
    ss = __fma_rn(d, d, ss);
    s += d;
    amax = a > amax ? a : amax;
  }
  // any element
  __device__ __forceinline__ void add(unsigned u) {
    const unsigned a = u & 0x7fffffffu;
    const bool finite = a < 0x7f800000u;
    const double d = finite ? (double)__uint_as_float(u) : 0.0;
    ss = __fma_rn(d, d, ss);
    s += d;
    amax = finite && a > amax ? a : amax;
    nan += a > 0x7f800000u;
    pinf += u == 0x7f800000u;
    ninf += u == 0xff800000u;
  }
  __device__ __forceinline__ void add(const dspn_stats_out &p) {
    ss += p.sumsq;
    s += p.sum;
    const unsigned a = __float_as_uint(p.absmax);
    amax = a > amax ? a : amax;
    nan += p.n_nan;
    pinf += p.n_posinf;
    ninf += p.n_neginf;
  }
  __device__ __forceinline__ void store(dspn_stats_out *o) const {
    o->sumsq = ss;
    o->sum = s;
    o->n_nan = nan;
    o->n_posinf = pinf;
    o->n_neginf = ninf;
    o->absmax = __uint_as_float(amax);
    o->reserved = 0;
  }
};

__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int off) {
  return (unsigned long long)__double_as_longlong(__shfl_xor(__longlong_as_double((long long)v), off));
}

// the fixed butterfly over the 64 lanes of a wave; every lane ends with the wave's totals
__device__ __forceinline__ void wave_reduce(Acc &a) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double ss = __shfl_xor(a.ss, off), s = __shfl_xor(a.s, off);
    const unsigned am = (unsigned)__shfl_xor((int)a.amax, off);
    const unsigned long long n0 = shfl_xor_u64(a.nan, off), n1 = shfl_xor_u64(a.pinf, off), n2 = shfl_xor_u64(a.ninf, off);
    a.ss += ss;
    a.s += s;
    a.amax = am > a.amax ? am : a.amax;
    a.nan += n0;
    a.pinf += n1;
    a.ninf += n2;
  }
}

struct F32 {
  using T = float;
  static constexpr int kVec = 4;
  __device__ static __forceinline__ unsigned bits(const T *p) { return __float_as_uint(*p); }
  __device__ static __forceinline__ unsigned lane(const uint4 &v, int k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; }
};
struct BF16 {
  using T = unsigned short;
  static constexpr int kVec = 8;
  __device__ static __forceinline__ unsigned bits(const T *p) { return (unsigned)*p << 16; }
  __device__ static __forceinline__ unsigned lane(const uint4 &v, int k) {
    const unsigned w = (k >> 1) == 0 ? v.x : (k >> 1) == 1 ? v.y : (k >> 1) == 2 ? v.z : v.w;
    return (k & 1) ? (w & 0xffff0000u) : (w << 16);
  }
};

// a whole vector: the usual one holds finite values only and takes the short way
template <typename E>
__device__ __forceinline__ void add_vector(const uint4 &v, Acc &acc) {
  unsigned b[E::kVec];
  bool finite = true;
#pragma unroll
  for (int k = 0; k < E::kVec; ++k) {
    b[k] = E::lane(v, k);
    finite = finite && (b[k] & 0x7fffffffu) < 0x7f800000u;
  }
  if (finite) {
#pragma unroll
    for (int k = 0; k < E::kVec; ++k) acc.add_finite(b[k]);
  } else {
#pragma unroll
    for (int k = 0; k < E::kVec; ++k) acc.add(b[k]);
  }
}

// elements [e0, e0 + n) of the row's logical order, n <= kChunk
template <typename E>
__device__ __forceinline__ void accumulate(const dspn_stats_row &row, long long e0, int n, Acc &acc) {
  using T = typename E::T;
  constexpr int kVec = E::kVec;
  const T *base = static_cast<const T *>(row.base);
  const int tid = threadIdx.x;
  if (row.ld == row.C) {
    const T *p = base + e0;
    int head = (int)(((16 - (reinterpret_cast<size_t>(p) & 15)) & 15) / sizeof(T));
    head = head < n ? head : n;
    const int nvec = (n - head) / kVec;
    if (tid < head) acc.add(E::bits(p + tid));
    const uint4 *pv = reinterpret_cast<const uint4 *>(p + head);
#pragma unroll 4
    for (int i = tid; i < nvec; i += kThreads) {
      add_vector<E>(pv[i], acc);
    }
    for (int i = head + nvec * kVec + tid; i < n; i += kThreads) acc.add(E::bits(p + i));
    return;
  }
  const unsigned C = (unsigned)row.C;
  const long long ld = row.ld;
  const long long r0 = e0 / row.C;
  const unsigned c0 = (unsigned)(e0 - r0 * row.C);             // the chunk is [c0, c0 + n) counted from the start of row r0
  const unsigned end = c0 + (unsigned)n;                       // < 2^31 + kChunk
  const bool wide = reinterpret_cast<size_t>(base) % 16 == 0 && (size_t)ld * sizeof(T) % 16 == 0;
  if (!wide) {
    for (unsigned lin = c0 + tid; lin < end; lin += kThreads) {
      const unsigned rr = lin / C;
      acc.add(E::bits(base + (r0 + rr) * ld + (lin - rr * C)));
    }
    return;
  }
  // vectors of the physical rows r0 .. r0 + nr - 1, numbered row by row: from the one that holds column c0 of the first row to
  // the one that holds the last element of the last
  const long long V = ld / kVec;
  const long long nr = (end - 1) / C + 1;
  const long long vbeg = c0 / kVec, vend = (nr - 1) * V + ((end - 1) - (unsigned)(nr - 1) * C) / kVec + 1;
  const long long first = vbeg + tid;
  long long rr = first / V, vc = first - rr * V;                // this lane's vector: row r0 + rr, vector vc of it
  const long long step_r = kThreads / V, step_c = kThreads - step_r * V;
  for (long long i = first; i < vend; i += kThreads) {
    const long long col0 = vc * kVec;
    if (col0 < C) {
      const long long lin0 = rr * C + col0;                     // position of the vector's first lane, counted as c0 is
      const T *q = base + (r0 + rr) * ld + col0;
      if (col0 + kVec <= C || r0 + rr + 1 < row.rows) {
        const uint4 v = *reinterpret_cast<const uint4 *>(q);
#pragma unroll
        for (int k = 0; k < kVec; ++k)
          if (col0 + k < C && lin0 + k >= c0 && lin0 + k < end) acc.add(E::lane(v, k));
      } else {                                                  // the last row's last vector: nothing is read behind column C - 1
        for (int k = 0; k < kVec; ++k)
          if (col0 + k < C && lin0 + k >= c0 && lin0 + k < end) acc.add(E::bits(q + k));
      }
    }
    rr += step_r;
    vc += step_c;
    if (vc >= V) { vc -= V; ++rr; }
  }
}

__global__ __launch_bounds__(kThreads) void tensor_stats_chunk_kernel(const dspn_stats_row *__restrict__ table, int n_rows,
                                                                      dspn_stats_out *__restrict__ partial) {
  __shared__ dspn_stats_out wave_part[kWaves];
  const long long chunk = blockIdx.x;
  int lo = 0, hi = n_rows - 1;                                  // the last row whose first chunk is not behind this one
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (table[mid].first_chunk <= chunk) lo = mid; else hi = mid - 1;
  }
  const dspn_stats_row row = table[lo];
  const long long e0 = (chunk - row.first_chunk) * kChunk, left = row.rows * row.C - e0;
  const int n = (int)(left < kChunk ? left : kChunk);
  Acc acc;
  if (n > 0) {
    if (row.dtype == DSPN_STATS_BF16) accumulate<BF16>(row, e0, n, acc);
    else accumulate<F32>(row, e0, n, acc);
  }
  wave_reduce(acc);
  if ((threadIdx.x & 63) == 0) acc.store(&wave_part[threadIdx.x >> 6]);
  __syncthreads();
  if (threadIdx.x == 0) {
    Acc all;
    for (int w = 0; w < kWaves; ++w) all.add(wave_part[w]);
    all.store(&partial[chunk]);
  }
}

__global__ __launch_bounds__(64) void tensor_stats_row_kernel(const dspn_stats_row *__restrict__ table, int n_rows, long long n_chunks,
                                                             const dspn_stats_out *__restrict__ partial,
                                                             dspn_stats_out *__restrict__ out) {
  const int r = blockIdx.x;
  const long long c0 = table[r].first_chunk, c1 = r + 1 < n_rows ? table[r + 1].first_chunk : n_chunks;
  Acc acc;
  for (long long c = c0 + threadIdx.x; c < c1; c += 64) acc.add(partial[c]);
  wave_reduce(acc);
  if (threadIdx.x == 0) acc.store(&out[r]);
}

}  // namespace

extern "C" {

int dspn_tensor_stats_chunk_elems(void) { return kChunk; }

size_t dspn_tensor_stats_workspace_bytes(int n_rows, long long n_chunks) {
  return n_rows > 0 && n_chunks > 0 ? sizeof(dspn_stats_out) * (size_t)n_chunks : 0;
}

int dspn_tensor_stats(const dspn_stats_row *table, int n_rows, long long n_chunks, dspn_stats_out *out, void *workspace,
                      size_t workspace_bytes, void *stream) {
  DSPN_REQUIRE(n_rows > 0, "tensor_stats: n_rows must be > 0");
  DSPN_REQUIRE(n_chunks >= n_rows && n_chunks < (1LL << 31), "tensor_stats: n_chunks must be in [n_rows, 2^31): every row has a chunk");
  DSPN_REQUIRE(table && out, "tensor_stats: null pointer");
  DSPN_REQUIRE(workspace && workspace_bytes >= dspn_tensor_stats_workspace_bytes(n_rows, n_chunks),
               "tensor_stats: workspace too small (%zu bytes, %zu needed)", workspace_bytes,
               dspn_tensor_stats_workspace_bytes(n_rows, n_chunks));
  hipStream_t s = (hipStream_t)stream;
  dspn_stats_out *partial = static_cast<dspn_stats_out *>(workspace);
  hipLaunchKernelGGL(tensor_stats_chunk_kernel, dim3((unsigned)n_chunks), dim3(kThreads), 0, s, table, n_rows, partial);
  hipLaunchKernelGGL(tensor_stats_row_kernel, dim3(n_rows), dim3(64), 0, s, table, n_rows, n_chunks, partial, out);
  return dspn::check_launch("tensor_stats");
}

}  // extern "C"

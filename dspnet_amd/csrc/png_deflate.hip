// The deflate of the PNG encode on the device (gfx950); C ABI, stream format and the output bound in
// include/dspn_png_encode.h, the rules in png_deflate_host.h (token_at, plan_block, the header writers), which both this file
// and the host encoder dspn_png_deflate_host run.  Matches have distance 1 only, so a byte's token follows from its place in
// its run of equal bytes and nothing in a block is serial but the Huffman construction over its 286 counters.  The unit of
// work is a BLOCK of kBlock input bytes of one image.  The launches of dspn_png_deflate_batch, all on the caller's stream:
//   plan      workgroup per block   lane = byte: ballot(byte != the one before) is a 64-bit word of run starts, kept in LDS;
//                                   a prefix maximum / suffix minimum over the 512 words gives every word the run start in
//                                   front of it and behind it, so a byte finds its run in O(1) (find_run).  Tokens are
//                                   counted with LDS atomics, the Adler-32 partials summed by wave shuffles, the used symbols
//                                   ranked by (count, symbol) by all threads; thread 0 runs plan_block (Huffman, limiter,
//                                   header symbols, cost, mode) in LDS, the workgroup copies the 920-byte plan out.
//   scan      workgroup per image   bit offsets of the blocks behind the image's 16 header bits: a stored block rounds up to
//                                   a whole byte in the middle of the stream, so the element is "add, round up to 8, add",
//                                   which composes in closed form (Seg, as in jpeg_entropy_encode.hip); also the image's
//                                   byte count and its Adler-32 from the blocks' partials (a plain sum, adler_term).
//   place     1 workgroup           exclusive sum of the byte counts: images lie back to back in `out`; `result`
//   zero      clears out[0 .. total)
//   emit      workgroup per block   the run words again, a workgroup scan of the token bit lengths per 256 bytes, and every
//                                   token ORed into an LDS image of the block's output (at most 21 bits each).  The first
//                                   block of an image adds the two header bytes, the last one BFINAL, the padding and the
//                                   trailer.  Whole dwords are stored; the dword at either end, shared with the neighbour
//                                   block (or image), is ORed atomically into the zeroed output.
// What bounds them: plan and emit read the block one byte per lane (the input has any alignment) twice each, the second time
// from the caches; thread 0's Huffman construction (about 600 dependent LDS steps) is the longest serial stretch, while the
// other 255 threads wait.  LDS: plan 12 KiB, emit 43 KiB (three workgroups per CU).  No workgroup waits for another one.
// Every index derives from the table the host checked and from counts this file produced within the header's bound.
#include <cstdint>
#include <vector>

#include "dspn_common.h"
#include "png_deflate_host.h"
#include "../../include/dspn_png_encode.h"

static_assert(DSPN_PNG_DEFLATE_BLOCK == dspn_png_deflate::kBlock, "block size");

namespace {

using namespace dspn_png_deflate;
typedef unsigned long long u64;

constexpr int kT = 256;
constexpr int kWaves = kT / 64;
constexpr int kWords = kBlock / 64;        // run-start words of a block
constexpr int kMaxGrid = 1 << 16;          // workgroups of a launch; each walks its blocks
constexpr int kPlanDwords = (int)sizeof(BlockPlan) / 4;
// the LDS image of a block's output: up to 31 bits in front (the dword it starts in), 16 header bits, 8 * kBlock + 42 bits
// of block (include/dspn_png_encode.h), 7 bits of padding and the 32 of the trailer
constexpr int kImageWords = (31 + 16 + 8 * kBlock + 42 + 7 + 32 + 31) / 32 + 1;

// composition of "add a, then (if hs) round up to 8 and add b"
struct Seg { long long a, b; int hs; };
__device__ __forceinline__ long long up8(long long x) { return (x + 7) & ~7LL; }
__device__ __forceinline__ long long apply(const Seg &f, long long x) { return f.hs ? up8(x + f.a) + f.b : x + f.a; }
__device__ __forceinline__ Seg then(const Seg &l, const Seg &r) {      // l first
  if (!r.hs) return l.hs ? Seg{l.a, l.b + r.a, 1} : Seg{l.a + r.a, 0, 0};
  return l.hs ? Seg{l.a, up8(l.b + r.a) + r.b, 1} : Seg{l.a + r.a, r.b, 1};
}

// the table the host writes at the head of the workspace, and what the launches add behind it
struct Layout {
  long long blocks;
  size_t in_off_at, in_size_at, first_block_at, image_bytes_at, image_adler_at, start_at, plans_at, rel_at, total;
};
Layout layout_of(long long n, long long block_cap) {
  Layout l;
  l.blocks = block_cap;
  size_t at = 0;
  l.in_off_at = at;      at += 8 * (size_t)n;
  l.in_size_at = at;     at += 8 * (size_t)n;
  l.first_block_at = at; at += 8 * ((size_t)n + 1);
  l.image_bytes_at = at; at += 8 * (size_t)n;
  l.image_adler_at = at; at += 8 * (size_t)n;
  l.start_at = at;       at += 8 * ((size_t)n + 1);
  l.plans_at = at;       at += sizeof(BlockPlan) * (size_t)block_cap;
  l.rel_at = at;         at += 8 * (size_t)block_cap;
  l.total = at;
  return l;
}

struct Table {
  const long long *in_off, *in_size, *first_block;
  int n;
};

// largest i in [0, n) with first[i] <= u (u < first[n])
__device__ __forceinline__ int find_image(const long long *first, int n, long long u) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (first[mid] <= u) lo = mid; else hi = mid;
  }
  return lo;
}

struct Block { const unsigned char *data; int bytes, image; long long index; bool last; };
__device__ __forceinline__ Block locate(const Table &t, const unsigned char *in, long long blk) {
  Block b;
  b.image = find_image(t.first_block, t.n, blk);
  b.index = blk - t.first_block[b.image];
  const long long size = t.in_size[b.image], at = b.index * kBlock;
  b.bytes = (int)(size - at < kBlock ? size - at : kBlock);
  b.data = in + t.in_off[b.image] + at;
  b.last = at + b.bytes == size;
  return b;
}

// inclusive scan over the workgroup; lds[0 .. kT - 1] holds the results until the next call
template <typename V, typename Op>
__device__ __forceinline__ V block_incl_scan(V v, V *lds, Op op) {
  __syncthreads();
  lds[threadIdx.x] = v;
  __syncthreads();
  for (int d = 1; d < kT; d <<= 1) {
    if ((int)threadIdx.x >= d) v = op(lds[threadIdx.x - d], v);
    __syncthreads();
    lds[threadIdx.x] = v;
    __syncthreads();
  }
  return v;
}

template <typename V>
__device__ __forceinline__ V wave_sum(V x) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d);
  return x;
}

// the runs of a block: a bit per byte that starts one (and per position behind the block), the last start in front of every
// word and the first one behind it
struct Runs {
  u64 mask[kWords];
  int before[kWords + 1];                  // [w]: the last start below 64 w ([0] unused: byte 0 starts a run)
  int behind[kWords + 1];                  // [w]: the first start at or above 64 w; [kWords] = kBlock
};

// fills r for the block; also the Adler-32 partials of this thread's bytes.  Ends with a barrier.
__device__ void find_runs(const Block &b, Runs &r, unsigned &sum1, u64 &sum2) {
  const int tid = threadIdx.x, lane = tid & 63, trips = (b.bytes + kT - 1) / kT;      // the same trips for every thread
  sum1 = 0;
  sum2 = 0;
  for (int w = trips * kWaves + tid; w < kWords; w += kT) r.mask[w] = ~0ULL;
  for (int it = 0; it < trips; ++it) {
    const int i = it * kT + tid;
    const bool valid = i < b.bytes;
    const int c = valid ? b.data[i] : 0;
    int prev = __shfl_up(c, 1);
    if (lane == 0) prev = (valid && i > 0) ? b.data[i - 1] : -1;
    const u64 m = __ballot(!valid || c != prev);
    if (lane == 0) r.mask[i >> 6] = m;
    if (valid) { sum1 += (unsigned)c; sum2 += (u64)(b.bytes - i) * (unsigned)c; }
  }
  __syncthreads();
  // inclusive prefix maximum of the last start inside a word, suffix minimum of the first: two words per thread
  for (int w = tid; w < kWords; w += kT) {
    const u64 m = r.mask[w];
    r.before[w + 1] = m ? 64 * w + 63 - __clzll((long long)m) : -1;
    r.behind[w] = m ? 64 * w + __ffsll((long long)m) - 1 : kBlock;
  }
  if (tid == 0) { r.before[0] = -1; r.behind[kWords] = kBlock; }
  __syncthreads();
  for (int d = 1; d < kWords; d <<= 1) {
    int up[2], down[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int w = tid + k * kT;
      up[k] = w >= d ? r.before[w + 1 - d] : -1;
      down[k] = w + d < kWords ? r.behind[w + d] : kBlock;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int w = tid + k * kT;
      if (up[k] > r.before[w + 1]) r.before[w + 1] = up[k];
      if (down[k] < r.behind[w]) r.behind[w] = down[k];
    }
    __syncthreads();
  }
}

// byte i's place j in its run and the run's length r (i < bytes)
__device__ __forceinline__ void find_run(const Runs &r, int bytes, int i, int &j, int &len) {
  const int w = i >> 6, l = i & 63;
  const u64 m = r.mask[w], upto = (2ULL << l) - 1ULL, below = m & upto, above = m & ~upto;
  const int s = below ? 64 * w + 63 - __clzll((long long)below) : r.before[w];
  int e = above ? 64 * w + __ffsll((long long)above) - 1 : r.behind[w + 1];
  if (e > bytes) e = bytes;
  j = i - s;
  len = e - s;
}

__global__ __launch_bounds__(kT) void png_deflate_plan_kernel(Table t, long long blocks, const unsigned char *__restrict__ in,
                                                              BlockPlan *__restrict__ plans) {
  __shared__ Runs runs;
  __shared__ unsigned hist[kLitLen + 2];
  __shared__ Work work;
  __shared__ BlockPlan plan;
  __shared__ u64 red[kWaves][2];
  __shared__ int used;
  const int tid = threadIdx.x;
  for (long long blk = blockIdx.x; blk < blocks; blk += gridDim.x) {
    const Block b = locate(t, in, blk);
    unsigned sum1;
    u64 sum2;
    for (int s = tid; s < kLitLen + 2; s += kT) hist[s] = s == kEob ? 1u : 0u;
    if (tid == 0) used = 0;
    find_runs(b, runs, sum1, sum2);
    const u64 s1 = wave_sum((u64)sum1), s2 = wave_sum(sum2);
    if ((tid & 63) == 0) { red[tid >> 6][0] = s1; red[tid >> 6][1] = s2; }
    for (int i = tid; i < b.bytes; i += kT) {
      int j, len;
      find_run(runs, b.bytes, i, j, len);
      const Token tok = token_at(b.data[i], j, len);
      if (tok.sym >= 0) atomicAdd(&hist[tok.sym], 1u);
    }
    __syncthreads();
    for (int s = tid; s < kLitLen; s += kT) {                      // rank by (count, symbol): sort_symbols' order
      const unsigned c = hist[s];
      if (!c) continue;
      int rank = 0;
      for (int o = 0; o < kLitLen; ++o) {
        const unsigned co = hist[o];
        rank += (co != 0 && (co < c || (co == c && o < s))) ? 1 : 0;
      }
      work.order[rank] = (unsigned short)s;
      atomicAdd(&used, 1);
    }
    __syncthreads();
    if (tid == 0) {
      plan_block(hist, b.bytes, used, work, plan);
      u64 a1 = 0, a2 = 0;
      for (int w = 0; w < kWaves; ++w) { a1 += red[w][0]; a2 += red[w][1]; }
      plan.sum1 = (unsigned)a1;
      plan.sum2 = a2;
      plan.reserved = 0;
    }
    __syncthreads();
    const unsigned *src = reinterpret_cast<const unsigned *>(&plan);
    unsigned *dst = reinterpret_cast<unsigned *>(plans + blk);
    for (int k = tid; k < kPlanDwords; k += kT) dst[k] = src[k];
    __syncthreads();                                               // LDS is the next block's
  }
}

// one workgroup per image at a time
__global__ __launch_bounds__(kT) void png_deflate_scan_kernel(Table t, const BlockPlan *__restrict__ plans, long long *__restrict__ rel,
                                                              long long *__restrict__ image_bytes, unsigned *__restrict__ image_adler) {
  __shared__ Seg lds[kT];
  __shared__ u64 sums[kT];
  const int tid = threadIdx.x;
  for (int im = blockIdx.x; im < t.n; im += gridDim.x) {
    const long long first = t.first_block[im], nb = t.first_block[im + 1] - first, size = t.in_size[im];
    long long carry = 16;                                          // the two header bytes
    u64 a = 0, bsum = 0;
    for (long long base = 0; base < nb; base += kT) {
      const long long k = base + tid;
      Seg f = {0, 0, 0};
      if (k < nb) {
        const BlockPlan &p = plans[first + k];
        const long long at = k * kBlock, bytes = size - at < kBlock ? size - at : kBlock;
        f = p.mode == kModeStored ? Seg{3, 32 + 8 * bytes, 1} : Seg{(long long)p.bits, 0, 0};
        a += p.sum1;
        bsum += adler_term(p.sum1, p.sum2, size - at - bytes);
      }
      block_incl_scan(f, lds, [](const Seg &l, const Seg &r) { return then(l, r); });
      if (k < nb) rel[first + k] = tid ? apply(lds[tid - 1], carry) : carry;
      carry = apply(lds[kT - 1], carry);
    }
    const u64 ta = block_incl_scan(a % kAdlerMod, sums, [](u64 x, u64 y) { return x + y; });
    const u64 tb = block_incl_scan(bsum, sums, [](u64 x, u64 y) { return x + y; });
    if (tid == kT - 1) {
      image_bytes[im] = (up8(carry) >> 3) + 4;
      image_adler[2 * im] = (unsigned)((tb + (u64)(size % kAdlerMod)) % kAdlerMod) << 16 | (unsigned)((ta + 1) % kAdlerMod);
    }
    __syncthreads();
  }
}

// one workgroup: where every image starts in `out`
__global__ __launch_bounds__(kT) void png_deflate_place_kernel(int n, const long long *__restrict__ image_bytes, long long *__restrict__ start,
                                                               long long *__restrict__ result) {
  __shared__ long long lds[kT];
  long long carry = 0;
  for (int base = 0; base <= n; base += kT) {
    const int i = base + threadIdx.x;
    const long long own = i < n ? image_bytes[i] : 0;
    const long long incl = block_incl_scan(own, lds, [](long long x, long long y) { return x + y; });
    if (i <= n) start[i] = carry + incl - own;
    if (i < n) { result[2 * i] = carry + incl - own; result[2 * i + 1] = own; }
    carry += lds[kT - 1];
  }
}

__global__ __launch_bounds__(kT) void png_deflate_zero_kernel(const long long *__restrict__ total_at, unsigned char *__restrict__ out) {
  const long long total = *total_at;
  const long long head = (long long)(-reinterpret_cast<uintptr_t>(out) & 15) < total ? (long long)(-reinterpret_cast<uintptr_t>(out) & 15) : total;
  const long long quads = (total - head) / 16, tail = head + 16 * quads;
  const long long gid = (long long)blockIdx.x * kT + threadIdx.x, step = (long long)gridDim.x * kT;
  if (gid < head) out[gid] = 0;
  if (gid < total - tail) out[tail + gid] = 0;                     // fewer than 16 bytes each
  uint4 *q = reinterpret_cast<uint4 *>(out + head);
  for (long long i = gid; i < quads; i += step) q[i] = make_uint4(0, 0, 0, 0);
}

struct LdsSink {
  unsigned *words;
  __device__ __forceinline__ void put(long long pos, unsigned v, int len) {
    (void)len;
    const u64 x = (u64)v << (pos & 31);
    if ((unsigned)x) atomicOr(&words[pos >> 5], (unsigned)x);
    if (x >> 32) atomicOr(&words[(pos >> 5) + 1], (unsigned)(x >> 32));
  }
};

// out_al: `out` rounded down to a dword, shift = 8 * (out & 3): bit positions count from out_al
__global__ __launch_bounds__(kT) void png_deflate_emit_kernel(Table t, long long blocks, const unsigned char *__restrict__ in,
                                                              const BlockPlan *__restrict__ plans, const long long *__restrict__ rel,
                                                              const long long *__restrict__ start, const unsigned *__restrict__ image_adler,
                                                              unsigned *__restrict__ out_al, int shift) {
  __shared__ Runs runs;
  __shared__ unsigned image[kImageWords];
  __shared__ BlockPlan plan;
  __shared__ unsigned short codes[kLitLen + 2], cl_codes[kClen + 1], next[16];
  __shared__ int wave_total[kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (long long blk = blockIdx.x; blk < blocks; blk += gridDim.x) {
    const Block b = locate(t, in, blk);
    {
      const unsigned *src = reinterpret_cast<const unsigned *>(plans + blk);
      unsigned *dst = reinterpret_cast<unsigned *>(&plan);
      for (int k = tid; k < kPlanDwords; k += kT) dst[k] = src[k];
    }
    for (int k = tid; k < kImageWords; k += kT) image[k] = 0;
    unsigned s1;
    u64 s2;
    find_runs(b, runs, s1, s2);                                    // ends with a barrier: plan and image are ready too
    const bool stored = plan.mode == kModeStored;
    // absolute bit positions from out_al; the image's word 0 is the dword the block's first bit falls in
    const long long at = 8 * start[b.image] + shift + rel[blk], from = b.index == 0 ? at - 16 : at;
    const long long word0 = from >> 5, origin = word0 << 5;
    LdsSink sink{image};
    if (tid == 0) {
      if (b.index == 0) sink.put(from - origin, 0x0178u, 16);      // 78 01: deflate, 32 KiB window, no dictionary
      if (!stored) {
        build_codes(plan.cl_len, kClen, next, cl_codes);
        build_codes(plan.ll_len, kLitLen, next, codes);
        put_dynamic_header(sink, at - origin, plan, cl_codes, b.last);
      } else {
        put_stored_header(sink, at - origin, b.bytes, b.last);
      }
    }
    __syncthreads();
    long long end;                                                 // the position behind the block
    if (stored) {
      end = stored_end(at, b.bytes);
      const long long first = end - 8LL * b.bytes - origin;
      for (int i = tid; i < b.bytes; i += kT) sink.put(first + 8LL * i, b.data[i], 8);
    } else {
      end = at + plan.bits;
      long long pos = at + plan.header_bits - origin;
      const int trips = (b.bytes + kT - 1) / kT;
      for (int it = 0; it < trips; ++it) {
        const int i = it * kT + tid;
        unsigned v = 0;
        int len = 0;
        if (i < b.bytes) {
          int j, r;
          find_run(runs, b.bytes, i, j, r);
          const Token tok = token_at(b.data[i], j, r);
          if (tok.sym >= 0) token_bits(tok, codes, plan.ll_len, v, len);
        }
        int incl = len;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const int y = __shfl_up(incl, d);
          if (lane >= d) incl += y;
        }
        if (lane == 63) wave_total[wave] = incl;
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) { before += w < wave ? wave_total[w] : 0; all += wave_total[w]; }
        if (len) sink.put(pos + before + incl - len, v, len);
        pos += all;
        __syncthreads();                                           // wave_total is the next trip's
      }
      if (tid == 0) sink.put(pos, codes[kEob], plan.ll_len[kEob]);
    }
    if (b.last) {                                                  // zeros up to a whole byte, then the Adler-32, big-endian
      end = up8(end - shift) + shift;                              // whole bytes count from `out`, and shift is a multiple of 8
      if (tid == 0) sink.put(end - origin, __builtin_bswap32(image_adler[2 * b.image]), 32);
      end += 32;
    }
    __syncthreads();
    const int words = (int)((end - origin + 31) >> 5);
    for (int k = tid; k < words; k += kT) {
      const unsigned w = image[k];
      const bool whole = (k > 0 || (from & 31) == 0) && (k < words - 1 || (end & 31) == 0);     // no neighbour's bit in it
      if (whole) out_al[word0 + k] = w;
      else if (w) atomicOr(&out_al[word0 + k], w);
    }
    __syncthreads();                                               // LDS is the next block's
  }
}

long long blocks_of(long long bytes) { return (bytes + kBlock - 1) / kBlock; }

}  // namespace

extern "C" long long dspn_png_deflate_bound(long long bytes) { return bytes >= 1 ? dspn_png_deflate::bound(bytes) : 0; }

extern "C" size_t dspn_png_deflate_workspace_bytes(int n, long long total_bytes) {
  if (n < 1 || total_bytes < n) return 0;
  return dspn::align_up(layout_of(n, total_bytes / kBlock + n).total, 8);
}

extern "C" int dspn_png_deflate_code_lengths(const unsigned *counts, int n, int limit, unsigned char *lengths) {
  DSPN_REQUIRE(counts && lengths, "png_deflate_code_lengths: null argument");
  DSPN_REQUIRE(n >= 1 && n <= kLitLen && limit >= 1 && limit <= 15, "png_deflate_code_lengths: 1 <= n <= %d and 1 <= limit <= 15, got n %d, limit %d",
               kLitLen, n, limit);
  unsigned long long sum = 0;
  int used = 0;
  for (int s = 0; s < n; ++s) { sum += counts[s]; used += counts[s] != 0; }
  DSPN_REQUIRE(sum <= 0xFFFFFFFFULL, "png_deflate_code_lengths: the counts must sum to less than 2^32");
  DSPN_REQUIRE(used <= (1 << limit), "png_deflate_code_lengths: %d used symbols do not fit codes of %d bits", used, limit);
  Work w;
  code_lengths_sorted(counts, n, limit, sort_symbols(counts, n, w.order), w, lengths);
  return 0;
}

extern "C" int dspn_png_deflate_host(const unsigned char *data, long long bytes, unsigned char *out, long long out_bytes, long long *length) {
  DSPN_REQUIRE(data && out && length, "png_deflate_host: null argument");
  DSPN_REQUIRE(bytes >= 1, "png_deflate_host: a stream of %lld bytes", bytes);
  DSPN_REQUIRE(out_bytes >= dspn_png_deflate::bound(bytes), "png_deflate_host: out_bytes %lld below the bound %lld", out_bytes,
               dspn_png_deflate::bound(bytes));
  *length = deflate_stream(data, bytes, out);
  if (*length < 0) return dspn::fail(DSPN_ERR_LAUNCH_, "png_deflate_host: the block plan and the writer disagree");
  return 0;
}

extern "C" int dspn_png_deflate_batch(const long long *in_offsets, const long long *in_sizes, int n, const unsigned char *in,
                                      long long in_bytes, unsigned char *out, long long out_bytes, long long *result, void *workspace,
                                      size_t workspace_bytes, void *stream) {
  DSPN_REQUIRE(n >= 0, "png_deflate: negative count (n %d)", n);
  if (n == 0) return 0;
  DSPN_REQUIRE(in_offsets && in_sizes && in && out && result && workspace, "png_deflate: null argument");
  DSPN_REQUIRE(in_bytes > 0 && out_bytes > 0, "png_deflate: empty pool (in_bytes %lld, out_bytes %lld)", in_bytes, out_bytes);
  DSPN_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0 && (reinterpret_cast<uintptr_t>(result) & 7) == 0,
               "png_deflate: workspace and result must be 8-byte aligned");
  long long total = 0, blocks = 0, bounds = 0;
  for (int i = 0; i < n; ++i) {
    const long long off = in_offsets[i], size = in_sizes[i];
    DSPN_REQUIRE(size >= 1, "png_deflate: image %d: a stream of %lld bytes", i, size);
    DSPN_REQUIRE(off >= 0 && size <= in_bytes && off <= in_bytes - size, "png_deflate: image %d: %lld bytes from offset %lld run past in_bytes %lld",
                 i, size, off, in_bytes);
    total += size;
    DSPN_REQUIRE(total <= (1LL << 56), "png_deflate: more than 2^56 bytes in one batch");
    blocks += blocks_of(size);
    bounds += dspn_png_deflate::bound(size);
  }
  DSPN_REQUIRE(out_bytes >= bounds, "png_deflate: out_bytes %lld below the sum of the bounds %lld", out_bytes, bounds);
  const Layout l = layout_of(n, total / kBlock + n);               // blocks <= total / kBlock + n
  const size_t need = dspn::align_up(l.total, 8);
  if (workspace_bytes < need) return dspn::fail(DSPN_ERR_WORKSPACE_, "png_deflate: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  std::vector<long long> table(3 * (size_t)n + 1);
  for (int i = 0, first = 0; i < n; ++i) {
    table[i] = in_offsets[i];
    table[n + i] = in_sizes[i];
    table[2 * (size_t)n + i] = i ? table[2 * (size_t)n + i - 1] + blocks_of(in_sizes[i - 1]) : first;
  }
  table[3 * (size_t)n] = blocks;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const hipError_t e = hipMemcpyWithStream(workspace, table.data(), table.size() * 8, hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return dspn::fail(DSPN_ERR_LAUNCH_, "png_deflate: copy of the image table: %s", hipGetErrorString(e));
  char *ws = static_cast<char *>(workspace);
  const Table t = {reinterpret_cast<const long long *>(ws + l.in_off_at), reinterpret_cast<const long long *>(ws + l.in_size_at),
                   reinterpret_cast<const long long *>(ws + l.first_block_at), n};
  long long *image_bytes = reinterpret_cast<long long *>(ws + l.image_bytes_at), *start = reinterpret_cast<long long *>(ws + l.start_at);
  unsigned *image_adler = reinterpret_cast<unsigned *>(ws + l.image_adler_at);
  BlockPlan *plans = reinterpret_cast<BlockPlan *>(ws + l.plans_at);
  long long *rel = reinterpret_cast<long long *>(ws + l.rel_at);
  const int block_grid = (int)std::min<long long>(blocks, kMaxGrid), image_grid = std::min(n, kMaxGrid);
  const int zero_grid = (int)std::min<long long>(kMaxGrid, (bounds / 16 + kT) / kT);
  const int shift = 8 * (int)(reinterpret_cast<uintptr_t>(out) & 3);
  unsigned *out_al = reinterpret_cast<unsigned *>(out - (reinterpret_cast<uintptr_t>(out) & 3));
  hipLaunchKernelGGL(png_deflate_plan_kernel, dim3(block_grid), dim3(kT), 0, st, t, blocks, in, plans);
  hipLaunchKernelGGL(png_deflate_scan_kernel, dim3(image_grid), dim3(kT), 0, st, t, plans, rel, image_bytes, image_adler);
  hipLaunchKernelGGL(png_deflate_place_kernel, dim3(1), dim3(kT), 0, st, n, image_bytes, start, result);
  hipLaunchKernelGGL(png_deflate_zero_kernel, dim3(zero_grid), dim3(kT), 0, st, start + n, out);
  hipLaunchKernelGGL(png_deflate_emit_kernel, dim3(block_grid), dim3(kT), 0, st, t, blocks, in, plans, rel, start, image_adler, out_al, shift);
  return dspn::check_launch("png_deflate");
}

// The entropy pass of the JPEG encode on the device (gfx950); C ABI and the workspace bound in include/dspn_jpeg_encode.h, the
// rules in jpeg_encode_host.h (encode_block, Out::put_bits, flush_ones, the MCU loop of entropy_encode), whose Annex K tables
// this file turns into code tables at compile time (kTables).  Only the bit position is serial in encoding, so the unit of
// work is a SLOT: one block of the MCU-interleaved scan, real or dummy.  A SEGMENT is one restart interval, or the whole
// image when there is none.  The launches of dspn_jpeg_entropy_encode_scan_batch, all on the caller's stream:
//   setup     1 workgroup     validates the descriptors, gives every image its run of slots (first_slot), refuses what the
//                             workspace cannot hold
//   count     wave per slot   lane = zigzag position.  ballot(v != 0) is the block's non-zero mask, a lane's run the distance
//                             to the set bit below it; a lane's share is at most 3 ZRL + one code + 10 value bits (59 bits),
//                             lane 0's the DC difference, lane 63's the EOB when coefficient 63 is zero.  A wave sum gives the
//                             slot's bit count; bit 31 marks the first slot of a segment, bit 30 one that follows a marker.
//   scan      3 launches      exclusive sum of the bit counts in which every segment starts on a whole byte: tiles of
//                             kScanTile slots are reduced, one workgroup scans the tile sums, the tiles are swept.  The
//                             element "x -> round x up to 8 (if a segment starts), then + bits" composes in closed form (Seg).
//                             This lays the segments back to back in the unstuffed stream: offs[slot] in bits, stream_bytes.
//   zero      the stream and the marker flags (one bit per stream byte), up to the next kChunk bytes
//   emit      wave per slot   the count's shares again, a wave scan for the offsets inside the block; the lanes OR their
//                             shares into kBlockWords words of LDS, the wave stores the words it owns whole and ORs the (at
//                             most two) it shares with its neighbours atomically.  The last slot of a segment adds the 1 bits.
//   ffcount   wave per chunk  lane = 16 bytes: FF bytes and marker flags per kChunk bytes, packed in one 64-bit count
//   chunkscan 1 workgroup     exclusive sum of those counts
//   finalize  1 workgroup     per image: the counts in front of its first byte (chunk sum + the partial chunk), and from the
//                             differences its exact size: bytes + FFs + 2 per marker
// and dspn_jpeg_entropy_encode_write_batch is one launch: lane = 16 bytes again, a wave scan of the counts gives every byte
// its final place; the lane writes its bytes, a zero after every FF and FF Dn in front of a flagged byte.
// Nothing about the batch is known on the host (the descriptors live in device memory), so every grid is fixed and strides
// over work it reads from the header; every index derives from descriptors setup has validated and from counts this file
// produced itself, within the bound the header states.
#include <cstdint>

#include "dspn_common.h"
#include "jpeg_encode_host.h"
#include "jpeg_encode_sample.h"

namespace {

using dspn_jpeg_enc::Codes;
typedef unsigned long long u64;

constexpr int kT = 256;
constexpr int kWaves = kT / 64;            // slots (count, emit) or chunks (ffcount, write) per workgroup and trip
constexpr int kMaxB = 1024;
constexpr int kGrid = 2048;
constexpr int kScanPer = 4;                // slots per thread in the scan
constexpr int kScanTile = kT * kScanPer;   // 1024 slots
constexpr int kChunk = 64 * 16;            // 1024 bytes of the unstuffed stream per wave in the stuffing pass
constexpr int kRealBytes = 209, kDummyBytes = 5;     // include/dspn_jpeg_encode.h derives them
constexpr int kBlockWords = 56;            // 31 bits of offset + 1660 + 7 bits of padding = 54 words
constexpr unsigned kStart = 1u << 31, kMarker = 1u << 30, kBitsMask = 0xFFFFu;
constexpr unsigned kMagic = 0x4a454e43u;
constexpr long long kMaxCoefs = 1LL << 30; // keeps the stream below 2^32 bytes: its FF count fits the packed 32 bits
constexpr long long kNoWrite = INT64_MIN;

struct Tables {
  unsigned ac[2][256];                     // code | size << 16, by symbol; [0] luminance, [1] chrominance
  unsigned dc[2][16];                      // by the number of bits of the difference
  unsigned natural[64];                    // zigzag position -> natural index
};

constexpr Tables make_tables() {
  using namespace dspn_jpeg_enc;
  Tables t{};
  const unsigned char *bits[4] = {kDcLumBits, kDcChrBits, kAcLumBits, kAcChrBits};
  const unsigned char *vals[4] = {kDcVals, kDcVals, kAcLumVals, kAcChrVals};
  for (int k = 0; k < 4; ++k) {
    Codes c{};
    build_codes(c, bits[k], vals[k]);
    for (int i = 0; i < (k < 2 ? 16 : 256); ++i) (k < 2 ? t.dc[k] : t.ac[k - 2])[i] = c.code[i] | (unsigned)c.size[i] << 16;
  }
  for (int i = 0; i < 64; ++i) t.natural[i] = dspn_jpeg::kNatural[i];
  return t;
}
__constant__ Tables kTables = make_tables();

// the head of the workspace: what setup, the scans and finalize leave for the launches behind them
struct Header {
  unsigned magic;
  int B;
  long long coef_count;                    // what the layout of the workspace follows from
  long long slots;                         // of the batch
  long long stream_bytes;                  // of the unstuffed stream
  long long first_slot[kMaxB + 1];
  long long first_byte[kMaxB + 1];         // of the image in the unstuffed stream
  u64 before[kMaxB + 1];                   // FF bytes (low half) and marker flags (high half) in front of first_byte
  long long scan_bytes[kMaxB];
  int status[kMaxB];
  int interval[kMaxB];
};

struct Layout {
  long long blocks, slot_cap, stream_cap, tile_cap, chunk_cap;
  size_t bits_at, offs_at, agg_at, tile_at, stream_at, flags_at, chunks_at, total;
};

// composition of "round up to 8 if a segment starts, then add": F(x) = hs ? up8(x + a) + b : x + a
struct Seg { long long a, b; int hs; };
__device__ __forceinline__ long long up8(long long x) { return (x + 7) & ~7LL; }
__device__ __forceinline__ long long apply(const Seg &f, long long x) { return f.hs ? up8(x + f.a) + f.b : x + f.a; }
__device__ __forceinline__ Seg then(const Seg &l, const Seg &r) {      // l first
  if (!r.hs) return l.hs ? Seg{l.a, l.b + r.a, 1} : Seg{l.a + r.a, 0, 0};
  return l.hs ? Seg{l.a, up8(l.b + r.a) + r.b, 1} : Seg{l.a + r.a, r.b, 1};
}
__device__ __forceinline__ Seg element(unsigned e) { return (e & kStart) ? Seg{0, (long long)(e & kBitsMask), 1} : Seg{(long long)(e & kBitsMask), 0, 0}; }

Layout layout_of(long long coef_count) {
  Layout l;
  l.blocks = coef_count / 64;
  l.slot_cap = 4 * l.blocks;
  l.stream_cap = (long long)dspn::align_up((size_t)((kRealBytes + 3 * kDummyBytes) * l.blocks), kChunk);
  l.tile_cap = (l.slot_cap + kScanTile - 1) / kScanTile;
  l.chunk_cap = l.stream_cap / kChunk;
  size_t at = dspn::align_up(sizeof(Header), 256);
  l.bits_at = at;   at = dspn::align_up(at + 4 * (size_t)l.slot_cap, 256);
  l.offs_at = at;   at = dspn::align_up(at + 8 * (size_t)l.slot_cap, 256);
  l.agg_at = at;    at = dspn::align_up(at + sizeof(Seg) * (size_t)l.tile_cap, 256);
  l.tile_at = at;   at = dspn::align_up(at + 8 * (size_t)l.tile_cap, 256);
  l.stream_at = at; at = dspn::align_up(at + (size_t)l.stream_cap, 256);
  l.flags_at = at;  at = dspn::align_up(at + (size_t)l.stream_cap / 8, 256);
  l.chunks_at = at; at = dspn::align_up(at + 8 * (size_t)(l.chunk_cap + 1), 256);
  l.total = at;
  return l;
}

// largest b in [0, B) with first[b] <= u (u < first[B])
__device__ __forceinline__ int find_image(const long long *first, int B, long long u) {
  int lo = 0, hi = B;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (first[mid] <= u) lo = mid; else hi = mid;
  }
  return lo;
}

template <typename V>
__device__ __forceinline__ V wave_incl_sum(V x, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const V y = __shfl_up(x, d);
    if (lane >= d) x += y;
  }
  return x;
}

// inclusive scan over the workgroup; lds[0 .. kT - 1] holds the results until the next call
template <typename V, typename Op>
__device__ __forceinline__ V block_incl_scan(V v, V *lds, Op op) {
  __syncthreads();                                          // readers of the previous call's results are done
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

__device__ __forceinline__ int mcus_across(const dspn_jpeg_enc_sample &s) {
  const int hs = s.ncomp == 3 ? s.hsamp : 1;
  return (s.width + 8 * hs - 1) / (8 * hs);
}

__global__ __launch_bounds__(kT) void jpeg_ent_setup_kernel(const dspn_jpeg_enc_sample *__restrict__ samples,
                                                            const int *__restrict__ intervals, int B, long long coef_count,
                                                            long long slot_cap, long long real_cap, Header *__restrict__ h) {
  __shared__ long long slots[kMaxB], reals[kMaxB];
  for (int b = threadIdx.x; b < B; b += kT) {
    const dspn_jpeg_enc_sample &s = samples[b];
    const int ri = intervals[b];
    int hs, vs;
    const bool ok = dspn_jpeg_enc::coefs_ok(s, coef_count, hs, vs) && ri >= 0 && ri <= 65535;
    long long n = 0, r = 0;
    if (ok) {
      const long long mcus = (long long)mcus_across(s) * ((s.height + 8 * vs - 1) / (8 * vs));
      n = mcus * (s.ncomp == 3 ? hs * vs + 2 : 1);
      for (int c = 0; c < s.ncomp; ++c) r += (long long)s.blocks_w[c] * s.blocks_h[c];
    }
    slots[b] = n;
    reals[b] = r;
    h->interval[b] = ok ? ri : 0;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    long long acc = 0, racc = 0;
    for (int b = 0; b < B; ++b) {
      h->first_slot[b] = acc;
      // descriptors may overlap: what the workspace was not sized for is refused like an untrusted sample
      const bool fits = slots[b] > 0 && acc + slots[b] <= slot_cap && racc + reals[b] <= real_cap;
      h->status[b] = fits ? 0 : 1;
      if (fits) { acc += slots[b]; racc += reals[b]; }
    }
    h->first_slot[B] = acc;
    h->slots = acc;
    h->B = B;
    h->coef_count = coef_count;
    h->magic = kMagic;
  }
}

// one slot of the scan, as the MCU loop of entropy_encode meets it
struct Slot {
  const short *blk;                        // nullptr: a dummy block
  int dc, pred, table;
  bool start, marker;                      // the first slot of a segment; of one that follows a marker
};

__device__ Slot locate(const dspn_jpeg_enc_sample &s, int ri, long long t, const short *__restrict__ coefs) {
  const bool colour = s.ncomp == 3;
  const int hs = colour ? s.hsamp : 1, vs = colour ? s.vsamp : 1, nl = hs * vs, per_mcu = colour ? nl + 2 : 1;
  const long long mcu = t / per_mcu;
  const int j = (int)(t - mcu * per_mcu);
  const int mcux = mcus_across(s);
  const int c = j < nl ? 0 : j - nl + 1, q = c ? 0 : j, ch = c ? 1 : hs, cv = c ? 1 : vs;
  const int bw = s.blocks_w[c], bh = s.blocks_h[c];
  const short *plane = coefs + s.coef_offset[c];
  // the block at place q (or the last real one before it) of this component in MCU m; place 0 is always real
  auto block_at = [&](long long m, int place) {
    const int my = (int)(m / mcux), mx = (int)(m - (long long)my * mcux);
    for (;; --place) {
      const int by = my * cv + place / ch, bx = mx * ch + place % ch;
      if (place == 0 || (by < bh && bx < bw)) return plane + 64 * ((long long)by * bw + bx);
    }
  };
  Slot sl;
  const int my = (int)(mcu / mcux), mx = (int)(mcu - (long long)my * mcux);
  const bool real = my * cv + q / ch < bh && mx * ch + q % ch < bw;
  const short *at = block_at(mcu, q);
  sl.blk = real ? at : nullptr;
  sl.dc = at[0];
  const bool first = ri ? mcu % ri == 0 : mcu == 0;
  sl.pred = q > 0 ? block_at(mcu, q - 1)[0] : (first ? 0 : block_at(mcu - 1, ch * cv - 1)[0]);
  sl.table = c ? 1 : 0;
  sl.start = first && j == 0;
  sl.marker = sl.start && mcu > 0;
  return sl;
}

struct LdsTables { unsigned ac[2][256], dc[2][16], natural[64]; };

__device__ void load_tables(LdsTables &t) {
  for (int i = threadIdx.x; i < 512; i += kT) t.ac[i >> 8][i & 255] = kTables.ac[i >> 8][i & 255];
  if (threadIdx.x < 32) t.dc[threadIdx.x >> 4][threadIdx.x & 15] = kTables.dc[threadIdx.x >> 4][threadIdx.x & 15];
  if (threadIdx.x < 64) t.natural[threadIdx.x] = kTables.natural[threadIdx.x];
}

// the bits lane `lane` contributes to the slot (MSB first in the low `len` bits); over: a value baseline coding cannot carry
// (coded as a zero, so that the count stays within the bound; the image is refused)
__device__ __forceinline__ void lane_share(const LdsTables &T, const Slot &sl, int lane, u64 &bits, int &len, bool &over) {
  int v = (sl.blk && lane) ? sl.blk[T.natural[lane]] : 0;
  const int m = v < 0 ? -v : v, nb = 32 - __clz(m);
  over = nb > 10;
  const bool nz = v != 0 && !over;
  const u64 mask = __ballot(nz);
  const unsigned *ac = T.ac[sl.table];
  bits = 0;
  len = 0;
  if (lane == 0) {
    int d = sl.dc - sl.pred;
    const int md = d < 0 ? -d : d;
    int nd = 32 - __clz(md);
    over = nd > 11;
    if (over) { d = 0; nd = 0; }
    const unsigned e = T.dc[sl.table][nd];
    bits = ((u64)(e & 0xFFFFu) << nd) | ((unsigned)(d < 0 ? d - 1 : d) & ((1u << nd) - 1u));
    len = (int)(e >> 16) + nd;
  } else if (nz) {
    const u64 below = mask & ((1ULL << lane) - 1ULL);
    const int run = lane - 1 - (below ? 63 - __clzll((long long)below) : 0);
    const unsigned zrl = ac[0xF0];
    for (int z = run >> 4; z > 0; --z) { bits = (bits << (zrl >> 16)) | (zrl & 0xFFFFu); len += (int)(zrl >> 16); }
    const unsigned e = ac[((run & 15) << 4) | nb];
    bits = (bits << (e >> 16)) | (e & 0xFFFFu);
    bits = (bits << nb) | ((unsigned)(v < 0 ? v - 1 : v) & ((1u << nb) - 1u));
    len += (int)(e >> 16) + nb;
  } else if (lane == 63) {                                  // coefficient 63 is zero: the block ends in a run, EOB
    bits = ac[0] & 0xFFFFu;
    len = (int)(ac[0] >> 16);
  }
}

__global__ __launch_bounds__(kT) void jpeg_ent_count_kernel(const short *__restrict__ coefs,
                                                            const dspn_jpeg_enc_sample *__restrict__ samples,
                                                            Header *__restrict__ h, unsigned *__restrict__ slot_bits) {
  __shared__ long long first[kMaxB + 1];
  __shared__ LdsTables T;
  const int B = h->B;
  for (int b = threadIdx.x; b <= B; b += kT) first[b] = h->first_slot[b];
  load_tables(T);
  __syncthreads();
  const long long N = first[B];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (long long u = (long long)blockIdx.x * kWaves + wave; u < N; u += (long long)gridDim.x * kWaves) {
    const int b = find_image(first, B, u);
    const Slot sl = locate(samples[b], h->interval[b], u - first[b], coefs);
    u64 bits;
    int len;
    bool over;
    lane_share(T, sl, lane, bits, len, over);
    const int total = __shfl(wave_incl_sum(len, lane), 63);
    const bool bad = __ballot(over) != 0;
    if (lane == 0) {
      slot_bits[u] = (unsigned)total | (sl.start ? kStart : 0u) | (sl.marker ? kMarker : 0u);
      if (bad) atomicMax(&h->status[b], 2);
    }
  }
}

__device__ __forceinline__ Seg thread_sum(const unsigned *__restrict__ slot_bits, long long at, long long N) {
  Seg f = {0, 0, 0};
  for (int i = 0; i < kScanPer; ++i)
    if (at + i < N) f = then(f, element(slot_bits[at + i]));
  return f;
}

__global__ __launch_bounds__(kT) void jpeg_ent_tile_sums_kernel(const Header *__restrict__ h, const unsigned *__restrict__ slot_bits,
                                                                Seg *__restrict__ agg) {
  __shared__ Seg lds[kT];
  const long long N = h->slots, tiles = (N + kScanTile - 1) / kScanTile;
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const Seg f = block_incl_scan(thread_sum(slot_bits, tile * kScanTile + threadIdx.x * kScanPer, N), lds, [](const Seg &l, const Seg &r) { return then(l, r); });
    if (threadIdx.x == kT - 1) agg[tile] = f;
  }
}

// one workgroup: where every tile starts, and the size of the stream
__global__ __launch_bounds__(kT) void jpeg_ent_tile_scan_kernel(Header *__restrict__ h, const Seg *__restrict__ agg,
                                                                long long *__restrict__ tile_start) {
  __shared__ Seg lds[kT];
  const long long N = h->slots, tiles = (N + kScanTile - 1) / kScanTile;
  long long carry = 0;
  for (long long base = 0; base < tiles; base += kT) {
    const long long tile = base + threadIdx.x;
    block_incl_scan(tile < tiles ? agg[tile] : Seg{0, 0, 0}, lds, [](const Seg &l, const Seg &r) { return then(l, r); });
    if (tile < tiles) tile_start[tile] = threadIdx.x ? apply(lds[threadIdx.x - 1], carry) : carry;
    carry = apply(lds[kT - 1], carry);
  }
  if (threadIdx.x == 0) h->stream_bytes = up8(carry) >> 3;
}

__global__ __launch_bounds__(kT) void jpeg_ent_tile_sweep_kernel(const Header *__restrict__ h, const unsigned *__restrict__ slot_bits,
                                                                 const long long *__restrict__ tile_start, long long *__restrict__ offs) {
  __shared__ Seg lds[kT];
  const long long N = h->slots, tiles = (N + kScanTile - 1) / kScanTile;
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long long at = tile * kScanTile + threadIdx.x * kScanPer;
    block_incl_scan(thread_sum(slot_bits, at, N), lds, [](const Seg &l, const Seg &r) { return then(l, r); });
    long long x = threadIdx.x ? apply(lds[threadIdx.x - 1], tile_start[tile]) : tile_start[tile];
    for (int i = 0; i < kScanPer; ++i)
      if (at + i < N) {
        const unsigned e = slot_bits[at + i];
        if (e & kStart) x = up8(x);
        offs[at + i] = x;
        x += e & kBitsMask;
      }
  }
}

__global__ __launch_bounds__(kT) void jpeg_ent_zero_kernel(const Header *__restrict__ h, uint4 *__restrict__ stream, uint4 *__restrict__ flags) {
  const long long bytes = (h->stream_bytes + kChunk - 1) / kChunk * kChunk, n = bytes / 16, nf = bytes / 8 / 16;
  const uint4 z = make_uint4(0, 0, 0, 0);
  for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < n; i += (long long)gridDim.x * kT) {
    stream[i] = z;
    if (i < nf) flags[i] = z;
  }
}

// ORs the low `len` bits of `bits` into the big-endian bit string `words` at bit `pos`
__device__ __forceinline__ void put_bits(unsigned *words, int pos, u64 bits, int len) {
  while (len > 0) {
    const int room = 32 - (pos & 31), take = len < room ? len : room;
    const unsigned piece = (unsigned)((bits >> (len - take)) & ((1ULL << take) - 1ULL));
    atomicOr(&words[pos >> 5], piece << (room - take));
    pos += take;
    len -= take;
  }
}

__global__ __launch_bounds__(kT) void jpeg_ent_emit_kernel(const short *__restrict__ coefs, const dspn_jpeg_enc_sample *__restrict__ samples,
                                                           const Header *__restrict__ h, const unsigned *__restrict__ slot_bits,
                                                           const long long *__restrict__ offs, unsigned *__restrict__ stream,
                                                           unsigned *__restrict__ flags) {
  __shared__ long long first[kMaxB + 1];
  __shared__ LdsTables T;
  __shared__ unsigned buf[kWaves][kBlockWords];
  const int B = h->B;
  for (int b = threadIdx.x; b <= B; b += kT) first[b] = h->first_slot[b];
  load_tables(T);
  const long long N = h->slots;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (long long base = (long long)blockIdx.x * kWaves; base < N; base += (long long)gridDim.x * kWaves) {   // the same trips for every wave
    const long long u = base + wave;
    const bool live = u < N;
    __syncthreads();                                        // the tables; the words of the previous trip are stored
    if (lane < kBlockWords) buf[wave][lane] = 0;
    __syncthreads();
    long long at = 0;
    int end = 0;
    if (live) {
      const int b = find_image(first, B, u);
      const Slot sl = locate(samples[b], h->interval[b], u - first[b], coefs);
      u64 bits;
      int len;
      bool over;
      lane_share(T, sl, lane, bits, len, over);
      const int incl = wave_incl_sum(len, lane), total = __shfl(incl, 63);
      at = offs[u];
      const int shift = (int)(at & 31);
      put_bits(buf[wave], shift + incl - len, bits, len);
      end = shift + total;
      if (lane == 0) {
        const bool last = u + 1 == N || (slot_bits[u + 1] & kStart);
        const int pad = last ? (int)(-(at + total) & 7) : 0;       // flush_ones
        put_bits(buf[wave], end, (1u << pad) - 1u, pad);
        end += pad;
        if (sl.marker) atomicOr(&flags[at >> 8], 1u << ((at >> 3) & 31));
      }
      end = __shfl(end, 0);
    }
    __syncthreads();
    const int words = (end + 31) >> 5;
    if (live && lane < words) {
      const unsigned w = __builtin_bswap32(buf[wave][lane]);
      unsigned *dst = stream + (at >> 5) + lane;
      const bool whole = (lane > 0 || (at & 31) == 0) && (lane < words - 1 || (end & 31) == 0);   // no neighbour's bit in it
      if (whole) *dst = w;
      else if (w) atomicOr(dst, w);
    }
  }
}

// FF bytes (low half) and set marker flags (high half) among the first `valid` of the 16 bytes w and their flag bits
__device__ __forceinline__ u64 count16(const uint4 &w, unsigned fl, int valid) {
  const unsigned ws[4] = {w.x, w.y, w.z, w.w};
  unsigned ff = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int nv = valid - 4 * i;
    const unsigned x = nv >= 4 ? ws[i] : (nv > 0 ? ws[i] & ((1u << (8 * nv)) - 1u) : 0u);
    ff += __popc(((x & 0x7F7F7F7Fu) + 0x01010101u) & x & 0x80808080u);      // bytes whose low seven bits and top bit are all set
  }
  const unsigned f = valid >= 16 ? fl : fl & ((1u << (valid > 0 ? valid : 0)) - 1u);
  return ff | (u64)__popc(f) << 32;
}

__device__ __forceinline__ unsigned flags16(const unsigned *__restrict__ flags, long long chunk, int lane) {
  return (flags[(chunk * 64 + lane) >> 1] >> ((lane & 1) * 16)) & 0xFFFFu;
}

__global__ __launch_bounds__(kT) void jpeg_ent_ffcount_kernel(const Header *__restrict__ h, const uint4 *__restrict__ stream,
                                                              const unsigned *__restrict__ flags, u64 *__restrict__ chunks) {
  const long long n = (h->stream_bytes + kChunk - 1) / kChunk;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (long long c = (long long)blockIdx.x * kWaves + wave; c < n; c += (long long)gridDim.x * kWaves) {
    const u64 sum = wave_incl_sum(count16(stream[c * 64 + lane], flags16(flags, c, lane), 16), lane);   // beyond the stream: zeros
    if (lane == 63) chunks[c] = sum;
  }
}

// one workgroup: chunks[c] becomes the count in front of chunk c, chunks[n] the whole count
__global__ __launch_bounds__(kT) void jpeg_ent_chunk_scan_kernel(const Header *__restrict__ h, u64 *__restrict__ chunks) {
  __shared__ u64 lds[kT];
  const long long n = (h->stream_bytes + kChunk - 1) / kChunk;
  u64 carry = 0;
  for (long long base = 0; base <= n; base += kT) {
    const long long c = base + threadIdx.x;
    const u64 own = c < n ? chunks[c] : 0;
    const u64 incl = block_incl_scan(own, lds, [](u64 a, u64 b) { return a + b; });
    if (c <= n) chunks[c] = carry + incl - own;
    carry += lds[kT - 1];
  }
}

__global__ __launch_bounds__(kT) void jpeg_ent_finalize_kernel(Header *h, const long long *__restrict__ offs,
                                                               const uint4 *__restrict__ stream, const unsigned *__restrict__ flags,
                                                               const u64 *__restrict__ chunks, long long *__restrict__ scan_bytes,
                                                               int *__restrict__ status) {
  const int B = h->B, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long N = h->slots, U = h->stream_bytes, n = (U + kChunk - 1) / kChunk;
  for (int b = wave; b <= B; b += kWaves) {
    const long long slot = h->first_slot[b], p = slot < N ? offs[slot] >> 3 : U, c = p / kChunk;
    u64 part = 0;
    if (c < n) {
      const long long valid = p - (c * kChunk + lane * 16);
      part = count16(stream[c * 64 + lane], flags16(flags, c, lane), (int)(valid < 0 ? 0 : (valid > 16 ? 16 : valid)));
    }
    part = wave_incl_sum(part, lane);
    if (lane == 63) {
      h->first_byte[b] = p;
      h->before[b] = chunks[c] + part;
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < B; b += kT) {
    const u64 d = h->before[b + 1] - h->before[b];          // both halves grow with b: no borrow between them
    const int st = h->status[b];
    const long long size = st ? 0 : h->first_byte[b + 1] - h->first_byte[b] + (long long)(d & 0xFFFFFFFFu) + 2 * (long long)(d >> 32);
    h->scan_bytes[b] = size;
    scan_bytes[b] = size;
    status[b] = st;
  }
}

__global__ __launch_bounds__(kT) void jpeg_ent_write_kernel(const Header *__restrict__ h, long long coef_count, int B, const long long *__restrict__ out_offsets,
                                                            unsigned char *__restrict__ out, long long out_bytes,
                                                            const uint4 *__restrict__ stream, const unsigned *__restrict__ flags,
                                                            const u64 *__restrict__ chunks) {
  __shared__ long long first[kMaxB + 1], place[kMaxB];      // place[b] + (byte index + FFs + 2 flags so far) is where a byte goes
  __shared__ unsigned markers[kMaxB];                       // marker flags in front of the image
  if (h->magic != kMagic || h->B != B || h->coef_count != coef_count) return;   // not the workspace of that scan call
  for (int b = threadIdx.x; b <= B; b += kT) first[b] = h->first_byte[b];
  for (int b = threadIdx.x; b < B; b += kT) {
    const long long size = h->scan_bytes[b], off = out_offsets[b];
    const u64 bf = h->before[b];
    const bool ok = h->status[b] == 0 && off >= 0 && off <= out_bytes - size;
    place[b] = ok ? off - h->first_byte[b] - (long long)(bf & 0xFFFFFFFFu) - 2 * (long long)(bf >> 32) : kNoWrite;
    markers[b] = (unsigned)(bf >> 32);
  }
  __syncthreads();
  const long long U = h->stream_bytes, n = (U + kChunk - 1) / kChunk;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (long long c = (long long)blockIdx.x * kWaves + wave; c < n; c += (long long)gridDim.x * kWaves) {
    const uint4 w = stream[c * 64 + lane];
    const unsigned fl = flags16(flags, c, lane);
    const u64 own = count16(w, fl, 16), upto = chunks[c] + wave_incl_sum(own, lane) - own;
    long long ff = (long long)(upto & 0xFFFFFFFFu), marks = (long long)(upto >> 32);
    const long long p0 = c * kChunk + lane * 16;
    if (p0 >= U) continue;
    int b = find_image(first, B, p0);
    const u64 half[2] = {w.x | (u64)w.y << 32, w.z | (u64)w.w << 32};
    for (int j = 0; j < 16 && p0 + j < U; ++j) {
      const long long p = p0 + j;
      while (p >= first[b + 1]) ++b;                        // p < U = first[B]
      const unsigned byte = (unsigned)((j < 8 ? half[0] : half[1]) >> (8 * (j & 7))) & 255u;
      const bool mark = (fl >> j) & 1u;
      marks += mark;
      if (place[b] != kNoWrite) {
        const long long at = place[b] + p + ff + 2 * marks;
        if (mark) {                                         // RSTn in front of the segment's first byte
          out[at - 2] = 0xFF;
          out[at - 1] = (unsigned char)(0xD0u + ((unsigned)(marks - markers[b] - 1) & 7u));
        }
        out[at] = (unsigned char)byte;
        if (byte == 0xFFu) out[at + 1] = 0;
      }
      ff += byte == 0xFFu;
    }
  }
}

}  // namespace

extern "C" int dspn_jpeg_encode_headers(const dspn_jpeg_enc_sample *s, int restart_interval, unsigned char *out, size_t capacity,
                                        size_t *length) {
  const int rc = dspn_jpeg_enc::encode_headers(s, restart_interval, out, capacity, length, dspn::last_error_buf(), 512);
  return rc == 0 ? 0 : (rc == dspn_jpeg_enc::kTooSmall ? DSPN_ERR_WORKSPACE_ : DSPN_ERR_ARG_);
}

extern "C" size_t dspn_jpeg_entropy_encode_workspace_bytes(long long coef_count, int B) {
  if (coef_count < 64 || coef_count > kMaxCoefs || B < 1 || B > kMaxB) return 0;
  return layout_of(coef_count).total;
}

extern "C" int dspn_jpeg_entropy_encode_scan_batch(const short *coefs, long long coef_count, const dspn_jpeg_enc_sample *samples,
                                                   const int *restart_intervals, int B, long long *scan_bytes, int *status,
                                                   void *workspace, size_t workspace_bytes, void *stream) {
  DSPN_REQUIRE(coefs && samples && restart_intervals && scan_bytes && status && workspace, "jpeg_entropy_encode_scan: null argument");
  DSPN_REQUIRE(B > 0 && B <= kMaxB, "jpeg_entropy_encode_scan: bad batch (0 < B <= %d)", kMaxB);
  DSPN_REQUIRE(coef_count > 0 && coef_count % 64 == 0 && coef_count <= kMaxCoefs,
               "jpeg_entropy_encode_scan: coef_count must be a multiple of 64 in 64..%lld", kMaxCoefs);
  DSPN_REQUIRE((reinterpret_cast<uintptr_t>(coefs) & 15) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(samples) & 7) == 0 && (reinterpret_cast<uintptr_t>(scan_bytes) & 7) == 0 &&
                   (reinterpret_cast<uintptr_t>(restart_intervals) & 3) == 0 && (reinterpret_cast<uintptr_t>(status) & 3) == 0,
               "jpeg_entropy_encode_scan: coefs and workspace must be 16-byte aligned, samples and scan_bytes 8-byte aligned");
  const Layout l = layout_of(coef_count);
  if (workspace_bytes < l.total)
    return dspn::fail(DSPN_ERR_WORKSPACE_, "jpeg_entropy_encode_scan: workspace of %zu bytes, %zu needed", workspace_bytes, l.total);
  hipStream_t s = static_cast<hipStream_t>(stream);
  char *ws = static_cast<char *>(workspace);
  Header *h = reinterpret_cast<Header *>(ws);
  unsigned *slot_bits = reinterpret_cast<unsigned *>(ws + l.bits_at);
  long long *offs = reinterpret_cast<long long *>(ws + l.offs_at), *tile_start = reinterpret_cast<long long *>(ws + l.tile_at);
  Seg *agg = reinterpret_cast<Seg *>(ws + l.agg_at);
  uint4 *bytes = reinterpret_cast<uint4 *>(ws + l.stream_at), *flags = reinterpret_cast<uint4 *>(ws + l.flags_at);
  u64 *chunks = reinterpret_cast<u64 *>(ws + l.chunks_at);
  const int slot_grid = (int)std::min<long long>(kGrid, (l.slot_cap + kWaves - 1) / kWaves);
  const int tile_grid = (int)std::min<long long>(kGrid, l.tile_cap), chunk_grid = (int)std::min<long long>(kGrid, (l.chunk_cap + kWaves - 1) / kWaves);
  const int zero_grid = (int)std::min<long long>(kGrid, (l.stream_cap / 16 + kT - 1) / kT);
  hipLaunchKernelGGL(jpeg_ent_setup_kernel, dim3(1), dim3(kT), 0, s, samples, restart_intervals, B, coef_count, l.slot_cap, l.blocks, h);
  hipLaunchKernelGGL(jpeg_ent_count_kernel, dim3(slot_grid), dim3(kT), 0, s, coefs, samples, h, slot_bits);
  hipLaunchKernelGGL(jpeg_ent_tile_sums_kernel, dim3(tile_grid), dim3(kT), 0, s, h, slot_bits, agg);
  hipLaunchKernelGGL(jpeg_ent_tile_scan_kernel, dim3(1), dim3(kT), 0, s, h, agg, tile_start);
  hipLaunchKernelGGL(jpeg_ent_tile_sweep_kernel, dim3(tile_grid), dim3(kT), 0, s, h, slot_bits, tile_start, offs);
  hipLaunchKernelGGL(jpeg_ent_zero_kernel, dim3(zero_grid), dim3(kT), 0, s, h, bytes, flags);
  hipLaunchKernelGGL(jpeg_ent_emit_kernel, dim3(slot_grid), dim3(kT), 0, s, coefs, samples, h, slot_bits, offs,
                     reinterpret_cast<unsigned *>(bytes), reinterpret_cast<unsigned *>(flags));
  hipLaunchKernelGGL(jpeg_ent_ffcount_kernel, dim3(chunk_grid), dim3(kT), 0, s, h, bytes, reinterpret_cast<unsigned *>(flags), chunks);
  hipLaunchKernelGGL(jpeg_ent_chunk_scan_kernel, dim3(1), dim3(kT), 0, s, h, chunks);
  hipLaunchKernelGGL(jpeg_ent_finalize_kernel, dim3(1), dim3(kT), 0, s, h, offs, bytes, reinterpret_cast<unsigned *>(flags), chunks,
                     scan_bytes, status);
  return dspn::check_launch("jpeg_entropy_encode_scan");
}

extern "C" int dspn_jpeg_entropy_encode_write_batch(long long coef_count, int B, const long long *out_offsets, unsigned char *out,
                                                    long long out_bytes, void *workspace, size_t workspace_bytes, void *stream) {
  DSPN_REQUIRE(out_offsets && out && workspace, "jpeg_entropy_encode_write: null argument");
  DSPN_REQUIRE(B > 0 && B <= kMaxB, "jpeg_entropy_encode_write: bad batch (0 < B <= %d)", kMaxB);
  DSPN_REQUIRE(coef_count > 0 && coef_count % 64 == 0 && coef_count <= kMaxCoefs && out_bytes > 0,
               "jpeg_entropy_encode_write: coef_count must be a multiple of 64 in 64..%lld and out_bytes positive", kMaxCoefs);
  DSPN_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0 && (reinterpret_cast<uintptr_t>(out_offsets) & 7) == 0,
               "jpeg_entropy_encode_write: workspace must be 16-byte aligned, out_offsets 8-byte aligned");
  const Layout l = layout_of(coef_count);
  if (workspace_bytes < l.total)
    return dspn::fail(DSPN_ERR_WORKSPACE_, "jpeg_entropy_encode_write: workspace of %zu bytes, %zu needed", workspace_bytes, l.total);
  char *ws = static_cast<char *>(workspace);
  const int chunk_grid = (int)std::min<long long>(kGrid, (l.chunk_cap + kWaves - 1) / kWaves);
  hipLaunchKernelGGL(jpeg_ent_write_kernel, dim3(chunk_grid), dim3(kT), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<const Header *>(ws), coef_count, B, out_offsets, out, out_bytes,
                     reinterpret_cast<const uint4 *>(ws + l.stream_at), reinterpret_cast<const unsigned *>(ws + l.flags_at),
                     reinterpret_cast<const u64 *>(ws + l.chunks_at));
  return dspn::check_launch("jpeg_entropy_encode_write");
}

// Huffman decoding of a baseline JPEG scan (include/dspn_jpeg.h), the only text of it: code derivation and lookahead table,
// bit reader, decode_symbol, receive_extend, decode_block and the zigzag order, as __host__ __device__ functions.  The host
// entropy pass (jpeg_host.h) calls decode_block with its own reader and AC-table type from its own walk over the MCUs; the
// rest of this file is ONE restart interval as the device pass sees it ("entropy pass on the device"), its walk over the
// interval's MCUs included: the kernel in jpeg.hip runs run_segment one interval per lane, the host build
// (dspn_jpeg_entropy_decode_segments, tools/jpeg_huff_check.cpp) runs it serially and under the host sanitizers.
// Nothing here trusts its input: `prepare` checks the descriptors of a sample against the pools, `run_segment` checks the
// two entries of the segment table it reads, the bit reader never passes the end of its segment, every table index is
// checked, and every loop has a fixed bound (64 coefficients, the blocks of an MCU, restart_interval MCUs).
#pragma once
#include <cstdint>
#include <cstring>

#include "../../include/dspn_jpeg.h"

#if defined(__HIPCC__)
#define DSPN_HD __host__ __device__ __forceinline__
#else
#define DSPN_HD inline
#endif

namespace dspn_jpeg_huff {

constexpr int kLookBits = 9;
constexpr int kSlots = 6;            // decode tables of one sample: DC and AC of up to three components

// one Huffman table ready for decoding (1424 bytes; the kernel keeps kSlots of them in LDS)
struct Table {
  uint16_t look[1 << kLookBits];     // (length << 8) | symbol for codes of up to kLookBits bits, 0: longer (or none)
  int maxcode[18];                   // largest code of each length, -1: none; [17]: sentinel
  int valoffset[17];                 // index of the first value of a length minus its first code
  int nvals;                         // < 0: the counts are not those of a prefix code
  unsigned char vals[256];
  // What decode_block does with this type as its AC table.  The device pass refuses an AC value of more than 10 bits
  // (DSPN_JPEG_BAD_SIZE): the DCT of 8-bit samples cannot give one.  The host pass (dspn_jpeg::Huff in jpeg_host.h) takes
  // every size a symbol can name, up to 15.  The difference is kept on purpose, it is not a bug
  // (tests/test_jpeg_entropy_limits.py pins both sides).
  static constexpr int kMaxAcSize = 10;
  static constexpr bool kFastAc = false;
};
static_assert(sizeof(Table) == 1424, "Table must not grow: kSlots of them sit in LDS");

// what a lane needs of its sample, checked
struct Layout {
  int ncomp, hs, vs;                 // luma sampling; one component: 1 x 1
  int blocks_w[3];
  long long coef_offset[3];
  int mcus_w, mcus, interval, segments;
  int dc_slot[3], ac_slot[3];        // which Table of the sample's kSlots each component decodes with
  int slot_table[kSlots];            // and which table of the descriptor a slot holds: 0..3 DC, 4..7 AC, -1 unused
  long long data_offset, data_bytes, first_segment;
};

// the part of a dspn_jpeg_sample that says where coefficients lie: true when every block of its grids is inside the pool
DSPN_HD bool coef_geometry_ok(const dspn_jpeg_sample &s, long long coef_count) {
  if (s.width < 1 || s.height < 1 || s.width > 65535 || s.height > 65535) return false;
  if (s.ncomp != 1 && s.ncomp != 3) return false;
  int hs = 1, vs = 1;
  if (s.ncomp == 3) {
    hs = s.hsamp; vs = s.vsamp;
    if (!((hs == 1 && vs == 1) || (hs == 2 && (vs == 1 || vs == 2)))) return false;
  }
  for (int c = 0; c < s.ncomp; ++c) {
    const int cw = c ? (s.width + hs - 1) / hs : s.width, ch = c ? (s.height + vs - 1) / vs : s.height;
    const int bw = s.blocks_w[c], bh = s.blocks_h[c];
    if (bw < 1 || bh < 1 || bw > 8192 || bh > 8192 || bw * 8 < cw || bh * 8 < ch) return false;
    const long long off = s.coef_offset[c];
    if (off < 0 || (off & 63) || off > coef_count - 64LL * bw * bh) return false;
  }
  return true;
}

// Checks sample and scan against each other and against the pools and fills `L`.  false: no work (skip, segments == 0, or
// descriptors that contradict themselves or could index outside a pool).
DSPN_HD bool prepare(const dspn_jpeg_sample &s, const dspn_jpeg_scan &sc, long long bytes_count, long long segment_count,
                     long long coef_count, Layout &L) {
  if (s.skip || sc.segments < 1) return false;
  if (!coef_geometry_ok(s, coef_count)) return false;
  const int nc = s.ncomp;
  L.ncomp = nc;
  L.hs = nc == 3 ? s.hsamp : 1;
  L.vs = nc == 3 ? s.vsamp : 1;
  if (sc.mcus_w < 1 || sc.mcus_h < 1 || sc.mcus_w > 8192 || sc.mcus_h > 8192) return false;
  for (int c = 0; c < 3; ++c) {
    L.blocks_w[c] = c < nc ? s.blocks_w[c] : 0;
    L.coef_offset[c] = c < nc ? s.coef_offset[c] : 0;
    if (c >= nc) continue;
    const int ch = c ? 1 : L.hs, cv = c ? 1 : L.vs;           // the stream carries every block of every MCU: the grids are whole MCUs
    if (s.blocks_w[c] != sc.mcus_w * ch || s.blocks_h[c] != sc.mcus_h * cv) return false;
  }
  L.mcus_w = sc.mcus_w;
  L.mcus = sc.mcus_w * sc.mcus_h;                             // <= 2^26
  L.interval = sc.restart_interval;
  L.segments = sc.segments;
  if (L.interval < 1 || L.interval > DSPN_JPEG_DEVICE_MAX_INTERVAL) return false;
  if (L.segments != (L.mcus + L.interval - 1) / L.interval) return false;
  if (sc.data_offset < 0 || sc.data_bytes < 0 || sc.data_bytes > 0xFFFFFFFFLL || sc.data_offset > bytes_count - sc.data_bytes)
    return false;
  if (sc.first_segment < 0 || sc.first_segment > segment_count - (long long)L.segments - 1) return false;
  L.data_offset = sc.data_offset;
  L.data_bytes = sc.data_bytes;
  L.first_segment = sc.first_segment;
  int used = 0;
  for (int k = 0; k < kSlots; ++k) L.slot_table[k] = -1;
  for (int c = 0; c < 3; ++c) {
    L.dc_slot[c] = L.ac_slot[c] = 0;
    if (c >= nc) continue;
    if (sc.dc_table[c] > 3 || sc.ac_table[c] > 3) return false;
    for (int pass = 0; pass < 2; ++pass) {
      const int want = pass ? 4 + sc.ac_table[c] : sc.dc_table[c];
      int slot = -1;
      for (int k = 0; k < kSlots; ++k)
        if (k < used && L.slot_table[k] == want) slot = k;
      if (slot < 0) { slot = used++; L.slot_table[slot] = want; }
      if (pass) L.ac_slot[c] = slot; else L.dc_slot[c] = slot;
    }
  }
  return true;
}

// Table building in two steps, so that a workgroup can share it: build_codes by ONE thread per table, then (after a barrier)
// build_look by any number of threads, each taking the windows first, first + step, ...
DSPN_HD void build_codes(Table &t, const unsigned char *counts /* [16] */, const unsigned char *vals /* [256] */) {
  int code = 0, k = 0;
  bool ok = true;
  for (int l = 1; l <= 16; ++l) {
    const int cnt = counts[l - 1];
    t.valoffset[l] = k - code;
    if (cnt) {
      if (code + cnt > (1 << l)) ok = false;
      code += cnt;
      k += cnt;
      t.maxcode[l] = code - 1;
    } else {
      t.maxcode[l] = -1;
    }
    code <<= 1;
  }
  t.maxcode[0] = -1;
  t.maxcode[17] = 0x7fffffff;
  t.valoffset[0] = 0;
  if (k > 256) ok = false;
  for (int i = 0; i < 256; ++i) t.vals[i] = vals[i];
  t.nvals = ok ? k : -1;
}

DSPN_HD void build_look(Table &t, int first, int step) {
  for (int i = first; i < (1 << kLookBits); i += step) {
    unsigned e = 0;
    if (t.nvals > 0)
      for (int l = 1; l <= kLookBits; ++l) {
        const int code = i >> (kLookBits - l);
        if (code <= t.maxcode[l]) {
          const int idx = t.valoffset[l] + code;
          if (idx >= 0 && idx < t.nvals) e = (unsigned)(l << 8) | t.vals[idx];
          break;
        }
      }
    t.look[i] = (uint16_t)e;
  }
}

// zigzag position -> natural (row-major) index, by walking the diagonals.  The one definition: dspn_jpeg::kNatural
// (jpeg_host.h) is this at compile time, the kernel runs it into LDS.
constexpr DSPN_HD void fill_natural(unsigned char *out /* [64] */) {
  int r = 0, c = 0;
  for (int k = 0; k < 64; ++k) {
    out[k] = (unsigned char)(r * 8 + c);
    if ((r + c) & 1) {               // down and to the left
      if (r == 7) ++c; else if (c == 0) ++r; else { ++r; --c; }
    } else {                         // up and to the right
      if (c == 7) ++r; else if (r == 0) ++c; else { --r; ++c; }
    }
  }
}

// MSB-first bit reader over [p, end): the top `bits` bits of `buf` are valid.  At a marker or at the end it feeds zero bits
// and counts them in `pad`; a decoder that has consumed padding (bits < pad) has run off the data.  Byte by byte: lanes of a
// wave sit at unrelated places of unrelated segments, so there is nothing to gain from wider loads.  (The host pass reads
// through dspn_jpeg::FastBitReader, which puts a wide load in front of this loop.)
struct BitReader {
  const unsigned char *p, *end;
  uint64_t buf;
  int bits, pad;
  bool stopped;                      // at a marker or at the end

  DSPN_HD void start(const unsigned char *from, const unsigned char *to) {
    p = from;
    end = to;
    buf = 0; bits = 0; pad = 0; stopped = false;
  }
  DSPN_HD void fill() {              // -> bits >= 57
    while (bits <= 56) {
      unsigned v = 0;
      if (!stopped) {
        if (p >= end) {
          stopped = true;
        } else {
          v = *p;
          if (v != 0xFF) ++p;
          else if (p + 1 < end && p[1] == 0x00) p += 2;
          else { stopped = true; v = 0; }   // a marker (or a lone 0xFF at the end): stay in front of it
        }
      }
      if (stopped) pad += 8;
      buf |= (uint64_t)v << (56 - bits);
      bits += 8;
    }
  }
  DSPN_HD unsigned peek(int k) const { return (unsigned)(buf >> (64 - k)); }   // 1 <= k <= 32
  DSPN_HD void drop(int k) { buf <<= k; bits -= k; }
};

template <class Reader>
DSPN_HD int decode_symbol(Reader &br, const Table &h) {      // needs bits >= 16; -1: no such code
  const unsigned e = h.look[br.peek(kLookBits)];
  if (e) { br.drop((int)(e >> 8)); return (int)(e & 255u); }
  for (int l = kLookBits + 1; l <= 16; ++l) {
    const int code = (int)br.peek(l);
    if (code <= h.maxcode[l]) {
      const int idx = h.valoffset[l] + code;
      if (idx < 0 || idx >= h.nvals) return -1;
      br.drop(l);
      return h.vals[idx];
    }
  }
  return -1;
}

template <class Reader>
DSPN_HD int receive_extend(Reader &br, int s) {              // 1 <= s <= 15, needs bits >= s
  const int v = (int)br.peek(s);
  br.drop(s);
  return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// One block into `sink` (cleared by the caller; decode_block only calls sink.set(natural index, value)).  The 64 values of a
// block are addressed by a zigzag position that only the data knows, so they must not be a per-lane array (it would live in
// scratch): Sink is LDS on the device, memory on the host.
// What differs between the passes is a compile-time property of the AC table's type: AcTable::kMaxAcSize, and
// AcTable::kFastAc, whether the table has fast_ac[], (value << 8) | (run << 4) | bits for a window that holds a whole code
// AND its magnitude bits -- run, size and value in one step.
template <class Reader, class AcTable, class Sink>
DSPN_HD int decode_block(Reader &br, const Table &dc, const AcTable &ac, int &pred, const unsigned char *natural, Sink &sink) {
  if (br.bits < 32) br.fill();
  int s = decode_symbol(br, dc);
  if (s < 0) return DSPN_JPEG_BAD_CODE;
  if (s > 11) return DSPN_JPEG_BAD_SIZE;
  if (s) pred += receive_extend(br, s);
  if (pred < -32768 || pred > 32767) return DSPN_JPEG_BAD_DC;
  sink.set(0, pred);
  for (int k = 1; k < 64;) {
    if (br.bits < 32) br.fill();
    if constexpr (AcTable::kFastAc) {
      const int f = ac.fast_ac[br.peek(kLookBits)];
      if (f) {
        k += (f >> 4) & 15;
        if (k > 63) return DSPN_JPEG_BAD_INDEX;
        sink.set(natural[k++], f >> 8);
        br.drop(f & 15);
        continue;
      }
    }
    const int rs = decode_symbol(br, ac);
    if (rs < 0) return DSPN_JPEG_BAD_CODE;
    const int r = rs >> 4;
    s = rs & 15;
    if (s) {
      k += r;
      if (k > 63) return DSPN_JPEG_BAD_INDEX;
      if (s > AcTable::kMaxAcSize) return DSPN_JPEG_BAD_SIZE;
      sink.set(natural[k], receive_extend(br, s));
      ++k;
    } else if (r == 15) {
      k += 16;
      if (k > 64) return DSPN_JPEG_BAD_INDEX;
    } else {
      break;                         // EOB (r < 15 with s == 0 is read as one, as libjpeg does)
    }
  }
  if (br.bits < br.pad) return DSPN_JPEG_BAD_END;
  return 0;
}

// Segment `i` (0 <= i < L.segments) of a prepared sample: the MCUs i * interval .. of the scan, out of
// bytes[data_offset + seg[i], data_offset + seg[i + 1]) and into the blocks of exactly those MCUs.  -> 0 or a DSPN_JPEG_BAD_ code.
// tables: the sample's kSlots tables, built; natural: zigzag position -> natural index, 64 bytes.
template <class Sink>
DSPN_HD int run_segment(const Layout &L, int i, const unsigned char *bytes, const unsigned int *segments, const Table *tables,
                        const unsigned char *natural, short *coefs, Sink &sink) {
  const long long a = segments[L.first_segment + i], b = segments[L.first_segment + i + 1];
  if (a > b || b > L.data_bytes) return DSPN_JPEG_BAD_SEGMENT;
  for (int c = 0; c < 3; ++c)
    if (c < L.ncomp && (tables[L.dc_slot[c]].nvals < 0 || tables[L.ac_slot[c]].nvals < 0)) return DSPN_JPEG_BAD_SEGMENT;
  BitReader br;
  br.start(bytes + L.data_offset + a, bytes + L.data_offset + b);
  const int first = i * L.interval;
  const int n = L.mcus - first < L.interval ? L.mcus - first : L.interval;
  int my = first / L.mcus_w, mx = first - my * L.mcus_w;
  int pred0 = 0, pred1 = 0, pred2 = 0;
  for (int m = 0; m < n; ++m) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (c >= L.ncomp) continue;
      const int ch = c ? 1 : L.hs, cv = c ? 1 : L.vs;
      const Table &dc = tables[L.dc_slot[c]], &ac = tables[L.ac_slot[c]];
      int &pred = c == 0 ? pred0 : (c == 1 ? pred1 : pred2);
      for (int v = 0; v < cv; ++v)
        for (int h = 0; h < ch; ++h) {
          sink.clear();
          const int code = decode_block(br, dc, ac, pred, natural, sink);
          if (code) return code;
          const long long blk = (long long)(my * cv + v) * L.blocks_w[c] + (mx * ch + h);
          sink.store(coefs + L.coef_offset[c] + 64 * blk);
        }
    }
    if (++mx == L.mcus_w) { mx = 0; ++my; }
  }
  // what is left: less than a byte of padding in the reader, then the end of the segment -- the restart marker (behind any
  // fill bytes) whose last byte closes the segment, or for the last segment nothing: it ends where the closing marker stands
  if (br.bits - br.pad >= 8) return DSPN_JPEG_BAD_REST;
  const unsigned char *t = br.p;
  while (t < br.end && *t == 0xFF) ++t;
  const bool at_end = t == br.end && t == br.p;
  const bool at_marker = t + 1 == br.end && t > br.p && (*t & 0xF8) == 0xD0;
  if (!(i + 1 == L.segments ? at_end : at_marker)) return DSPN_JPEG_BAD_REST;
  return 0;
}

DSPN_HD int status_word(int code, int segment) {
  return ((DSPN_JPEG_STATUS_SEGMENTS - segment) << 3) | code;
}

// ---- the host build --------------------------------------------------------------------------------------------------
struct HostSink {
  short blk[64];
  inline void clear() { memset(blk, 0, sizeof(blk)); }
  inline void set(int at, int v) { blk[at] = (short)v; }
  inline void store(short *dst) const { memcpy(dst, blk, sizeof(blk)); }
};

// every segment of one sample, serially -> the status word the device would leave (0: decoded; also 0 for "no work")
inline int decode_sample(const unsigned char *bytes, long long bytes_count, const dspn_jpeg_sample &s, const dspn_jpeg_scan &sc,
                         const unsigned int *segments, long long segment_count, short *coefs, long long coef_count) {
  Layout L;
  if (!prepare(s, sc, bytes_count, segment_count, coef_count, L)) return 0;
  unsigned char natural[64];
  fill_natural(natural);
  Table *tables = new Table[kSlots];
  for (int k = 0; k < kSlots; ++k) {
    const int t = L.slot_table[k];
    if (t < 0) { tables[k].nvals = -1; continue; }
    build_codes(tables[k], t < 4 ? sc.dc_counts[t] : sc.ac_counts[t - 4], t < 4 ? sc.dc_values[t] : sc.ac_values[t - 4]);
    build_look(tables[k], 0, 1);
  }
  HostSink sink;
  int status = 0;
  for (int i = 0; i < L.segments; ++i) {
    const int code = run_segment(L, i, bytes, segments, tables, natural, coefs, sink);
    if (code) {
      const int w = status_word(code, i);
      if (w > status) status = w;
    }
  }
  delete[] tables;
  return status;
}

}  // namespace dspn_jpeg_huff

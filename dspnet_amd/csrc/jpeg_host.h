// Host half of the JPEG decode (include/dspn_jpeg.h): marker parsing, the scan index, and the host entropy pass -- the walk
// over the MCUs, the restart markers between intervals, the end of the scan and the error texts around the Huffman decode of
// jpeg_huff.h (tables, bit reader, decode_block), which this pass shares with the device.  Plain C++ with no HIP call and no
// global state, so that it also builds into a stand-alone program under the host sanitizers (tools/jpeg_host_check.cpp).
// Every read is checked against the end of the input and every block is written through the geometry this file derived
// itself and compared with the caller's `info`.
#pragma once
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/dspn_jpeg.h"
#include "jpeg_huff.h"

namespace dspn_jpeg {

namespace hf = dspn_jpeg_huff;
using hf::kLookBits;

constexpr int kErr = -1;

struct Natural {
  unsigned char at[64];
  constexpr Natural() : at{} { hf::fill_natural(at); }
};
static constexpr Natural kNaturalOrder;
static constexpr const unsigned char (&kNatural)[64] = kNaturalOrder.at;   // zigzag position -> natural (row-major) index

// a table of the stream: the shared decode table and what only the host needs
struct Huff : hf::Table {
  bool present = false;
  unsigned char counts[16] = {};    // codes per length 1..16, as the DHT segment carries them
  // AC tables: (value << 8) | (run << 4) | bits for a window that holds a whole code AND its magnitude bits
  // (code length + size <= kLookBits, value in -128..127), 0: take the two steps
  int16_t fast_ac[1 << kLookBits];
  // What decode_block does with this type as its AC table.  The host pass takes every AC size a symbol can name, up to 15,
  // where the device pass (hf::Table) refuses more than 10.  The difference is kept on purpose, it is not a bug:
  // tests/test_jpeg_entropy_limits.py.
  static constexpr int kMaxAcSize = 15;
  static constexpr bool kFastAc = true;
};

struct Parsed {
  dspn_jpeg_info info;
  int comp_id[4], comp_tq[4], comp_td[4], comp_ta[4];
  bool quant_present[4] = {}, quant_wide[4] = {};
  unsigned char quant[4][64];
  Huff dc[4], ac[4];
  size_t scan_pos = 0;              // first byte of entropy-coded data
};

inline int fail(char *err, size_t errn, const char *fmt, ...) {
  if (err && errn) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err, errn, fmt, ap);
    va_end(ap);
  }
  return kErr;
}

inline int build_huff(Huff &h, const unsigned char *bits /* [1..16] at bits[0..15] */, const unsigned char *vals, int nvals,
                      char *err, size_t errn) {
  unsigned char padded[256] = {};   // build_codes copies 256 values, the segment holds nvals
  memcpy(padded, vals, (size_t)nvals);
  h.present = true;
  memcpy(h.counts, bits, 16);
  hf::build_codes(h, bits, padded);
  for (int l = 1; l <= 16; ++l)
    if (h.maxcode[l] >= (1 << l)) return fail(err, errn, "jpeg: Huffman table has more codes of length %d than fit", l);
  hf::build_look(h, 0, 1);
  for (int i = 0; i < (1 << kLookBits); ++i) {
    h.fast_ac[i] = 0;
    const int len = h.look[i] >> 8, run = (h.look[i] >> 4) & 15, mag = h.look[i] & 15;
    if (!len || !mag || len + mag > kLookBits) continue;
    int v = ((i << len) & ((1 << kLookBits) - 1)) >> (kLookBits - mag);
    if (v < (1 << (mag - 1))) v += 1 - (1 << mag);
    if (v >= -128 && v <= 127) h.fast_ac[i] = (int16_t)(v * 256 + run * 16 + len + mag);
  }
  return 0;
}

// Markers up to the first SOS.  An unsupported frame returns at its frame header: width, height and ncomp are known by then.
inline int parse(const unsigned char *b, size_t n, Parsed &P, char *err, size_t errn) {
  dspn_jpeg_info &I = P.info;
  memset(&I, 0, sizeof(I));
  if (!b || n < 4 || b[0] != 0xFF || b[1] != 0xD8) return fail(err, errn, "jpeg: no SOI marker (%zu bytes)", n);
  size_t p = 2;
  bool have_frame = false, jfif = false, adobe = false;
  int adobe_transform = -1;
  for (;;) {
    if (p >= n) return fail(err, errn, "jpeg: truncated before SOS (at byte %zu)", p);
    if (b[p] != 0xFF) return fail(err, errn, "jpeg: expected a marker at byte %zu", p);
    while (p < n && b[p] == 0xFF) ++p;        // fill bytes
    if (p >= n) return fail(err, errn, "jpeg: truncated inside a marker");
    const int m = b[p++];
    if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;   // stand-alone markers
    if (m == 0xD9) return fail(err, errn, "jpeg: EOI before any scan");
    if (m == 0x00) return fail(err, errn, "jpeg: stuffed byte outside a scan at byte %zu", p);
    if (p + 2 > n) return fail(err, errn, "jpeg: truncated segment length");
    const size_t L = ((size_t)b[p] << 8) | b[p + 1];
    if (L < 2 || p + L > n) return fail(err, errn, "jpeg: segment 0x%02X of %zu bytes runs past the end", m, L);
    const unsigned char *s = b + p + 2;
    const size_t sl = L - 2;
    p += L;
    if (m >= 0xC0 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {      // SOFn
      if (have_frame) return fail(err, errn, "jpeg: two frame headers");
      if (sl < 6) return fail(err, errn, "jpeg: short frame header");
      const int prec = s[0], nc = s[5];
      I.height = (s[1] << 8) | s[2];
      I.width = (s[3] << 8) | s[4];
      I.ncomp = nc;
      if (I.width <= 0 || I.height <= 0) return fail(err, errn, "jpeg: empty frame (%d x %d)", I.width, I.height);
      if (nc < 1 || nc > 4 || sl != (size_t)(6 + 3 * nc)) return fail(err, errn, "jpeg: bad frame header (%d components)", nc);
      have_frame = true;
      int why = DSPN_JPEG_OK;
      if (m == 0xC2) why = DSPN_JPEG_PROGRESSIVE;
      else if (m == 0xC1) why = DSPN_JPEG_EXTENDED;
      else if (m >= 0xC9) why = DSPN_JPEG_ARITHMETIC;
      else if (m != 0xC0) why = DSPN_JPEG_LOSSLESS_HIERARCHICAL;
      else if (prec != 8) why = DSPN_JPEG_PRECISION;
      else if (nc != 1 && nc != 3) why = DSPN_JPEG_COMPONENTS;
      for (int c = 0; c < nc; ++c) {
        P.comp_id[c] = s[6 + 3 * c];
        const int hv = s[7 + 3 * c];
        P.comp_tq[c] = s[8 + 3 * c];
        if (c < 3) { I.hsamp[c] = hv >> 4; I.vsamp[c] = hv & 15; }
        if ((hv >> 4) < 1 || (hv >> 4) > 4 || (hv & 15) < 1 || (hv & 15) > 4 || P.comp_tq[c] > 3)
          return fail(err, errn, "jpeg: component %d has sampling %dx%d, table %d", c, hv >> 4, hv & 15, P.comp_tq[c]);
      }
      if (why == DSPN_JPEG_OK && nc == 3) {
        const bool luma_ok = (I.hsamp[0] == 1 && I.vsamp[0] == 1) || (I.hsamp[0] == 2 && I.vsamp[0] <= 2);
        if (!luma_ok || I.hsamp[1] != 1 || I.vsamp[1] != 1 || I.hsamp[2] != 1 || I.vsamp[2] != 1) why = DSPN_JPEG_SAMPLING;
      }
      if (why != DSPN_JPEG_OK) { I.reason = why; I.supported = 0; return 0; }   // sizes are known: enough for the caller
    } else if (m == 0xDB) {                                                     // DQT
      size_t q = 0;
      while (q < sl) {
        const int pq = s[q] >> 4, tq = s[q] & 15;
        const size_t need = pq ? 128 : 64;
        if (tq > 3 || pq > 1 || q + 1 + need > sl) return fail(err, errn, "jpeg: bad quantisation table segment");
        P.quant_present[tq] = true;
        P.quant_wide[tq] = pq != 0;
        if (!pq)
          for (int i = 0; i < 64; ++i) P.quant[tq][kNatural[i]] = s[q + 1 + i];
        q += 1 + need;
      }
    } else if (m == 0xC4) {                                                     // DHT
      size_t q = 0;
      while (q < sl) {
        if (q + 17 > sl) return fail(err, errn, "jpeg: short Huffman table segment");
        const int tc = s[q] >> 4, th = s[q] & 15;
        int cnt = 0;
        for (int i = 0; i < 16; ++i) cnt += s[q + 1 + i];
        if (tc > 1 || th > 3 || cnt > 256 || q + 17 + (size_t)cnt > sl) return fail(err, errn, "jpeg: bad Huffman table segment");
        if (build_huff(tc ? P.ac[th] : P.dc[th], s + q + 1, s + q + 17, cnt, err, errn)) return kErr;
        q += 17 + (size_t)cnt;
      }
    } else if (m == 0xDD) {                                                     // DRI
      if (sl != 2) return fail(err, errn, "jpeg: bad restart interval segment");
      I.restart_interval = (s[0] << 8) | s[1];
    } else if (m == 0xE0) {
      if (sl >= 5 && !memcmp(s, "JFIF\0", 5)) jfif = true;
    } else if (m == 0xEE) {
      if (sl >= 12 && !memcmp(s, "Adobe", 5)) { adobe = true; adobe_transform = s[11]; }
    } else if (m == 0xDA) {                                                     // SOS
      if (!have_frame) return fail(err, errn, "jpeg: scan before the frame header");
      const int nc = I.ncomp;
      if (sl < 1 || s[0] < 1 || s[0] > 4 || sl != (size_t)(4 + 2 * s[0])) return fail(err, errn, "jpeg: bad scan header");
      bool whole = s[0] == nc;
      for (int c = 0; whole && c < nc; ++c) whole = s[1 + 2 * c] == P.comp_id[c];
      if (!whole) { I.reason = DSPN_JPEG_MULTISCAN; I.supported = 0; return 0; }
      for (int c = 0; c < nc; ++c) {
        P.comp_td[c] = s[2 + 2 * c] >> 4;
        P.comp_ta[c] = s[2 + 2 * c] & 15;
        if (P.comp_td[c] > 3 || P.comp_ta[c] > 3 || !P.dc[P.comp_td[c]].present || !P.ac[P.comp_ta[c]].present)
          return fail(err, errn, "jpeg: component %d names a Huffman table that is out of range or undefined", c);
        if (!P.quant_present[P.comp_tq[c]]) return fail(err, errn, "jpeg: component %d names an undefined quantisation table", c);
        if (P.quant_wide[P.comp_tq[c]]) { I.reason = DSPN_JPEG_QUANT_16BIT; I.supported = 0; return 0; }
      }
      if (nc == 3) {
        bool ycc = true;                                                        // libjpeg's guess, in its order
        if (jfif) ycc = true;
        else if (adobe) ycc = adobe_transform == 1;
        else if (P.comp_id[0] == 'R' && P.comp_id[1] == 'G' && P.comp_id[2] == 'B') ycc = false;
        if (!ycc) { I.reason = DSPN_JPEG_COLOR_TRANSFORM; I.supported = 0; return 0; }
      }
      P.scan_pos = p;
      break;
    }
    // every other segment (APPn, COM, ...) is skipped by its length
  }
  // geometry
  const int hmax = I.ncomp == 1 ? 1 : I.hsamp[0], vmax = I.ncomp == 1 ? 1 : I.vsamp[0];
  if (I.ncomp == 1) I.hsamp[0] = I.vsamp[0] = 1;     // a single-component scan is not interleaved: one block per MCU
  const int mcux = (I.width + 8 * hmax - 1) / (8 * hmax), mcuy = (I.height + 8 * vmax - 1) / (8 * vmax);
  long long off = 0;
  for (int c = 0; c < I.ncomp; ++c) {
    I.blocks_w[c] = mcux * I.hsamp[c];
    I.blocks_h[c] = mcuy * I.vsamp[c];
    I.coef_offset[c] = off;
    off += 64LL * I.blocks_w[c] * I.blocks_h[c];
    memcpy(I.quant[c], P.quant[P.comp_tq[c]], 64);
  }
  I.coef_count = off;
  I.supported = 1;
  I.reason = DSPN_JPEG_OK;
  return 0;
}

inline int probe(const unsigned char *b, size_t n, dspn_jpeg_info *info, char *err, size_t errn) {
  if (!info) return fail(err, errn, "jpeg_probe: null argument");
  Parsed P;
  const int rc = parse(b, n, P, err, errn);
  *info = P.info;
  if (rc) memset(info, 0, sizeof(*info));
  return rc;
}

// The shared bit reader behind a wide load: eight bytes at once where none of them is 0xFF.  Host only.
struct FastBitReader : hf::BitReader {
  inline void fill() {              // -> bits >= 57
    if (!stopped && end - p >= 8) {
      uint64_t w;
      memcpy(&w, p, 8);
      const uint64_t x = ~w;        // a 0xFF byte of w is a zero byte of x
      if (!((x - 0x0101010101010101ULL) & ~x & 0x8080808080808080ULL)) {
        const int take = (64 - bits) >> 3;
        if (take == 0) return;
        w = __builtin_bswap64(w);
        if (take == 8) buf = w;
        else buf |= (w >> (64 - 8 * take)) << (64 - bits - 8 * take);
        bits += 8 * take;
        p += take;
        return;
      }
    }
    hf::BitReader::fill();
  }
};

// the caller's `info` against what these bytes parse to
inline bool same_info(const dspn_jpeg_info &info, const dspn_jpeg_info &I) {
  bool same = info.supported && info.width == I.width && info.height == I.height && info.ncomp == I.ncomp &&
              info.coef_count == I.coef_count;
  for (int c = 0; same && c < I.ncomp; ++c)
    same = info.blocks_w[c] == I.blocks_w[c] && info.blocks_h[c] == I.blocks_h[c] && info.coef_offset[c] == I.coef_offset[c];
  return same;
}

// decode_block straight into the output plane (the caller clears the block)
struct PlaneSink {
  int16_t *blk;
  inline void set(int at, int v) { blk[at] = (int16_t)v; }
};

// the DSPN_JPEG_BAD_ codes decode_block returns, in the host pass's words
static const char *const kBlockError[] = {
    "ok", "a Huffman code that is not in its table", "a coefficient index or a zero run past 63",
    "a DC difference of more than 11 bits", "scan data ends inside a block", "", "a DC value out of range"};
static_assert(sizeof(kBlockError) / sizeof(kBlockError[0]) == DSPN_JPEG_BAD_DC + 1, "one text per code decode_block returns");
static_assert(Huff::kMaxAcSize == 15, "the text of DSPN_JPEG_BAD_SIZE names DC alone: no AC symbol names more than 15 bits");

inline int entropy_decode(const unsigned char *b, size_t n, const dspn_jpeg_info *info, int16_t *out, char *err, size_t errn) {
  if (!info || !out) return fail(err, errn, "jpeg_entropy_decode: null argument");
  Parsed P;
  if (parse(b, n, P, err, errn)) return kErr;
  const dspn_jpeg_info &I = P.info;
  if (!I.supported) return fail(err, errn, "jpeg_entropy_decode: unsupported stream (reason %d)", I.reason);
  if (!same_info(*info, I)) return fail(err, errn, "jpeg_entropy_decode: info does not describe these bytes");
  FastBitReader br;
  br.start(b + P.scan_pos, b + n);
  int pred[3] = {0, 0, 0};
  const int nc = I.ncomp;
  const int mcux = I.blocks_w[0] / I.hsamp[0], mcuy = I.blocks_h[0] / I.vsamp[0];
  const int ri = I.restart_interval;
  int until_restart = ri, next_rst = 0;
  // the walk over the MCUs: run_segment (jpeg_huff.h) has the same one for a single interval, kept apart because the
  // kernel's code changes when the loop becomes a function shared with this one (profiles/jpeg_entropy_one_core.txt)
  for (int my = 0; my < mcuy; ++my)
    for (int mx = 0; mx < mcux; ++mx) {
      if (ri && until_restart == 0) {
        if (br.bits - br.pad >= 8) return fail(err, errn, "jpeg: data where restart marker %d belongs", next_rst);
        const unsigned char *q = br.p;
        if (q >= br.end || *q != 0xFF) return fail(err, errn, "jpeg: missing restart marker %d", next_rst);
        while (q < br.end && *q == 0xFF) ++q;
        if (q >= br.end || *q != 0xD0 + next_rst) return fail(err, errn, "jpeg: missing restart marker %d", next_rst);
        br.start(q + 1, br.end);
        pred[0] = pred[1] = pred[2] = 0;
        next_rst = (next_rst + 1) & 7;
        until_restart = ri;
      }
      for (int c = 0; c < nc; ++c) {
        const Huff &dc = P.dc[P.comp_td[c]], &ac = P.ac[P.comp_ta[c]];
        int16_t *plane = out + I.coef_offset[c];
        for (int v = 0; v < I.vsamp[c]; ++v)
          for (int h = 0; h < I.hsamp[c]; ++h) {
            const long long blk = (long long)(my * I.vsamp[c] + v) * I.blocks_w[c] + (mx * I.hsamp[c] + h);
            PlaneSink sink = {plane + 64 * blk};
            memset(sink.blk, 0, 64 * sizeof(int16_t));
            const int code = hf::decode_block(br, dc, ac, pred[c], kNatural, sink);
            if (code) return fail(err, errn, "jpeg: %s", kBlockError[code]);
          }
      }
      --until_restart;
    }
  // what follows the last MCU is a marker (EOI, as a rule), after less than a byte of padding: a stream that lost its place
  // and still decoded "something" ends elsewhere
  if (br.bits - br.pad >= 8 || br.p + 1 >= br.end || br.p[0] != 0xFF || br.p[1] == 0x00)
    return fail(err, errn, "jpeg: the scan does not end at a marker");
  return 0;
}

// restart intervals of a supported scan, 0 without a restart interval
inline long long scan_segments(const dspn_jpeg_info &I) {
  if (!I.supported || I.restart_interval < 1 || I.hsamp[0] < 1 || I.vsamp[0] < 1) return 0;
  const long long mcus = (long long)(I.blocks_w[0] / I.hsamp[0]) * (I.blocks_h[0] / I.vsamp[0]);
  return (mcus + I.restart_interval - 1) / I.restart_interval;
}

// The restart intervals of the scan for the device entropy pass (dspn_jpeg_scan_index): a walk over the 0xFF bytes of the
// entropy-coded data, no Huffman work.  Where the entropy pass above would miss a restart marker, so does this, in its words.
inline int scan_index(const unsigned char *b, size_t n, const dspn_jpeg_info *info, dspn_jpeg_scan *scan, unsigned *seg,
                      size_t seg_capacity, char *err, size_t errn) {
  if (!info || !scan || !seg) return fail(err, errn, "jpeg_scan_index: null argument");
  Parsed P;
  if (parse(b, n, P, err, errn)) return kErr;
  const dspn_jpeg_info &I = P.info;
  if (!I.supported) return fail(err, errn, "jpeg_scan_index: unsupported stream (reason %d)", I.reason);
  if (!same_info(*info, I)) return fail(err, errn, "jpeg_scan_index: info does not describe these bytes");
  const int ri = I.restart_interval;
  if (ri == 0) return fail(err, errn, "jpeg_scan_index: the stream has no restart interval: its entropy pass stays on the host");
  if (ri > DSPN_JPEG_DEVICE_MAX_INTERVAL)
    return fail(err, errn, "jpeg_scan_index: a restart interval of %d MCUs, the device pass takes up to %d: its entropy pass stays on the host",
                ri, DSPN_JPEG_DEVICE_MAX_INTERVAL);
  if (n - P.scan_pos > 0xFFFFFFFFull) return fail(err, errn, "jpeg_scan_index: a scan of more than 4 GiB");
  const long long nseg = scan_segments(I);
  if ((unsigned long long)nseg + 1 > seg_capacity)
    return fail(err, errn, "jpeg_scan_index: %lld segment offsets, the table holds %zu", nseg + 1, seg_capacity);
  long long count = 1;
  int next_rst = 0;
  size_t p = P.scan_pos, closing = 0;
  seg[0] = 0;
  for (;;) {
    const unsigned char *q = p < n ? static_cast<const unsigned char *>(memchr(b + p, 0xFF, n - p)) : nullptr;
    if (!q) return fail(err, errn, "jpeg: the scan does not end at a marker");
    const size_t at = (size_t)(q - b);
    size_t r = at + 1;
    while (r < n && b[r] == 0xFF) ++r;                    // fill bytes
    if (r >= n) return fail(err, errn, "jpeg: the scan does not end at a marker");
    const int m = b[r];
    if (m == 0x00 && r == at + 1) { p = r + 1; continue; }   // a stuffed 0xFF: data
    if (m >= 0xD0 && m <= 0xD7) {
      if (count == nseg) return fail(err, errn, "jpeg: restart marker %d behind the last restart interval", m - 0xD0);
      if (m != 0xD0 + next_rst) return fail(err, errn, "jpeg: missing restart marker %d", next_rst);
      seg[count++] = (unsigned)(r + 1 - P.scan_pos);
      next_rst = (next_rst + 1) & 7;
      p = r + 1;
      continue;
    }
    // any other marker ends the scan (fill bytes in front of a stuffed zero are not a marker: the entropy pass looks for a
    // restart marker there and misses it)
    if (m == 0x00 || count != nseg) return fail(err, errn, "jpeg: missing restart marker %d", next_rst);
    closing = at - P.scan_pos;
    break;
  }
  seg[nseg] = (unsigned)closing;
  memset(scan, 0, sizeof(*scan));
  scan->data_offset = (long long)P.scan_pos;
  scan->data_bytes = (long long)closing;
  scan->first_segment = 0;
  scan->segments = (int)nseg;
  scan->restart_interval = ri;
  scan->mcus_w = I.blocks_w[0] / I.hsamp[0];
  scan->mcus_h = I.blocks_h[0] / I.vsamp[0];
  for (int c = 0; c < I.ncomp; ++c) {
    scan->dc_table[c] = (unsigned char)P.comp_td[c];
    scan->ac_table[c] = (unsigned char)P.comp_ta[c];
  }
  for (int t = 0; t < 4; ++t) {
    if (P.dc[t].present) { memcpy(scan->dc_counts[t], P.dc[t].counts, 16); memcpy(scan->dc_values[t], P.dc[t].vals, (size_t)P.dc[t].nvals); }
    if (P.ac[t].present) { memcpy(scan->ac_counts[t], P.ac[t].counts, 16); memcpy(scan->ac_values[t], P.ac[t].vals, (size_t)P.ac[t].nvals); }
  }
  return 0;
}

}  // namespace dspn_jpeg

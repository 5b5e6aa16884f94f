// Host half of the JPEG decode (include/dspn_jpeg.h): marker parsing and Huffman decoding of a baseline stream into
// quantised DCT coefficients.  Plain C++ with no HIP call and no global state, so that it also builds into a stand-alone
// program under the host sanitizers (tools/jpeg_host_check.cpp).  Every read is checked against the end of the input and
// every block is written through the geometry this file derived itself and compared with the caller's `info`.
#pragma once
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/dspn_jpeg.h"

namespace dspn_jpeg {

constexpr int kErr = -1;
constexpr int kLookBits = 9;

static const unsigned char kNatural[64] = {   // zigzag position -> natural (row-major) index
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Huff {
  bool present = false;
  int nvals = 0;
  unsigned char counts[16] = {};    // codes per length 1..16, as the DHT segment carries them
  unsigned char vals[256];
  int maxcode[18];                  // largest code of each length, -1: none
  int valoffset[17];                // index of the first value of a length minus its first code
  uint16_t look[1 << kLookBits];    // (length << 8) | symbol for codes of up to kLookBits bits, 0: longer
  // AC tables: (value << 8) | (run << 4) | bits for a window that holds a whole code AND its magnitude bits
  // (code length + size <= kLookBits, value in -128..127), 0: take the two steps
  int16_t fast_ac[1 << kLookBits];
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
  h.present = true;
  h.nvals = nvals;
  memcpy(h.counts, bits, 16);
  memcpy(h.vals, vals, (size_t)nvals);
  memset(h.look, 0, sizeof(h.look));
  int code = 0, k = 0;
  for (int l = 1; l <= 16; ++l) {
    const int cnt = bits[l - 1];
    h.valoffset[l] = k - code;
    if (cnt) {
      if (code + cnt > (1 << l)) return fail(err, errn, "jpeg: Huffman table has more codes of length %d than fit", l);
      if (l <= kLookBits)
        for (int i = 0; i < cnt; ++i) {
          const int first = (code + i) << (kLookBits - l);
          for (int j = 0; j < (1 << (kLookBits - l)); ++j) h.look[first + j] = (uint16_t)((l << 8) | vals[k + i]);
        }
      code += cnt;
      k += cnt;
      h.maxcode[l] = code - 1;
    } else {
      h.maxcode[l] = -1;
    }
    code <<= 1;
  }
  h.maxcode[17] = 0x7fffffff;
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

// MSB-first bit reader over the entropy-coded segment: the top `bits` bits of `buf` are valid.  At a marker or at the end of
// the input it feeds zero bits and counts them in `pad`; a decoder that has consumed padding (bits < pad) has run off the data.
struct BitReader {
  const unsigned char *p, *end;
  uint64_t buf = 0;
  int bits = 0, pad = 0;
  bool stopped = false;             // at a marker or at the end

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
    while (bits <= 56) {
      unsigned v = 0;
      if (!stopped) {
        if (p >= end) stopped = true;
        else if (*p != 0xFF) v = *p++;
        else if (p + 1 < end && p[1] == 0x00) { v = 0xFF; p += 2; }
        else stopped = true;        // a marker (or a lone 0xFF at the end): stay in front of it
      }
      if (stopped) pad += 8;
      buf |= (uint64_t)v << (56 - bits);
      bits += 8;
    }
  }
  inline unsigned peek(int k) const { return (unsigned)(buf >> (64 - k)); }   // 1 <= k <= 32
  inline void drop(int k) { buf <<= k; bits -= k; }
};

inline int decode_symbol(BitReader &br, const Huff &h) {     // needs bits >= 16; -1: no such code
  const unsigned e = h.look[br.peek(kLookBits)];
  if (e) { br.drop((int)(e >> 8)); return (int)(e & 255); }
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

inline int receive_extend(BitReader &br, int s) {            // 1 <= s <= 15, needs bits >= s
  const int v = (int)br.peek(s);
  br.drop(s);
  return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

inline int decode_block(BitReader &br, const Huff &dc, const Huff &ac, int &pred, int16_t *blk, char *err, size_t errn) {
  memset(blk, 0, 64 * sizeof(int16_t));
  if (br.bits < 32) br.fill();
  int s = decode_symbol(br, dc);
  if (s < 0) return fail(err, errn, "jpeg: DC code not in its table");
  if (s > 11) return fail(err, errn, "jpeg: DC difference of %d bits", s);
  if (s) pred += receive_extend(br, s);
  if (pred < -32768 || pred > 32767) return fail(err, errn, "jpeg: DC value out of range");
  blk[0] = (int16_t)pred;
  for (int k = 1; k < 64;) {
    if (br.bits < 32) br.fill();
    const int f = ac.fast_ac[br.peek(kLookBits)];
    if (f) {                        // run, size and value in one step
      k += (f >> 4) & 15;
      if (k > 63) return fail(err, errn, "jpeg: coefficient index past 63");
      blk[kNatural[k++]] = (int16_t)(f >> 8);
      br.drop(f & 15);
      continue;
    }
    const int rs = decode_symbol(br, ac);
    if (rs < 0) return fail(err, errn, "jpeg: AC code not in its table");
    const int r = rs >> 4;
    s = rs & 15;
    if (s) {
      k += r;
      if (k > 63) return fail(err, errn, "jpeg: coefficient index past 63");
      blk[kNatural[k]] = (int16_t)receive_extend(br, s);
      ++k;
    } else if (r == 15) {
      k += 16;
      if (k > 64) return fail(err, errn, "jpeg: zero run past coefficient 63");
    } else {
      break;                        // EOB (r < 15 with s == 0 is read as one, as libjpeg does)
    }
  }
  if (br.bits < br.pad) return fail(err, errn, "jpeg: scan data ends inside a block");
  return 0;
}

// the caller's `info` against what these bytes parse to
inline bool same_info(const dspn_jpeg_info &info, const dspn_jpeg_info &I) {
  bool same = info.supported && info.width == I.width && info.height == I.height && info.ncomp == I.ncomp &&
              info.coef_count == I.coef_count;
  for (int c = 0; same && c < I.ncomp; ++c)
    same = info.blocks_w[c] == I.blocks_w[c] && info.blocks_h[c] == I.blocks_h[c] && info.coef_offset[c] == I.coef_offset[c];
  return same;
}

inline int entropy_decode(const unsigned char *b, size_t n, const dspn_jpeg_info *info, int16_t *out, char *err, size_t errn) {
  if (!info || !out) return fail(err, errn, "jpeg_entropy_decode: null argument");
  Parsed P;
  if (parse(b, n, P, err, errn)) return kErr;
  const dspn_jpeg_info &I = P.info;
  if (!I.supported) return fail(err, errn, "jpeg_entropy_decode: unsupported stream (reason %d)", I.reason);
  if (!same_info(*info, I)) return fail(err, errn, "jpeg_entropy_decode: info does not describe these bytes");
  BitReader br;
  br.p = b + P.scan_pos;
  br.end = b + n;
  int pred[3] = {0, 0, 0};
  const int nc = I.ncomp;
  const int mcux = I.blocks_w[0] / I.hsamp[0], mcuy = I.blocks_h[0] / I.vsamp[0];
  const int ri = I.restart_interval;
  int until_restart = ri, next_rst = 0;
  for (int my = 0; my < mcuy; ++my)
    for (int mx = 0; mx < mcux; ++mx) {
      if (ri && until_restart == 0) {
        if (br.bits - br.pad >= 8) return fail(err, errn, "jpeg: data where restart marker %d belongs", next_rst);
        const unsigned char *q = br.p;
        if (q >= br.end || *q != 0xFF) return fail(err, errn, "jpeg: missing restart marker %d", next_rst);
        while (q < br.end && *q == 0xFF) ++q;
        if (q >= br.end || *q != 0xD0 + next_rst) return fail(err, errn, "jpeg: missing restart marker %d", next_rst);
        br.p = q + 1;
        br.buf = 0; br.bits = 0; br.pad = 0; br.stopped = false;
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
            if (decode_block(br, dc, ac, pred[c], plane + 64 * blk, err, errn)) return kErr;
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

// Host half of the JPEG encode (include/dspn_jpeg_encode.h): the quantisation tables of a quality, the geometry of an image,
// and the markers and Huffman coding of a baseline file from quantised coefficients.  Plain C++ with no HIP call and no global
// state, so that it also builds into a stand-alone program under the host sanitizers (tools/jpeg_encode_host_check.cpp).
// Every output byte goes through Out::put, which counts it and stores it only below the capacity; every block is read through
// the geometry this file derived itself and compared with the caller's descriptor.
#pragma once
#include <cstdint>
#include <cstring>

#include "../../include/dspn_jpeg_encode.h"
#include "jpeg_host.h"

namespace dspn_jpeg_enc {

using dspn_jpeg::fail;
using dspn_jpeg::kErr;
using dspn_jpeg::kNatural;
constexpr int kTooSmall = -2;

// Annex K, tables K.1 and K.2, natural order
static const unsigned char kStdLum[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
                                          14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                                          18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                                          49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
static const unsigned char kStdChr[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99,
                                          24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                                          99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                          99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
// Annex K, tables K.3 - K.6: code counts per length 1..16, then the symbols
static const unsigned char kDcLumBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
static const unsigned char kDcChrBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
static const unsigned char kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
static const unsigned char kAcLumBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
static const unsigned char kAcLumVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
    0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
    0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
    0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
    0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
    0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
static const unsigned char kAcChrBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
static const unsigned char kAcChrVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
    0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
    0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
    0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
    0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
    0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
    0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

inline int quant_tables(int quality, unsigned char *lum, unsigned char *chr, char *err, size_t errn) {
  if (!lum || !chr) return fail(err, errn, "jpeg_quant_tables: null argument");
  if (quality < 1 || quality > 100) return fail(err, errn, "jpeg_quant_tables: quality %d is outside 1..100", quality);
  const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  for (int i = 0; i < 64; ++i) {
    const int l = (kStdLum[i] * scale + 50) / 100, c = (kStdChr[i] * scale + 50) / 100;
    lum[i] = (unsigned char)(l < 1 ? 1 : (l > 255 ? 255 : l));
    chr[i] = (unsigned char)(c < 1 ? 1 : (c > 255 ? 255 : c));
  }
  return 0;
}

struct Geometry {
  int ncomp, hs, vs;                // luma sampling (chroma 1 x 1)
  int bw[3], bh[3];                 // real grids
  int mcux, mcuy;
  long long count;                  // coefficients of the image
};

inline int geometry(int width, int height, int ncomp, int hsamp, int vsamp, Geometry &g, char *err, size_t errn) {
  if (width < 1 || height < 1 || width > 65535 || height > 65535)
    return fail(err, errn, "jpeg_encode: an image of %d x %d (width x height; 1..65535 each)", width, height);
  if (ncomp != 1 && ncomp != 3) return fail(err, errn, "jpeg_encode: %d components (1 or 3)", ncomp);
  g.ncomp = ncomp;
  g.hs = ncomp == 1 ? 1 : hsamp;
  g.vs = ncomp == 1 ? 1 : vsamp;
  if (!((g.hs == 1 && g.vs == 1) || (g.hs == 2 && (g.vs == 1 || g.vs == 2))))
    return fail(err, errn, "jpeg_encode: luma sampling %d x %d (1x1, 2x1 or 2x2)", hsamp, vsamp);
  g.mcux = (width + 8 * g.hs - 1) / (8 * g.hs);
  g.mcuy = (height + 8 * g.vs - 1) / (8 * g.vs);
  g.count = 0;
  for (int c = 0; c < ncomp; ++c) {
    const int cw = c ? (width + g.hs - 1) / g.hs : width, ch = c ? (height + g.vs - 1) / g.vs : height;
    g.bw[c] = (cw + 7) / 8;
    g.bh[c] = (ch + 7) / 8;
    g.count += 64LL * g.bw[c] * g.bh[c];
  }
  return 0;
}

inline int fill_geometry(dspn_jpeg_enc_sample *s, long long coef_base, long long *coef_count, char *err, size_t errn) {
  if (!s || !coef_count) return fail(err, errn, "jpeg_encode_geometry: null argument");
  if (coef_base < 0 || (coef_base & 63)) return fail(err, errn, "jpeg_encode_geometry: coef_base must be a multiple of 64, >= 0");
  Geometry g;
  if (geometry(s->width, s->height, s->ncomp, s->hsamp, s->vsamp, g, err, errn)) return kErr;
  s->hsamp = g.hs;
  s->vsamp = g.vs;
  long long off = coef_base;
  for (int c = 0; c < 3; ++c) {
    s->blocks_w[c] = c < g.ncomp ? g.bw[c] : 0;
    s->blocks_h[c] = c < g.ncomp ? g.bh[c] : 0;
    s->coef_offset[c] = c < g.ncomp ? off : 0;
    if (c < g.ncomp) off += 64LL * g.bw[c] * g.bh[c];
  }
  *coef_count = g.count;
  return 0;
}

// canonical codes of one table, by symbol
struct Codes {
  uint16_t code[256];
  unsigned char size[256];          // 0: the symbol has no code
};

constexpr void build_codes(Codes &t, const unsigned char *bits, const unsigned char *vals) {   // constexpr: the device pass builds its tables at compile time
  t = Codes{};
  int code = 0, k = 0;
  for (int l = 1; l <= 16; ++l) {
    for (int i = 0; i < bits[l - 1]; ++i, ++k) {
      t.code[vals[k]] = (uint16_t)code++;
      t.size[vals[k]] = (unsigned char)l;
    }
    code <<= 1;
  }
}

// the output: every byte is counted, and stored only below the capacity
struct Out {
  unsigned char *p;
  size_t cap, n = 0;
  uint64_t acc = 0;                 // the low `bits` bits are pending, MSB first
  int bits = 0;

  inline void put(unsigned v) {
    if (n < cap) p[n] = (unsigned char)v;
    ++n;
  }
  inline void put2(unsigned v) { put(v >> 8); put(v & 255u); }
  inline void put_bits(unsigned v, int k) {      // 0 <= k <= 16, v < (1 << k)
    acc = (acc << k) | v;
    bits += k;
    while (bits >= 8) {
      const unsigned b = (unsigned)(acc >> (bits - 8)) & 255u;
      put(b);
      if (b == 0xFF) put(0);
      bits -= 8;
    }
  }
  inline void flush_ones() {
    if (bits) put_bits((1u << (8 - bits)) - 1u, 8 - bits);
    acc = 0;
    bits = 0;
  }
};

inline int bit_length(unsigned v) { return v ? 32 - __builtin_clz(v) : 0; }

// one block: blk is its 64 coefficients in natural order (nullptr: all AC zero), dc its DC value
inline int encode_block(Out &o, const Codes &dct, const Codes &act, const int16_t *blk, int dc, int &pred, char *err, size_t errn) {
  int d = dc - pred;
  pred = dc;
  int m = d;
  if (d < 0) { m = -d; d -= 1; }
  int nb = bit_length((unsigned)m);
  if (nb > 11) return fail(err, errn, "jpeg_encode: a DC difference of %d bits (baseline coding carries 11)", nb);
  o.put_bits(dct.code[nb], dct.size[nb]);
  if (nb) o.put_bits((unsigned)d & ((1u << nb) - 1u), nb);
  int run = 0;
  if (blk)
    for (int k = 1; k < 64; ++k) {
      int v = blk[kNatural[k]];
      if (v == 0) { ++run; continue; }
      while (run > 15) { o.put_bits(act.code[0xF0], act.size[0xF0]); run -= 16; }
      m = v;
      if (v < 0) { m = -v; v -= 1; }
      nb = bit_length((unsigned)m);
      if (nb > 10) return fail(err, errn, "jpeg_encode: an AC coefficient of %d bits (baseline coding carries 10)", nb);
      const int sym = (run << 4) | nb;
      o.put_bits(act.code[sym], act.size[sym]);
      o.put_bits((unsigned)v & ((1u << nb) - 1u), nb);
      run = 0;
    }
  else
    run = 63;
  if (run > 0) o.put_bits(act.code[0], act.size[0]);   // EOB
  return 0;
}

inline void put_dqt(Out &o, int id, const unsigned char *q) {
  o.put2(0xFFDB); o.put2(67); o.put((unsigned)id);
  for (int i = 0; i < 64; ++i) o.put(q[kNatural[i]]);
}

inline void put_dht(Out &o, int tc_th, const unsigned char *bits, const unsigned char *vals) {
  int n = 0;
  for (int i = 0; i < 16; ++i) n += bits[i];
  o.put2(0xFFC4); o.put2((unsigned)(19 + n)); o.put((unsigned)tc_th);
  for (int i = 0; i < 16; ++i) o.put(bits[i]);
  for (int i = 0; i < n; ++i) o.put(vals[i]);
}

// what both the file writer and the header writer ask of a descriptor; g receives its geometry
inline int check_descriptor(const char *who, const dspn_jpeg_enc_sample *s, int restart_interval, Geometry &g, char *err, size_t errn) {
  if (restart_interval < 0 || restart_interval > 65535)
    return fail(err, errn, "%s: a restart interval of %d MCUs (0..65535)", who, restart_interval);
  if (geometry(s->width, s->height, s->ncomp, s->hsamp, s->vsamp, g, err, errn)) return kErr;
  for (int c = 0; c < g.ncomp; ++c) {
    if (s->blocks_w[c] != g.bw[c] || s->blocks_h[c] != g.bh[c])
      return fail(err, errn, "%s: component %d has a grid of %d x %d blocks, its real grid is %d x %d", who, c,
                  s->blocks_w[c], s->blocks_h[c], g.bw[c], g.bh[c]);
    if (s->coef_offset[c] < 0 || (s->coef_offset[c] & 63))
      return fail(err, errn, "%s: coef_offset[%d] must be a multiple of 64, >= 0", who, c);
    for (int i = 0; i < 64; ++i)
      if (s->quant[c][i] == 0) return fail(err, errn, "%s: a zero in the quantisation table of component %d", who, c);
  }
  if (g.ncomp == 3 && memcmp(s->quant[1], s->quant[2], 64))
    return fail(err, errn, "%s: the two chroma components must share one quantisation table", who);
  return 0;
}

// SOI through the SOS header: everything in front of the first byte of the scan
inline void put_headers(Out &o, const dspn_jpeg_enc_sample *s, const Geometry &g, int restart_interval) {
  o.put2(0xFFD8);
  o.put2(0xFFE0); o.put2(16);
  for (const char *j = "JFIF"; *j; ++j) o.put((unsigned char)*j);
  o.put(0); o.put(1); o.put(1); o.put(0); o.put2(1); o.put2(1); o.put(0); o.put(0);
  put_dqt(o, 0, s->quant[0]);
  if (g.ncomp == 3) put_dqt(o, 1, s->quant[1]);
  o.put2(0xFFC0); o.put2((unsigned)(8 + 3 * g.ncomp)); o.put(8); o.put2((unsigned)s->height); o.put2((unsigned)s->width);
  o.put((unsigned)g.ncomp);
  for (int c = 0; c < g.ncomp; ++c) {
    o.put((unsigned)(c + 1));
    o.put(c == 0 ? (unsigned)((g.hs << 4) | g.vs) : 0x11u);
    o.put(c ? 1u : 0u);
  }
  put_dht(o, 0x00, kDcLumBits, kDcVals);
  put_dht(o, 0x10, kAcLumBits, kAcLumVals);
  if (g.ncomp == 3) {
    put_dht(o, 0x01, kDcChrBits, kDcVals);
    put_dht(o, 0x11, kAcChrBits, kAcChrVals);
  }
  if (restart_interval) { o.put2(0xFFDD); o.put2(4); o.put2((unsigned)restart_interval); }   // where libjpeg writes it: with the scan header
  o.put2(0xFFDA); o.put2((unsigned)(6 + 2 * g.ncomp)); o.put((unsigned)g.ncomp);
  for (int c = 0; c < g.ncomp; ++c) { o.put((unsigned)(c + 1)); o.put(c ? 0x11u : 0x00u); }
  o.put(0); o.put(63); o.put(0);
}

// the headers alone (dspn_jpeg_encode_headers) -> 0, kErr, or kTooSmall as below
inline int encode_headers(const dspn_jpeg_enc_sample *s, int restart_interval, unsigned char *out, size_t capacity, size_t *length,
                          char *err, size_t errn) {
  if (!s || !length || (!out && capacity)) return fail(err, errn, "jpeg_encode_headers: null argument");
  *length = 0;
  Geometry g;
  if (check_descriptor("jpeg_encode_headers", s, restart_interval, g, err, errn)) return kErr;
  Out o;
  o.p = out;
  o.cap = capacity;
  put_headers(o, s, g, restart_interval);
  *length = o.n;
  if (o.n > capacity) {
    fail(err, errn, "jpeg_encode_headers: the headers need %zu bytes, the buffer holds %zu", o.n, capacity);
    return kTooSmall;
  }
  return 0;
}

// -> 0, kErr, or kTooSmall (the file needs *length > capacity bytes; out[0 .. capacity - 1] hold its beginning)
// restart_interval: MCUs between restart markers, 0: none (and no DRI segment)
inline int entropy_encode(const int16_t *coefs, const dspn_jpeg_enc_sample *s, int restart_interval, unsigned char *out,
                          size_t capacity, size_t *length, char *err, size_t errn) {
  if (!coefs || !s || !length || (!out && capacity)) return fail(err, errn, "jpeg_entropy_encode: null argument");
  *length = 0;
  Geometry g;
  if (check_descriptor("jpeg_entropy_encode", s, restart_interval, g, err, errn)) return kErr;

  Codes dc[2], ac[2];
  build_codes(dc[0], kDcLumBits, kDcVals);
  build_codes(ac[0], kAcLumBits, kAcLumVals);
  build_codes(dc[1], kDcChrBits, kDcVals);
  build_codes(ac[1], kAcChrBits, kAcChrVals);

  Out o;
  o.p = out;
  o.cap = capacity;
  put_headers(o, s, g, restart_interval);

  int pred[3] = {0, 0, 0};
  int until_restart = restart_interval, next_rst = 0;
  for (int my = 0; my < g.mcuy; ++my)
    for (int mx = 0; mx < g.mcux; ++mx) {
      if (restart_interval) {
        if (until_restart == 0) {                         // the partial byte padded with 1 bits, RSTn, the predictors reset
          o.flush_ones();
          o.put2(0xFFD0u + (unsigned)next_rst);
          next_rst = (next_rst + 1) & 7;
          pred[0] = pred[1] = pred[2] = 0;
          until_restart = restart_interval;
        }
        --until_restart;
      }
      for (int c = 0; c < g.ncomp; ++c) {
        const int t = c ? 1 : 0;
        const int ch = c ? 1 : g.hs, cv = c ? 1 : g.vs;
        const int16_t *plane = coefs + s->coef_offset[c];
        int last_dc = 0;                                  // DC of the previous block of this component in this MCU
        for (int v = 0; v < cv; ++v)
          for (int h = 0; h < ch; ++h) {
            const int by = my * cv + v, bx = mx * ch + h;
            const int16_t *blk = nullptr;
            if (by < g.bh[c] && bx < g.bw[c]) {
              blk = plane + 64 * ((long long)by * g.bw[c] + bx);
              last_dc = blk[0];
            }                                             // else a dummy block: AC zero, DC as the block before it
            if (encode_block(o, dc[t], ac[t], blk, last_dc, pred[c], err, errn)) return kErr;
          }
      }
    }
  o.flush_ones();
  o.put2(0xFFD9);
  *length = o.n;
  if (o.n > capacity) {
    fail(err, errn, "jpeg_entropy_encode: the file needs %zu bytes, the buffer holds %zu", o.n, capacity);
    return kTooSmall;
  }
  return 0;
}

inline int entropy_encode(const int16_t *coefs, const dspn_jpeg_enc_sample *s, unsigned char *out, size_t capacity, size_t *length,
                          char *err, size_t errn) {
  return entropy_encode(coefs, s, 0, out, capacity, length, err, errn);
}

}  // namespace dspn_jpeg_enc

// The rules of the PNG encoder's deflate (include/dspn_png_encode.h states the stream format), compiled for both sides: the
// device kernels of png_deflate.hip and the host encoder dspn_png_deflate_host run this text, so their streams are equal
// byte for byte.  No allocation, no recursion, no local array with a computed index (the callers hand in the work memory, LDS
// on the device, so that nothing spills to scratch).
//
//   roles          token_at: what a byte contributes, from its place j in its run of r equal bytes (runs are cut at a block's
//                  first byte): j = 0 a literal; match pieces of distance 1 start at j = 1 + 258 k with length
//                  min(258, r - j) when that is at least 3, else the remaining 1 or 2 bytes are literals
//   code lengths   sort_symbols + code_lengths_sorted: Huffman over the used symbols in ascending (count, symbol) order by the
//                  two-queue merge (a leaf goes before an internal node of the same weight), depths cut at the limit, the
//                  Kraft excess taken back zlib's way (one leaf from the deepest level below the limit and one from the limit
//                  both go one below the former), and the lengths handed out again in that order, longest first.  So the
//                  cost equals the unlimited code's wherever that fits the limit.  One used symbol gets length 1.
//   header         header_symbols: the HLIT literal/length lengths and the one distance length as ONE sequence under the
//                  repeat symbols: a zero run takes 18 while 11 or more remain, then 17 for 3 or more; a non-zero length is
//                  sent once and repeated by 16 while 3 or more remain
//   plan_block     all of the above for one block's histogram, and the block's mode: stored when the dynamic form takes more
//                  than 8 * (bytes + 5) bits
//   bits           deflate packs from the least significant bit; Huffman codes are kept bit-reversed, ready to be ORed in
#ifndef DSPN_PNG_DEFLATE_HOST_H_
#define DSPN_PNG_DEFLATE_HOST_H_

#include <stdint.h>

#if defined(__HIPCC__)
#define DSPN_PD_HD __host__ __device__ inline
#else
#define DSPN_PD_HD inline
#endif

namespace dspn_png_deflate {

constexpr int kBlock = 32768;              // DSPN_PNG_DEFLATE_BLOCK
constexpr int kLitLen = 286, kClen = 19, kEob = 256;
constexpr int kLitLenLimit = 15, kClenLimit = 7;
constexpr int kMaxHeaderSyms = 288;        // HLIT + 1 lengths, one symbol each at the most
constexpr unsigned kAdlerMod = 65521;
constexpr int kModeDynamic = 2, kModeStored = 0;

// bytes of a zlib stream around `bytes` input bytes at the most (include/dspn_png_encode.h derives it)
DSPN_PD_HD long long bound(long long bytes) { return bytes + 6 * ((bytes + kBlock - 1) / kBlock) + 7; }

struct Token { int sym, ebits, eval; };    // sym < 0: the byte lies inside a match piece; ebits > 0 or sym > 256: a match

DSPN_PD_HD int length_extra_bits(int sym) { return sym < 265 || sym == 285 ? 0 : (sym - 261) >> 2; }

DSPN_PD_HD Token token_at(int byte, int j, int r) {
  if (j == 0) return {byte, 0, 0};
  const int p = (j - 1) % 258, left = r - (j - p), len = left < 258 ? left : 258;
  if (len < 3) return {byte, 0, 0};
  if (p) return {-1, 0, 0};
  if (len == 258) return {285, 0, 0};
  const int l = len - 3;
  if (l < 8) return {257 + l, 0, 0};
  int e = 1;
  while ((l >> (e + 3)) != 0) ++e;         // e = floor(log2 l) - 2
  return {261 + 4 * e + ((l >> e) & 3), e, l & ((1 << e) - 1)};
}

// work memory of the planner: one per block being planned
struct Work {
  unsigned weight[kLitLen];                // internal nodes: weights, then depths
  unsigned short parent[2 * kLitLen];      // of leaf i of the order at [i], of internal node k at [used + k]
  unsigned short order[kLitLen];           // used symbols, ascending (count, symbol)
  unsigned short level[16];                // symbols per code length; next code per length
  unsigned clen_count[kClen];
};

// -> the number of used symbols; order[0 .. used) ascending by (count, symbol)
DSPN_PD_HD int sort_symbols(const unsigned *counts, int n, unsigned short *order) {
  int used = 0;
  for (int s = 0; s < n; ++s) {
    const unsigned c = counts[s];
    if (!c) continue;
    int at = used++;
    while (at > 0 && counts[order[at - 1]] > c) { order[at] = order[at - 1]; --at; }   // later symbols go behind equal counts
    order[at] = (unsigned short)s;
  }
  return used;
}

// lengths[0 .. n) from counts and their order; the sum of the counts must fit 32 bits, used <= 2^limit
DSPN_PD_HD void code_lengths_sorted(const unsigned *counts, int n, int limit, int used, Work &w, unsigned char *lengths) {
  for (int s = 0; s < n; ++s) lengths[s] = 0;
  if (used == 0) return;
  if (used == 1) { lengths[w.order[0]] = 1; return; }
  int li = 0, qi = 0;
  for (int k = 0; k < used - 1; ++k) {     // internal node k; nodes 0 .. k - 1 wait in weight order
    unsigned sum = 0;
    for (int t = 0; t < 2; ++t) {
      if (li < used && (qi >= k || counts[w.order[li]] <= w.weight[qi])) { sum += counts[w.order[li]]; w.parent[li++] = (unsigned short)k; }
      else { sum += w.weight[qi]; w.parent[used + qi++] = (unsigned short)k; }
    }
    w.weight[k] = sum;
  }
  w.weight[used - 2] = 0;                  // the root's depth
  for (int k = used - 3; k >= 0; --k) w.weight[k] = w.weight[w.parent[used + k]] + 1;
  for (int b = 0; b <= 15; ++b) w.level[b] = 0;
  for (int i = 0; i < used; ++i) {
    const int d = (int)w.weight[w.parent[i]] + 1;
    ++w.level[d < limit ? d : limit];
  }
  long long excess = -(1LL << limit);      // Kraft sum - 1 in units of 2^-limit
  for (int b = 1; b <= limit; ++b) excess += (long long)w.level[b] << (limit - b);
  for (; excess > 0; --excess) {
    int b = limit - 1;
    while (b > 0 && w.level[b] == 0) --b;
    if (b == 0) break;                     // cannot happen with used <= 2^limit
    --w.level[b];
    w.level[b + 1] += 2;
    --w.level[limit];
  }
  int at = 0;
  for (int b = limit; b >= 1; --b)
    for (int c = w.level[b]; c > 0; --c) lengths[w.order[at++]] = (unsigned char)b;
}

DSPN_PD_HD unsigned reverse_bits(unsigned code, int len) {
  unsigned r = 0;
  for (int i = 0; i < len; ++i) r |= ((code >> i) & 1u) << (len - 1 - i);
  return r;
}

// canonical codes of RFC 1951 3.2.2, bit-reversed; next: 16 entries of work memory
DSPN_PD_HD void build_codes(const unsigned char *lengths, int n, unsigned short *next, unsigned short *codes) {
  for (int b = 0; b <= 15; ++b) next[b] = 0;
  for (int s = 0; s < n; ++s) ++next[lengths[s]];
  unsigned code = 0, before = 0;
  next[0] = 0;
  for (int b = 1; b <= 15; ++b) {
    code = (code + before) << 1;
    before = next[b];
    next[b] = (unsigned short)code;
  }
  for (int s = 0; s < n; ++s) {
    const int len = lengths[s];
    codes[s] = len ? (unsigned short)reverse_bits(next[len]++, len) : 0;
  }
}

// what the planner leaves for a block: 920 bytes
struct BlockPlan {
  unsigned bits;                           // of the dynamic form, header and end-of-block symbol included
  unsigned header_bits;                    // of those, in front of the first token
  unsigned short mode, hlit, hclen, nsym;  // hlit: literal/length codes sent (257 ..), hclen: code-length codes sent (4 ..)
  unsigned long long sum2;                 // Adler-32 partials of the block: the sum of (bytes - i) * d[i], and
  unsigned sum1, reserved;                 // the sum of d[i]
  unsigned char ll_len[288];
  unsigned char cl_len[24];
  unsigned short hsym[kMaxHeaderSyms];     // symbol | extra value << 8
};
static_assert(sizeof(BlockPlan) == 920, "BlockPlan layout");

DSPN_PD_HD int clen_order(int i) {         // the order the code-length code's lengths are sent in
  return i < 3 ? 16 + i : (i == 3 ? 0 : ((i & 1) ? 7 - ((i - 5) >> 1) : 6 + (i >> 1)));
}
DSPN_PD_HD int clen_extra_bits(int sym) { return sym == 16 ? 2 : (sym == 17 ? 3 : (sym == 18 ? 7 : 0)); }

// the sequence ll_len[0 .. hlit), 1 -> hsym; the number of symbols
DSPN_PD_HD int header_symbols(const unsigned char *ll_len, int hlit, unsigned short *hsym) {
  int n = 0, i = 0;
  const int total = hlit + 1;
  while (i < total) {
    const int v = i < hlit ? ll_len[i] : 1;
    int r = 1;
    while (i + r < total && (i + r < hlit ? ll_len[i + r] : 1) == v) ++r;
    i += r;
    if (v == 0) {
      while (r >= 11) { const int t = r < 138 ? r : 138; hsym[n++] = (unsigned short)(18 | (t - 11) << 8); r -= t; }
      if (r >= 3) { hsym[n++] = (unsigned short)(17 | (r - 3) << 8); r = 0; }
      for (; r > 0; --r) hsym[n++] = 0;
    } else {
      hsym[n++] = (unsigned short)v;
      --r;
      while (r >= 3) { const int t = r < 6 ? r : 6; hsym[n++] = (unsigned short)(16 | (t - 3) << 8); r -= t; }
      for (; r > 0; --r) hsym[n++] = (unsigned short)v;
    }
  }
  return n;
}

// hist: the block's 286 counters, end-of-block counted; w.order[0 .. used) their order.  Fills everything of p but the sums.
DSPN_PD_HD void plan_block(const unsigned *hist, int bytes, int used, Work &w, BlockPlan &p) {
  code_lengths_sorted(hist, kLitLen, kLitLenLimit, used, w, p.ll_len);
  p.ll_len[286] = p.ll_len[287] = 0;
  int hlit = 257;
  for (int s = 257; s < kLitLen; ++s)
    if (p.ll_len[s]) hlit = s + 1;
  const int nsym = header_symbols(p.ll_len, hlit, p.hsym);
  for (int s = 0; s < kClen; ++s) w.clen_count[s] = 0;
  for (int i = 0; i < nsym; ++i) ++w.clen_count[p.hsym[i] & 255];
  const int clen_used = sort_symbols(w.clen_count, kClen, w.order);
  code_lengths_sorted(w.clen_count, kClen, kClenLimit, clen_used, w, p.cl_len);
  for (int s = kClen; s < 24; ++s) p.cl_len[s] = 0;
  int hclen = 4;
  for (int i = 4; i < kClen; ++i)
    if (p.cl_len[clen_order(i)]) hclen = i + 1;
  unsigned long long bits = 3 + 5 + 5 + 4 + 3 * (unsigned)hclen;
  for (int s = 0; s < kClen; ++s) bits += (unsigned long long)w.clen_count[s] * (unsigned)(p.cl_len[s] + clen_extra_bits(s));
  p.header_bits = (unsigned)bits;
  for (int s = 0; s < kLitLen; ++s)
    bits += (unsigned long long)hist[s] * (unsigned)(p.ll_len[s] + (s > 256 ? length_extra_bits(s) + 1 : 0));   // + the distance bit
  // the code-length code of one symbol alone would be incomplete, which inflate refuses; it cannot arise (zero and non-zero
  // lengths both occur), and is stored if it ever does
  const bool dynamic = clen_used >= 2 && bits <= 8ULL * ((unsigned)bytes + 5);
  p.bits = dynamic ? (unsigned)bits : 0;
  p.mode = dynamic ? kModeDynamic : kModeStored;
  p.hlit = (unsigned short)hlit;
  p.hclen = (unsigned short)hclen;
  p.nsym = (unsigned short)nsym;
}

// the low `len` bits of v and len for a token: code, extra bits, and the distance code's one zero bit behind a length
DSPN_PD_HD void token_bits(const Token &t, const unsigned short *codes, const unsigned char *lengths, unsigned &v, int &len) {
  const int cl = lengths[t.sym];
  v = codes[t.sym] | (unsigned)t.eval << cl;
  len = cl + t.ebits + (t.sym > 256 ? 1 : 0);
}

// the header of a dynamic block through Sink::put(bit position, value, bits); cl_codes: the code-length code.  -> the position behind
template <typename Sink>
DSPN_PD_HD long long put_dynamic_header(Sink &s, long long pos, const BlockPlan &p, const unsigned short *cl_codes, bool last) {
  s.put(pos, (last ? 1u : 0u) | 2u << 1, 3); pos += 3;
  s.put(pos, (unsigned)(p.hlit - 257), 5); pos += 5;
  s.put(pos, 0u, 5); pos += 5;
  s.put(pos, (unsigned)(p.hclen - 4), 4); pos += 4;
  for (int i = 0; i < p.hclen; ++i) { s.put(pos, p.cl_len[clen_order(i)], 3); pos += 3; }
  for (int i = 0; i < p.nsym; ++i) {
    const int sym = p.hsym[i] & 255, cl = p.cl_len[sym], eb = clen_extra_bits(sym);
    s.put(pos, cl_codes[sym] | (unsigned)(p.hsym[i] >> 8) << cl, cl + eb);
    pos += cl + eb;
  }
  return pos;
}

// the header of a stored block: three bits, zeros up to a whole byte, LEN and its complement.  -> the position of the first byte
template <typename Sink>
DSPN_PD_HD long long put_stored_header(Sink &s, long long pos, int bytes, bool last) {
  s.put(pos, last ? 1u : 0u, 3);
  pos = (pos + 3 + 7) & ~7LL;
  s.put(pos, (unsigned)bytes | (~(unsigned)bytes & 0xFFFFu) << 16, 32);
  return pos + 32;
}

// bits a stored block takes from bit position pos
DSPN_PD_HD long long stored_end(long long pos, int bytes) { return ((pos + 3 + 7) & ~7LL) + 32 + 8LL * bytes; }

// Adler-32 of a stream from the partials of its pieces: a = 1 + sum of sum1, b = bytes + sum of (sum2 + bytes behind * sum1)
DSPN_PD_HD unsigned adler_term(unsigned sum1, unsigned long long sum2, long long behind) {
  return (unsigned)((sum2 % kAdlerMod + (unsigned long long)(behind % kAdlerMod) * (sum1 % kAdlerMod)) % kAdlerMod);
}

// ---- the host encoder ----
struct ByteSink {
  unsigned char *out;                      // zeroed
  void put(long long pos, unsigned v, int len) {
    unsigned long long x = (unsigned long long)v << (pos & 7);
    for (long long at = pos >> 3, end = (pos + len + 7) >> 3; at < end; ++at, x >>= 8) out[at] |= (unsigned char)x;
  }
};

// one zlib stream over data[0 .. bytes) into out (capacity >= bound(bytes), zeroed here); -> its length
inline long long deflate_stream(const unsigned char *data, long long bytes, unsigned char *out) {
  const long long cap = bound(bytes);
  for (long long i = 0; i < cap; ++i) out[i] = 0;
  ByteSink sink{out};
  sink.put(0, 0x78, 8);
  sink.put(8, 0x01, 8);
  long long pos = 16;
  unsigned long long a = 1, b = (unsigned long long)(bytes % kAdlerMod);
  static thread_local Work w;
  static thread_local BlockPlan p;
  static thread_local unsigned hist[kLitLen];
  static thread_local unsigned short codes[kLitLen], cl_codes[kClen], next[16];
  for (long long base = 0; base < bytes; base += kBlock) {
    const unsigned char *d = data + base;
    const int n = (int)(bytes - base < kBlock ? bytes - base : kBlock);
    const bool last = base + n == bytes;
    for (int s = 0; s < kLitLen; ++s) hist[s] = 0;
    hist[kEob] = 1;
    unsigned sum1 = 0;
    unsigned long long sum2 = 0;
    for (int i = 0, s = 0, e = 0; i < n; ++i) {
      if (i == e) { s = i; for (e = i + 1; e < n && d[e] == d[s]; ++e) {} }
      const Token t = token_at(d[i], i - s, e - s);
      if (t.sym >= 0) ++hist[t.sym];
      sum1 += d[i];
      sum2 += (unsigned long long)(n - i) * d[i];
    }
    a += sum1;
    b += adler_term(sum1, sum2, bytes - base - n);
    plan_block(hist, n, sort_symbols(hist, kLitLen, w.order), w, p);
    if (p.mode == kModeStored) {
      pos = put_stored_header(sink, pos, n, last);
      for (int i = 0; i < n; ++i) out[(pos >> 3) + i] = d[i];
      pos += 8LL * n;
      continue;
    }
    build_codes(p.cl_len, kClen, next, cl_codes);
    build_codes(p.ll_len, kLitLen, next, codes);
    const long long end = pos + p.bits;
    pos = put_dynamic_header(sink, pos, p, cl_codes, last);
    for (int i = 0, s = 0, e = 0; i < n; ++i) {
      if (i == e) { s = i; for (e = i + 1; e < n && d[e] == d[s]; ++e) {} }
      const Token t = token_at(d[i], i - s, e - s);
      if (t.sym < 0) continue;
      unsigned v;
      int len;
      token_bits(t, codes, p.ll_len, v, len);
      sink.put(pos, v, len);
      pos += len;
    }
    sink.put(pos, codes[kEob], p.ll_len[kEob]);
    pos += p.ll_len[kEob];
    if (pos != end) return -1;             // the plan's count and the writer disagree: a bug, never a property of the data
  }
  pos = (pos + 7) & ~7LL;
  const unsigned adler = (unsigned)(b % kAdlerMod) << 16 | (unsigned)(a % kAdlerMod);
  for (int i = 0; i < 4; ++i) out[(pos >> 3) + i] = (unsigned char)(adler >> (24 - 8 * i));
  return (pos >> 3) + 4;
}

}  // namespace dspn_png_deflate
#endif  // DSPN_PNG_DEFLATE_HOST_H_

// Stand-alone check of the host half of the JPEG encode (dspnet_amd/csrc/jpeg_encode_host.h) for the host sanitizers:
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_encode_host_check.cpp -o jpeg_encode_host_check
//   ./jpeg_encode_host_check a.jpg b.jpg ...
// Every file named is a baseline stream with standard Huffman tables and no restart markers, as Pillow writes it by default.
// Its coefficients are read back with the decoder's host half, the blocks of the real grids are copied into an exactly-sized
// heap buffer, and the entropy encoder must reproduce the file byte for byte in an exactly-sized output buffer; then again
// with every capacity from 0 to one byte short (a write past the capacity is a heap overflow the sanitizer sees), each of
// which must be refused with the needed size.  The header writer alone (encode_headers, with and without a DRI segment) goes
// through the same capacities and must give the file's prefix.  The quantisation tables of every quality are formed as well.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../dspnet_amd/csrc/jpeg_encode_host.h"

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s stream.jpg ...\n", argv[0]); return 2; }
  char err[256] = "";
  for (int q = -1; q <= 102; ++q) {
    unsigned char *lum = static_cast<unsigned char *>(malloc(64)), *chr = static_cast<unsigned char *>(malloc(64));
    const int rc = dspn_jpeg_enc::quant_tables(q, lum, chr, err, sizeof(err));
    if ((rc == 0) != (q >= 1 && q <= 100)) { fprintf(stderr, "quality %d: status %d\n", q, rc); return 1; }
    free(lum); free(chr);
  }
  long refused = 0;
  for (int a = 1; a < argc; ++a) {
    FILE *f = fopen(argv[a], "rb");
    if (!f) { perror(argv[a]); return 2; }
    std::vector<unsigned char> data;
    unsigned char chunk[65536];
    size_t got;
    while ((got = fread(chunk, 1, sizeof(chunk), f)) > 0) data.insert(data.end(), chunk, chunk + got);
    fclose(f);
    dspn_jpeg_info info;
    if (dspn_jpeg::probe(data.data(), data.size(), &info, err, sizeof(err)) || !info.supported) {
      fprintf(stderr, "%s: not a supported stream (%s)\n", argv[a], err);
      return 1;
    }
    std::vector<int16_t> padded((size_t)info.coef_count);
    if (dspn_jpeg::entropy_decode(data.data(), data.size(), &info, padded.data(), err, sizeof(err))) {
      fprintf(stderr, "%s: %s\n", argv[a], err);
      return 1;
    }
    dspn_jpeg_enc_sample s;
    memset(&s, 0, sizeof(s));
    s.width = info.width; s.height = info.height; s.ncomp = info.ncomp; s.hsamp = info.hsamp[0]; s.vsamp = info.vsamp[0];
    long long count = 0;
    if (dspn_jpeg_enc::fill_geometry(&s, 0, &count, err, sizeof(err))) { fprintf(stderr, "%s: %s\n", argv[a], err); return 1; }
    memcpy(s.quant, info.quant, sizeof(s.quant));
    int16_t *real = static_cast<int16_t *>(malloc(sizeof(int16_t) * (size_t)count));      // exactly the real grids
    for (int c = 0; c < s.ncomp; ++c)
      for (int by = 0; by < s.blocks_h[c]; ++by)
        memcpy(real + s.coef_offset[c] + 64LL * by * s.blocks_w[c], padded.data() + info.coef_offset[c] + 64LL * by * info.blocks_w[c],
               sizeof(int16_t) * 64 * (size_t)s.blocks_w[c]);
    for (size_t cap = 0; cap <= data.size(); ++cap) {
      unsigned char *out = static_cast<unsigned char *>(malloc(cap ? cap : 1));
      size_t n = 0;
      const int rc = dspn_jpeg_enc::entropy_encode(real, &s, out, cap, &n, err, sizeof(err));
      if (n != data.size()) { fprintf(stderr, "%s: length %zu, the file has %zu\n", argv[a], n, data.size()); return 1; }
      if (cap < data.size()) {
        if (rc != dspn_jpeg_enc::kTooSmall || !strstr(err, "needs")) { fprintf(stderr, "%s: capacity %zu gave status %d\n", argv[a], cap, rc); return 1; }
        ++refused;
      } else if (rc != 0) {
        fprintf(stderr, "%s: %s\n", argv[a], err);
        return 1;
      }
      if (memcmp(out, data.data(), cap)) { fprintf(stderr, "%s: bytes differ (capacity %zu)\n", argv[a], cap); return 1; }
      free(out);
    }
    free(real);
    // the headers alone (dspn_jpeg_encode_headers): the file's prefix up to the scan, with and without a DRI segment, at every capacity
    for (int interval = 0; interval <= 5; interval += 5) {
      size_t need = 0;
      if (dspn_jpeg_enc::encode_headers(&s, interval, nullptr, 0, &need, err, sizeof(err)) != dspn_jpeg_enc::kTooSmall || !need) {
        fprintf(stderr, "%s: the headers' size was not named\n", argv[a]);
        return 1;
      }
      unsigned char *whole = static_cast<unsigned char *>(malloc(need));
      size_t n = 0;
      if (dspn_jpeg_enc::encode_headers(&s, interval, whole, need, &n, err, sizeof(err)) || n != need) { fprintf(stderr, "%s: %s\n", argv[a], err); return 1; }
      if (interval == 0 && (need + 2 > data.size() || memcmp(whole, data.data(), need))) { fprintf(stderr, "%s: the headers are not the file's prefix\n", argv[a]); return 1; }
      for (size_t cap = 0; cap < need; ++cap) {
        unsigned char *out = static_cast<unsigned char *>(malloc(cap ? cap : 1));
        const int rc = dspn_jpeg_enc::encode_headers(&s, interval, out, cap, &n, err, sizeof(err));
        if (rc != dspn_jpeg_enc::kTooSmall || n != need || memcmp(out, whole, cap)) { fprintf(stderr, "%s: headers at capacity %zu gave status %d\n", argv[a], cap, rc); return 1; }
        ++refused;
        free(out);
      }
      free(whole);
    }
    printf("%s: %zu bytes reproduced\n", argv[a], data.size());
  }
  printf("jpeg_encode_host_check: ok (%ld short capacities refused)\n", refused);
  return 0;
}

// Stand-alone check of the scan index (dspnet_amd/csrc/jpeg_host.h) and of the device's Huffman decode built for the host
// (dspnet_amd/csrc/jpeg_huff.h: the text the kernel runs) for the host sanitizers:
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_huff_check.cpp -o jpeg_huff_check
//   ./jpeg_huff_check a.jpg b.jpg ...            (small streams WITH restart intervals)
// For every file named it runs probe, scan index and the segment decode on the whole stream, on EVERY truncation of it, on
// every single-bit flip, on every byte set to 0x00 and to 0xFF, and with 1..8 bytes cut out in front of every restart marker
// -- each from an exactly-sized heap copy (a read past the end is a heap overflow the sanitizer sees), into an exactly-sized
// segment table and an exactly-sized coefficient buffer.  The whole stream must decode to the host entropy pass's
// coefficients; every damaged one must be refused by the index with a message, or leave a status word, or -- where the host
// entropy pass decodes it too -- give that pass's coefficients.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../dspnet_amd/csrc/jpeg_host.h"
#include "../dspnet_amd/csrc/jpeg_huff.h"

struct Tally { long runs = 0, refused = 0, flagged = 0, decoded = 0; };

// -> 0: decoded (coefficients in *keep), 1: refused by probe or index, 2: a status word
static int run(const unsigned char *src, size_t n, std::vector<int16_t> *keep, Tally &tally) {
  unsigned char *copy = static_cast<unsigned char *>(malloc(n ? n : 1));   // exactly n bytes: no slack behind the stream
  if (n) memcpy(copy, src, n);
  char err[256] = "";
  dspn_jpeg_info info;
  int result = 1;
  ++tally.runs;
  int rc = dspn_jpeg::probe(copy, n, &info, err, sizeof(err));
  if (rc == 0 && info.supported && dspn_jpeg::scan_segments(info) > 0) {
    const size_t nseg = (size_t)dspn_jpeg::scan_segments(info) + 1;
    unsigned *seg = static_cast<unsigned *>(malloc(sizeof(unsigned) * nseg));
    dspn_jpeg_scan scan;
    rc = dspn_jpeg::scan_index(copy, n, &info, &scan, seg, nseg, err, sizeof(err));
    if (rc == 0) {
      dspn_jpeg_sample s;
      memset(&s, 0, sizeof(s));
      for (int c = 0; c < 3; ++c) { s.coef_offset[c] = info.coef_offset[c]; s.blocks_w[c] = info.blocks_w[c]; s.blocks_h[c] = info.blocks_h[c]; }
      s.width = info.width; s.height = info.height; s.ncomp = info.ncomp; s.hsamp = info.hsamp[0]; s.vsamp = info.vsamp[0];
      int16_t *coef = static_cast<int16_t *>(malloc(sizeof(int16_t) * (size_t)info.coef_count));
      memset(coef, 0x5A, sizeof(int16_t) * (size_t)info.coef_count);
      const int status = dspn_jpeg_huff::decode_sample(copy, (long long)n, s, scan, seg, (long long)nseg, coef, info.coef_count);
      result = status ? 2 : 0;
      if (status == 0) {
        int16_t *host = static_cast<int16_t *>(malloc(sizeof(int16_t) * (size_t)info.coef_count));
        char err2[256] = "";
        if (dspn_jpeg::entropy_decode(copy, n, &info, host, err2, sizeof(err2)) == 0 &&
            memcmp(host, coef, sizeof(int16_t) * (size_t)info.coef_count)) {
          fprintf(stderr, "both passes decode the stream, to different coefficients\n");
          exit(1);
        }
        free(host);
        if (keep) keep->assign(coef, coef + info.coef_count);
      }
      free(coef);
    }
    free(seg);
  }
  if (result == 1 && rc != 0 && strlen(err) < 6) { fprintf(stderr, "status %d without a message\n", rc); exit(2); }
  free(copy);
  if (result == 0) ++tally.decoded; else if (result == 1) ++tally.refused; else ++tally.flagged;
  return result;
}

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s stream.jpg ...\n", argv[0]); return 2; }
  Tally tally;
  for (int a = 1; a < argc; ++a) {
    FILE *f = fopen(argv[a], "rb");
    if (!f) { perror(argv[a]); return 2; }
    std::vector<unsigned char> data;
    unsigned char chunk[65536];
    size_t got;
    while ((got = fread(chunk, 1, sizeof(chunk), f)) > 0) data.insert(data.end(), chunk, chunk + got);
    fclose(f);
    std::vector<int16_t> whole;
    Tally first;
    if (run(data.data(), data.size(), &whole, first) != 0) { fprintf(stderr, "%s does not decode\n", argv[a]); return 1; }
    dspn_jpeg_info info;
    char err[256];
    dspn_jpeg::probe(data.data(), data.size(), &info, err, sizeof(err));
    std::vector<int16_t> host((size_t)info.coef_count);
    if (dspn_jpeg::entropy_decode(data.data(), data.size(), &info, host.data(), err, sizeof(err)) || host != whole) {
      fprintf(stderr, "%s: not the host entropy pass's coefficients\n", argv[a]);
      return 1;
    }
    printf("%s: %zu bytes, %lld restart intervals, decoded\n", argv[a], data.size(), dspn_jpeg::scan_segments(info));
    for (size_t cut = 0; cut < data.size(); ++cut) run(data.data(), cut, nullptr, tally);
    std::vector<unsigned char> bad(data);
    for (size_t at = 0; at < data.size(); ++at) {
      for (int k = 0; k < 10; ++k) {
        const unsigned char v = k < 8 ? (unsigned char)(data[at] ^ (1u << k)) : (k == 8 ? 0x00 : 0xFF);
        if (v == data[at]) continue;
        bad[at] = v;
        run(bad.data(), bad.size(), nullptr, tally);
      }
      bad[at] = data[at];
    }
    for (size_t at = 2; at + 1 < data.size(); ++at)
      if (data[at] == 0xFF && data[at + 1] >= 0xD0 && data[at + 1] <= 0xD7)
        for (size_t k = 1; k <= 8 && k < at; ++k) {
          std::vector<unsigned char> shorter(data.begin(), data.begin() + (at - k));
          shorter.insert(shorter.end(), data.begin() + at, data.end());
          run(shorter.data(), shorter.size(), nullptr, tally);
        }
  }
  printf("jpeg_huff_check: ok (%ld damaged streams: %ld refused, %ld left a status word, %ld decoded)\n", tally.runs, tally.refused,
         tally.flagged, tally.decoded);
  return 0;
}

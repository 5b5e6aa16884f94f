// Stand-alone check of the host half of the JPEG decode (dspnet_amd/csrc/jpeg_host.h) for the host sanitizers:
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_host_check.cpp -o jpeg_host_check
//   ./jpeg_host_check a.jpg b.jpg ...
// For every file named it runs probe and entropy decode on the whole stream and on EVERY truncation of it, each from an
// exactly-sized heap copy (so a read past the end is a heap overflow the sanitizer sees) into an exactly-sized coefficient
// buffer.  The whole stream must decode; every truncation must either fail with a message or (the last bytes only: EOI and
// what follows it) decode to the same coefficients.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../dspnet_amd/csrc/jpeg_host.h"

static int run(const unsigned char *src, size_t n, std::vector<int16_t> *keep, bool *decoded) {
  unsigned char *copy = static_cast<unsigned char *>(malloc(n ? n : 1));   // exactly n bytes: no slack behind the stream
  if (n) memcpy(copy, src, n);
  char err[256] = "";
  dspn_jpeg_info info;
  *decoded = false;
  int rc = dspn_jpeg::probe(copy, n, &info, err, sizeof(err));
  if (rc == 0 && info.supported) {
    int16_t *coef = static_cast<int16_t *>(malloc(sizeof(int16_t) * (size_t)info.coef_count));
    rc = dspn_jpeg::entropy_decode(copy, n, &info, coef, err, sizeof(err));
    if (rc == 0) {
      *decoded = true;
      if (keep) keep->assign(coef, coef + info.coef_count);
    }
    free(coef);
  }
  if (rc != 0 && strlen(err) < 6) { fprintf(stderr, "status %d without a message\n", rc); exit(2); }
  free(copy);
  return rc;
}

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s stream.jpg ...\n", argv[0]); return 2; }
  long total = 0, refused = 0;
  for (int a = 1; a < argc; ++a) {
    FILE *f = fopen(argv[a], "rb");
    if (!f) { perror(argv[a]); return 2; }
    std::vector<unsigned char> data;
    unsigned char chunk[65536];
    size_t got;
    while ((got = fread(chunk, 1, sizeof(chunk), f)) > 0) data.insert(data.end(), chunk, chunk + got);
    fclose(f);
    std::vector<int16_t> whole, part;
    bool decoded = false;
    const int rc = run(data.data(), data.size(), &whole, &decoded);
    printf("%s: %zu bytes, status %d%s\n", argv[a], data.size(), rc, decoded ? ", decoded" : "");
    for (size_t cut = 0; cut < data.size(); ++cut) {
      bool ok = false;
      const int r = run(data.data(), cut, &part, &ok);
      ++total;
      if (r != 0) ++refused;
      if (ok && part != whole) { fprintf(stderr, "%s cut at %zu decoded to other coefficients\n", argv[a], cut); return 1; }
    }
  }
  printf("jpeg_host_check: ok (%ld truncations, %ld refused)\n", total, refused);
  return 0;
}

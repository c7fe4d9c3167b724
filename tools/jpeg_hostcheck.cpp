// Stand-alone robustness check of the host JPEG entropy decoder, for a sanitizer build
// (CPU only; the decoder makes no GPU call):
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude tools/jpeg_hostcheck.cpp styletransfer_amd/csrc/jpeg_host.cpp -o jpeg_hostcheck
//   ./jpeg_hostcheck a.jpg b.jpg ...
//
// For every file: the whole stream, the stream cut at every length, and the stream with
// each byte after the SOS marker replaced in turn by 3 other values (and each header byte
// by one).  Input and output live in exact-size heap blocks, so AddressSanitizer sees a
// read past len or a write past coef_bytes; the decoder has to answer with a status every
// time.  Exit status 0 and a line of counts per file when nothing tripped.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "stx.h"

static int decode(const uint8_t* data, size_t len, size_t coef_bytes, int ncomp) {
  // exact-size copies: the redzones sit right behind the last valid byte
  uint8_t* in = (uint8_t*)malloc(len ? len : 1);
  if (len) memcpy(in, data, len);
  short* coef = (short*)malloc(coef_bytes ? coef_bytes : 1);
  unsigned short* qtab = (unsigned short*)malloc((size_t)(ncomp > 0 ? ncomp : 1) * 128);
  stx_jpeg_desc d;
  const int si = stx_jpeg_info(len ? in : nullptr, len, &d);
  int st = stx_jpeg_entropy_decode(len ? in : nullptr, len, coef, coef_bytes, qtab);
  if (si != STX_JPEG_OK && st == STX_JPEG_OK) {
    fprintf(stderr, "decode succeeded where the info query failed (%d)\n", si);
    exit(2);
  }
  if (st == STX_JPEG_OK && (size_t)d.coef_bytes > coef_bytes) {
    fprintf(stderr, "decode succeeded into a buffer that is too small\n");
    exit(2);
  }
  free(in);
  free(coef);
  free(qtab);
  return st;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s file.jpg ...\n", argv[0]);
    return 1;
  }
  for (int a = 1; a < argc; ++a) {
    FILE* f = fopen(argv[a], "rb");
    if (!f) {
      perror(argv[a]);
      return 1;
    }
    std::vector<uint8_t> buf;
    uint8_t chunk[65536];
    size_t n;
    while ((n = fread(chunk, 1, sizeof(chunk), f)) > 0) buf.insert(buf.end(), chunk, chunk + n);
    fclose(f);
    stx_jpeg_desc d;
    if (stx_jpeg_info(buf.data(), buf.size(), &d) != STX_JPEG_OK) {
      printf("%s: not decodable here (status %d), only cut and flipped\n", argv[a], d.status);
      d.coef_bytes = 4096;
      d.ncomp = 3;
    } else if (decode(buf.data(), buf.size(), (size_t)d.coef_bytes, d.ncomp) != STX_JPEG_OK) {
      fprintf(stderr, "%s: the intact file does not decode\n", argv[a]);
      return 2;
    }
    long counts[4] = {0, 0, 0, 0};
    const size_t cb = (size_t)d.coef_bytes;
    for (size_t len = 0; len < buf.size(); ++len) {
      const int st = decode(buf.data(), len, cb, d.ncomp);
      if (st == STX_JPEG_OK) {
        fprintf(stderr, "%s: a %zu-byte prefix decoded as if whole\n", argv[a], len);
        return 2;
      }
      counts[st & 3]++;
    }
    size_t sos = 0;
    while (sos + 1 < buf.size() && !(buf[sos] == 0xFF && buf[sos + 1] == 0xDA)) ++sos;
    uint32_t rng = 12345u + (uint32_t)a;
    for (size_t pos = 0; pos < buf.size(); ++pos) {
      const uint8_t keep = buf[pos];
      for (int k = 0; k < (pos >= sos ? 3 : 1); ++k) {
        rng = rng * 1664525u + 1013904223u;
        buf[pos] = (uint8_t)(keep ^ (1 + (rng >> 24) % 255));
        counts[decode(buf.data(), buf.size(), cb, d.ncomp) & 3]++;
      }
      buf[pos] = keep;
    }
    // a buffer that is too small is refused, whatever the stream
    if (cb >= 128 && decode(buf.data(), buf.size(), cb - 128, d.ncomp) == STX_JPEG_OK) {
      fprintf(stderr, "%s: decoded into a short buffer\n", argv[a]);
      return 2;
    }
    printf("%s: %zu bytes, ok %ld unsupported %ld corrupt %ld bad-args %ld\n", argv[a], buf.size(),
           counts[0], counts[1], counts[2], counts[3]);
  }
  return 0;
}

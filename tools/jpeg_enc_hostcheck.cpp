// Stand-alone robustness check of the host JPEG entropy encoder, for a sanitizer build
// (CPU only; the encoder makes no GPU call):
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude tools/jpeg_enc_hostcheck.cpp styletransfer_amd/csrc/jpeg_host.cpp \
//       -o jpeg_enc_hostcheck
//   ./jpeg_enc_hostcheck
//
// For a few geometries (1 and 3 components, the three samplings, sizes with dummy blocks):
// coefficient arrays that a conforming encoder could produce (sparse, bounded), dense
// arrays at the limits and hostile arrays (any int16), each from an exact-size heap block
// into an exact-size output block, so AddressSanitizer sees a read past coef_bytes or a
// write past cap.  A file that was written has to decode back (stx_jpeg_entropy_decode) to
// the same coefficients and tables and has to fit the bound.  Then, for the bounded arrays,
// every cap from 0 up to the file's size (strided in the middle of a file over 2 KiB): one
// byte short is refused, the exact size passes.
// Exit status 0 and a line of counts per geometry when nothing tripped.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "stx.h"

static uint32_t rng_state = 2463534242u;
static uint32_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 17;
  rng_state ^= rng_state << 5;
  return rng_state;
}

struct Geo {
  int h, w, ncomp, hmax, vmax;
};

static size_t grid_bytes(const Geo& g) {
  const size_t mx = (size_t)(g.w + 8 * g.hmax - 1) / (8 * g.hmax);
  const size_t my = (size_t)(g.h + 8 * g.vmax - 1) / (8 * g.vmax);
  return mx * my * (size_t)(g.ncomp == 1 ? 1 : g.hmax * g.vmax + 2) * 128;
}

// encode from exact-size copies; returns the status, the file in `file`
static int encode(const Geo& g, const std::vector<short>& coef, size_t coef_bytes,
                  const unsigned short* qtab, size_t cap, std::vector<uint8_t>* file) {
  short* in = (short*)malloc(coef_bytes ? coef_bytes : 1);
  memcpy(in, coef.data(), coef_bytes);
  unsigned short* q = (unsigned short*)malloc((size_t)g.ncomp * 128);
  memcpy(q, qtab, (size_t)g.ncomp * 128);
  uint8_t* out = (uint8_t*)malloc(cap ? cap : 1);
  size_t len = 777;
  const int st = stx_jpeg_entropy_encode(in, coef_bytes, g.h, g.w, g.ncomp, g.hmax, g.vmax, q,
                                         cap ? out : nullptr, cap, &len);
  if (st != STX_JPEG_OK && len != 0) {
    fprintf(stderr, "a refused call reported %zu bytes\n", len);
    exit(2);
  }
  if (st == STX_JPEG_OK && (len > cap || len < 4)) {
    fprintf(stderr, "a file of %zu bytes in a buffer of %zu\n", len, cap);
    exit(2);
  }
  if (file) file->assign(out, out + (st == STX_JPEG_OK ? len : 0));
  free(in);
  free(q);
  free(out);
  return st;
}

static void round_trip(const Geo& g, const std::vector<short>& coef, const unsigned short* qtab,
                       const std::vector<uint8_t>& file) {
  std::vector<short> back(coef.size());
  unsigned short q[3 * 64];
  stx_jpeg_desc d;
  if (stx_jpeg_info(file.data(), file.size(), &d) != STX_JPEG_OK || d.h != g.h || d.w != g.w ||
      d.ncomp != g.ncomp || (size_t)d.coef_bytes != coef.size() * 2) {
    fprintf(stderr, "the written file does not parse back to its geometry\n");
    exit(2);
  }
  if (stx_jpeg_entropy_decode(file.data(), file.size(), back.data(), back.size() * 2, q) !=
          STX_JPEG_OK ||
      memcmp(back.data(), coef.data(), coef.size() * 2) != 0 ||
      memcmp(q, qtab, (size_t)g.ncomp * 128) != 0) {
    fprintf(stderr, "the written file does not decode back to its coefficients\n");
    exit(2);
  }
}

int main() {
  const Geo geos[] = {{1, 1, 1, 1, 1},   {9, 17, 1, 1, 1},  {8, 8, 3, 1, 1},  {17, 33, 3, 1, 1},
                      {24, 40, 3, 2, 1}, {24, 40, 3, 2, 2}, {50, 100, 3, 2, 2}, {7, 9, 3, 2, 2}};
  unsigned short qtab[3 * 64];
  stx_jpeg_quant_tables(90, qtab);
  memcpy(qtab + 128, qtab + 64, 128);
  for (const Geo& g : geos) {
    const size_t bytes = grid_bytes(g), n = bytes / 2;
    const size_t bound = stx_jpeg_encode_bound(g.h, g.w, g.ncomp, g.hmax, g.vmax);
    if (!bound) {
      fprintf(stderr, "no bound for a supported geometry\n");
      return 2;
    }
    long ok = 0, refused = 0, caps = 0;
    std::vector<short> coef(n);
    std::vector<uint8_t> file;
    for (int round = 0; round < 60; ++round) {
      const int kind = round % 4;
      for (size_t i = 0; i < n; ++i) {
        const uint32_t r = rnd();
        if (kind == 0)       // sparse, small: what a picture gives
          coef[i] = (short)((r & 7) ? 0 : (int)((r >> 8) % 61) - 30);
        else if (kind == 1)  // dense at the limits (DC kept small: differences stay legal)
          coef[i] = (short)((i % 64) ? ((r & 1) ? 1023 : -1023) : (int)((r >> 8) % 2047) - 1023);
        else if (kind == 2)  // all ones: the longest runs of FF bytes
          coef[i] = (short)((i % 64) ? -1 : 0);
        else                 // hostile: any int16
          coef[i] = (short)(r >> 16);
      }
      const int st = encode(g, coef, bytes, qtab, bound, &file);
      if (kind != 3) {
        if (st != STX_JPEG_OK) {
          fprintf(stderr, "%dx%d: a legal array was refused (%d)\n", g.h, g.w, st);
          return 2;
        }
        round_trip(g, coef, qtab, file);
        ++ok;
        if (round < 8) {  // every cap up to the size (a long file: strided in its middle)
          std::vector<uint8_t> again;
          for (size_t cap = 0; cap <= file.size();
               cap += (cap < 1024 || cap + 1024 >= file.size()) ? 1 : 13, ++caps) {
            const int s2 = encode(g, coef, bytes, qtab, cap, &again);
            if ((s2 == STX_JPEG_OK) != (cap == file.size()) ||
                (s2 == STX_JPEG_OK && again != file)) {
              fprintf(stderr, "%dx%d: cap %zu of %zu gave %d\n", g.h, g.w, cap, file.size(), s2);
              return 2;
            }
          }
        }
      } else {
        if (st == STX_JPEG_OK) round_trip(g, coef, qtab, file); else ++refused;
      }
      // a coefficient array one value short is refused, whatever it holds
      if (encode(g, coef, bytes - 2, qtab, bound, nullptr) != STX_JPEG_BAD_ARGS) {
        fprintf(stderr, "%dx%d: a short coefficient array was taken\n", g.h, g.w);
        return 2;
      }
    }
    printf("%dx%d ncomp %d %dx%d: bound %zu, ok %ld, hostile refused %ld, caps tried %ld\n", g.h,
           g.w, g.ncomp, g.hmax, g.vmax, bound, ok, refused, caps);
  }
  return 0;
}

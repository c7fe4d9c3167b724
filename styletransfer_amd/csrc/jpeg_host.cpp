// Host half of the GPU JPEG decode: marker parsing and Huffman (entropy) decoding of
// baseline / extended-sequential 8-bit JPEGs into quantised DCT coefficients.  The
// device half (jpeg.hip) dequantises, runs the IDCT, upsamples and converts colours.
//
// Plain C++17: no HIP header, no HIP call -- loader workers run this and must never
// open the GPU.  Every read is bounded by `len`, every write by `coef_bytes`; a stream
// this decoder does not like is reported (UNSUPPORTED / CORRUPT) and the caller decodes
// it with its image library instead, so strictness costs nothing: anything libjpeg would
// only warn about (garbage before a restart marker, a missing EOI, a run past
// coefficient 63) is CORRUPT here.
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#if defined(__SSE2__)
#include <emmintrin.h>
#endif

#include "../../include/stx.h"

namespace {

// zigzag index -> natural (row-major) index
const uint8_t ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,
                            12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                            35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                            58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

constexpr int LOOK = 10;  // bits of the one-step Huffman lookup

struct Huff {
  bool defined = false;
  uint8_t counts[17];     // codes of each length 1..16
  uint8_t syms[256];
  uint16_t look[1 << LOOK];  // (length << 8) | symbol for codes of <= LOOK bits, else 0
  // AC only: a whole (run, size, value) that fits the lookup: (value << 8) | (run << 4) | total
  // bits, 0 when the code + its value bits do not fit (or the symbol is EOB / ZRL)
  int16_t fast[1 << LOOK];
  int32_t maxcode[18];    // largest code of each length, left-aligned to 16 bits, + 1
  int32_t delta[17];      // symbol index = (code >> (16 - l)) + delta[l]
};

struct Comp {
  int id = 0, hs = 0, vs = 0, tq = 0, td = 0, ta = 0;
};

struct Parsed {
  int h = 0, w = 0, ncomp = 0;
  Comp comp[3];
  int hmax = 1, vmax = 1;
  int bw[3] = {0, 0, 0}, bh[3] = {0, 0, 0};
  int mcux = 0, mcuy = 0;
  int restart = 0;
  bool have_q[4] = {false, false, false, false};
  uint16_t q[4][64];      // natural order
  Huff dc[4], ac[4];
  size_t scan = 0;        // offset of the entropy-coded data
  long long coef_bytes = 0;
};

// false: the table is not a prefix code libjpeg would accept
bool build_huff(Huff& h, bool is_ac) {
  int n = 0;
  for (int l = 1; l <= 16; ++l) n += h.counts[l];
  if (n > 256) return false;
  memset(h.look, 0, sizeof(h.look));
  memset(h.fast, 0, sizeof(h.fast));
  uint32_t code = 0;
  int k = 0;
  for (int l = 1; l <= 16; ++l) {
    h.delta[l] = k - (int32_t)code;
    if (code + h.counts[l] > (1u << l)) return false;
    for (int i = 0; i < h.counts[l]; ++i, ++k, ++code) {
      if (l <= LOOK) {
        const uint32_t first = code << (LOOK - l);
        for (uint32_t j = 0; j < (1u << (LOOK - l)); ++j)
          h.look[first + j] = (uint16_t)((l << 8) | h.syms[k]);
      }
    }
    h.maxcode[l] = (int32_t)(code << (16 - l));
    code <<= 1;
  }
  h.maxcode[17] = 0x7fffffff;
  if (is_ac) {
    for (int i = 0; i < (1 << LOOK); ++i) {
      const int len = h.look[i] >> 8, sym = h.look[i] & 255;
      const int run = sym >> 4, size = sym & 15;
      if (len == 0 || size == 0 || len + size > LOOK) continue;
      int v = (i >> (LOOK - len - size)) & ((1 << size) - 1);
      if (v < (1 << (size - 1))) v -= (1 << size) - 1;
      if (v >= -128 && v <= 127) h.fast[i] = (int16_t)(v * 256 + run * 16 + len + size);
    }
  }
  h.defined = true;
  return true;
}

inline int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// Walk the markers up to the first SOS.  Returns an STX_JPEG_* status.
int parse(const uint8_t* d, size_t len, Parsed& P, bool tables) {
  if (!d || len < 2) return STX_JPEG_CORRUPT;
  if (d[0] != 0xFF || d[1] != 0xD8) return STX_JPEG_UNSUPPORTED;  // not a JPEG
  size_t p = 2;
  bool sof = false, jfif = false, adobe = false;
  int adobe_transform = 0;
  for (;;) {
    if (p + 2 > len) return STX_JPEG_CORRUPT;
    if (d[p] != 0xFF) return STX_JPEG_CORRUPT;
    while (p + 1 < len && d[p + 1] == 0xFF) ++p;  // fill bytes
    if (p + 2 > len) return STX_JPEG_CORRUPT;
    const int m = d[p + 1];
    p += 2;
    if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;  // no payload
    if (m == 0xD9 || m == 0x00) return STX_JPEG_CORRUPT;               // EOI before a scan
    if (p + 2 > len) return STX_JPEG_CORRUPT;
    const size_t L = (size_t)be16(d + p);
    if (L < 2 || p + L > len) return STX_JPEG_CORRUPT;
    const uint8_t* s = d + p + 2;
    const size_t n = L - 2;
    if (m == 0xC0 || m == 0xC1) {
      if (sof) return STX_JPEG_UNSUPPORTED;  // a second frame
      if (n < 6) return STX_JPEG_CORRUPT;
      if (s[0] != 8) return STX_JPEG_UNSUPPORTED;
      P.h = be16(s + 1);
      P.w = be16(s + 3);
      P.ncomp = s[5];
      if (P.h == 0 || P.w == 0) return STX_JPEG_UNSUPPORTED;  // (a DNL-defined height)
      if (P.ncomp != 1 && P.ncomp != 3) return STX_JPEG_UNSUPPORTED;
      if (n != (size_t)(6 + 3 * P.ncomp)) return STX_JPEG_CORRUPT;
      for (int c = 0; c < P.ncomp; ++c) {
        Comp& k = P.comp[c];
        k.id = s[6 + 3 * c];
        k.hs = s[7 + 3 * c] >> 4;
        k.vs = s[7 + 3 * c] & 15;
        k.tq = s[8 + 3 * c];
        if (k.hs < 1 || k.hs > 4 || k.vs < 1 || k.vs > 4) return STX_JPEG_CORRUPT;
        if (k.tq > 3) return STX_JPEG_CORRUPT;
      }
      if (P.ncomp == 1) {
        P.comp[0].hs = P.comp[0].vs = 1;  // a lone component is never interleaved
      } else {
        const int hs = P.comp[0].hs, vs = P.comp[0].vs;
        if (P.comp[1].hs != 1 || P.comp[1].vs != 1 || P.comp[2].hs != 1 || P.comp[2].vs != 1)
          return STX_JPEG_UNSUPPORTED;
        if (!((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2)))
          return STX_JPEG_UNSUPPORTED;
      }
      sof = true;
    } else if (m >= 0xC0 && m <= 0xCF && m != 0xC4) {
      return STX_JPEG_UNSUPPORTED;  // progressive, lossless, hierarchical, arithmetic
    } else if (m == 0xC4) {
      size_t o = 0;
      while (o < n) {
        if (o + 17 > n) return STX_JPEG_CORRUPT;
        const int tc = s[o] >> 4, th = s[o] & 15;
        if (tc > 1 || th > 3) return STX_JPEG_CORRUPT;
        int cnt = 0;
        for (int l = 1; l <= 16; ++l) cnt += s[o + l];
        if (cnt > 256 || o + 17 + (size_t)cnt > n) return STX_JPEG_CORRUPT;
        if (tables) {
          Huff& hf = tc ? P.ac[th] : P.dc[th];
          hf.counts[0] = 0;
          for (int l = 1; l <= 16; ++l) hf.counts[l] = s[o + l];
          memset(hf.syms, 0, sizeof(hf.syms));
          memcpy(hf.syms, s + o + 17, (size_t)cnt);
          if (!build_huff(hf, tc == 1)) return STX_JPEG_CORRUPT;
        }
        o += 17 + (size_t)cnt;
      }
    } else if (m == 0xDB) {
      size_t o = 0;
      while (o < n) {
        const int pq = s[o] >> 4, tq = s[o] & 15;
        if (pq > 1 || tq > 3) return STX_JPEG_CORRUPT;
        if (pq == 1) return STX_JPEG_UNSUPPORTED;  // 16-bit table
        if (o + 65 > n) return STX_JPEG_CORRUPT;
        for (int i = 0; i < 64; ++i) P.q[tq][ZIGZAG[i]] = s[o + 1 + i];
        P.have_q[tq] = true;
        o += 65;
      }
    } else if (m == 0xDD) {
      if (n != 2) return STX_JPEG_CORRUPT;
      P.restart = be16(s);
    } else if (m == 0xE0) {
      if (n >= 5 && memcmp(s, "JFIF", 5) == 0) jfif = true;
    } else if (m == 0xEE) {
      if (n >= 12 && memcmp(s, "Adobe", 5) == 0) {
        adobe = true;
        adobe_transform = s[11];
      }
    } else if (m == 0xDA) {
      if (!sof) return STX_JPEG_CORRUPT;
      if (n < 1) return STX_JPEG_CORRUPT;
      const int ns = s[0];
      if (ns < 1 || ns > 4 || n != (size_t)(4 + 2 * ns)) return STX_JPEG_CORRUPT;
      if (ns != P.ncomp) return STX_JPEG_UNSUPPORTED;  // several scans
      for (int c = 0; c < ns; ++c) {
        if (s[1 + 2 * c] != P.comp[c].id) return STX_JPEG_UNSUPPORTED;  // (reordered scan)
        P.comp[c].td = s[2 + 2 * c] >> 4;
        P.comp[c].ta = s[2 + 2 * c] & 15;
        if (P.comp[c].td > 3 || P.comp[c].ta > 3) return STX_JPEG_CORRUPT;
      }
      if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0)
        return STX_JPEG_UNSUPPORTED;
      // colour space, as libjpeg guesses it: 3 components are YCbCr unless an Adobe marker
      // says otherwise or (without JFIF / Adobe) the component ids spell "RGB"
      if (P.ncomp == 3) {
        if (adobe && adobe_transform != 1) return STX_JPEG_UNSUPPORTED;
        if (!adobe && !jfif && P.comp[0].id == 'R' && P.comp[1].id == 'G' &&
            P.comp[2].id == 'B')
          return STX_JPEG_UNSUPPORTED;
      }
      for (int c = 0; c < P.ncomp; ++c)
        if (!P.have_q[P.comp[c].tq]) return STX_JPEG_CORRUPT;
      P.hmax = P.comp[0].hs;
      P.vmax = P.comp[0].vs;
      P.mcux = (P.w + 8 * P.hmax - 1) / (8 * P.hmax);
      P.mcuy = (P.h + 8 * P.vmax - 1) / (8 * P.vmax);
      P.coef_bytes = 0;
      for (int c = 0; c < P.ncomp; ++c) {
        P.bw[c] = P.mcux * P.comp[c].hs;
        P.bh[c] = P.mcuy * P.comp[c].vs;
        P.coef_bytes += (long long)P.bw[c] * P.bh[c] * 64 * 2;
      }
      P.scan = p + L;
      return STX_JPEG_OK;
    }
    p += L;
  }
}

// MSB-first bit reader over the entropy-coded segment: un-stuffs FF00, stops feeding at a
// marker or at the end of the data and pads with zero bits from there on; `npad` counts
// the padding at the tail of the buffer, so nbits < npad means padding was consumed.
struct Bits {
  const uint8_t* d;
  size_t len, pos;
  uint64_t buf = 0;
  int nbits = 0, npad = 0;
  bool stopped = false;

  Bits(const uint8_t* d_, size_t len_, size_t pos_) : d(d_), len(len_), pos(pos_) {}

  inline void fill() {  // at least 32 bits afterwards (57 when it loads any)
    if (nbits >= 32) return;
    if (!stopped && pos + 8 <= len) {
      uint64_t v;
      memcpy(&v, d + pos, 8);
      v = __builtin_bswap64(v);
      const uint64_t x = ~v;  // a zero byte of x is an FF byte of v
      if (!((x - 0x0101010101010101ull) & ~x & 0x8080808080808080ull)) {
        const int k = (64 - nbits) >> 3;
        if (k > 0) {
          v = k == 8 ? v : (v >> (64 - 8 * k)) << (64 - 8 * k);
          buf |= nbits ? v >> nbits : v;
          nbits += 8 * k;
          pos += (size_t)k;
        }
        return;
      }
    }
    while (nbits <= 56) {
      uint64_t b = 0;
      if (!stopped) {
        if (pos >= len) {
          stopped = true;
        } else if (d[pos] != 0xFF) {
          b = d[pos++];
        } else if (pos + 1 < len && d[pos + 1] == 0) {
          b = 0xFF;
          pos += 2;
        } else {
          stopped = true;  // a marker (or a lone FF at the end): pos stays on it
        }
      }
      if (stopped) npad += 8;
      buf |= b << (56 - nbits);
      nbits += 8;
    }
  }
  inline uint32_t peek(int n) const { return (uint32_t)(buf >> (64 - n)); }  // 1 <= n <= 32
  inline void skip(int n) {
    buf <<= n;
    nbits -= n;
  }
  inline bool overrun() const { return nbits < npad; }
};

// one Huffman symbol (needs >= 16 bits in the buffer); -1 on a code no table entry has
inline int decode_sym(Bits& b, const Huff& h) {
  const uint32_t e = h.look[b.peek(LOOK)];
  if (e) {
    b.skip((int)(e >> 8));
    return (int)(e & 255);
  }
  const int32_t c16 = (int32_t)b.peek(16);
  int l = LOOK + 1;
  while (c16 >= h.maxcode[l]) ++l;
  if (l > 16) return -1;
  const int idx = (c16 >> (16 - l)) + h.delta[l];
  if (idx < 0 || idx > 255) return -1;
  b.skip(l);
  return h.syms[idx];
}

inline int extend(uint32_t v, int s) {
  return (int)v < (1 << (s - 1)) ? (int)v - ((1 << s) - 1) : (int)v;
}

// one 8x8 block into blk (natural order, zeroed here); false on a corrupt stream
inline bool decode_block(Bits& b, const Huff& dc, const Huff& ac, uint32_t& pred, int16_t* blk) {
  memset(blk, 0, 64 * sizeof(int16_t));
  b.fill();
  int s = decode_sym(b, dc);
  if (s < 0 || s > 11) return false;
  if (s) {
    pred += (uint32_t)extend(b.peek(s), s);
    b.skip(s);
  }
  blk[0] = (int16_t)(uint16_t)pred;
  for (int k = 1; k < 64;) {
    b.fill();  // >= 32 bits: a 16-bit code + 15 value bits
    const int f = ac.fast[b.peek(LOOK)];
    if (f) {
      k += (f >> 4) & 15;
      if (k > 63) return false;
      b.skip(f & 15);
      blk[ZIGZAG[k++]] = (int16_t)(f >> 8);
      continue;
    }
    const int rs = decode_sym(b, ac);
    if (rs < 0) return false;
    const int r = rs >> 4;
    s = rs & 15;
    if (s == 0) {
      if (r != 15) break;  // EOB
      k += 16;
      if (k > 64) return false;  // a zero run past coefficient 63
      continue;
    }
    k += r;
    if (k > 63) return false;
    blk[ZIGZAG[k++]] = (int16_t)extend(b.peek(s), s);
    b.skip(s);
  }
  return !b.overrun();
}

}  // namespace

extern "C" int stx_jpeg_layout(long long* out, int n) {
  const long long v[] = {(long long)sizeof(stx_jpeg_desc),
                         (long long)offsetof(stx_jpeg_desc, coef_bytes),
                         (long long)sizeof(stx_jpeg_job), (long long)offsetof(stx_jpeg_job, bh)};
  const int m = (int)(sizeof(v) / sizeof(v[0]));
  for (int i = 0; out && i < n && i < m; ++i) out[i] = v[i];
  return m;
}

// ------------------------------------------------------------------------ the encoder
namespace {

// ITU T.81 Annex K.1: the example quantisation tables (natural order)
const uint8_t K_LUMA[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
                            14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                            18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                            49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
const uint8_t K_CHROMA[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99,
                              24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                              99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                              99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

// Annex K.3: the typical Huffman tables, as (counts of lengths 1..16, symbols)
struct StdHuff {
  uint8_t counts[16];
  int nsyms;
  const uint8_t* syms;
};
const uint8_t DC_SYMS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t AC0_SYMS[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07,
    0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0,
    0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49,
    0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7,
    0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5,
    0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa};
const uint8_t AC1_SYMS[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71,
    0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0,
    0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
    0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
    0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa};
// [class * 2 + id]: DC0, DC1, AC0, AC1
const StdHuff STD_HUFF[4] = {
    {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, 12, DC_SYMS},
    {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, 12, DC_SYMS},
    {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, 162, AC0_SYMS},
    {{0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}, 162, AC1_SYMS}};

// symbol -> (code, length); length 0: the table has no such symbol
struct EncHuff {
  uint16_t code[256];
  uint8_t len[256];
};
struct EncTables {
  EncHuff h[4];
  uint8_t zpos[64];  // natural index -> zigzag index
  EncTables() {
    memset(h, 0, sizeof(h));
    for (int i = 0; i < 64; ++i) zpos[ZIGZAG[i]] = (uint8_t)i;
    for (int t = 0; t < 4; ++t) {
      uint32_t code = 0;
      int k = 0;
      for (int l = 1; l <= 16; ++l) {
        for (int i = 0; i < STD_HUFF[t].counts[l - 1]; ++i, ++k, ++code) {
          h[t].code[STD_HUFF[t].syms[k]] = (uint16_t)code;
          h[t].len[STD_HUFF[t].syms[k]] = (uint8_t)l;
        }
        code <<= 1;
      }
    }
  }
};
const EncTables ENC;

constexpr size_t ENC_HEADER_MAX = 1024;     // all markers of a 3-component file: 623 bytes
constexpr size_t ENC_BLOCK_MAX = 2 * 212;   // 20 DC + 63 * 26 AC bits, every byte stuffed

bool enc_sampling_ok(int h, int w, int ncomp, int hmax, int vmax) {
  if (h < 1 || h > 65535 || w < 1 || w > 65535) return false;
  if (ncomp == 1) return hmax == 1 && vmax == 1;
  if (ncomp != 3) return false;
  return (hmax == 1 && vmax == 1) || (hmax == 2 && vmax == 1) || (hmax == 2 && vmax == 2);
}

// MSB-first bit writer bounded by cap: a byte that does not fit is dropped and `ok` cleared
struct BitOut {
  uint8_t* p;
  size_t cap, pos = 0;
  uint64_t acc = 0;
  int n = 0;
  bool ok = true;
  BitOut(uint8_t* p_, size_t cap_) : p(p_), cap(cap_) {}
  inline void byte(uint8_t b) {
    if (pos < cap) p[pos++] = b; else ok = false;
  }
  inline void bytes(const void* s, size_t k) {
    if (k <= cap - pos) { memcpy(p + pos, s, k); pos += k; } else ok = false;
  }
  inline void be16(int v) { byte((uint8_t)(v >> 8)); byte((uint8_t)v); }
  inline void drain() {  // whole bytes out, FF followed by 00
    if (n >= 32 && cap - pos >= 4) {  // four bytes at once when none of them is FF
      const uint32_t v = (uint32_t)(acc >> (n - 32)), x = ~v;
      if (!((x - 0x01010101u) & ~x & 0x80808080u)) {
        const uint32_t be = __builtin_bswap32(v);
        memcpy(p + pos, &be, 4);
        pos += 4;
        n -= 32;
      }
    }
    while (n >= 8) {
      const uint8_t b = (uint8_t)(acc >> (n - 8));
      n -= 8;
      byte(b);
      if (b == 0xFF) byte(0);
    }
  }
  inline void put(uint32_t code, int len) {  // len <= 32, at most 31 bits pending
    acc = (acc << len) | code;
    n += len;
    if (n >= 32) drain();
  }
  inline void finish() {  // pad the last byte with 1-bits
    if (n & 7) put((1u << (8 - (n & 7))) - 1u, 8 - (n & 7));
    drain();
  }
};

inline int bit_size(uint32_t a) { return a ? 32 - __builtin_clz(a) : 0; }

// bit i set: b[i] != 0 (natural order)
inline uint64_t nonzero_mask(const int16_t* b) {
  uint64_t m = 0;
#if defined(__SSE2__)
  const __m128i z = _mm_setzero_si128();
  for (int r = 0; r < 4; ++r) {
    const __m128i lo = _mm_cmpeq_epi16(_mm_loadu_si128((const __m128i*)(b + 16 * r)), z);
    const __m128i hi = _mm_cmpeq_epi16(_mm_loadu_si128((const __m128i*)(b + 16 * r + 8)), z);
    m |= (uint64_t)(uint16_t)~_mm_movemask_epi8(_mm_packs_epi16(lo, hi)) << (16 * r);
  }
#else
  for (int i = 0; i < 64; ++i) m |= (uint64_t)(b[i] != 0) << i;
#endif
  return m;
}

}  // namespace

extern "C" int stx_jpeg_quant_tables(int quality, unsigned short* qtab) {
  if (!qtab) return STX_JPEG_BAD_ARGS;
  const int q = quality < 1 ? 1 : (quality > 100 ? 100 : quality);
  const int scale = q < 50 ? 5000 / q : 200 - 2 * q;
  for (int t = 0; t < 2; ++t)
    for (int i = 0; i < 64; ++i) {
      const int v = ((t ? K_CHROMA : K_LUMA)[i] * scale + 50) / 100;
      qtab[64 * t + i] = (unsigned short)(v < 1 ? 1 : (v > 255 ? 255 : v));
    }
  return STX_JPEG_OK;
}

extern "C" size_t stx_jpeg_encode_bound(int h, int w, int ncomp, int hmax, int vmax) {
  if (!enc_sampling_ok(h, w, ncomp, hmax, vmax)) return 0;
  const size_t mx = ((size_t)w + 8 * hmax - 1) / (8 * hmax);
  const size_t my = ((size_t)h + 8 * vmax - 1) / (8 * vmax);
  const size_t blocks = mx * my * (size_t)(ncomp == 1 ? 1 : hmax * vmax + 2);
  return ENC_HEADER_MAX + blocks * ENC_BLOCK_MAX;
}

extern "C" int stx_jpeg_entropy_encode(const short* coef, size_t coef_bytes, int h, int w,
                                       int ncomp, int hmax, int vmax,
                                       const unsigned short* qtab, void* out, size_t cap,
                                       size_t* len) {
  if (len) *len = 0;
  if (!coef || !qtab || !len || (!out && cap) || !enc_sampling_ok(h, w, ncomp, hmax, vmax))
    return STX_JPEG_BAD_ARGS;
  const int mcux = (w + 8 * hmax - 1) / (8 * hmax), mcuy = (h + 8 * vmax - 1) / (8 * vmax);
  int hs[3] = {hmax, 1, 1}, vs[3] = {vmax, 1, 1}, bw[3];
  const int16_t* base[3];
  size_t need = 0;
  for (int c = 0; c < ncomp; ++c) {
    bw[c] = mcux * hs[c];
    base[c] = (const int16_t*)coef + need / 2;
    need += (size_t)bw[c] * ((size_t)mcuy * vs[c]) * 128;
  }
  if (coef_bytes < need) return STX_JPEG_BAD_ARGS;
  for (int t = 0; t < ncomp; ++t)
    for (int i = 0; i < 64; ++i)
      if (qtab[64 * t + i] < 1 || qtab[64 * t + i] > 255) return STX_JPEG_BAD_ARGS;
  if (ncomp == 3 && memcmp(qtab + 64, qtab + 128, 128) != 0) return STX_JPEG_BAD_ARGS;

  BitOut o((uint8_t*)out, cap);
  static const uint8_t APP0[] = {0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0,
                                 1,    1,    0,    0,    1, 0,  1,   0,   0};
  o.bytes(APP0, sizeof(APP0));
  const int ntab = ncomp == 1 ? 1 : 2;
  for (int t = 0; t < ntab; ++t) {
    const uint8_t hd[] = {0xFF, 0xDB, 0, 67, (uint8_t)t};
    o.bytes(hd, sizeof(hd));
    for (int i = 0; i < 64; ++i) o.byte((uint8_t)qtab[64 * t + ZIGZAG[i]]);
  }
  {
    const uint8_t hd[] = {0xFF, 0xC0, 0, (uint8_t)(8 + 3 * ncomp), 8};
    o.bytes(hd, sizeof(hd));
    o.be16(h);
    o.be16(w);
    o.byte((uint8_t)ncomp);
    for (int c = 0; c < ncomp; ++c) {
      o.byte((uint8_t)(c + 1));
      o.byte((uint8_t)((hs[c] << 4) | vs[c]));
      o.byte((uint8_t)(c ? 1 : 0));
    }
  }
  for (int id = 0; id < ntab; ++id)
    for (int cls = 0; cls < 2; ++cls) {  // DC0, AC0, DC1, AC1
      const StdHuff& s = STD_HUFF[cls * 2 + id];
      const uint8_t hd[] = {0xFF, 0xC4, 0, (uint8_t)(19 + s.nsyms), (uint8_t)((cls << 4) | id)};
      o.bytes(hd, sizeof(hd));
      o.bytes(s.counts, 16);
      o.bytes(s.syms, (size_t)s.nsyms);
    }
  {
    const uint8_t hd[] = {0xFF, 0xDA, 0, (uint8_t)(6 + 2 * ncomp), (uint8_t)ncomp};
    o.bytes(hd, sizeof(hd));
    for (int c = 0; c < ncomp; ++c) {
      o.byte((uint8_t)(c + 1));
      o.byte((uint8_t)(c ? 0x11 : 0x00));
    }
    const uint8_t tl[] = {0, 63, 0};
    o.bytes(tl, sizeof(tl));
  }
  if (!o.ok) return STX_JPEG_BAD_ARGS;

  int pred[3] = {0, 0, 0};
  for (int my = 0; my < mcuy; ++my) {
    for (int mx = 0; mx < mcux; ++mx) {
      for (int c = 0; c < ncomp; ++c) {
        const EncHuff& dc = ENC.h[c ? 1 : 0];
        const EncHuff& ac = ENC.h[c ? 3 : 2];
        for (int by = 0; by < vs[c]; ++by)
          for (int bx = 0; bx < hs[c]; ++bx) {
            const int16_t* blk =
                base[c] + ((size_t)(my * vs[c] + by) * bw[c] + (size_t)(mx * hs[c] + bx)) * 64;
            const int diff = (int)blk[0] - pred[c];
            pred[c] = blk[0];
            if (diff < -2047 || diff > 2047) return STX_JPEG_BAD_ARGS;
            int s = bit_size((uint32_t)(diff < 0 ? -diff : diff));  // <= 11
            o.put(dc.code[s], dc.len[s]);
            if (s) o.put((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << s) - 1u), s);
            // the non-zero AC coefficients as a bit mask in zigzag order: only they are visited
            uint64_t zz = 0;
            for (uint64_t m = nonzero_mask(blk) & ~1ull; m; m &= m - 1)
              zz |= 1ull << ENC.zpos[__builtin_ctzll(m)];
            int prev = 0;
            for (; zz; zz &= zz - 1) {
              const int k = __builtin_ctzll(zz);
              int run = k - prev - 1;
              prev = k;
              const int v = blk[ZIGZAG[k]];
              if (v < -1023 || v > 1023) return STX_JPEG_BAD_ARGS;
              for (; run > 15; run -= 16) o.put(ac.code[0xF0], ac.len[0xF0]);
              s = bit_size((uint32_t)(v < 0 ? -v : v));  // 1..10
              const int sym = (run << 4) | s;
              o.put(ac.code[sym], ac.len[sym]);
              o.put((uint32_t)(v < 0 ? v - 1 : v) & ((1u << s) - 1u), s);
            }
            if (prev != 63) o.put(ac.code[0], ac.len[0]);
            if (!o.ok) return STX_JPEG_BAD_ARGS;
          }
      }
    }
  }
  o.finish();
  o.byte(0xFF);
  o.byte(0xD9);
  if (!o.ok) return STX_JPEG_BAD_ARGS;
  *len = o.pos;
  return STX_JPEG_OK;
}

extern "C" int stx_jpeg_enc_layout(long long* out, int n) {
  const long long v[] = {(long long)sizeof(stx_jpeg_enc_job),
                         (long long)offsetof(stx_jpeg_enc_job, std_)};
  const int m = (int)(sizeof(v) / sizeof(v[0]));
  for (int i = 0; out && i < n && i < m; ++i) out[i] = v[i];
  return m;
}

extern "C" int stx_jpeg_info(const void* data, size_t len, stx_jpeg_desc* info) {
  if (!info) return STX_JPEG_BAD_ARGS;
  memset(info, 0, sizeof(*info));
  Parsed P;
  const int st = parse((const uint8_t*)data, len, P, false);
  info->status = st;
  if (st != STX_JPEG_OK) return st;
  info->h = P.h;
  info->w = P.w;
  info->ncomp = P.ncomp;
  info->restart_interval = P.restart;
  for (int c = 0; c < P.ncomp; ++c) {
    info->hs[c] = P.comp[c].hs;
    info->vs[c] = P.comp[c].vs;
    info->bw[c] = P.bw[c];
    info->bh[c] = P.bh[c];
  }
  info->coef_bytes = P.coef_bytes;
  return STX_JPEG_OK;
}

extern "C" int stx_jpeg_entropy_decode(const void* data, size_t len, short* coef,
                                       size_t coef_bytes, unsigned short* qtab) {
  if (!coef || !qtab) return STX_JPEG_BAD_ARGS;
  static thread_local Parsed P;  // ~20 KB of tables: kept off the stack and out of malloc
  P = Parsed();
  const uint8_t* d = (const uint8_t*)data;
  const int st = parse(d, len, P, true);
  if (st != STX_JPEG_OK) return st;
  if ((unsigned long long)P.coef_bytes > (unsigned long long)coef_bytes) return STX_JPEG_BAD_ARGS;
  for (int c = 0; c < P.ncomp; ++c) {
    if (!P.dc[P.comp[c].td].defined || !P.ac[P.comp[c].ta].defined) return STX_JPEG_CORRUPT;
    memcpy(qtab + 64 * c, P.q[P.comp[c].tq], 64 * sizeof(uint16_t));
  }
  int16_t* base[3];
  {
    int16_t* o = (int16_t*)coef;
    for (int c = 0; c < P.ncomp; ++c) {
      base[c] = o;
      o += (size_t)P.bw[c] * P.bh[c] * 64;
    }
  }
  Bits b(d, len, P.scan);
  uint32_t pred[3] = {0, 0, 0};
  long long mcu = 0;
  int togo = P.restart;
  for (int my = 0; my < P.mcuy; ++my) {
    for (int mx = 0; mx < P.mcux; ++mx, ++mcu) {
      if (P.restart && togo == 0) {
        // the restart marker: only the final byte's padding may be left, and the marker
        // must be the next thing in the stream and carry the expected number
        if (b.overrun() || b.nbits - b.npad >= 8) return STX_JPEG_CORRUPT;
        size_t p = b.pos;
        while (p + 2 < len && d[p] == 0xFF && d[p + 1] == 0xFF) ++p;
        if (p + 2 > len || d[p] != 0xFF) return STX_JPEG_CORRUPT;
        const int want = 0xD0 + (int)((mcu / P.restart - 1) & 7);
        if (d[p + 1] != want) return STX_JPEG_CORRUPT;
        b = Bits(d, len, p + 2);
        pred[0] = pred[1] = pred[2] = 0;
        togo = P.restart;
      }
      for (int c = 0; c < P.ncomp; ++c) {
        const Comp& k = P.comp[c];
        for (int by = 0; by < k.vs; ++by)
          for (int bx = 0; bx < k.hs; ++bx) {
            const size_t idx = (size_t)(my * k.vs + by) * P.bw[c] + (size_t)(mx * k.hs + bx);
            if (!decode_block(b, P.dc[k.td], P.ac[k.ta], pred[c], base[c] + idx * 64))
              return STX_JPEG_CORRUPT;
          }
      }
      --togo;
    }
  }
  // the scan must end where the data says it does: EOI right after the last byte's padding
  if (b.overrun() || b.nbits - b.npad >= 8) return STX_JPEG_CORRUPT;
  size_t p = b.pos;
  while (p + 2 < len && d[p] == 0xFF && d[p + 1] == 0xFF) ++p;
  if (p + 2 > len || d[p] != 0xFF || d[p + 1] != 0xD9) return STX_JPEG_CORRUPT;
  return STX_JPEG_OK;
}

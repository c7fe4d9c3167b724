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

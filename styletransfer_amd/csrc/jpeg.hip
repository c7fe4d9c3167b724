// Device half of the JPEG decode (the host half, jpeg_host.cpp, Huffman-decodes the scan):
// quantised DCT coefficients -> packed HxWx3 uint8 RGB, byte for byte what libjpeg (and so
// Pillow) produces, into the buffer stx_image_condition reads.
//
// Two kernels per batch, every image of the batch in the same launch (blockIdx.y = job):
//  (a) jpeg_idct_kernel: one thread per 8x8 block.  The thread reads its 64 int16
//      coefficients as eight 16-byte loads, multiplies by the component's quantisation
//      table, runs libjpeg's "islow" integer IDCT (jidctint.c's arithmetic: columns first,
//      13-bit constants, 2 extra bits between the passes) wholly in registers and writes
//      eight 8-byte rows of clamp(v + 128) to the component's plane.  Neighbouring
//      threads hold neighbouring blocks, so a wave's row stores are 512 contiguous bytes.
//  (b) jpeg_color_kernel: one thread per output pixel: Y, the two chroma samples through
//      libjpeg's "fancy" (triangle) upsampling for 2x1 / 2x2 subsampling, YCbCr -> RGB in
//      16-bit fixed point, three bytes out.  A raw job (an image the host decoded
//      itself) is copied through by the same threads.
// All integer arithmetic is done on uint32 (wraps, no undefined behaviour) and shifted
// right as int32, so hostile coefficients give unspecified pixels and nothing else.
// Every address is derived from the job's grid, which the entry point checks against
// (h, w, sampling) and the workspace size before it launches anything.
#include "common.h"
#include "../../include/stx.h"

namespace stx {

struct JpegJobs {
  stx_jpeg_job j[STX_JPEG_CHUNK];
};

typedef unsigned int u32;

// FIX(x) = round(x * 2^13)
constexpr u32 F_0_298 = 2446, F_0_390 = 3196, F_0_541 = 4433, F_0_765 = 6270, F_0_899 = 7373,
              F_1_175 = 9633, F_1_501 = 12299, F_1_847 = 15137, F_1_961 = 16069,
              F_2_053 = 16819, F_2_562 = 20995, F_3_072 = 25172;

// arithmetic shift right with round-half-up of a wrapped 32-bit value
__device__ __forceinline__ u32 descale(u32 v, int n) {
  return (u32)((int)(v + (1u << (n - 1))) >> n);
}

// one 8-point pass of jidctint.c's jpeg_idct_islow on d[0..7], descaled by SHIFT
template <int SHIFT>
__device__ __forceinline__ void idct8(u32 (&d)[8]) {
  u32 z2 = d[2], z3 = d[6];
  u32 z1 = (z2 + z3) * F_0_541;
  u32 tmp2 = z1 - z3 * F_1_847;
  u32 tmp3 = z1 + z2 * F_0_765;
  u32 tmp0 = (d[0] + d[4]) << 13;
  u32 tmp1 = (d[0] - d[4]) << 13;
  const u32 tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3;
  const u32 tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  tmp0 = d[7];
  tmp1 = d[5];
  tmp2 = d[3];
  tmp3 = d[1];
  z1 = tmp0 + tmp3;
  z2 = tmp1 + tmp2;
  z3 = tmp0 + tmp2;
  u32 z4 = tmp1 + tmp3;
  const u32 z5 = (z3 + z4) * F_1_175;
  tmp0 *= F_0_298;
  tmp1 *= F_2_053;
  tmp2 *= F_3_072;
  tmp3 *= F_1_501;
  z1 *= 0u - F_0_899;
  z2 *= 0u - F_2_562;
  z3 = z3 * (0u - F_1_961) + z5;
  z4 = z4 * (0u - F_0_390) + z5;
  tmp0 += z1 + z3;
  tmp1 += z2 + z4;
  tmp2 += z2 + z3;
  tmp3 += z1 + z4;
  d[0] = descale(tmp10 + tmp3, SHIFT);
  d[7] = descale(tmp10 - tmp3, SHIFT);
  d[1] = descale(tmp11 + tmp2, SHIFT);
  d[6] = descale(tmp11 - tmp2, SHIFT);
  d[2] = descale(tmp12 + tmp1, SHIFT);
  d[5] = descale(tmp12 - tmp1, SHIFT);
  d[3] = descale(tmp13 + tmp0, SHIFT);
  d[4] = descale(tmp13 - tmp0, SHIFT);
}

__device__ __forceinline__ u32 limit8(u32 v) {  // clamp(v + 128, 0, 255)
  const int x = (int)(v + 128u);
  return (u32)(x < 0 ? 0 : (x > 255 ? 255 : x));
}

__global__ void __launch_bounds__(256)
jpeg_idct_kernel(const JpegJobs jobs, const uint8_t* __restrict__ coef_base,
                 uint8_t* __restrict__ tmp) {
  const stx_jpeg_job& J = jobs.j[blockIdx.y];
  if (J.raw) return;
  long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  // which component this block belongs to; its plane and coefficients
  long long coef_off = J.coef_offset, plane_off = J.tmp_offset;
  int c = 0;
  for (; c < J.ncomp; ++c) {
    const long long nb = (long long)J.bw[c] * J.bh[c];
    if (t < nb) break;
    t -= nb;
    coef_off += nb * 128;
    plane_off += nb * 64;
  }
  if (c >= J.ncomp) return;
  const int bw = J.bw[c];
  const int by = (int)(t / bw), bx = (int)(t - (long long)by * bw);
  const uint4* __restrict__ src = (const uint4*)(coef_base + coef_off + t * 128);
  const uint4* __restrict__ q = (const uint4*)(coef_base + J.qtab_offset + c * 128);
  u32 ws[8][8];  // [row][column], fully unrolled: registers
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const uint4 v = src[r], k = q[r];
    const u32 cv[4] = {v.x, v.y, v.z, v.w}, kv[4] = {k.x, k.y, k.z, k.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      // int16 coefficient (sign-extended) times uint16 table entry
      ws[r][2 * i] = (u32)(int)(short)(cv[i] & 0xffffu) * (kv[i] & 0xffffu);
      ws[r][2 * i + 1] = (u32)((int)cv[i] >> 16) * (kv[i] >> 16);
    }
  }
#pragma unroll
  for (int x = 0; x < 8; ++x) {  // columns
    u32 d[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) d[r] = ws[r][x];
    idct8<11>(d);
#pragma unroll
    for (int r = 0; r < 8; ++r) ws[r][x] = d[r];
  }
  const size_t pitch = (size_t)bw * 8;
  uint8_t* __restrict__ dst = tmp + plane_off + (size_t)by * 8 * pitch + (size_t)bx * 8;
#pragma unroll
  for (int r = 0; r < 8; ++r) {  // rows
    idct8<18>(ws[r]);
    uint2 o;
    o.x = limit8(ws[r][0]) | (limit8(ws[r][1]) << 8) | (limit8(ws[r][2]) << 16) |
          (limit8(ws[r][3]) << 24);
    o.y = limit8(ws[r][4]) | (limit8(ws[r][5]) << 8) | (limit8(ws[r][6]) << 16) |
          (limit8(ws[r][7]) << 24);
    *(uint2*)(dst + (size_t)r * pitch) = o;
  }
}

// chroma sample of one plane at output pixel (x, y): libjpeg's fancy upsampling on a
// plane of cw x ch samples with row pitch `pitch`
__device__ __forceinline__ int chroma_at(const uint8_t* __restrict__ p, size_t pitch, int cw,
                                         int ch, int hmax, int vmax, int x, int y) {
  if (hmax == 1) return p[(size_t)y * pitch + x];
  const int cx = x >> 1;
  const int xn = (x & 1) ? min(cx + 1, cw - 1) : max(cx - 1, 0);  // the nearer neighbour
  const bool edge = (x & 1) ? cx == cw - 1 : cx == 0;
  if (vmax == 1) {
    const uint8_t* row = p + (size_t)y * pitch;
    const int c = row[cx];
    if (edge) return c;
    return (3 * c + row[xn] + ((x & 1) ? 2 : 1)) >> 2;
  }
  const int cy = y >> 1;
  const int yn = (y & 1) ? min(cy + 1, ch - 1) : max(cy - 1, 0);
  const uint8_t* r0 = p + (size_t)cy * pitch;
  const uint8_t* r1 = p + (size_t)yn * pitch;
  const int s = 3 * r0[cx] + r1[cx];
  const int bias = (x & 1) ? 7 : 8;
  if (edge) return (4 * s + bias) >> 4;
  const int sn = 3 * r0[xn] + r1[xn];
  return (3 * s + sn + bias) >> 4;
}

__device__ __forceinline__ uint8_t clamp8(int v) {
  return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

__global__ void __launch_bounds__(256)
jpeg_color_kernel(const JpegJobs jobs, const uint8_t* __restrict__ coef_base,
                  const uint8_t* __restrict__ tmp, uint8_t* __restrict__ rgb_base) {
  const stx_jpeg_job& J = jobs.j[blockIdx.y];
  const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  const long long total = (long long)J.h * J.w;
  if (i >= total) return;
  uint8_t* __restrict__ o = rgb_base + J.rgb_offset + i * 3;
  if (J.raw) {
    const uint8_t* __restrict__ s = coef_base + J.coef_offset + i * 3;
    o[0] = s[0];
    o[1] = s[1];
    o[2] = s[2];
    return;
  }
  const int y = (int)(i / J.w), x = (int)(i - (long long)y * J.w);
  const uint8_t* __restrict__ py = tmp + J.tmp_offset;
  const size_t pitch0 = (size_t)J.bw[0] * 8;
  const int Y = py[(size_t)y * pitch0 + x];
  if (J.ncomp == 1) {
    o[0] = o[1] = o[2] = (uint8_t)Y;
    return;
  }
  const uint8_t* __restrict__ pcb = py + pitch0 * J.bh[0] * 8;
  const size_t pitch1 = (size_t)J.bw[1] * 8, pitch2 = (size_t)J.bw[2] * 8;
  const uint8_t* __restrict__ pcr = pcb + pitch1 * J.bh[1] * 8;
  const int cw = (J.w + J.hmax - 1) / J.hmax, ch = (J.h + J.vmax - 1) / J.vmax;
  const int cb = chroma_at(pcb, pitch1, cw, ch, J.hmax, J.vmax, x, y) - 128;
  const int cr = chroma_at(pcr, pitch2, cw, ch, J.hmax, J.vmax, x, y) - 128;
  o[0] = clamp8(Y + ((91881 * cr + 32768) >> 16));
  o[1] = clamp8(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
  o[2] = clamp8(Y + ((116130 * cb + 32768) >> 16));
}

// ------------------------------------------------------------------------ the encoder
// The decode's mirror, two kernels per batch (blockIdx.y = job):
//  (a) jpeg_enc_color_kernel: one thread per chroma sample of the padded grid, i.e. per
//      hmax x vmax group of source pixels: bytes from the packed uint8 or the normalised
//      planar fp32 source (edges replicated), Y for each pixel, Cb / Cr downsampled, to the
//      component planes in tmp.
//  (b) jpeg_fdct_kernel: one thread per 8x8 block: eight 8-byte row loads, jfdctint.c's
//      islow forward DCT in registers (rows first), quantisation, eight 16-byte stores.  A
//      dummy block (padding outside the component's real extent) takes the DC of the
//      block before it in MCU order from the sum of that block's samples, so it waits for
//      no other thread.
struct JpegEncJobs {
  stx_jpeg_enc_job j[STX_JPEG_CHUNK];
};

// one source pixel (x, y already clamped into the image) as three bytes
__device__ __forceinline__ void enc_rgb(const stx_jpeg_enc_job& J, const uint8_t* __restrict__ s,
                                        int x, int y, int (&c)[3]) {
  const size_t i = (size_t)y * J.w + x;
  if (J.fp32) {
#pragma clang fp contract(off)  // x * std + mean is two roundings, as torch's two ops
    const float* __restrict__ f = (const float*)s;
    const size_t plane = (size_t)J.h * J.w;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      float v = f[k * plane + i] * J.std_[k];
      v = v + J.mean[k];
      v = fminf(fmaxf(v, 0.0f), 255.0f);
      const int b = (int)(v * 255.0f);
      c[k] = b > 255 ? 255 : b;
    }
  } else if (J.ncomp == 1) {
    c[0] = c[1] = c[2] = s[i];
  } else {
    c[0] = s[3 * i];
    c[1] = s[3 * i + 1];
    c[2] = s[3 * i + 2];
  }
}

__global__ void __launch_bounds__(256)
jpeg_enc_color_kernel(const JpegEncJobs jobs, const uint8_t* __restrict__ src_base,
                      uint8_t* __restrict__ tmp) {
  const stx_jpeg_enc_job& J = jobs.j[blockIdx.y];
  const int cc = J.ncomp == 1 ? 0 : 1;  // the component sampled 1x1
  const int pw = J.bw[cc] * 8, ph = J.bh[cc] * 8;
  const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (t >= (long long)pw * ph) return;
  const int cy = (int)(t / pw), cx = (int)(t - (long long)cy * pw);
  const uint8_t* __restrict__ s = src_base + J.src_offset;
  uint8_t* __restrict__ py = tmp + J.tmp_offset;
  const size_t pitch0 = (size_t)J.bw[0] * 8;
  if (J.ncomp == 1) {
    py[(size_t)cy * pitch0 + cx] = s[(size_t)min(cy, J.h - 1) * J.w + min(cx, J.w - 1)];
    return;
  }
  // chroma rows past the last real one replicate it (the DOWNSAMPLED row, not the source's)
  const int ch = (J.h + J.vmax - 1) / J.vmax;
  const int sy = min(cy, ch - 1) * J.vmax;
  int cb = 0, cr = 0;
  for (int dy = 0; dy < J.vmax; ++dy) {
    for (int dx = 0; dx < J.hmax; ++dx) {
      const int x = cx * J.hmax + dx;
      int c[3];
      // the luma sample of this position: its own row, clamped to the image
      enc_rgb(J, s, min(x, J.w - 1), min(cy * J.vmax + dy, J.h - 1), c);
      py[(size_t)(cy * J.vmax + dy) * pitch0 + x] =
          (uint8_t)((19595 * c[0] + 38470 * c[1] + 7471 * c[2] + 32768) >> 16);
      if (sy != cy * J.vmax) enc_rgb(J, s, min(x, J.w - 1), min(sy + dy, J.h - 1), c);
      cb += (-11059 * c[0] - 21709 * c[1] + 32768 * c[2] + 8388608 + 32767) >> 16;
      cr += (32768 * c[0] - 27439 * c[1] - 5329 * c[2] + 8388608 + 32767) >> 16;
    }
  }
  if (J.hmax == 2) {
    // 2x2: bias 1, 2 alternating, >> 2; 2x1: bias 0, 1, >> 1
    const int sh = J.vmax, bias = (J.vmax == 2 ? 1 : 0) + (cx & 1);
    cb = (cb + bias) >> sh;
    cr = (cr + bias) >> sh;
  }
  uint8_t* __restrict__ pcb = py + pitch0 * J.bh[0] * 8;
  const size_t pitch1 = (size_t)pw;
  pcb[(size_t)cy * pitch1 + cx] = (uint8_t)cb;
  pcb[pitch1 * ph + (size_t)cy * pitch1 + cx] = (uint8_t)cr;
}

// one 8-point pass of jfdctint.c's jpeg_fdct_islow on d[0..7]; FIRST: the row pass
template <bool FIRST>
__device__ __forceinline__ void fdct8(u32 (&d)[8]) {
  const u32 tmp0 = d[0] + d[7], tmp7 = d[0] - d[7], tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
  const u32 tmp2 = d[2] + d[5], tmp5 = d[2] - d[5], tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
  const u32 tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  constexpr int SH = FIRST ? 11 : 15;
  if (FIRST) {
    d[0] = (tmp10 + tmp11) << 2;
    d[4] = (tmp10 - tmp11) << 2;
  } else {
    d[0] = descale(tmp10 + tmp11, 2);
    d[4] = descale(tmp10 - tmp11, 2);
  }
  u32 z1 = (tmp12 + tmp13) * F_0_541;
  d[2] = descale(z1 + tmp13 * F_0_765, SH);
  d[6] = descale(z1 - tmp12 * F_1_847, SH);
  z1 = tmp4 + tmp7;
  u32 z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
  const u32 z5 = (z3 + z4) * F_1_175;
  const u32 t4 = tmp4 * F_0_298, t5 = tmp5 * F_2_053, t6 = tmp6 * F_3_072, t7 = tmp7 * F_1_501;
  z1 *= 0u - F_0_899;
  z2 *= 0u - F_2_562;
  z3 = z3 * (0u - F_1_961) + z5;
  z4 = z4 * (0u - F_0_390) + z5;
  d[7] = descale(t4 + z1 + z3, SH);
  d[5] = descale(t5 + z2 + z4, SH);
  d[3] = descale(t6 + z2 + z3, SH);
  d[1] = descale(t7 + z1 + z4, SH);
}

// (|c| + 4 q) / (8 q), truncated, the sign restored; c is a wrapped int32, q in 1..65535
__device__ __forceinline__ u32 enc_quant(u32 c, u32 q) {
  const bool neg = (int)c < 0;
  const u32 a = ((neg ? 0u - c : c) + 4u * q) / (8u * q);
  return (neg ? 0u - a : a) & 0xffffu;
}

__global__ void __launch_bounds__(256)
jpeg_fdct_kernel(const JpegEncJobs jobs, uint8_t* __restrict__ coef_base,
                 const uint8_t* __restrict__ tmp) {
  const stx_jpeg_enc_job& J = jobs.j[blockIdx.y];
  long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  long long coef_off = J.coef_offset, plane_off = J.tmp_offset;
  int c = 0;
  for (; c < J.ncomp; ++c) {
    const long long nb = (long long)J.bw[c] * J.bh[c];
    if (t < nb) break;
    t -= nb;
    coef_off += nb * 128;
    plane_off += nb * 64;
  }
  if (c >= J.ncomp) return;
  const int bw = J.bw[c];
  int by = (int)(t / bw), bx = (int)(t - (long long)by * bw);
  const int hs = c ? 1 : J.hmax, vs = c ? 1 : J.vmax;
  // the component's real extent in blocks
  const int rbw = ((J.w * hs + J.hmax - 1) / J.hmax + 7) >> 3;
  const int rbh = ((J.h * vs + J.vmax - 1) / J.vmax + 7) >> 3;
  const bool dummy = bx >= rbw || by >= rbh;
  if (dummy) {
    // walk back in MCU order to the nearest real block (the MCU's first block always is)
    const int mx = bx / hs, my = by / vs;
    int pos = (by - my * vs) * hs + (bx - mx * hs);
    while (pos > 0 && (bx >= rbw || by >= rbh)) {
      --pos;
      by = my * vs + pos / hs;
      bx = mx * hs + pos % hs;
    }
  }
  const size_t pitch = (size_t)bw * 8;
  const uint8_t* __restrict__ src = tmp + plane_off + (size_t)by * 8 * pitch + (size_t)bx * 8;
  const unsigned short* __restrict__ q =
      (const unsigned short*)(coef_base + J.qtab_offset) + (c ? 64 : 0);
  uint4* __restrict__ dst = (uint4*)(coef_base + coef_off + t * 128);
  u32 ws[8][8];  // [row][column], fully unrolled: registers
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const uint2 v = *(const uint2*)(src + (size_t)r * pitch);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      ws[r][i] = ((v.x >> (8 * i)) & 255u) - 128u;
      ws[r][4 + i] = ((v.y >> (8 * i)) & 255u) - 128u;
    }
  }
  if (dummy) {
    u32 sum = 0;
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
      for (int x = 0; x < 8; ++x) sum += ws[r][x];
    dst[0] = make_uint4(enc_quant(sum, q[0]), 0u, 0u, 0u);
#pragma unroll
    for (int r = 1; r < 8; ++r) dst[r] = make_uint4(0u, 0u, 0u, 0u);
    return;
  }
#pragma unroll
  for (int r = 0; r < 8; ++r) fdct8<true>(ws[r]);
#pragma unroll
  for (int x = 0; x < 8; ++x) {
    u32 d[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) d[r] = ws[r][x];
    fdct8<false>(d);
#pragma unroll
    for (int r = 0; r < 8; ++r) ws[r][x] = d[r];
  }
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const uint4 k = ((const uint4*)q)[r];
    const u32 kv[4] = {k.x, k.y, k.z, k.w};
    u32 o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
      o[i] = enc_quant(ws[r][2 * i], kv[i] & 0xffffu) |
             (enc_quant(ws[r][2 * i + 1], kv[i] >> 16) << 16);
    dst[r] = make_uint4(o[0], o[1], o[2], o[3]);
  }
}

}  // namespace stx

using namespace stx;

extern "C" int stx_jpeg_encode_batch(const stx_jpeg_enc_job* jobs, int njobs,
                                     const void* src_base, void* coef_base, void* tmp,
                                     size_t tmp_bytes, void* stream) {
  if (!jobs || njobs <= 0 || !src_base || !coef_base || !tmp || ((uintptr_t)src_base & 15) ||
      ((uintptr_t)coef_base & 15) || ((uintptr_t)tmp & 15)) {
    set_error("stx_jpeg_encode_batch: invalid arguments");
    return STX_E_INVALID;
  }
  for (int i = 0; i < njobs; ++i) {
    const stx_jpeg_enc_job& J = jobs[i];
    bool ok = J.h >= 1 && J.h <= 65535 && J.w >= 1 && J.w <= 65535 && J.src_offset >= 0 &&
              J.coef_offset >= 0 && J.qtab_offset >= 0 && J.tmp_offset >= 0 &&
              !(J.src_offset & 15) && !(J.coef_offset & 15) && !(J.qtab_offset & 15) &&
              !(J.tmp_offset & 15) && (J.ncomp == 1 || J.ncomp == 3);
    if (ok && J.ncomp == 1) ok = J.hmax == 1 && J.vmax == 1 && !J.fp32;
    if (ok && J.ncomp == 3)
      ok = (J.hmax == 1 && J.vmax == 1) || (J.hmax == 2 && J.vmax == 1) ||
           (J.hmax == 2 && J.vmax == 2);
    long long planes = 0;
    if (ok) {
      const int mx = cdiv(J.w, 8 * J.hmax), my = cdiv(J.h, 8 * J.vmax);
      for (int c = 0; c < J.ncomp; ++c) {
        ok = ok && J.bw[c] == mx * (c ? 1 : J.hmax) && J.bh[c] == my * (c ? 1 : J.vmax);
        planes += (long long)J.bw[c] * J.bh[c] * 64;
      }
    }
    if (!ok) {
      set_error("stx_jpeg_encode_batch: job %d is inconsistent", i);
      return STX_E_INVALID;
    }
    if ((unsigned long long)J.tmp_offset + (unsigned long long)planes >
        (unsigned long long)tmp_bytes) {
      set_error("stx_jpeg_encode_batch: job %d needs %lld workspace bytes at %lld of %zu", i,
                planes, J.tmp_offset, tmp_bytes);
      return STX_E_WORKSPACE;
    }
  }
  hipStream_t st = (hipStream_t)stream;
  for (int first = 0; first < njobs; first += STX_JPEG_CHUNK) {
    const int n = njobs - first < STX_JPEG_CHUNK ? njobs - first : STX_JPEG_CHUNK;
    JpegEncJobs P = {};
    long long max_blocks = 0, max_px = 0;
    for (int i = 0; i < n; ++i) {
      const stx_jpeg_enc_job& J = P.j[i] = jobs[first + i];
      long long nb = 0;
      for (int c = 0; c < J.ncomp; ++c) nb += (long long)J.bw[c] * J.bh[c];
      max_blocks = nb > max_blocks ? nb : max_blocks;
      const int cc = J.ncomp == 1 ? 0 : 1;
      const long long px = (long long)J.bw[cc] * J.bh[cc] * 64;
      max_px = px > max_px ? px : max_px;
    }
    // a chunk shorter than STX_JPEG_CHUNK leaves zeroed jobs behind n: blockIdx.y < n
    hipLaunchKernelGGL(jpeg_enc_color_kernel, dim3((unsigned)((max_px + 255) / 256), n),
                       dim3(256), 0, st, P, (const uint8_t*)src_base, (uint8_t*)tmp);
    hipLaunchKernelGGL(jpeg_fdct_kernel, dim3((unsigned)((max_blocks + 255) / 256), n), dim3(256),
                       0, st, P, (uint8_t*)coef_base, (const uint8_t*)tmp);
  }
  return check_launch("stx_jpeg_encode_batch");
}

extern "C" int stx_jpeg_decode_batch(const stx_jpeg_job* jobs, int njobs, const void* coef_base,
                                     void* rgb_base, void* tmp, size_t tmp_bytes,
                                     void* stream) {
  if (!jobs || njobs <= 0 || !coef_base || !rgb_base || ((uintptr_t)coef_base & 15) ||
      ((uintptr_t)tmp & 15)) {
    set_error("stx_jpeg_decode_batch: invalid arguments");
    return STX_E_INVALID;
  }
  for (int i = 0; i < njobs; ++i) {
    const stx_jpeg_job& J = jobs[i];
    bool ok = J.h >= 1 && J.h <= 65535 && J.w >= 1 && J.w <= 65535 && J.rgb_offset >= 0 &&
              J.coef_offset >= 0;
    if (ok && !J.raw) {
      ok = (J.ncomp == 1 || J.ncomp == 3) && J.qtab_offset >= 0 && J.tmp_offset >= 0 &&
           !(J.coef_offset & 15) && !(J.qtab_offset & 15) && !(J.tmp_offset & 15);
      if (ok && J.ncomp == 1) ok = J.hmax == 1 && J.vmax == 1;
      if (ok && J.ncomp == 3)
        ok = (J.hmax == 1 && J.vmax == 1) || (J.hmax == 2 && J.vmax == 1) ||
             (J.hmax == 2 && J.vmax == 2);
      long long planes = 0;
      if (ok) {
        const int mx = cdiv(J.w, 8 * J.hmax), my = cdiv(J.h, 8 * J.vmax);
        for (int c = 0; c < J.ncomp; ++c) {
          ok = ok && J.bw[c] == mx * (c ? 1 : J.hmax) && J.bh[c] == my * (c ? 1 : J.vmax);
          planes += (long long)J.bw[c] * J.bh[c] * 64;
        }
      }
      if (ok && (!tmp || (unsigned long long)J.tmp_offset + (unsigned long long)planes >
                             (unsigned long long)tmp_bytes)) {
        set_error("stx_jpeg_decode_batch: job %d needs %lld workspace bytes at %lld of %zu", i,
                  planes, J.tmp_offset, tmp_bytes);
        return STX_E_WORKSPACE;
      }
    }
    if (!ok) {
      set_error("stx_jpeg_decode_batch: job %d is inconsistent", i);
      return STX_E_INVALID;
    }
  }
  hipStream_t st = (hipStream_t)stream;
  for (int first = 0; first < njobs; first += STX_JPEG_CHUNK) {
    const int n = njobs - first < STX_JPEG_CHUNK ? njobs - first : STX_JPEG_CHUNK;
    JpegJobs P = {};
    long long max_blocks = 0, max_px = 0;
    for (int i = 0; i < n; ++i) {
      const stx_jpeg_job& J = P.j[i] = jobs[first + i];
      if (!J.raw) {
        long long nb = 0;
        for (int c = 0; c < J.ncomp; ++c) nb += (long long)J.bw[c] * J.bh[c];
        max_blocks = nb > max_blocks ? nb : max_blocks;
      }
      const long long px = (long long)J.h * J.w;
      max_px = px > max_px ? px : max_px;
    }
    if (max_blocks > 0)
      hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((max_blocks + 255) / 256), n),
                         dim3(256), 0, st, P, (const uint8_t*)coef_base, (uint8_t*)tmp);
    hipLaunchKernelGGL(jpeg_color_kernel, dim3((unsigned)((max_px + 255) / 256), n), dim3(256), 0,
                       st, P, (const uint8_t*)coef_base, (const uint8_t*)tmp,
                       (uint8_t*)rgb_base);
  }
  return check_launch("stx_jpeg_decode_batch");
}

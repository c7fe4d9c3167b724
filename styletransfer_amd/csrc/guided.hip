// Guided (region-weighted) Gram matrices and their backward for gfx950 -- the spatial
// control of Gatys et al. 2017, "Controlling Perceptual Factors in Neural Style Transfer".
//
//   G[b][r] = (1 / (c hw)) sum_p wts[r][p] z[b][:,p] z[b][:,p]^T        R regions per image
//   loss_r  = mean over (b, i, j) of (G[b][r] - T[r])^2
//   A[b][r] = weight lambda_r 4 / (b c^3 hw) (G[b][r] - T[r])
//   dz[b]   (+)= s sum_r wts[r] o (A[b][r] z[b])
//
// Forward: the tiling, split-K and fixed-order reductions of gram.hip's 64 x 64-tile
// kernels with the pixel weight folded into the A operand (rows I carry w z, rows J carry
// z), so G stays a plain MFMA product.  The region is part of the block index: the R
// blocks of one (tile, pixel split) sit 8 apart in the launch order, i.e. on one XCD
// under round-robin dispatch, back to back, so that the second to R-th read of a z panel
// comes from that XCD's L2.  (One block for all R regions would keep R x 4 accumulator
// quadrants live: 256 VGPRs at R = 4 before any operand.)
// Backward: one block per pixel tile stages z once (split to fp16 hi/lo once) in LDS and
// runs every region's A_r z on the MFMA out of it; the 32 x 32 MFMA output has one pixel
// per lane, so the region weight is one value per lane and the sum over regions is a
// per-register fma.
#include <algorithm>

#include "common.h"

namespace stx {
namespace guided {

constexpr int GT = 64;   // Gram tile
constexpr int GKC = 64;  // pixels per LDS stage (fp32 kernel)
constexpr int GP = GKC + 1;

typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
#define MF16(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0)

struct Lam {
  float v[STX_GUIDE_MAX];
};

__device__ __forceinline__ void tile_ij(int t, int nt, int& I, int& J) {
  // upper triangle row-major: (0,0),(0,1)..(0,nt-1),(1,1)...
  int i = 0;
  while (t >= nt - i) {
    t -= nt - i;
    ++i;
  }
  I = i;
  J = i + t;
}

// s * w * x = hi + lo (fp16 each), 8 pixels
__device__ __forceinline__ void split8w(const f32x4& x0, const f32x4& x1, const f32x4& w0,
                                        const f32x4& w1, float s, f16x8_t& hi, f16x8_t& lo) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float v = (e < 4 ? x0[e] * w0[e] : x1[e - 4] * w1[e - 4]) * s;
    const _Float16 vh = (_Float16)v;
    hi[e] = vh;
    lo[e] = (_Float16)(v - (float)vh);
  }
}

__device__ __forceinline__ void split8(const f32x4& x0, const f32x4& x1, float s, f16x8_t& hi,
                                       f16x8_t& lo) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float v = (e < 4 ? x0[e] : x1[e - 4]) * s;
    const _Float16 vh = (_Float16)v;
    hi[e] = vh;
    lo[e] = (_Float16)(v - (float)vh);
  }
}

// ---------------------------------------------------------------- forward, fp16 hi/lo split
// hw % 8 == 0.  Lane (r, h) feeds pixels [8h, 8h + 8) of each 16-pixel step from its own
// rows; the A operand (rows I) is s_a w z, the B operand (rows J) s_z z, three products
// hi*hi + hi*lo + lo*hi accumulated in fp32 and de-scaled by 1 / (s_a s_z) (exact).  A wave
// walks 32-pixel groups with the next group's loads in flight; the 4 wave partials are
// summed through LDS in a fixed order.
template <bool DIAG>
__device__ __forceinline__ void guided_f16_tile(const float* __restrict__ zb,
                                                const float* __restrict__ wr,
                                                float* __restrict__ out, int c, int hw,
                                                int split_len, int ez, int ea, int I, int J,
                                                int split, float* red) {
  const int p_begin = split * split_len;
  const int p_end = min(hw, p_begin + split_len);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = lane >> 5, r = lane & 31;
  const int ra0 = I * GT + r, ra1 = I * GT + 32 + r;
  const int rb0 = J * GT + r, rb1 = J * GT + 32 + r;
  // rows past c and pixels past the split read 0 through the descriptor's range check
  const auto rz = make_srd(zb, (uint32_t)c * (uint32_t)hw * 4u);
  const auto rw = make_srd(wr, (uint32_t)hw * 4u);
  const uint32_t oa0 = ra0 < c ? (uint32_t)(ra0 * hw + 8 * h) * 4u : BUF_OOB;
  const uint32_t oa1 = ra1 < c ? (uint32_t)(ra1 * hw + 8 * h) * 4u : BUF_OOB;
  const uint32_t ob0 = rb0 < c ? (uint32_t)(rb0 * hw + 8 * h) * 4u : BUF_OOB;
  const uint32_t ob1 = rb1 < c ? (uint32_t)(rb1 * hw + 8 * h) * 4u : BUF_OOB;
  const float sz = __builtin_ldexpf(1.f, 15 - ez), sa = __builtin_ldexpf(1.f, 15 - ea);
  const float inv2 = __builtin_ldexpf(1.f, ez + ea - 30);

  f32x16 a00, a01, a10, a11;
#pragma unroll
  for (int q = 0; q < 16; ++q) a00[q] = a01[q] = a10[q] = a11[q] = 0.f;

  struct Grp {
    f32x4 x[4][2][2];  // [row a0, a1, b0, b1][step][float4]
    f32x4 w[2][2];     // the 8 pixel weights of each step
  };
  auto load = [&](int p0, Grp& g) {
#pragma unroll
    for (int st = 0; st < 2; ++st) {
      const int pp = p0 + 16 * st;         // + 8h folded into the row offsets
      const bool ok = pp + 8 * h < p_end;  // hw % 8 == 0: a lane's 8 pixels all in or out
      const uint32_t po = ok ? (uint32_t)pp * 4u : BUF_OOB;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        g.x[0][st][q] = buf_ld4(rz, (oa0 | (po & BUF_OOB)) + (po & ~BUF_OOB) + 16u * q);
        g.x[1][st][q] = buf_ld4(rz, (oa1 | (po & BUF_OOB)) + (po & ~BUF_OOB) + 16u * q);
        if (!DIAG) {
          g.x[2][st][q] = buf_ld4(rz, (ob0 | (po & BUF_OOB)) + (po & ~BUF_OOB) + 16u * q);
          g.x[3][st][q] = buf_ld4(rz, (ob1 | (po & BUF_OOB)) + (po & ~BUF_OOB) + 16u * q);
        }
        g.w[st][q] = buf_ld4(rw, ok ? (uint32_t)(pp + 8 * h) * 4u + 16u * q : BUF_OOB);
      }
    }
  };
  auto compute = [&](const Grp& g) {
#pragma unroll
    for (int st = 0; st < 2; ++st) {
      f16x8_t ah0, al0, ah1, al1, g0, m0, g1, m1;
      split8w(g.x[0][st][0], g.x[0][st][1], g.w[st][0], g.w[st][1], sa, ah0, al0);
      split8w(g.x[1][st][0], g.x[1][st][1], g.w[st][0], g.w[st][1], sa, ah1, al1);
      if (DIAG) {
        split8(g.x[0][st][0], g.x[0][st][1], sz, g0, m0);
        split8(g.x[1][st][0], g.x[1][st][1], sz, g1, m1);
        a00 = MF16(ah0, g0, a00); a01 = MF16(ah0, g1, a01); a11 = MF16(ah1, g1, a11);
        a00 = MF16(ah0, m0, a00); a01 = MF16(ah0, m1, a01); a11 = MF16(ah1, m1, a11);
        a00 = MF16(al0, g0, a00); a01 = MF16(al0, g1, a01); a11 = MF16(al1, g1, a11);
      } else {
        split8(g.x[2][st][0], g.x[2][st][1], sz, g0, m0);
        split8(g.x[3][st][0], g.x[3][st][1], sz, g1, m1);
        a00 = MF16(ah0, g0, a00); a01 = MF16(ah0, g1, a01);
        a10 = MF16(ah1, g0, a10); a11 = MF16(ah1, g1, a11);
        a00 = MF16(ah0, m0, a00); a01 = MF16(ah0, m1, a01);
        a10 = MF16(ah1, m0, a10); a11 = MF16(ah1, m1, a11);
        a00 = MF16(al0, g0, a00); a01 = MF16(al0, g1, a01);
        a10 = MF16(al1, g0, a10); a11 = MF16(al1, g1, a11);
      }
    }
  };
  // waves interleave 32-pixel groups: wave w takes p_begin + 32 (w + 4 i)
  int p0 = p_begin + wave * 32;
  if (p0 < p_end) {
    Grp cur, nxt;
    load(p0, cur);
    for (; p0 < p_end; p0 += 128) {
      if (p0 + 128 < p_end) load(p0 + 128, nxt);
      compute(cur);
      cur = nxt;
    }
  }
  // 4 wave partials -> 2 LDS images: waves 2,3 store, waves 0,1 add, then sum
  auto put = [&](float* img, bool add) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int row = (q & 3) + 8 * (q >> 2) + 4 * h;
      float* q00 = img + row * GT + r;
      float* q01 = img + row * GT + 32 + r;
      float* q11 = img + (32 + row) * GT + 32 + r;
      float* q10 = img + (32 + row) * GT + r;
      *q00 = add ? *q00 + a00[q] : a00[q];
      *q01 = add ? *q01 + a01[q] : a01[q];
      *q11 = add ? *q11 + a11[q] : a11[q];
      if (!DIAG) *q10 = add ? *q10 + a10[q] : a10[q];
    }
  };
  if (wave >= 2) put(red + (wave - 2) * GT * GT, false);
  __syncthreads();
  if (wave < 2) put(red + wave * GT * GT, true);
  __syncthreads();
#pragma unroll
  for (int q = 0; q < (GT * GT) / 256; ++q) {
    const int el = q * 256 + tid;
    int row = el / GT, col = el % GT;
    if (DIAG && row >= 32 && col < 32) {  // mirrored quadrant of a diagonal tile
      const int t = row;
      row = col;
      col = t;
    }
    const int o = row * GT + col;
    out[el] = (red[o] + red[GT * GT + o]) * inv2;
  }
}

// block L of grid (nsplit * ntu * R, 1, b): xcd = L % 8, then region, tile, split group --
// the R regions of one (tile, split) are blocks L, L + 8, ..: the same XCD, adjacent
__global__ void __launch_bounds__(256, 2)
guided_partial_f16_kernel(const float* __restrict__ z, const float* __restrict__ wts,
                          float* __restrict__ ws, int c, int hw, int R, int nsplit,
                          int split_len, float w_max, const float* __restrict__ z_amax) {
  __shared__ __attribute__((aligned(16))) float red[2 * GT * GT];
  const int nt = cdiv(c, GT), ntu = nt * (nt + 1) / 2;
  const int L = blockIdx.x;
  const int xcd = L & 7;
  int rest = L >> 3;
  const int reg = rest % R;
  rest /= R;
  const int k = rest % ntu, split = (rest / ntu) * 8 + xcd;
  int I, J;
  tile_ij(k, nt, I, J);
  const int b = blockIdx.z;
  const float az = read_amax(z_amax);
  const int ez = amax_exp(az), ea = amax_exp(az * w_max);
  const float* zb = z + (size_t)b * c * hw;
  const float* wr = wts + (size_t)reg * hw;
  float* out = ws + ((((size_t)b * R + reg) * ntu + k) * nsplit + split) * (GT * GT);
  if (I == J)
    guided_f16_tile<true>(zb, wr, out, c, hw, split_len, ez, ea, I, J, split, red);
  else
    guided_f16_tile<false>(zb, wr, out, c, hw, split_len, ez, ea, I, J, split, red);
}

// ---------------------------------------------------------------- forward, fp32 MFMA
// Any hw.  One block = one 64 x 64 tile (I <= J) of one (image, region) over one pixel
// split: 64 rows x 64 pixels of tile-rows I (times the pixel weight, applied as the tile
// is staged) and J in LDS (pitch 65), each wave a 32 x 32 quadrant on
// v_mfma_f32_32x32x2_f32.  grid (nsplit * R, ntu, b), region fastest.
__global__ void __launch_bounds__(256)
guided_partial_f32_kernel(const float* __restrict__ z, const float* __restrict__ wts,
                          float* __restrict__ ws, int c, int hw, int R, int nsplit,
                          int split_len) {
  __shared__ __attribute__((aligned(16))) float smem[2 * GT * GP];
  float* rI = smem;
  float* rJ = smem + GT * GP;
  const int nt = cdiv(c, GT), ntu = nt * (nt + 1) / 2;
  int I, J;
  tile_ij(blockIdx.y, nt, I, J);
  const int reg = blockIdx.x % R, split = blockIdx.x / R, b = blockIdx.z;
  const int p_begin = split * split_len;
  const int p_end = min(hw, p_begin + split_len);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = lane >> 5, l32 = lane & 31;
  const int qi = wave >> 1, qj = wave & 1;
  const float* zb = z + (size_t)b * c * hw;
  const float* wr = wts + (size_t)reg * hw;

  // loader: thread -> (row = tid / 4, 16 consecutive pixels at (tid % 4) * 16)
  const int lrow = tid >> 2, lseg = (tid & 3) * 16;
  const int gi = I * GT + lrow, gj = J * GT + lrow;
  float regI[16], regJ[16];
  auto fetch = [&](int p0) {
    const float* srcI = zb + (size_t)gi * hw + p0 + lseg;
    const float* srcJ = zb + (size_t)gj * hw + p0 + lseg;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int pp = p0 + lseg + e;
      const bool ok = pp < p_end;
      regI[e] = (ok && gi < c) ? srcI[e] * wr[pp] : 0.f;
      regJ[e] = (ok && gj < c) ? srcJ[e] : 0.f;
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      rI[lrow * GP + lseg + e] = regI[e];
      rJ[lrow * GP + lseg + e] = regJ[e];
    }
  };

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  const int a_off = (qi * 32 + l32) * GP + h * 32;
  const int b_off = (qj * 32 + l32) * GP + h * 32;

  if (p_begin < p_end) fetch(p_begin);
  for (int p0 = p_begin; p0 < p_end; p0 += GKC) {
    __syncthreads();
    store();
    __syncthreads();
    if (p0 + GKC < p_end) fetch(p0 + GKC);
#pragma unroll
    for (int s = 0; s < 32; ++s)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(rI[a_off + s], rJ[b_off + s], acc, 0, 0, 0);
  }
  float* out = ws + ((((size_t)b * R + reg) * ntu + blockIdx.y) * nsplit + split) * (GT * GT);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = qi * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
    out[row * GT + qj * 32 + l32] = acc[r];
  }
}

// ---------------------------------------------------------------- finalize
// grid (ntu * FSUB, b * R), 512 threads: 64 tile elements (16 lanes x float4) x 32
// split-lanes.  Split-lane kl sums partials kl, kl + 32, ..; the 32 lane sums of an element
// are added through LDS in split-lane order: bit-reproducible.  Then scale, mirror, G - T,
// the sub-tile's loss partial and A.
constexpr int FEL = 64, FKL = 32, FNT = FEL / 4 * FKL;
constexpr int FSUB = GT * GT / FEL;

__global__ void __launch_bounds__(FNT)
guided_finalize_kernel(const float* __restrict__ ws, int c, int b, int R, int nsplit,
                       float scale, float* __restrict__ g_out, const float* __restrict__ target,
                       float* __restrict__ coef, int cpad, float cA, Lam lam,
                       float* __restrict__ loss_parts) {
  __shared__ float part[FKL * (FEL + 1)];
  const int nt = cdiv(c, GT), ntu = nt * (nt + 1) / 2;
  const int tile = blockIdx.x / FSUB, sub = blockIdx.x % FSUB;
  int I, J;
  tile_ij(tile, nt, I, J);
  const int bb = blockIdx.y, bi = bb / R, reg = bb % R;
  const float* src = ws + ((size_t)bb * ntu + tile) * nsplit * (GT * GT) + sub * FEL;
  const int q4 = threadIdx.x % (FEL / 4), kl = threadIdx.x / (FEL / 4);
  {
    f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0, s2 = s0, s3 = s0;
    const f32x4* p4 = reinterpret_cast<const f32x4*>(src) + q4;
    constexpr int ST = GT * GT / 4;  // float4s per partial
    int k = kl;
    for (; k + 3 * FKL < nsplit; k += 4 * FKL) {
      const f32x4 a0 = p4[(size_t)(k + 0 * FKL) * ST], a1 = p4[(size_t)(k + 1 * FKL) * ST];
      const f32x4 a2 = p4[(size_t)(k + 2 * FKL) * ST], a3 = p4[(size_t)(k + 3 * FKL) * ST];
      s0 += a0;
      s1 += a1;
      s2 += a2;
      s3 += a3;
    }
    for (; k < nsplit; k += FKL) s0 += p4[(size_t)k * ST];
    const f32x4 t = (s0 + s1) + (s2 + s3);
#pragma unroll
    for (int i = 0; i < 4; ++i) part[kl * (FEL + 1) + 4 * q4 + i] = t[i];
  }
  __syncthreads();
  if (threadIdx.x < FEL) {  // one wave
    const int el = threadIdx.x, e = sub * FEL + el;
    float s = 0.f;
#pragma unroll 8
    for (int q = 0; q < FKL; ++q) s += part[q * (FEL + 1) + el];
    const int gi = I * GT + e / GT, gj = J * GT + e % GT;
    float sq = 0.f;
    if (gi < c && gj < c) {
      const float g = s * scale;
      if (g_out) {
        g_out[((size_t)bb * c + gi) * c + gj] = g;
        if (I != J) g_out[((size_t)bb * c + gj) * c + gi] = g;
      }
      const float d = g - target[((size_t)reg * c + gi) * c + gj];
      sq = (I != J ? 2.f : 1.f) * d * d;
      if (coef) {
        const float a = cA * lam.v[reg] * d;
        float* cb = coef + (size_t)bb * cpad * cpad;
        cb[(size_t)gi * cpad + gj] = a;
        if (I != J) cb[(size_t)gj * cpad + gi] = a;
      }
    }
    const float t = wave_sum(sq);
    if (el == 0)
      loss_parts[((size_t)reg * b + bi) * ntu * FSUB + (size_t)tile * FSUB + sub] = t;
  }
}

// block r (one wave): loss_r[r] = inv * sum of region r's n partials, in a fixed order
__global__ void __launch_bounds__(64)
guided_loss_kernel(const float* __restrict__ parts, int n, float inv, float* __restrict__ loss_r) {
  const float* p = parts + (size_t)blockIdx.x * n;
  const int lane = threadIdx.x;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  int i = lane;
  for (; i + 192 < n; i += 256) {
    s0 += p[i];
    s1 += p[i + 64];
    s2 += p[i + 128];
    s3 += p[i + 192];
  }
  for (; i < n; i += 64) s0 += p[i];
  const float s = wave_sum((s0 + s1) + (s2 + s3));
  if (lane == 0) loss_r[blockIdx.x] = s * inv;
}

__global__ void guided_zero_kernel(float* p, long long n) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x)
    p[i] = 0.f;
}

// ---------------------------------------------------------------- backward
// One block = PT pixels of one image, every output channel, every region.  The c x PT slab
// of z goes to LDS once -- split path: fp16 hi/lo planes of s_z z as 16-B units (8 channels
// of one pixel) at [pixel][unit ^ (pixel & 7) within each group of 8 units], so the
// fragment reads of 32 lanes (32 pixels, one unit index) spread over the banks; fp32 path:
// [channel][pixel] floats.  Wave w owns the 32-pixel sub-tile w % (PT / 32) and the 32-row
// output blocks w / (PT / 32), + 4 / (PT / 32), ..: per block and region it runs A_r z over
// all channels (A fragments straight from global: a lane reads 8 consecutive floats of its
// row; z fragments from LDS), then total += (w_r[p] / scale) * acc per register -- p is the
// lane's pixel in the 32 x 32 MFMA output layout.
template <int PT, bool F16>
__global__ void __launch_bounds__(256)
guided_bwd_kernel(const float* __restrict__ coef, const float* __restrict__ z,
                  const float* __restrict__ wts, float* __restrict__ dz, int c, int hw, int R,
                  int cpad, const float* __restrict__ acc_scale, int accumulate,
                  const float* __restrict__ z_amax, const float* __restrict__ coef_amax) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  constexpr int NSUB = PT / 32, GPP = 256 / PT;  // sub-tiles; 8-channel groups per pass
  const int CU = rup(c, 64), CK = rup(c, 16), NU = CU / 8;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = lane >> 5, l32 = lane & 31;
  const int b = blockIdx.y, p0 = blockIdx.x * PT;
  const float* zb = z + (size_t)b * c * hw;
  float* dzb = dz + (size_t)b * c * hw;
  const auto rz = make_srd(zb, (uint32_t)c * (uint32_t)hw * 4u);
  int ez = 0, ec = 0;
  if (F16) {
    ez = amax_exp(read_amax(z_amax));
    ec = amax_exp(read_amax(coef_amax));
  }
  const float sz = __builtin_ldexpf(1.f, 15 - ez), sc = __builtin_ldexpf(1.f, 15 - ec);
  const float inv2 = F16 ? __builtin_ldexpf(1.f, ez + ec - 30) : 1.f;
  const int plane = PT * CU * 2;  // bytes of one fp16 plane

  {  // stage: thread -> pixel tid % PT, 8-channel group tid / PT of each pass
    const int px = tid % PT, grp = tid / PT;
    const bool pok = p0 + px < hw;
    for (int u = grp; u < NU; u += GPP) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int ch = u * 8 + j;
        v[j] = buf_ld(rz, (pok && ch < c) ? (uint32_t)(ch * hw + p0 + px) * 4u : BUF_OOB);
      }
      if (F16) {
        f16x8_t hi, lo;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float t = v[j] * sz;
          hi[j] = (_Float16)t;
          lo[j] = (_Float16)(t - (float)hi[j]);
        }
        const int us = (u & ~7) | ((u ^ px) & 7);
        *reinterpret_cast<f16x8_t*>(lds + (px * NU + us) * 16) = hi;
        *reinterpret_cast<f16x8_t*>(lds + plane + (px * NU + us) * 16) = lo;
      } else {
        float* zs = reinterpret_cast<float*>(lds);
#pragma unroll
        for (int j = 0; j < 8; ++j) zs[(u * 8 + j) * PT + px] = v[j];
      }
    }
  }
  __syncthreads();

  const int sub = wave % NSUB;
  const int px = sub * 32 + l32, p = p0 + px;
  const bool pok = p < hw;
  const float s = acc_scale ? *acc_scale : 1.f;
  float wv[STX_GUIDE_MAX];
#pragma unroll
  for (int r = 0; r < STX_GUIDE_MAX; ++r)
    wv[r] = (r < R && pok) ? wts[(size_t)r * hw + p] * inv2 : 0.f;
  const int nmb = cdiv(c, 32);
  const float* coefb = coef + (size_t)b * R * cpad * cpad;
  for (int mb = wave / NSUB; mb < nmb; mb += 4 / NSUB) {
    f32x16 total;
#pragma unroll
    for (int k = 0; k < 16; ++k) total[k] = 0.f;
#pragma unroll
    for (int r = 0; r < STX_GUIDE_MAX; ++r) {
      if (r >= R) continue;
      const float* arow = coefb + ((size_t)r * cpad + mb * 32 + l32) * cpad + 8 * h;
      f32x16 acc;
#pragma unroll
      for (int k = 0; k < 16; ++k) acc[k] = 0.f;
      for (int ks = 0; ks < CK / 16; ++ks) {
        const f32x4 a0 = *reinterpret_cast<const f32x4*>(arow + ks * 16);
        const f32x4 a1 = *reinterpret_cast<const f32x4*>(arow + ks * 16 + 4);
        if (F16) {
          f16x8_t ah, al;
          split8(a0, a1, sc, ah, al);
          const int u = ks * 2 + h, us = (u & ~7) | ((u ^ px) & 7);
          const f16x8_t bh = *reinterpret_cast<const f16x8_t*>(lds + (px * NU + us) * 16);
          const f16x8_t bl =
              *reinterpret_cast<const f16x8_t*>(lds + plane + (px * NU + us) * 16);
          acc = MF16(ah, bh, acc);
          acc = MF16(ah, bl, acc);
          acc = MF16(al, bh, acc);
        } else {
          const float* zs = reinterpret_cast<const float*>(lds) + (ks * 16 + 8 * h) * PT + px;
#pragma unroll
          for (int j = 0; j < 8; ++j)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(j < 4 ? a0[j] : a1[j - 4], zs[j * PT],
                                                       acc, 0, 0, 0);
        }
      }
#pragma unroll
      for (int k = 0; k < 16; ++k) total[k] = __builtin_fmaf(wv[r], acc[k], total[k]);
    }
    if (pok) {
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int row = mb * 32 + (k & 3) + 8 * (k >> 2) + 4 * h;
        if (row < c) {
          float* o = dzb + (size_t)row * hw + p;
          *o = accumulate ? *o + s * total[k] : s * total[k];
        }
      }
    }
  }
}
#undef MF16

// ---------------------------------------------------------------- host
struct Geo {
  int ntu, ns16, sl16, ns32, sl32;
};

static Geo geometry(int bR, int c, int hw) {
  Geo g;
  const int nt = cdiv(c, GT);
  g.ntu = nt * (nt + 1) / 2;
  {  // split kernel: 32-pixel groups over 4 waves, splits of whole 256-pixel runs, in
     // multiples of 8 (XCD grouping), ~640 blocks
    int want = rup(cdiv(640, g.ntu * bR), 8);
    const int max_splits = std::max(1, cdiv(hw, 256));
    want = std::max(8, std::min(want, rup(max_splits, 8)));
    g.sl16 = rup(cdiv(hw, want), 256);
    g.ns16 = rup(cdiv(hw, g.sl16), 8);
  }
  {  // fp32 kernel: ~512 blocks, at least 8 chunks (512 pixels) per split
    const int chunks = cdiv(hw, GKC);
    int want = cdiv(512, g.ntu * bR);
    want = std::max(1, std::min(want, cdiv(chunks, 8)));
    g.sl32 = cdiv(chunks, want) * GKC;
    g.ns32 = cdiv(hw, g.sl32);
  }
  return g;
}

static size_t parts_offset(int b, int c, int hw, int R) {
  const Geo g = geometry(b * R, c, hw);
  return (size_t)b * R * g.ntu * std::max(g.ns16, g.ns32) * GT * GT * sizeof(float);
}

static size_t ws_bytes_needed(int b, int c, int hw, int R) {
  const Geo g = geometry(b * R, c, hw);
  return parts_offset(b, c, hw, R) + ((size_t)R * b * g.ntu * FSUB + 64) * sizeof(float);
}

static bool dims_ok(int b, int c, int hw, int R) {
  return b > 0 && c > 0 && hw > 0 && R >= 1 && R <= STX_GUIDE_MAX &&
         (long long)c * hw * 4 < (1ll << 31) && (long long)b * R <= 65535;
}

}  // namespace guided
}  // namespace stx

using namespace stx;
using namespace stx::guided;

extern "C" size_t stx_guided_style_ws(int b, int c, int hw, int R) {
  if (!dims_ok(b, c, hw, R)) return 0;
  return ws_bytes_needed(b, c, hw, R);
}

extern "C" int stx_guided_style_loss(const float* z, const float* wts, float w_max,
                                     const float* target, float* g_out, float* coef,
                                     float* loss_r, int b, int c, int hw, int R,
                                     const float* lambda, float weight, const float* z_amax,
                                     void* ws, size_t ws_bytes, void* stream) {
  if (R < 1 || R > STX_GUIDE_MAX) {
    set_error("stx_guided_style_loss: 1 <= R <= %d required (got %d)", STX_GUIDE_MAX, R);
    return STX_E_INVALID;
  }
  if (!z || !wts || !target || !loss_r || !lambda) {
    set_error("stx_guided_style_loss: z, wts, target, loss_r and lambda are required");
    return STX_E_INVALID;
  }
  if (!dims_ok(b, c, hw, R) || !(w_max > 0.f)) {
    set_error("stx_guided_style_loss: invalid dims or w_max");
    return STX_E_INVALID;
  }
  const size_t need = ws_bytes_needed(b, c, hw, R);
  if (!ws || ws_bytes < need) {
    set_error("stx_guided_style_loss: workspace %zu < %zu", ws_bytes, need);
    return STX_E_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  const Geo g = geometry(b * R, c, hw);
  float* slabs = (float*)ws;
  float* parts = (float*)((char*)ws + parts_offset(b, c, hw, R));
  const bool f16 = z_amax && hw % 8 == 0 && (reinterpret_cast<uintptr_t>(z) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(wts) & 15) == 0;
  int nsplit;
  if (f16) {
    nsplit = g.ns16;
    hipLaunchKernelGGL(guided_partial_f16_kernel, dim3(nsplit * g.ntu * R, 1, b), dim3(256), 0,
                       st, z, wts, slabs, c, hw, R, nsplit, g.sl16, w_max, z_amax);
  } else {
    nsplit = g.ns32;
    hipLaunchKernelGGL(guided_partial_f32_kernel, dim3(nsplit * R, g.ntu, b), dim3(256), 0, st,
                       z, wts, slabs, c, hw, R, nsplit, g.sl32);
  }
  const int cpad = stx_gram_coef_pitch(c);
  if (coef && cpad != c) {  // zero the padding (the finalize writes c x c)
    const long long cnt = (long long)b * R * cpad * cpad;
    hipLaunchKernelGGL(guided_zero_kernel, dim3((int)std::min<long long>((cnt + 255) / 256, 2048)),
                       dim3(256), 0, st, coef, cnt);
  }
  Lam lam{};
  for (int r = 0; r < R; ++r) lam.v[r] = lambda[r];
  const double n = (double)c * hw;
  const float cA = (float)(weight * 4.0 / ((double)b * c * c * n));
  hipLaunchKernelGGL(guided_finalize_kernel, dim3(g.ntu * FSUB, b * R), dim3(FNT), 0, st, slabs,
                     c, b, R, nsplit, (float)(1.0 / n), g_out, target, coef, cpad, cA, lam,
                     parts);
  hipLaunchKernelGGL(guided_loss_kernel, dim3(R), dim3(64), 0, st, parts, b * g.ntu * FSUB,
                     (float)(1.0 / ((double)b * c * c)), loss_r);
  return check_launch("stx_guided_style_loss");
}

extern "C" int stx_guided_gram_bwd(const float* coef, const float* z, const float* wts,
                                   float* dz, int b, int c, int h, int w, int R,
                                   const float* acc_scale_dev, int accumulate,
                                   const float* z_amax, const float* coef_amax, void* stream) {
  if (R < 1 || R > STX_GUIDE_MAX) {
    set_error("stx_guided_gram_bwd: 1 <= R <= %d required (got %d)", STX_GUIDE_MAX, R);
    return STX_E_INVALID;
  }
  if (!coef || !z || !wts || !dz) {
    set_error("stx_guided_gram_bwd: coef, z, wts and dz are required");
    return STX_E_INVALID;
  }
  const long long hwl = (long long)h * w;
  if (h <= 0 || w <= 0 || hwl >= (1ll << 31) || !dims_ok(b, c, (int)hwl, R) || c > 512 ||
      (reinterpret_cast<uintptr_t>(coef) & 15)) {
    set_error("stx_guided_gram_bwd: invalid dims (c <= 512, coef 16-byte aligned)");
    return STX_E_INVALID;
  }
  const int hw = (int)hwl, cpad = stx_gram_coef_pitch(c), CU = rup(c, 64);
  const bool f16 = z_amax && coef_amax;
  hipStream_t st = (hipStream_t)stream;
  // 64 pixels per block while the c x 64 slab fits 64 KB of LDS, else 32
  if (CU <= 256) {
    const dim3 grid(cdiv(hw, 64), b);
    const size_t lds = (size_t)64 * CU * 4;
    if (f16)
      hipLaunchKernelGGL((guided_bwd_kernel<64, true>), grid, dim3(256), lds, st, coef, z, wts,
                         dz, c, hw, R, cpad, acc_scale_dev, accumulate, z_amax, coef_amax);
    else
      hipLaunchKernelGGL((guided_bwd_kernel<64, false>), grid, dim3(256), lds, st, coef, z, wts,
                         dz, c, hw, R, cpad, acc_scale_dev, accumulate, z_amax, coef_amax);
  } else {
    const dim3 grid(cdiv(hw, 32), b);
    const size_t lds = (size_t)32 * CU * 4;
    if (f16)
      hipLaunchKernelGGL((guided_bwd_kernel<32, true>), grid, dim3(256), lds, st, coef, z, wts,
                         dz, c, hw, R, cpad, acc_scale_dev, accumulate, z_amax, coef_amax);
    else
      hipLaunchKernelGGL((guided_bwd_kernel<32, false>), grid, dim3(256), lds, st, coef, z, wts,
                         dz, c, hw, R, cpad, acc_scale_dev, accumulate, z_amax, coef_amax);
  }
  return check_launch("stx_guided_gram_bwd");
}

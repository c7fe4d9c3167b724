// Dense optical flow between two conditioned frames: coarse-to-fine Horn-Schunck with
// warping, relaxed by Jacobi iterations (include/stx.h states every expression; DESIGN.md
// 3.8).  The pieces: luma planes, the linearisation of the data term at the current flow,
// the Jacobi relaxation and the scaling of a prolonged flow.  The pyramid and the
// prolongation themselves are stx_resample2d (triangle).
//
// flow_jacobi_kernel is the hot path: levels x warps x iters iterations per frame pair, each
// a 9-point stencil over 8 B of state per pixel.  A block owns a JT x JT tile and relaxes the
// tile plus a JK-cell halo (clipped at the image border) in LDS for up to JK iterations:
// after iteration r the outermost r rings of the halo are stale, the tile never is, and
// every cell is computed by the same instructions whichever block or launch computes it --
// K fused iterations are K single ones bit for bit.  An image that one tile covers has no
// halo at all and takes any number of iterations in one launch.
#include "common.h"
#include "../../include/stx.h"

#include <climits>

#pragma clang fp contract(off)  // the expressions are the header's: no fusing beyond the fmaf written

namespace stx {

constexpr int EB = 256;  // threads per block, all kernels

static bool est_aligned16(const void* p) { return !(reinterpret_cast<uintptr_t>(p) & 15); }

static bool est_dims_ok(int n, int h, int w) {
  return n >= 1 && n <= 65535 && h >= 2 && w >= 2 && (long long)h * w <= INT_MAX / 4;
}

// ------------------------------------------------------------------------------- luma
struct LumaK {
  float mean[3], std_[3];
};

__device__ __forceinline__ float luma1(float r, float g, float b, const LumaK& k) {
  const float R = fmaf(r, k.std_[0], k.mean[0]);
  const float G = fmaf(g, k.std_[1], k.mean[1]);
  const float B = fmaf(b, k.std_[2], k.mean[2]);
  float l = 0.299f * R;
  l = fmaf(0.587f, G, l);
  l = fmaf(0.114f, B, l);
  return 255.f * l;
}

// one float4 (vec) or one float per thread; blockIdx.y: the image
__global__ void __launch_bounds__(EB)
flow_luma_kernel(const float* __restrict__ img, float* __restrict__ grey, int hw, LumaK k,
                 int vec) {
  const size_t b = blockIdx.y;
  const float* p = img + b * 3 * (size_t)hw;
  float* q = grey + b * (size_t)hw;
  const int t = blockIdx.x * EB + threadIdx.x;
  if (vec) {
    const int hw4 = hw >> 2;
    if (t >= hw4) return;
    const f32x4 r = reinterpret_cast<const f32x4*>(p)[t];
    const f32x4 g = reinterpret_cast<const f32x4*>(p + hw)[t];
    const f32x4 bl = reinterpret_cast<const f32x4*>(p + 2 * (size_t)hw)[t];
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = luma1(r[e], g[e], bl[e], k);
    reinterpret_cast<f32x4*>(q)[t] = o;
  } else {
    if (t >= hw) return;
    q[t] = luma1(p[t], p[hw + t], p[2 * (size_t)hw + t], k);
  }
}

// -------------------------------------------------------------------------- linearize
// w00 a00 + w01 a01 + w10 a10 + w11 a11: one product and three fmaf (stx_flow_warp's sum)
__device__ __forceinline__ float blend4(float w00, float w01, float w10, float w11, float a00,
                                        float a01, float a10, float a11) {
  float v = w00 * a00;
  v = fmaf(w01, a01, v);
  v = fmaf(w10, a10, v);
  return fmaf(w11, a11, v);
}

__global__ void __launch_bounds__(EB)
flow_linearize_kernel(const float* __restrict__ a, const float* __restrict__ b,
                      const float* __restrict__ flow, float* __restrict__ coef, int h, int w) {
  const int hw = h * w;
  const int p = blockIdx.x * EB + threadIdx.x;
  if (p >= hw) return;
  const size_t img = blockIdx.y;
  const int i = p / w, j = p - i * w;
  const float* f = flow + img * 2 * (size_t)hw;
  const float u = f[p], v = f[hw + p];
  // fmaxf / fminf return the other operand of a NaN: a NaN coordinate becomes 0, and
  // whatever the flow's bits the taps lie in the plane
  const float y = fminf(fmaxf((float)i + v, 0.f), (float)(h - 1));
  const float x = fminf(fmaxf((float)j + u, 0.f), (float)(w - 1));
  const int y0 = min((int)floorf(y), h - 2), x0 = min((int)floorf(x), w - 2);
  const float fy = y - (float)y0, fx = x - (float)x0;
  const float gy = 1.f - fy, gx = 1.f - fx;
  const float w00 = gy * gx, w01 = gy * fx, w10 = fy * gx, w11 = fy * fx;
  // rows y0-1 .. y0+2 and columns x0-1 .. x0+2 of B, indices clamped to the plane
  const float* B = b + img * (size_t)hw;
  int ro[4], co[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    ro[k] = min(max(y0 - 1 + k, 0), h - 1) * w;
    co[k] = min(max(x0 - 1 + k, 0), w - 1);
  }
  float P[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) P[r][c] = B[ro[r] + co[c]];
  const float bw = blend4(w00, w01, w10, w11, P[1][1], P[1][2], P[2][1], P[2][2]);
  const float ix = blend4(w00, w01, w10, w11, 0.5f * (P[1][2] - P[1][0]), 0.5f * (P[1][3] - P[1][1]),
                          0.5f * (P[2][2] - P[2][0]), 0.5f * (P[2][3] - P[2][1]));
  const float iy = blend4(w00, w01, w10, w11, 0.5f * (P[2][1] - P[0][1]), 0.5f * (P[2][2] - P[0][2]),
                          0.5f * (P[3][1] - P[1][1]), 0.5f * (P[3][2] - P[1][2]));
  const float av = a[img * (size_t)hw + p];
  float* o = coef + img * 3 * (size_t)hw;
  o[p] = ix;
  o[hw + p] = iy;
  o[2 * (size_t)hw + p] = fmaf(iy, v, fmaf(ix, u, av - bw));
}

// ----------------------------------------------------------------------------- jacobi
// Tile, halo and block size by measurement: 16 waves per block hide the LDS
// and load latency that 4 waves of 9 cells each (251 VGPRs) could not.
constexpr int JT = 32;                       // tile side
constexpr int JK = STX_FLOW_JACOBI_MAXFUSE;  // halo = the most iterations of a tiled launch
constexpr int JB = 1024;                     // threads per block
constexpr int JCELLS = (JT + 2 * JK) * (JT + 2 * JK);  // the region: tile and halo
constexpr int JC = (JCELLS + JB - 1) / JB;             // cells per thread (3, the last partly)

enum { NB_UP = 1, NB_DN = 2, NB_LF = 4, NB_RT = 8, NB_TILE = 16, NB_ON = 32 };

// The region's cells are numbered row by row at the region's own width: a wave's 64
// consecutive cells are 64 consecutive float2 of LDS (no bank conflict at any width).
// Thread t owns cells t, t + JB, ...: their coefficients and reciprocals stay in
// registers over the iterations, (u, v) ping-pongs between the two LDS buffers.
__global__ void __launch_bounds__(JB)
flow_jacobi_kernel(const float* __restrict__ coef, const float* __restrict__ uv_in,
                   float* __restrict__ uv_out, int h, int w, float a2, int iters) {
  __shared__ float2 buf[2][JCELLS];
  const int ty0 = blockIdx.y * JT, tx0 = blockIdx.x * JT;
  const int r0 = max(ty0 - JK, 0), r1 = min(ty0 + JT + JK, h);
  const int c0 = max(tx0 - JK, 0), c1 = min(tx0 + JT + JK, w);
  const int rh = r1 - r0, rw = c1 - c0, cells = rh * rw;
  const size_t hw = (size_t)h * w, img = blockIdx.z;
  const float* cf = coef + img * 3 * hw;
  const float* ui = uv_in + img * 2 * hw;
  float* uo = uv_out + img * 2 * hw;

  float ix[JC], iy[JC], cc[JC], ru[JC], rv[JC];
  int nb[JC];
#pragma unroll
  for (int k = 0; k < JC; ++k) {
    const int cell = threadIdx.x + k * JB;
    nb[k] = 0;
    ix[k] = iy[k] = cc[k] = ru[k] = rv[k] = 0.f;
    if (cell < cells) {
      const int lr = cell / rw, lc = cell - lr * rw;
      const int gi = r0 + lr, gj = c0 + lc;
      const size_t g = (size_t)gi * w + gj;
      ix[k] = cf[g];
      iy[k] = cf[hw + g];
      cc[k] = cf[2 * hw + g];
      ru[k] = 1.f / fmaf(ix[k], ix[k], a2);
      rv[k] = 1.f / fmaf(iy[k], iy[k], a2);
      buf[0][cell] = make_float2(ui[g], ui[hw + g]);
      const bool tile = gi >= ty0 && gi < ty0 + JT && gj >= tx0 && gj < tx0 + JT;
      nb[k] = NB_ON | (lr > 0 ? NB_UP : 0) | (lr < rh - 1 ? NB_DN : 0) | (lc > 0 ? NB_LF : 0) |
              (lc < rw - 1 ? NB_RT : 0) | (tile ? NB_TILE : 0);
    }
  }
  __syncthreads();

  for (int it = 0; it < iters; ++it) {
    const float2* s = buf[it & 1];
    float2* d = buf[(it & 1) ^ 1];
    const bool last = it == iters - 1;
#pragma unroll
    for (int k = 0; k < JC; ++k) {
      if (!(nb[k] & NB_ON)) continue;
      const int cell = threadIdx.x + k * JB;
      // a neighbour past a region edge is the cell itself along that axis: the image's
      // replicated edge where the region ends at the image, a stale halo cell elsewhere
      const int n_ = cell - ((nb[k] & NB_UP) ? rw : 0), s_ = cell + ((nb[k] & NB_DN) ? rw : 0);
      const int lf = (nb[k] & NB_LF) ? 1 : 0, rt = (nb[k] & NB_RT) ? 1 : 0;
      const float2 m = s[cell];
      const float2 vn = s[n_], vs = s[s_], vw = s[cell - lf], ve = s[cell + rt];
      const float2 vnw = s[n_ - lf], vne = s[n_ + rt], vsw = s[s_ - lf], vse = s[s_ + rt];
      const float eu = (vn.x + vs.x) + (vw.x + ve.x), du = (vnw.x + vne.x) + (vsw.x + vse.x);
      const float ev = (vn.y + vs.y) + (vw.y + ve.y), dv = (vnw.y + vne.y) + (vsw.y + vse.y);
      const float ub = fmaf(du, 1.f / 12.f, eu * (1.f / 6.f));
      const float vb = fmaf(dv, 1.f / 12.f, ev * (1.f / 6.f));
      const float un = fmaf(fmaf(-iy[k], m.y, cc[k]), ix[k], a2 * ub) * ru[k];
      const float vv = fmaf(fmaf(-ix[k], m.x, cc[k]), iy[k], a2 * vb) * rv[k];
      if (!last) {
        d[cell] = make_float2(un, vv);
      } else if (nb[k] & NB_TILE) {
        const int lr = cell / rw, lc = cell - lr * rw;
        const size_t g = (size_t)(r0 + lr) * w + (c0 + lc);
        uo[g] = un;
        uo[hw + g] = vv;
      }
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------ scale
__global__ void __launch_bounds__(EB)
flow_scale_kernel(float* __restrict__ flow, int hw, float sx, float sy) {
  const int p = blockIdx.x * EB + threadIdx.x;
  if (p >= hw) return;
  float* f = flow + (size_t)blockIdx.y * 2 * hw;
  f[p] *= sx;
  f[hw + p] *= sy;
}

}  // namespace stx

using namespace stx;

extern "C" int stx_flow_pyramid(int h, int w, int min_side, int* hs, int* ws, int cap) {
  if (h < 2 || w < 2 || min_side < 2 || cap < 0 || ((hs || ws) && !(hs && ws))) {
    set_error("stx_flow_pyramid: invalid arguments (h %d w %d min_side %d; h, w, min_side >= 2)",
              h, w, min_side);
    return -STX_E_INVALID;
  }
  int levels = 0;
  for (;;) {
    if (hs && levels < cap) {
      hs[levels] = h;
      ws[levels] = w;
    }
    ++levels;
    if ((h < w ? h : w) / 2 < min_side) break;
    h = (h + 1) / 2;
    w = (w + 1) / 2;
  }
  return levels;
}

extern "C" int stx_flow_luma(const float* img, float* grey, int n, int h, int w,
                             const float* mean, const float* std_, void* stream) {
  if (!img || !grey || !mean || !std_ || !est_dims_ok(n, h, w)) {
    set_error("stx_flow_luma: invalid arguments (n %d h %d w %d; h, w >= 2)", n, h, w);
    return STX_E_INVALID;
  }
  LumaK k;
  for (int c = 0; c < 3; ++c) {
    k.mean[c] = mean[c];
    k.std_[c] = std_[c];
  }
  const int hw = h * w;
  const int vec = hw % 4 == 0 && est_aligned16(img) && est_aligned16(grey);
  hipLaunchKernelGGL(flow_luma_kernel, dim3(cdiv(vec ? hw / 4 : hw, EB), n), dim3(EB), 0,
                     (hipStream_t)stream, img, grey, hw, k, vec);
  return check_launch("stx_flow_luma");
}

extern "C" int stx_flow_linearize(const float* a, const float* b, const float* flow, float* coef,
                                  int n, int h, int w, void* stream) {
  if (!a || !b || !flow || !coef || coef == flow || !est_dims_ok(n, h, w)) {
    set_error("stx_flow_linearize: invalid arguments (n %d h %d w %d; h, w >= 2)", n, h, w);
    return STX_E_INVALID;
  }
  hipLaunchKernelGGL(flow_linearize_kernel, dim3(cdiv(h * w, EB), n), dim3(EB), 0,
                     (hipStream_t)stream, a, b, flow, coef, h, w);
  return check_launch("stx_flow_linearize");
}

extern "C" int stx_flow_scale(float* flow, int n, int h, int w, float sx, float sy, void* stream) {
  if (!flow || !est_dims_ok(n, h, w)) {
    set_error("stx_flow_scale: invalid arguments (n %d h %d w %d; h, w >= 2)", n, h, w);
    return STX_E_INVALID;
  }
  hipLaunchKernelGGL(flow_scale_kernel, dim3(cdiv(h * w, EB), n), dim3(EB), 0, (hipStream_t)stream,
                     flow, h * w, sx, sy);
  return check_launch("stx_flow_scale");
}

extern "C" size_t stx_flow_jacobi_ws(int n, int h, int w) {
  if (!est_dims_ok(n, h, w)) return 0;
  return (size_t)n * 2 * h * w * sizeof(float);
}

extern "C" int stx_flow_jacobi(const float* coef, const float* uv_in, float* uv_out, int n, int h,
                               int w, float alpha, int iters, int fuse, void* ws, size_t ws_bytes,
                               void* stream) {
  if (!coef || !uv_in || !uv_out || uv_in == uv_out || !est_dims_ok(n, h, w) || iters < 1 ||
      fuse < 0 || fuse > STX_FLOW_JACOBI_MAXFUSE || !(alpha > 0.f)) {
    set_error("stx_flow_jacobi: invalid arguments (n %d h %d w %d alpha %g iters %d fuse %d; "
              "h, w >= 2, alpha > 0, iters >= 1, 0 <= fuse <= %d, uv_out != uv_in)",
              n, h, w, (double)alpha, iters, fuse, STX_FLOW_JACOBI_MAXFUSE);
    return STX_E_INVALID;
  }
  // a single launch needs no workspace
  const bool single = (fuse ? fuse : (h <= JT && w <= JT ? iters : JK)) >= iters;
  if (!single && (!ws || ws_bytes < stx_flow_jacobi_ws(n, h, w))) {
    set_error("stx_flow_jacobi: workspace (%zu bytes needed)", stx_flow_jacobi_ws(n, h, w));
    return STX_E_WORKSPACE;
  }
  if (!single && (ws == (const void*)uv_in || ws == (void*)uv_out)) {
    set_error("stx_flow_jacobi: the workspace is uv_in or uv_out");
    return STX_E_INVALID;
  }
  const float a2 = alpha * alpha;
  const int per = fuse ? fuse : (h <= JT && w <= JT ? iters : JK);
  const int launches = cdiv(iters, per);
  const dim3 grid(cdiv(w, JT), cdiv(h, JT), n);
  const float* src = uv_in;
  for (int l = 0, left = iters; l < launches; ++l, left -= per) {
    // the last launch writes uv_out; the ones before it alternate so that it can
    float* dst = (launches - 1 - l) % 2 == 0 ? uv_out : (float*)ws;
    hipLaunchKernelGGL(flow_jacobi_kernel, grid, dim3(JB), 0, (hipStream_t)stream, coef, src, dst,
                       h, w, a2, left < per ? left : per);
    src = dst;
  }
  return check_launch("stx_flow_jacobi");
}

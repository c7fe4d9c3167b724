// Colour control of Gatys et al. 2017, "Controlling Perceptual Factors in Neural Style
// Transfer", section 5 (the reference project has no such feature): the two device
// passes that colour matching (5.2) and luminance-only transfer (5.1) need.
//
//   stx_color_stats   per image, the RGB mean and population covariance in fp64
//   stx_color_affine  out = clamp(base + M (x - base) + b), a 3x3 transform per pixel
//
// Stats: CS_BLOCKS blocks per image whatever its size; every thread keeps the 3 first and
// 6 second moments of its pixels in fp64 registers (fp64 VALU is full rate on gfx950; the
// pass reads 12 h w bytes per image and nothing else), a shuffle + LDS reduction in a fixed
// order gives one partial row per block, and a one-block finalize per image stages the rows
// in LDS, sums them in index order and forms cov = E[x x^T] - mu mu^T.  Image k's blocks read image k and
// write rows k * CS_BLOCKS ..: its result does not depend on the batch it sits in.
//
// Affine: one thread owns all three channels of its pixels, reads them (and base's) before
// it writes any, so out may alias x or base.  The arithmetic is an explicit fma chain.
#include "common.h"
#include "../../include/stx.h"

namespace stx {

constexpr int CB = 256;        // threads per block
constexpr int CS_BLOCKS = 128; // blocks per image (fixed: the summation order never changes)
constexpr int CS_MOM = 9;      // sum r g b, then rr rg rb gg gb bb

__device__ __forceinline__ void mom_add(double (&m)[CS_MOM], float fr, float fg, float fb) {
  const double r = fr, g = fg, b = fb;
  m[0] += r;
  m[1] += g;
  m[2] += b;
  m[3] = fma(r, r, m[3]);
  m[4] = fma(r, g, m[4]);
  m[5] = fma(r, b, m[5]);
  m[6] = fma(g, g, m[6]);
  m[7] = fma(g, b, m[7]);
  m[8] = fma(b, b, m[8]);
}

__global__ void __launch_bounds__(CB)
color_stats_partial_kernel(const float* __restrict__ x, long long hw, double* __restrict__ parts,
                           int vec) {
  const int k = blockIdx.y;
  const float* r = x + (long long)k * 3 * hw;
  const float* g = r + hw;
  const float* b = g + hw;
  double m[CS_MOM];
#pragma unroll
  for (int j = 0; j < CS_MOM; ++j) m[j] = 0.0;
  const long long stride = (long long)CS_BLOCKS * CB;
  const long long t0 = (long long)blockIdx.x * CB + threadIdx.x;
  if (vec) {  // hw % 4 == 0 and a 16-byte aligned x: every plane starts aligned
    const long long hw4 = hw >> 2;
#pragma unroll 2
    for (long long i = t0; i < hw4; i += stride) {
      const f32x4 vr = reinterpret_cast<const f32x4*>(r)[i];
      const f32x4 vg = reinterpret_cast<const f32x4*>(g)[i];
      const f32x4 vb = reinterpret_cast<const f32x4*>(b)[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) mom_add(m, vr[e], vg[e], vb[e]);
    }
  } else {
    for (long long i = t0; i < hw; i += stride) mom_add(m, r[i], g[i], b[i]);
  }
  __shared__ double red[CB / 64][CS_MOM];
  const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
#pragma unroll
  for (int j = 0; j < CS_MOM; ++j) {
    double v = m[j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (ln == 0) red[wv][j] = v;
  }
  __syncthreads();
  if (threadIdx.x < CS_MOM) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < CB / 64; ++i) s += red[i][threadIdx.x];
    parts[((long long)k * CS_BLOCKS + blockIdx.x) * CS_MOM + threadIdx.x] = s;
  }
}

__global__ void __launch_bounds__(CB)
color_stats_final_kernel(const double* __restrict__ parts, long long hw,
                         double* __restrict__ stats) {
  const int k = blockIdx.x, j = threadIdx.x;
  // the image's partial rows into LDS with every load in flight at once (a thread that
  // summed straight from global would wait out CS_BLOCKS dependent load latencies)
  __shared__ double rows[CS_BLOCKS * CS_MOM];
  __shared__ double mom[CS_MOM];
  const double* src = parts + (long long)k * CS_BLOCKS * CS_MOM;
  for (int i = j; i < CS_BLOCKS * CS_MOM; i += CB) rows[i] = src[i];
  __syncthreads();
  if (j < CS_MOM) {
    double s = 0.0;
#pragma unroll 16
    for (int i = 0; i < CS_BLOCKS; ++i) s += rows[i * CS_MOM + j];  // index order
    mom[j] = s / (double)hw;
  }
  __syncthreads();
  double* out = stats + (long long)k * CS_MOM;
  if (j < 3) {
    out[j] = mom[j];
  } else if (j < CS_MOM) {
    // upper triangle rr rg rb gg gb bb
    const int a = j < 6 ? 0 : (j < 8 ? 1 : 2);
    const int c = j < 6 ? j - 3 : (j < 8 ? j - 5 : 2);
    out[j] = mom[j] - mom[a] * mom[c];
  }
}

struct ColorAffine {
  float M[9], b[3], lo[3], hi[3];
};

template <bool BASE>
__device__ __forceinline__ void affine_px(const ColorAffine& A, int clamp, const float (&x)[3],
                                          const float (&bs)[3], float (&o)[3]) {
  float t[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) t[d] = BASE ? x[d] - bs[d] : x[d];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float v = fmaf(A.M[3 * c + 0], t[0], A.b[c]);
    v = fmaf(A.M[3 * c + 1], t[1], v);
    v = fmaf(A.M[3 * c + 2], t[2], v);
    if (BASE) v = bs[c] + v;
    if (clamp) v = fminf(fmaxf(v, A.lo[c]), A.hi[c]);
    o[c] = v;
  }
}

// x, base and out carry no __restrict__: out may be x or base
template <bool BASE>
__global__ void __launch_bounds__(CB)
color_affine_kernel(const float* x, const float* base, float* out, long long hw, ColorAffine A,
                    int clamp, int vec) {
  const long long off = (long long)blockIdx.y * 3 * hw;
  const float* xp = x + off;
  const float* bp = BASE ? base + off : nullptr;
  float* op = out + off;
  const long long stride = (long long)gridDim.x * CB;
  const long long t0 = (long long)blockIdx.x * CB + threadIdx.x;
  if (vec) {
    const long long hw4 = hw >> 2;
    for (long long i = t0; i < hw4; i += stride) {
      f32x4 vx[3], vb[3], vo[3];
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        vx[d] = reinterpret_cast<const f32x4*>(xp + d * hw)[i];
        if (BASE) vb[d] = reinterpret_cast<const f32x4*>(bp + d * hw)[i];
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float px[3] = {vx[0][e], vx[1][e], vx[2][e]};
        const float pb[3] = {BASE ? vb[0][e] : 0.f, BASE ? vb[1][e] : 0.f, BASE ? vb[2][e] : 0.f};
        float po[3];
        affine_px<BASE>(A, clamp, px, pb, po);
        vo[0][e] = po[0];
        vo[1][e] = po[1];
        vo[2][e] = po[2];
      }
#pragma unroll
      for (int d = 0; d < 3; ++d) reinterpret_cast<f32x4*>(op + d * hw)[i] = vo[d];
    }
  } else {
    for (long long i = t0; i < hw; i += stride) {
      const float px[3] = {xp[i], xp[hw + i], xp[2 * hw + i]};
      const float pb[3] = {BASE ? bp[i] : 0.f, BASE ? bp[hw + i] : 0.f,
                           BASE ? bp[2 * hw + i] : 0.f};
      float po[3];
      affine_px<BASE>(A, clamp, px, pb, po);
      op[i] = po[0];
      op[hw + i] = po[1];
      op[2 * hw + i] = po[2];
    }
  }
}

static bool color_aligned16(const void* p) { return !(reinterpret_cast<uintptr_t>(p) & 15); }

// n, h, w of an [n][3][h][w] batch: n images as grid.y, h w pixels per plane
static bool color_dims_ok(int n, int h, int w) {
  return n > 0 && n <= 65535 && h > 0 && w > 0 && (long long)h * w <= (1ll << 40);
}

}  // namespace stx

using namespace stx;

extern "C" size_t stx_color_stats_ws(int n, int h, int w) {
  if (!color_dims_ok(n, h, w)) return 0;
  return (size_t)n * CS_BLOCKS * CS_MOM * sizeof(double);
}

extern "C" int stx_color_stats(const float* x, double* stats, int n, int h, int w, void* ws,
                               size_t ws_bytes, void* stream) {
  if (!x || !stats) {
    set_error("stx_color_stats: x and stats are required");
    return STX_E_INVALID;
  }
  if (!color_dims_ok(n, h, w)) {
    set_error("stx_color_stats: unsupported dims n=%d h=%d w=%d", n, h, w);
    return STX_E_INVALID;
  }
  if (!ws || ws_bytes < stx_color_stats_ws(n, h, w) || !color_aligned16(ws)) {
    set_error("stx_color_stats: workspace of %zu bytes (16-byte aligned) needed, got %zu",
              stx_color_stats_ws(n, h, w), ws ? ws_bytes : (size_t)0);
    return STX_E_INVALID;
  }
  const long long hw = (long long)h * w;
  const int vec = (hw % 4 == 0) && color_aligned16(x);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(color_stats_partial_kernel, dim3(CS_BLOCKS, n), dim3(CB), 0, st, x, hw,
                     (double*)ws, vec);
  hipLaunchKernelGGL(color_stats_final_kernel, dim3(n), dim3(CB), 0, st, (const double*)ws, hw,
                     stats);
  return check_launch("stx_color_stats");
}

extern "C" int stx_color_affine(const float* x, const float* base, float* out, int n, int h, int w,
                                const float* M, const float* b, const float* lo, const float* hi,
                                void* stream) {
  if (!x || !out || !M) {
    set_error("stx_color_affine: x, out and M are required");
    return STX_E_INVALID;
  }
  if (!color_dims_ok(n, h, w)) {
    set_error("stx_color_affine: unsupported dims n=%d h=%d w=%d", n, h, w);
    return STX_E_INVALID;
  }
  if ((lo == nullptr) != (hi == nullptr)) {
    set_error("stx_color_affine: lo and hi come together (both NULL: no clamp)");
    return STX_E_INVALID;
  }
  ColorAffine A;
  for (int i = 0; i < 9; ++i) A.M[i] = M[i];
  for (int c = 0; c < 3; ++c) {
    A.b[c] = b ? b[c] : 0.f;
    A.lo[c] = lo ? lo[c] : 0.f;
    A.hi[c] = hi ? hi[c] : 0.f;
  }
  const int clamp = lo != nullptr;
  const long long hw = (long long)h * w;
  const int vec = (hw % 4 == 0) && color_aligned16(x) && color_aligned16(out) &&
                  (!base || color_aligned16(base));
  const long long work = vec ? hw >> 2 : hw;
  const int gx = (int)std::min<long long>((work + CB - 1) / CB, 1024);
  hipStream_t st = (hipStream_t)stream;
  if (base)
    hipLaunchKernelGGL(color_affine_kernel<true>, dim3(gx, n), dim3(CB), 0, st, x, base, out, hw,
                       A, clamp, vec);
  else
    hipLaunchKernelGGL(color_affine_kernel<false>, dim3(gx, n), dim3(CB), 0, st, x, base, out, hw,
                       A, clamp, vec);
  return check_launch("stx_color_affine");
}

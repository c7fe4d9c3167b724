// fp32 separable resampling for the scale control of Gatys et al. 2017, "Controlling
// Perceptual Factors in Neural Style Transfer", section 6 (the reference project has no
// such feature): every pyramid level needs the content, the style, the guides and the
// running image at a new size, on the device.
//
//   stx_resample_plan  host: per output index the first tap, the tap count and k weights
//   stx_resample2d     [nc][hi][wi] -> [nc][ho][wo]: a horizontal pass into the workspace,
//                      then a vertical pass
//
// The tables are those of an antialiased triangle / Keys cubic (a = -0.5) resize with
// half-pixel centres: per axis scale = in / out, s = max(scale, 1), support = radius s,
// centre c = scale (i + 0.5), taps [max(0, int(c - support + 0.5)), min(in, int(c + support
// + 0.5))), weight f((j - c + 0.5) / s) divided by the taps' sum; fp64 on the host, rounded
// to fp32 once.
//
// Both passes: one thread per output (per four outputs along w on the 16-byte path), an
// explicit fmaf chain over its taps in ascending order starting from w0 x0 -- an output's
// bits depend on its own taps alone, not on the grid, the plane count or the path taken.
// The horizontal pass gathers its taps straight from cache (neighbouring outputs share
// most of them; no LDS stage); the vertical pass reads and writes whole rows, lanes along w.
// An axis whose size does not change is skipped; an identity resize is a device copy.
#include <cmath>
#include <vector>

#include "common.h"
#include "../../include/stx.h"

namespace stx {

constexpr int RB = 256;           // threads per block
constexpr int RS_GRID_X = 2048;   // blocks per plane at most (the rest: grid stride)
constexpr int RS_MAX_SIDE = 4096; // per axis, so a plane holds at most 2^24 elements
constexpr int RS_MAX_NC = 65535;  // planes ride grid.y

// Horizontal: y[p][r][xo] = sum_j w[xo][j] x[p][r][first[xo] + j]
template <int V>
__global__ void __launch_bounds__(RB)
resample_h_kernel(const float* __restrict__ x, float* __restrict__ y, int rows, int wi, int wo,
                  const int* __restrict__ first, const int* __restrict__ count,
                  const float* __restrict__ wt, int k) {
  const float* xp = x + (size_t)blockIdx.y * rows * wi;
  float* yp = y + (size_t)blockIdx.y * rows * wo;
  const int wq = wo / V;
  const int work = rows * wq;  // <= 2^24
  for (int i = blockIdx.x * RB + threadIdx.x; i < work; i += gridDim.x * RB) {
    const int r = i / wq, xo = (i - r * wq) * V;
    const float* row = xp + (size_t)r * wi;
    float o[V];
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const int f = first[xo + e];
      // (tables are the caller's: never read past the row whatever they say)
      const int n = f < 0 ? 0 : min(min(count[xo + e], k), wi - f);
      const float* wk = wt + (size_t)(xo + e) * k;
      float acc = 0.f;
      if (n > 0) {
        acc = wk[0] * row[f];
        int j = 1;
        for (; j + 4 <= n; j += 4) {  // four taps' loads in flight, the chain in tap order
          const float w0 = wk[j], w1 = wk[j + 1], w2 = wk[j + 2], w3 = wk[j + 3];
          const float a0 = row[f + j], a1 = row[f + j + 1], a2 = row[f + j + 2],
                      a3 = row[f + j + 3];
          acc = fmaf(w3, a3, fmaf(w2, a2, fmaf(w1, a1, fmaf(w0, a0, acc))));
        }
        for (; j < n; ++j) acc = fmaf(wk[j], row[f + j], acc);
      }
      o[e] = acc;
    }
    float* dst = yp + (size_t)r * wo + xo;
    if (V == 4) {
      f32x4 v = {o[0], o[1], o[2], o[3]};
      *reinterpret_cast<f32x4*>(dst) = v;
    } else {
      dst[0] = o[0];
    }
  }
}

// Vertical: y[p][yo][c] = sum_j w[yo][j] x[p][first[yo] + j][c], lanes along c
template <int V>
__global__ void __launch_bounds__(RB)
resample_v_kernel(const float* __restrict__ x, float* __restrict__ y, int hi, int ho, int w,
                  const int* __restrict__ first, const int* __restrict__ count,
                  const float* __restrict__ wt, int k) {
  const float* xp = x + (size_t)blockIdx.y * hi * w;
  float* yp = y + (size_t)blockIdx.y * ho * w;
  const int wq = w / V;
  const int work = ho * wq;  // <= 2^24
  for (int i = blockIdx.x * RB + threadIdx.x; i < work; i += gridDim.x * RB) {
    const int yo = i / wq, c = (i - yo * wq) * V;
    const int f = first[yo];
    const int n = f < 0 ? 0 : min(min(count[yo], k), hi - f);
    const float* wk = wt + (size_t)yo * k;
    const float* col = xp + (size_t)f * w + c;
    float* dst = yp + (size_t)yo * w + c;
    if (V == 4) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      if (n > 0) {
        const f32x4 v0 = *reinterpret_cast<const f32x4*>(col);
        const float w0 = wk[0];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = w0 * v0[e];
        int j = 1;
        for (; j + 4 <= n; j += 4) {  // four rows' loads in flight, the chain in tap order
          f32x4 v[4];
          float wj[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            v[q] = *reinterpret_cast<const f32x4*>(col + (size_t)(j + q) * w);
            wj[q] = wk[j + q];
          }
#pragma unroll
          for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = fmaf(wj[q], v[q][e], acc[e]);
        }
        for (; j < n; ++j) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(col + (size_t)j * w);
          const float wj = wk[j];
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[e] = fmaf(wj, v[e], acc[e]);
        }
      }
      *reinterpret_cast<f32x4*>(dst) = acc;
    } else {
      float acc = 0.f;
      if (n > 0) {
        acc = wk[0] * col[0];
        int j = 1;
        for (; j + 4 <= n; j += 4) {
          const float w0 = wk[j], w1 = wk[j + 1], w2 = wk[j + 2], w3 = wk[j + 3];
          const float a0 = col[(size_t)j * w], a1 = col[(size_t)(j + 1) * w],
                      a2 = col[(size_t)(j + 2) * w], a3 = col[(size_t)(j + 3) * w];
          acc = fmaf(w3, a3, fmaf(w2, a2, fmaf(w1, a1, fmaf(w0, a0, acc))));
        }
        for (; j < n; ++j) acc = fmaf(wk[j], col[(size_t)j * w], acc);
      }
      dst[0] = acc;
    }
  }
}

static bool rs_aligned16(const void* p) { return !(reinterpret_cast<uintptr_t>(p) & 15); }

static bool rs_dims_ok(int nc, int hi, int wi, int ho, int wo) {
  return nc > 0 && nc <= RS_MAX_NC && hi > 0 && wi > 0 && ho > 0 && wo > 0 &&
         hi <= RS_MAX_SIDE && wi <= RS_MAX_SIDE && ho <= RS_MAX_SIDE && wo <= RS_MAX_SIDE;
}

static double rs_filter(int filter, double t) {
  t = std::fabs(t);
  if (filter == STX_FILTER_TRIANGLE) return t < 1.0 ? 1.0 - t : 0.0;
  const double a = -0.5;  // Keys
  if (t < 1.0) return ((a + 2.0) * t - (a + 3.0)) * t * t + 1.0;
  if (t < 2.0) return ((a * t - 5.0 * a) * t + 8.0 * a) * t - 4.0 * a;
  return 0.0;
}

static int rs_grid_x(int work) { return std::min(cdiv(work, RB), RS_GRID_X); }

}  // namespace stx

using namespace stx;

extern "C" int stx_resample_plan(int in_size, int out_size, int filter, int* first, int* count,
                                 float* w, int k) {
  if (in_size <= 0 || out_size <= 0) {
    set_error("stx_resample_plan: sizes must be positive (in=%d out=%d)", in_size, out_size);
    return -STX_E_INVALID;
  }
  if (filter != STX_FILTER_TRIANGLE && filter != STX_FILTER_CUBIC) {
    set_error("stx_resample_plan: unknown filter %d", filter);
    return -STX_E_INVALID;
  }
  const double scale = (double)in_size / out_size;
  const double s = scale < 1.0 ? 1.0 : scale;
  const double support = (filter == STX_FILTER_CUBIC ? 2.0 : 1.0) * s;
  auto taps = [&](int i, int& lo) {
    const double c = scale * (i + 0.5);
    lo = std::max(0, (int)(c - support + 0.5));
    return std::min(in_size, (int)(c + support + 0.5)) - lo;
  };
  int need = 0, lo;
  for (int i = 0; i < out_size; ++i) need = std::max(need, taps(i, lo));
  if (!first && !count && !w) return need;  // size query
  if (!first || !count || !w) {
    set_error("stx_resample_plan: first, count and w come together (all NULL: size query)");
    return -STX_E_INVALID;
  }
  if (k < need) {
    set_error("stx_resample_plan: %d weights per output needed, room for %d", need, k);
    return -STX_E_INVALID;
  }
  std::vector<double> v(need);
  for (int i = 0; i < out_size; ++i) {
    const int n = taps(i, lo);
    const double c = scale * (i + 0.5);
    double sum = 0.0;
    for (int j = 0; j < n; ++j) {
      v[j] = rs_filter(filter, (lo + j - c + 0.5) / s);
      sum += v[j];
    }
    for (int j = 0; j < k; ++j)
      w[(size_t)i * k + j] = j < n ? (float)(sum != 0.0 ? v[j] / sum : v[j]) : 0.f;
    first[i] = lo;
    count[i] = n;
  }
  return need;
}

extern "C" size_t stx_resample2d_ws(int nc, int hi, int wi, int ho, int wo) {
  if (!rs_dims_ok(nc, hi, wi, ho, wo) || wi == wo || hi == ho) return 0;
  return (size_t)nc * hi * wo * sizeof(float);  // the horizontal pass's output
}

extern "C" int stx_resample2d(const float* x, float* y, int nc, int hi, int wi, int ho, int wo,
                              const int* xfirst, const int* xcount, const float* xw, int xk,
                              const int* yfirst, const int* ycount, const float* yw, int yk,
                              void* ws, size_t ws_bytes, void* stream) {
  if (!x || !y) {
    set_error("stx_resample2d: x and y are required");
    return STX_E_INVALID;
  }
  if (!rs_dims_ok(nc, hi, wi, ho, wo)) {
    set_error("stx_resample2d: unsupported dims nc=%d %dx%d -> %dx%d (nc <= %d, sides <= %d)", nc,
              hi, wi, ho, wo, RS_MAX_NC, RS_MAX_SIDE);
    return STX_E_INVALID;
  }
  const size_t in_bytes = (size_t)nc * hi * wi * sizeof(float);
  const size_t out_bytes = (size_t)nc * ho * wo * sizeof(float);
  const char* xb = reinterpret_cast<const char*>(x);
  const char* yb = reinterpret_cast<const char*>(y);
  if (xb < yb + out_bytes && yb < xb + in_bytes) {
    set_error("stx_resample2d: y must not alias x");
    return STX_E_INVALID;
  }
  const bool do_h = wi != wo, do_v = hi != ho;
  if (do_h && (!xfirst || !xcount || !xw || xk <= 0)) {
    set_error("stx_resample2d: the x tables (stx_resample_plan of %d -> %d) are required", wi, wo);
    return STX_E_INVALID;
  }
  if (do_v && (!yfirst || !ycount || !yw || yk <= 0)) {
    set_error("stx_resample2d: the y tables (stx_resample_plan of %d -> %d) are required", hi, ho);
    return STX_E_INVALID;
  }
  const size_t need = stx_resample2d_ws(nc, hi, wi, ho, wo);
  if (need && (!ws || ws_bytes < need || !rs_aligned16(ws))) {
    set_error("stx_resample2d: workspace of %zu bytes (16-byte aligned) needed, got %zu", need,
              ws ? ws_bytes : (size_t)0);
    return STX_E_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  if (!do_h && !do_v) {  // identity: an exact copy
    hipError_t e = hipMemcpyAsync(y, x, in_bytes, hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) {
      set_error("stx_resample2d: copy: %s", hipGetErrorString(e));
      return (int)e;
    }
    return STX_OK;
  }
  const float* vin = x;
  if (do_h) {
    float* hout = do_v ? (float*)ws : y;
    const bool vec = wo % 4 == 0 && rs_aligned16(hout);
    const dim3 grid(rs_grid_x(hi * (vec ? wo / 4 : wo)), nc);
    if (vec)
      hipLaunchKernelGGL(resample_h_kernel<4>, grid, dim3(RB), 0, st, x, hout, hi, wi, wo, xfirst,
                         xcount, xw, xk);
    else
      hipLaunchKernelGGL(resample_h_kernel<1>, grid, dim3(RB), 0, st, x, hout, hi, wi, wo, xfirst,
                         xcount, xw, xk);
    vin = hout;
  }
  if (do_v) {
    const bool vec = wo % 4 == 0 && rs_aligned16(vin) && rs_aligned16(y);
    const dim3 grid(rs_grid_x(ho * (vec ? wo / 4 : wo)), nc);
    if (vec)
      hipLaunchKernelGGL(resample_v_kernel<4>, grid, dim3(RB), 0, st, vin, y, hi, ho, wo, yfirst,
                         ycount, yw, yk);
    else
      hipLaunchKernelGGL(resample_v_kernel<1>, grid, dim3(RB), 0, st, vin, y, hi, ho, wo, yfirst,
                         ycount, yw, yk);
  }
  return check_launch("stx_resample2d");
}

// Temporal consistency of optimisation-based video transfer (Ruder, Dosovitskiy & Brox 2016,
// "Artistic Style Transfer for Videos"): the backward warp of the previous result along
// the optical flow, the per-pixel consistency mask (disocclusions and motion boundaries,
// their eq. 5 and 6) and the masked squared error that ties a frame to that warp.
//
// Flows are [n][2][h][w]: channel 0 the column displacement dx, channel 1 the row
// displacement dy.  Pixel (i, j) samples its source at y = i + dy, x = j + dx (fp32, one
// rounding each); it is valid when 0 <= y <= h-1 and 0 <= x <= w-1 as computed, so a NaN
// coordinate is invalid and an invalid pixel reads no tap.
//
// All three are HBM / L2 streaming kernels: flow_warp moves 8 B of flow + 8 c B of taps
// (L2 hits for a smooth flow: 4 c B from HBM) + 4 c B out per pixel, flow_consistency 24 B
// in (bwd and its four neighbours from L2) + 4 B out, masked_mse 8 B + 4/c B in per
// element and 8 B more with an accumulated gradient.  flow_compose is the consistency test
// and the warp of up to four earlier frames in one pass (the long-term loss's set-up): a
// pixel settled at the first offset moves 16 B of flows + 4 c B of taps in, 8 c + 5 B out.
#include "common.h"
#include "../../include/stx.h"

#include <climits>

namespace stx {

constexpr int FB = 256;      // threads per block
constexpr int FPARTS = 512;  // partial blocks (fixed: the reduction order never changes)

// The four taps of one pixel: computed once, reused over the channels.
struct Taps {
  int o00, o01, o10, o11;  // offsets in a plane
  float w00, w01, w10, w11;
};

// y, x: valid coordinates (0 <= y <= h-1, 0 <= x <= w-1; h, w >= 2).  fy = y - y0 is exact
// (Sterbenz); 1 - fy, 1 - fx and each weight's product round once: three roundings at most
// on a weight.
__device__ __forceinline__ Taps make_taps(float y, float x, int h, int w) {
  const int y0 = min((int)floorf(y), h - 2), x0 = min((int)floorf(x), w - 2);
  const float fy = y - (float)y0, fx = x - (float)x0;
  const float gy = 1.f - fy, gx = 1.f - fx;
  Taps t;
  t.o00 = y0 * w + x0;
  t.o01 = t.o00 + 1;
  t.o10 = t.o00 + w;
  t.o11 = t.o10 + 1;
  t.w00 = gy * gx;
  t.w01 = gy * fx;
  t.w10 = fy * gx;
  t.w11 = fy * fx;
  return t;
}

// w00 a00 + w01 a01 + w10 a10 + w11 a11 as one product and three fmaf: four roundings.
__device__ __forceinline__ float blend(const Taps& t, const float* __restrict__ p) {
  float v = t.w00 * p[t.o00];
  v = fmaf(t.w01, p[t.o01], v);
  v = fmaf(t.w10, p[t.o10], v);
  return fmaf(t.w11, p[t.o11], v);
}

__device__ __forceinline__ bool in_range(float y, float x, int h, int w) {
  return y >= 0.f && y <= (float)(h - 1) && x >= 0.f && x <= (float)(w - 1);
}

// The source of pixel p = (i, j) along the flow f [2][hw]: y = i + dy, x = j + dx.  True and
// the taps in t when it lies in the image; false (t untouched, no tap read) otherwise.
__device__ __forceinline__ bool warp_taps(const float* __restrict__ f, int hw, int p, int i,
                                          int j, int h, int w, Taps& t) {
  const float y = (float)i + f[hw + p], x = (float)j + f[p];
  const bool ok = in_range(y, x, h, w);
  if (ok) t = make_taps(y, x, h, w);
  return ok;
}

__global__ void __launch_bounds__(FB)
flow_warp_kernel(const float* __restrict__ src, const float* __restrict__ flow,
                 const float* __restrict__ fill, float* __restrict__ out,
                 float* __restrict__ valid, int c, int h, int w) {
  const int hw = h * w;
  const int p = blockIdx.x * FB + threadIdx.x;
  if (p >= hw) return;
  const size_t b = blockIdx.y;
  const int i = p / w, j = p - i * w;
  Taps t;
  const bool ok = warp_taps(flow + b * 2 * hw, hw, p, i, j, h, w, t);
  if (valid) valid[b * hw + p] = ok ? 1.f : 0.f;
  const size_t base = b * c * hw;
  if (ok) {
    for (int k = 0; k < c; ++k) out[base + (size_t)k * hw + p] = blend(t, src + base + (size_t)k * hw);
  } else {
    for (int k = 0; k < c; ++k) {
      const size_t o = base + (size_t)k * hw + p;
      out[o] = fill ? fill[o] : 0.f;
    }
  }
}

// Central difference halved in the interior, one-sided and unhalved in the first and last
// row / column (k: the pixel's index along the axis, n: the axis' size, s: its stride).
__device__ __forceinline__ float diff(const float* __restrict__ u, int p, int k, int n, int s) {
  if (k == 0) return u[p + s] - u[p];
  if (k == n - 1) return u[p] - u[p - s];
  return (u[p + s] - u[p - s]) * 0.5f;
}

// The consistency predicate at pixel p = (i, j) of one sample (fu: fwd, bu: bwd, each
// [2][hw]): valid and not occluded and not boundary.  t receives the taps of the pixel's
// source along bwd whenever that source lies in the image (they are flow_warp's).
__device__ __forceinline__ bool consistent_at(const float* __restrict__ fu,
                                              const float* __restrict__ bu, int hw, int p, int i,
                                              int j, int h, int w, Taps& t) {
  const float* bv = bu + hw;
  const float u = bu[p], v = bv[p];
  bool ok = warp_taps(bu, hw, p, i, j, h, w, t);
  if (ok) {
    // every comparison is false on a NaN operand: the test then does not fire
    const float wu = blend(t, fu), wv = blend(t, fu + hw);
    const float su = wu + u, sv = wv + v;
    const float m_b = u * u + v * v;
    const bool occluded = su * su + sv * sv > 0.01f * ((wu * wu + wv * wv) + m_b) + 0.5f;
    const float ux = diff(bu, p, j, w, 1), uy = diff(bu, p, i, h, w);
    const float vx = diff(bv, p, j, w, 1), vy = diff(bv, p, i, h, w);
    const bool boundary = (ux * ux + uy * uy) + (vx * vx + vy * vy) > 0.01f * m_b + 0.002f;
    ok = !occluded && !boundary;
  }
  return ok;
}

__global__ void __launch_bounds__(FB)
flow_consistency_kernel(const float* __restrict__ fwd, const float* __restrict__ bwd,
                        float* __restrict__ cmask, int h, int w) {
  const int hw = h * w;
  const int p = blockIdx.x * FB + threadIdx.x;
  if (p >= hw) return;
  const size_t b = blockIdx.y;
  const int i = p / w, j = p - i * w;
  Taps t;
  const bool ok = consistent_at(fwd + b * 2 * hw, bwd + b * 2 * hw, hw, p, i, j, h, w, t);
  cmask[b * hw + p] = ok ? 1.f : 0.f;
}

// Long-term consistency (Ruder et al. eq. 9, 10 with 0/1 masks): per pixel the nearest offset
// q whose predicate holds supplies the reference.  The table of pointers travels in the
// kernel's arguments; the loop is unrolled so that every index into it is a constant.
constexpr int FCOMPOSE_MAX = 4;
struct ComposeSrc {
  const float* prev[FCOMPOSE_MAX];
  const float* fwd[FCOMPOSE_MAX];
  const float* bwd[FCOMPOSE_MAX];
};

__global__ void __launch_bounds__(FB)
flow_compose_kernel(ComposeSrc a, int count, const float* __restrict__ fill,
                    float* __restrict__ ref, float* __restrict__ cmask, float* __restrict__ init,
                    unsigned char* __restrict__ which, int c, int h, int w) {
  const int hw = h * w;
  const int p = blockIdx.x * FB + threadIdx.x;
  if (p >= hw) return;
  const size_t b = blockIdx.y;
  const int i = p / w, j = p - i * w;
  const size_t fb = b * 2 * hw, base = b * c * hw;
  Taps t;
  const float* src = nullptr;
  int sel = -1;
#pragma unroll
  for (int q = 0; q < FCOMPOSE_MAX; ++q) {
    // a settled pixel looks at no later offset: no flow and no tap of it is read
    if (q < count && sel < 0 && consistent_at(a.fwd[q] + fb, a.bwd[q] + fb, hw, p, i, j, h, w, t)) {
      sel = q;
      src = a.prev[q];
    }
  }
  cmask[b * hw + p] = sel >= 0 ? 1.f : 0.f;
  if (which) which[b * hw + p] = sel >= 0 ? (unsigned char)sel : (unsigned char)255;
  if (sel >= 0) {
    for (int k = 0; k < c; ++k) {
      const size_t o = base + (size_t)k * hw + p;
      const float v = blend(t, src + base + (size_t)k * hw);
      ref[o] = v;
      if (init) init[o] = v;
    }
  } else {
    // no consistent source: the reference is unused (+0); the start is the nearest
    // frame's warp where that lies in the image, the frame itself elsewhere
    const bool ok = init && warp_taps(a.bwd[0] + fb, hw, p, i, j, h, w, t);
    for (int k = 0; k < c; ++k) {
      const size_t o = base + (size_t)k * hw + p;
      ref[o] = 0.f;
      if (init) init[o] = ok ? blend(t, a.prev[0] + base + (size_t)k * hw) : fill[o];
    }
  }
}

// One streaming pass: sum of mask-selected (x - ref)^2 per block, and the gradient written
// or accumulated.  A pixel whose mask is 0 contributes nothing and, when accumulating,
// its gradient is not rewritten (bit-unchanged, a -0 included).  total < 2^31.
__global__ void __launch_bounds__(FB)
masked_mse_partial_kernel(const float* __restrict__ x, const float* __restrict__ ref,
                          const float* __restrict__ mask, unsigned c, unsigned hw,
                          unsigned total, float gs, float* __restrict__ grad, int accumulate,
                          float* __restrict__ parts, int vec) {
  float s = 0.f;
  const unsigned stride = FPARTS * FB;
  const unsigned t0 = blockIdx.x * FB + threadIdx.x;
  if (vec) {  // hw % 4 == 0: a float4 lies inside one plane
    const unsigned n4 = total >> 2, hw4 = hw >> 2;
    for (unsigned i = t0; i < n4; i += stride) {
      const unsigned plane = i / hw4, q = i - plane * hw4;
      const f32x4 m = reinterpret_cast<const f32x4*>(mask)[(size_t)(plane / c) * hw4 + q];
      const f32x4 xv = reinterpret_cast<const f32x4*>(x)[i];
      const f32x4 rv = reinterpret_cast<const f32x4*>(ref)[i];
      f32x4 g = {0.f, 0.f, 0.f, 0.f};
      if (grad && accumulate) g = reinterpret_cast<f32x4*>(grad)[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float d = xv[e] - rv[e];
        const bool on = m[e] != 0.f;
        s = on ? fmaf(d, d, s) : s;
        g[e] = on ? (accumulate ? g[e] + gs * d : gs * d) : g[e];
      }
      if (grad) reinterpret_cast<f32x4*>(grad)[i] = g;
    }
  } else {
    for (unsigned i = t0; i < total; i += stride) {
      const unsigned plane = i / hw, q = i - plane * hw;
      const bool on = mask[(size_t)(plane / c) * hw + q] != 0.f;
      const float d = x[i] - ref[i];
      s = on ? fmaf(d, d, s) : s;
      if (grad) {
        if (accumulate) {
          if (on) grad[i] += gs * d;
        } else {
          grad[i] = on ? gs * d : 0.f;
        }
      }
    }
  }
  __shared__ float red[FB / 64];
  s = block_sum<FB>(s, red);
  if (threadIdx.x == 0) parts[blockIdx.x] = s;
}

__global__ void __launch_bounds__(FB)
masked_mse_final_kernel(const float* __restrict__ parts, double scale, float* __restrict__ out,
                        float* __restrict__ add_to) {
  float s = 0.f;
  for (int i = threadIdx.x; i < FPARTS; i += FB) s += parts[i];  // fixed assignment and order
  __shared__ float red[FB / 64];
  s = block_sum<FB>(s, red);
  if (threadIdx.x == 0) {
    const float l = (float)((double)s * scale);
    out[0] = l;
    if (add_to) *add_to += l;
  }
}

static bool aligned16(const void* p) { return !(reinterpret_cast<uintptr_t>(p) & 15); }

// n, h, w of a flow-shaped problem: h, w >= 2, h w <= INT_MAX, n within a grid's y extent
static bool flow_dims_ok(int n, int h, int w) {
  return n >= 1 && n <= 65535 && h >= 2 && w >= 2 && (long long)h * w <= INT_MAX;
}

}  // namespace stx

using namespace stx;

extern "C" int stx_flow_warp(const float* src, const float* flow, const float* fill, float* out,
                             float* valid, int n, int c, int h, int w, void* stream) {
  if (!src || !flow || !out || out == src || c < 1 || !flow_dims_ok(n, h, w)) {
    set_error("stx_flow_warp: invalid arguments (n %d c %d h %d w %d; h, w >= 2, out != src)",
              n, c, h, w);
    return STX_E_INVALID;
  }
  hipLaunchKernelGGL(flow_warp_kernel, dim3(cdiv(h * w, FB), n), dim3(FB), 0, (hipStream_t)stream,
                     src, flow, fill, out, valid, c, h, w);
  return check_launch("stx_flow_warp");
}

extern "C" int stx_flow_consistency(const float* fwd, const float* bwd, float* cmask, int n,
                                    int h, int w, void* stream) {
  if (!fwd || !bwd || !cmask || !flow_dims_ok(n, h, w)) {
    set_error("stx_flow_consistency: invalid arguments (n %d h %d w %d; h, w >= 2)", n, h, w);
    return STX_E_INVALID;
  }
  hipLaunchKernelGGL(flow_consistency_kernel, dim3(cdiv(h * w, FB), n), dim3(FB), 0,
                     (hipStream_t)stream, fwd, bwd, cmask, h, w);
  return check_launch("stx_flow_consistency");
}

extern "C" int stx_flow_compose(const float* const* prev, const float* const* fwd,
                                const float* const* bwd, int count, const float* fill,
                                float* ref, float* cmask, float* init, unsigned char* which,
                                int n, int c, int h, int w, void* stream) {
  bool ok = prev && fwd && bwd && count >= 1 && count <= FCOMPOSE_MAX && fill && ref && cmask &&
            c >= 1 && flow_dims_ok(n, h, w) && ref != cmask && ref != init && cmask != init &&
            ref != fill && init != fill && cmask != fill;
  ComposeSrc a = {};
  for (int q = 0; ok && q < count; ++q) {
    a.prev[q] = prev[q];
    a.fwd[q] = fwd[q];
    a.bwd[q] = bwd[q];
    for (const float* in : {prev[q], fwd[q], bwd[q]})
      ok = ok && in && in != ref && in != cmask && in != init;
  }
  if (!ok) {
    set_error("stx_flow_compose: invalid arguments (count %d n %d c %d h %d w %d; 1 <= count <= "
              "%d, no null entry, fill given, h, w >= 2, outputs apart from the inputs)",
              count, n, c, h, w, FCOMPOSE_MAX);
    return STX_E_INVALID;
  }
  hipLaunchKernelGGL(flow_compose_kernel, dim3(cdiv(h * w, FB), n), dim3(FB), 0,
                     (hipStream_t)stream, a, count, fill, ref, cmask, init, which, c, h, w);
  return check_launch("stx_flow_compose");
}

extern "C" size_t stx_masked_mse_ws(void) { return FPARTS * sizeof(float); }

extern "C" int stx_masked_mse(const float* x, const float* ref, const float* mask, int n, int c,
                              int hw, float weight, float* out, float* add_to, float* grad,
                              int accumulate, void* ws, size_t ws_bytes, void* stream) {
  const long long total = (long long)n * c * hw;
  if (!x || !ref || !mask || !out || n < 1 || c < 1 || hw < 1 || total > INT_MAX) {
    set_error("stx_masked_mse: invalid arguments (n %d c %d hw %d; n c hw < 2^31)", n, c, hw);
    return STX_E_INVALID;
  }
  if (!ws || ws_bytes < stx_masked_mse_ws()) {
    set_error("stx_masked_mse: workspace");
    return STX_E_WORKSPACE;
  }
  // views at odd offsets and planes of hw % 4 != 0 take the scalar loop: the same result
  // contract, no alignment contract on the caller
  const int vec = hw % 4 == 0 && aligned16(x) && aligned16(ref) && aligned16(mask) &&
                  (!grad || aligned16(grad));
  const double inv = (double)weight / (double)total;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(masked_mse_partial_kernel, dim3(FPARTS), dim3(FB), 0, st, x, ref, mask,
                     (unsigned)c, (unsigned)hw, (unsigned)total, (float)(2.0 * inv), grad,
                     accumulate, (float*)ws, vec);
  hipLaunchKernelGGL(masked_mse_final_kernel, dim3(1), dim3(FB), 0, st, (const float*)ws, inv,
                     out, add_to);
  return check_launch("stx_masked_mse");
}

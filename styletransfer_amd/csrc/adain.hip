// Adaptive instance normalisation (Huang & Belongie 2017, "Arbitrary Style Transfer in
// Real-time with Adaptive Instance Normalization") for gfx950: per-plane channel
// statistics, the AdaIN transform with style blending and strength, and the mean/std
// style loss with its backward.  No reference counterpart (include/stx.h states the
// contract; tests/adain_ref.py restates it in fp64).
//
// One block per (n, c) plane.  mean = sum x / hw, then the squared deviations about that
// computed mean (two passes inside the block, never sum x^2 - mean^2), unbiased variance,
// std = sqrt(var + eps).  Every entry point that forms statistics does it through
// plane_stats_reg / plane_stats_loop under one selection (plane_variant), so the same
// plane has the same mean / std bits whichever entry point computed them.
//
// Variants, by plane size (hw % 4 == 0 and a 16-byte aligned x for the register ones):
//   hw <= 4096   256 threads x 4 float4     (relu4_1 at 256^2 and 512^2: 1024, 4096)
//   hw <= 16384  512 threads x 8 float4     (relu2_1 at 256^2)
//   hw <= 65536  1024 threads x 16 float4   (relu1_1 at 256^2)
//   otherwise    the loop kernel, 256 threads below 16384 floats and 1024 from there
//                (float4 trips where aligned, else scalar): the plane is re-read from L2
// A register variant reads the plane once; AdaIN writes y from the registers.  stx_adain on
// planes of up to 4096 floats walks four planes per block from 512 blocks (2048 planes),
// loading the next plane before this one's reductions and stores (plane_reg_kernel).
#include "common.h"
#include "conv_epi.h"
#include "../../include/stx.h"

#include <climits>

namespace stx {
namespace {

template <int NT>
__device__ __forceinline__ float bsum(float v, float* red) {
  v = wave_sum(v);
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  __syncthreads();
  if (l == 0) red[w] = v;
  __syncthreads();
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NT / 64; ++i) s += red[i];
  return s;
}

// max of IEEE bit patterns of |.| over the block (NaN sorts above inf), one atomic per block
template <int NT>
__device__ __forceinline__ void bmax_to(float* group, uint32_t mu, float* red, int bid) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mu = max(mu, (uint32_t)__shfl_xor((int)mu, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = __uint_as_float(mu);
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t r = 0u;
#pragma unroll
    for (int i = 0; i < NT / 64; ++i) r = max(r, __float_as_uint(red[i]));
    atomic_max_abs(group + (bid & (STX_AMAX_SLOTS - 1)), __uint_as_float(r));
  }
}

// the fmas written out, as instnorm.hip's sq4: every variant squares alike
__device__ __forceinline__ float sq4(const f32x4& d) {
  return __builtin_fmaf(d[0], d[0], d[1] * d[1]) + __builtin_fmaf(d[2], d[2], d[3] * d[3]);
}

// stx_relu_fwd's form: a NaN stays a NaN
template <bool RELU>
__device__ __forceinline__ float tin(float v) {
  if constexpr (RELU) return v <= 0.f ? 0.f : v;
  return v;
}

template <bool RELU>
__device__ __forceinline__ f32x4 tin4(f32x4 v) {
  if constexpr (RELU) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = tin<true>(v[e]);
  }
  return v;
}

// var -> std; a plane without finite statistics (a NaN or Inf in it: std is NaN) gets a
// NaN mean too
__device__ __forceinline__ void stats_close(float q, int hw, float eps, float& mean, float& sd) {
  const float var = q / (float)(hw - 1);
  sd = sqrtf(var + eps);
  if (sd != sd) mean = sd;
}

// one plane into registers: thread t holds float4s t, t + NT, ... (zeros past the plane)
template <int NT, int R4, bool RELU>
__device__ __forceinline__ void plane_load(const float* __restrict__ xp, int n4, f32x4 (&u)[R4]) {
  const f32x4* p = reinterpret_cast<const f32x4*>(xp);
#pragma unroll
  for (int k = 0; k < R4; ++k) {
    const int i = threadIdx.x + k * NT;
    u[k] = i < n4 ? tin4<RELU>(p[i]) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
}

template <int NT, int R4>
__device__ __forceinline__ void plane_stats_reg(const f32x4 (&u)[R4], int hw, float eps,
                                                float* red, float& mean, float& sd) {
  const int n4 = hw >> 2;
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < R4; ++k) s += (u[k][0] + u[k][1]) + (u[k][2] + u[k][3]);
  mean = bsum<NT>(s, red) / (float)hw;
  float q = 0.f;
#pragma unroll
  for (int k = 0; k < R4; ++k) {
    if ((int)threadIdx.x + k * NT < n4) {
      const f32x4 d = u[k] - mean;
      q += sq4(d);
    }
  }
  q = bsum<NT>(q, red);
  stats_close(q, hw, eps, mean, sd);
}

template <int NT, bool RELU>
__device__ __forceinline__ void plane_stats_loop(const float* __restrict__ xp, int hw, bool vec,
                                                 float eps, float* red, float& mean, float& sd) {
  float s = 0.f;
  if (vec) {
    for (int i = threadIdx.x * 4; i < hw; i += NT * 4) {
      const f32x4 v = tin4<RELU>(*reinterpret_cast<const f32x4*>(xp + i));
      s += (v[0] + v[1]) + (v[2] + v[3]);
    }
  } else {
    for (int i = threadIdx.x; i < hw; i += NT) s += tin<RELU>(xp[i]);
  }
  mean = bsum<NT>(s, red) / (float)hw;
  float q = 0.f;
  if (vec) {
    for (int i = threadIdx.x * 4; i < hw; i += NT * 4) {
      const f32x4 d = tin4<RELU>(*reinterpret_cast<const f32x4*>(xp + i)) - mean;
      q += sq4(d);
    }
  } else {
    for (int i = threadIdx.x; i < hw; i += NT) {
      const float d = tin<RELU>(xp[i]) - mean;
      q = __builtin_fmaf(d, d, q);
    }
  }
  q = bsum<NT>(q, red);
  stats_close(q, hw, eps, mean, sd);
}

enum { M_STATS = 0, M_STATS_RELU = 1, M_ADAIN = 2, M_LOSS = 3 };

struct PlaneArgs {
  const float* x;
  float* mean;  // [n*c] or NULL
  float* sd;    // [n*c] or NULL
  int c, hw;
  float eps;
  int xvec;  // loop kernels: float4 trips over x
  // AdaIN
  const float* smean;
  const float* sstd;  // [S][c]
  const float* mix;   // [n][S]
  float alpha;
  float* y;
  int yvec;  // y is 16-byte aligned (hw % 4 == 0 is the variant's)
  float* out_amax;
  int S;
  // loss
  const float* tmean;
  const float* tstd;  // [n*c]
  float* parts;       // [n*c][2]
};

// What a plane's result needs besides its statistics, read before them so that these loads
// are in flight with the plane's: AdaIN's M, G as fma chains from 0 with s ascending
// (stx_cin_mix's form: a one-hot row reproduces the table row's bits); the loss's targets
template <int MODE>
__device__ __forceinline__ void plane_tables(const PlaneArgs& p, int plane, float& t0, float& t1) {
  t0 = t1 = 0.f;
  if constexpr (MODE == M_ADAIN) {
    const int k = plane / p.c, ch = plane - k * p.c;
    const float* m = p.mix + (size_t)k * p.S;
    for (int s = 0; s < p.S; ++s) {
      const float w = m[s];
      t0 = __builtin_fmaf(w, p.smean[(size_t)s * p.c + ch], t0);
      t1 = __builtin_fmaf(w, p.sstd[(size_t)s * p.c + ch], t1);
    }
  } else if constexpr (MODE == M_LOSS) {
    t0 = p.tmean[plane];
    t1 = p.tstd[plane];
  }
}

// the per-plane outputs; AdaIN's a, b of y = fma(x, a, b): r = G / std,
// a = fma(alpha, r, 1 - alpha), b = alpha * fma(-r, mean, M)
template <int MODE>
__device__ __forceinline__ void plane_outputs(const PlaneArgs& p, int plane, float mean, float sd,
                                              float t0, float t1, float& a, float& b) {
  if (threadIdx.x == 0) {
    if (p.mean) p.mean[plane] = mean;
    if (p.sd) p.sd[plane] = sd;
    if constexpr (MODE == M_LOSS) {
      const float dm = mean - t0, ds = sd - t1;
      p.parts[2 * (size_t)plane] = dm * dm;
      p.parts[2 * (size_t)plane + 1] = ds * ds;
    }
  }
  if constexpr (MODE == M_ADAIN) {
    const float r = t1 / sd;
    a = __builtin_fmaf(p.alpha, r, 1.f - p.alpha);
    b = p.alpha * __builtin_fmaf(-r, mean, t0);
  }
}

// Register variant (hw % 4 == 0, x 16-byte aligned, hw <= 4 NT R4).  A block walks PPB
// consecutive planes and issues the next plane's loads before this plane's reductions and
// stores, so the chip's load and store phases overlap instead of every resident block
// loading, reducing and storing in lockstep (instnorm.hip's pipelined kernel; PPB = 1 is the
// plain one-plane block).  The same arithmetic per plane whatever PPB: the same bits.
template <int NT, int R4, int MODE, int PPB>
__global__ void __launch_bounds__(NT) plane_reg_kernel(PlaneArgs p) {
  constexpr bool RELU = MODE == M_STATS_RELU;
  __shared__ float red[NT / 64];
  const int n4 = p.hw >> 2;
  const int p0 = blockIdx.x * PPB;
  f32x4 ub[PPB > 1 ? 2 : 1][R4];
  plane_load<NT, R4, RELU>(p.x + (size_t)p0 * p.hw, n4, ub[0]);
  uint32_t om = 0u;  // max |y| as IEEE bits
#pragma unroll
  for (int j = 0; j < PPB; ++j) {
    const int bi = j & 1, plane = p0 + j;
    if (j + 1 < PPB)
      plane_load<NT, R4, RELU>(p.x + (size_t)(plane + 1) * p.hw, n4, ub[bi ^ 1]);
    float t0, t1, mean, sd, a, b;
    plane_tables<MODE>(p, plane, t0, t1);
    plane_stats_reg<NT, R4>(ub[bi], p.hw, p.eps, red, mean, sd);
    plane_outputs<MODE>(p, plane, mean, sd, t0, t1, a, b);
    if constexpr (MODE == M_ADAIN) {
      float* yp = p.y + (size_t)plane * p.hw;
#pragma unroll
      for (int k = 0; k < R4; ++k) {
        const int i = threadIdx.x + k * NT;
        if (i < n4) {
          f32x4 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            o[e] = __builtin_fmaf(ub[bi][k][e], a, b);
            om = max(om, __float_as_uint(o[e]) & 0x7fffffffu);
          }
          if (p.yvec) {
            reinterpret_cast<f32x4*>(yp)[i] = o;
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) yp[4 * i + e] = o[e];
          }
        }
      }
    }
  }
  if constexpr (MODE == M_ADAIN)
    if (p.out_amax) bmax_to<NT>(p.out_amax, om, red, blockIdx.x);
}

// Loop variant: any hw and alignment; the plane is re-read (from L2) for each pass
template <int NT, int MODE>
__global__ void __launch_bounds__(NT) plane_loop_kernel(PlaneArgs p) {
  constexpr bool RELU = MODE == M_STATS_RELU;
  __shared__ float red[NT / 64];
  const int plane = blockIdx.x;
  const size_t base = (size_t)plane * p.hw;
  const float* xp = p.x + base;
  float t0, t1, mean, sd, a, b;
  plane_tables<MODE>(p, plane, t0, t1);
  plane_stats_loop<NT, RELU>(xp, p.hw, p.xvec != 0, p.eps, red, mean, sd);
  plane_outputs<MODE>(p, plane, mean, sd, t0, t1, a, b);
  if constexpr (MODE == M_ADAIN) {
    float* yp = p.y + base;
    uint32_t om = 0u;
    if (p.xvec && p.yvec) {
      for (int i = threadIdx.x * 4; i < p.hw; i += NT * 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(xp + i);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          o[e] = __builtin_fmaf(v[e], a, b);
          om = max(om, __float_as_uint(o[e]) & 0x7fffffffu);
        }
        *reinterpret_cast<f32x4*>(yp + i) = o;
      }
    } else {
      for (int i = threadIdx.x; i < p.hw; i += NT) {
        const float o = __builtin_fmaf(xp[i], a, b);
        yp[i] = o;
        om = max(om, __float_as_uint(o) & 0x7fffffffu);
      }
    }
    if (p.out_amax) bmax_to<NT>(p.out_amax, om, red, plane);
  }
}

// out[1] = scale * sum of the mean parts, out[2] = scale * sum of the std parts, planes
// strided over the 256 threads in a fixed order; out[0] = out[1] + out[2]
constexpr int LFB = 256;
__global__ void __launch_bounds__(LFB)
stats_loss_final_kernel(const float* __restrict__ parts, int planes, double scale,
                        float* __restrict__ out, float* __restrict__ add_to) {
  __shared__ float red[LFB / 64];
  float sm = 0.f, ss = 0.f;
  for (int i = threadIdx.x; i < planes; i += LFB) {
    sm += parts[2 * (size_t)i];
    ss += parts[2 * (size_t)i + 1];
  }
  sm = bsum<LFB>(sm, red);
  ss = bsum<LFB>(ss, red);
  if (threadIdx.x == 0) {
    const float lm = (float)((double)sm * scale), ls = (float)((double)ss * scale);
    const float l = lm + ls;
    out[0] = l;
    out[1] = lm;
    out[2] = ls;
    if (add_to) *add_to += l;
  }
}

// dx = A + B (x - mean) per plane, A = kk 2 (mean - tmean) / hw, B = kk 2 (std - tstd) /
// ((hw - 1) std), kk = g weight / (n c): the coefficients once per block, then one
// streaming pass.  grid (planes, chunks of BW_CHUNK floats); on the float4 path a thread
// issues all of its chunk's loads (BW_R4 float4s of x, and of dx with accumulate) before the
// first use, so a block keeps 32 KB (64 KB) in flight
constexpr int BW_NT = 256, BW_R4 = 8, BW_CHUNK = 4 * BW_NT * BW_R4;
__global__ void __launch_bounds__(BW_NT)
stats_loss_bwd_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                      const float* __restrict__ sd, const float* __restrict__ tmean,
                      const float* __restrict__ tstd, int hw, float k,
                      const float* __restrict__ g_dev, float* __restrict__ dx, int accumulate,
                      float* __restrict__ out_amax, int vec) {
  __shared__ float red[BW_NT / 64];
  const int plane = blockIdx.x;
  const size_t base = (size_t)plane * hw;
  const float* xp = x + base;
  float* dp = dx + base;
  const int i0 = blockIdx.y * BW_CHUNK, i1 = min(hw, i0 + BW_CHUNK);
  const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 v[BW_R4], o[BW_R4];
  if (vec) {
#pragma unroll
    for (int r = 0; r < BW_R4; ++r) {
      const int i = i0 + (threadIdx.x + r * BW_NT) * 4;
      v[r] = i < i1 ? *reinterpret_cast<const f32x4*>(xp + i) : z4;
    }
    if (accumulate) {
#pragma unroll
      for (int r = 0; r < BW_R4; ++r) {
        const int i = i0 + (threadIdx.x + r * BW_NT) * 4;
        o[r] = i < i1 ? *reinterpret_cast<const f32x4*>(dp + i) : z4;
      }
    }
  }
  const float m = mean[plane], s = sd[plane];
  const float kk = g_dev ? k * g_dev[0] : k;
  const float A = kk * (2.f * (m - tmean[plane]) / (float)hw);
  const float B = kk * (2.f * (s - tstd[plane]) / ((float)(hw - 1) * s));
  uint32_t om = 0u;
  // with accumulate a zero term leaves the old value as it is, bit for bit (-0 included)
  auto put = [&](float xv, float old) {
    const float t = __builtin_fmaf(B, xv - m, A);
    const float ov = accumulate ? (t == 0.f ? old : old + t) : t;
    om = max(om, __float_as_uint(ov) & 0x7fffffffu);
    return ov;
  };
  if (vec) {
#pragma unroll
    for (int r = 0; r < BW_R4; ++r) {
      const int i = i0 + (threadIdx.x + r * BW_NT) * 4;
      if (i < i1) {
        f32x4 w;
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] = put(v[r][e], accumulate ? o[r][e] : 0.f);
        *reinterpret_cast<f32x4*>(dp + i) = w;
      }
    }
  } else {
    for (int i = i0 + threadIdx.x; i < i1; i += BW_NT) dp[i] = put(xp[i], accumulate ? dp[i] : 0.f);
  }
  if (out_amax) bmax_to<BW_NT>(out_amax, om, red, blockIdx.x + gridDim.x * blockIdx.y);
}

bool al16(const void* p) { return !(reinterpret_cast<uintptr_t>(p) & 15); }

// planes per block of the pipelined small-plane kernel, and the block count from which it
// is used (two blocks per CU: fewer and the one-plane blocks fill the chip better)
constexpr int PIPE_PPB = 4, PIPE_MIN_BLOCKS = 512;

template <int MODE>
void launch_plane(const PlaneArgs& a, int planes, hipStream_t st) {
  const int hw = a.hw;
  const bool reg = hw % 4 == 0 && al16(a.x);
  const dim3 grid(planes);
  if (reg && hw <= 4 * 256 * 4) {
    if (MODE == M_ADAIN && planes % PIPE_PPB == 0 && planes / PIPE_PPB >= PIPE_MIN_BLOCKS)
      hipLaunchKernelGGL((plane_reg_kernel<256, 4, MODE, PIPE_PPB>), dim3(planes / PIPE_PPB),
                         dim3(256), 0, st, a);
    else
      hipLaunchKernelGGL((plane_reg_kernel<256, 4, MODE, 1>), grid, dim3(256), 0, st, a);
  } else if (reg && hw <= 4 * 512 * 8)
    hipLaunchKernelGGL((plane_reg_kernel<512, 8, MODE, 1>), grid, dim3(512), 0, st, a);
  else if (reg && hw <= 4 * 1024 * 16)
    hipLaunchKernelGGL((plane_reg_kernel<1024, 16, MODE, 1>), grid, dim3(1024), 0, st, a);
  else if (hw >= 16384)
    hipLaunchKernelGGL((plane_loop_kernel<1024, MODE>), grid, dim3(1024), 0, st, a);
  else
    hipLaunchKernelGGL((plane_loop_kernel<256, MODE>), grid, dim3(256), 0, st, a);
}

// n, c > 0, hw >= 2, n c and n c hw within an int / a grid's x extent
bool plane_dims_ok(int n, int c, int hw) {
  return n > 0 && c > 0 && hw >= 2 && hw <= (1 << 30) && (long long)n * c <= INT_MAX;
}

}  // namespace
}  // namespace stx

using namespace stx;

extern "C" int stx_chan_stats(const float* x, float* mean, float* std_, int n, int c, int hw,
                              float eps, int relu_input, void* stream) {
  if (!x || !mean || !std_ || !plane_dims_ok(n, c, hw)) {
    set_error("stx_chan_stats: invalid arguments (n %d c %d hw %d; x, mean, std given, hw >= 2)",
              n, c, hw);
    return STX_E_INVALID;
  }
  PlaneArgs a{};
  a.x = x, a.mean = mean, a.sd = std_, a.c = c, a.hw = hw, a.eps = eps;
  a.xvec = hw % 4 == 0 && al16(x);
  if (relu_input)
    launch_plane<M_STATS_RELU>(a, n * c, (hipStream_t)stream);
  else
    launch_plane<M_STATS>(a, n * c, (hipStream_t)stream);
  return check_launch("stx_chan_stats");
}

extern "C" int stx_adain(const float* x, const float* smean, const float* sstd, const float* mix,
                         float alpha, float* y, float* mean, float* std_, int n, int c, int hw,
                         int S, float eps, float* out_amax, void* stream) {
  if (!x || !smean || !sstd || !mix || !y || S <= 0 || !plane_dims_ok(n, c, hw)) {
    set_error("stx_adain: invalid arguments (n %d c %d hw %d S %d; x, smean, sstd, mix, y given, "
              "hw >= 2, S > 0)", n, c, hw, S);
    return STX_E_INVALID;
  }
  PlaneArgs a{};
  a.x = x, a.mean = mean, a.sd = std_, a.c = c, a.hw = hw, a.eps = eps;
  a.xvec = hw % 4 == 0 && al16(x);
  a.smean = smean, a.sstd = sstd, a.mix = mix, a.alpha = alpha, a.y = y, a.S = S;
  a.yvec = hw % 4 == 0 && al16(y);
  a.out_amax = out_amax;
  launch_plane<M_ADAIN>(a, n * c, (hipStream_t)stream);
  return check_launch("stx_adain");
}

extern "C" size_t stx_stats_loss_ws(int n, int c) {
  return (size_t)2 * (n > 0 ? n : 0) * (c > 0 ? c : 0) * sizeof(float) + 64;
}

extern "C" int stx_stats_loss(const float* x, const float* tmean, const float* tstd, int n, int c,
                              int hw, float eps, float weight, float* out, float* add_to,
                              float* mean, float* std_, void* ws, size_t ws_bytes, void* stream) {
  if (!x || !tmean || !tstd || !out || !plane_dims_ok(n, c, hw)) {
    set_error("stx_stats_loss: invalid arguments (n %d c %d hw %d; x, tmean, tstd, out given, "
              "hw >= 2)", n, c, hw);
    return STX_E_INVALID;
  }
  if (!ws || ws_bytes < stx_stats_loss_ws(n, c)) {
    set_error("stx_stats_loss: workspace too small");
    return STX_E_WORKSPACE;
  }
  PlaneArgs a{};
  a.x = x, a.mean = mean, a.sd = std_, a.c = c, a.hw = hw, a.eps = eps;
  a.xvec = hw % 4 == 0 && al16(x);
  a.tmean = tmean, a.tstd = tstd, a.parts = (float*)ws;
  hipStream_t st = (hipStream_t)stream;
  launch_plane<M_LOSS>(a, n * c, st);
  hipLaunchKernelGGL(stats_loss_final_kernel, dim3(1), dim3(LFB), 0, st, (const float*)ws, n * c,
                     (double)weight / ((double)n * c), out, add_to);
  return check_launch("stx_stats_loss");
}

extern "C" int stx_stats_loss_bwd(const float* x, const float* mean, const float* std_,
                                  const float* tmean, const float* tstd, int n, int c, int hw,
                                  float weight, const float* g_dev, float* dx, int accumulate,
                                  float* out_amax, void* stream) {
  if (!x || !mean || !std_ || !tmean || !tstd || !dx || !plane_dims_ok(n, c, hw) ||
      cdiv(hw, BW_CHUNK) > 65535) {
    set_error("stx_stats_loss_bwd: invalid arguments (n %d c %d hw %d; x, mean, std, tmean, tstd, "
              "dx given, hw >= 2)", n, c, hw);
    return STX_E_INVALID;
  }
  const int vec = hw % 4 == 0 && al16(x) && al16(dx);
  const float k = (float)((double)weight / ((double)n * c));
  hipLaunchKernelGGL(stats_loss_bwd_kernel, dim3(n * c, cdiv(hw, BW_CHUNK)), dim3(BW_NT), 0,
                     (hipStream_t)stream, x, mean, std_, tmean, tstd, hw, k, g_dev, dx,
                     accumulate, out_amax, vec);
  return check_launch("stx_stats_loss_bwd");
}

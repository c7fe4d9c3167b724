// Bodies of the one-block kernels at the end of a Gatys iteration's forward and in front
// of its Adam update (loss_finalize_kernel, adam_prepare_kernel), shared with the riders
// of the compose launch (weight_compose16_tail_kernel, conv16.hip): a rider block runs
// one of these bodies beside the compose grid instead of as a launch of its own.  One
// definition each, so the stand-alone launch and the rider give the same bits.
#ifndef STX_TAIL_H_
#define STX_TAIL_H_

#include "common.h"
#include "../../include/stx.h"

namespace stx {

// one wave: the fixed-order sum of n loss partials (4 lane-strided accumulators, then a
// wave tree) -- shared by sum_parts_kernel and the loss finalize so the deferred and
// direct style losses are the same bits
__device__ __forceinline__ float wave_sum_parts(const float* __restrict__ parts, int n, int lane) {
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  int i = lane;
  for (; i + 192 < n; i += 256) {
    s0 += parts[i];
    s1 += parts[i + 64];
    s2 += parts[i + 128];
    s3 += parts[i + 192];
  }
  for (; i < n; i += 64) s0 += parts[i];
  return wave_sum((s0 + s1) + (s2 + s3));
}

struct LossWF {
  float w[16];
};

// one block of NW waves: losses[i] = inv_i * sum(parts_i) (one wave per loss, the order of
// sum_parts_kernel, so the values are identical; wave w takes losses w, w + NW, ...), then
// thread 0 the weighted total.  lv: 8 floats of LDS.
template <int NW>
__device__ __forceinline__ void loss_finalize_body(const stx_loss_parts& lp,
                                                   float* __restrict__ losses,
                                                   const float* __restrict__ extra, int m,
                                                   const LossWF& w, float* __restrict__ total,
                                                   float* lv) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int i = wave; i < lp.k; i += NW) {
    const float s = wave_sum_parts(lp.parts[i], lp.nparts[i], lane);
    if (lane == 0) lv[i] = s * lp.inv[i];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int i = 0; i < lp.k; ++i) {
      losses[i] = lv[i];
      t += w.w[i] * lv[i];
    }
    for (int j = 0; j < m; ++j) t += w.w[lp.k + j] * extra[j];
    if (total) *total = t;
  }
}

// torch.optim.Adam's per-step scalars (elementwise.hip), computed in fp64 like torch's
// Python floats
struct AdamScalars {
  float step_size;   // lr / bc1
  float bc2_sqrt;    // sqrt(1 - b2^t)
};

// one thread: the step counter and the bias corrections
__device__ __forceinline__ void adam_prepare_body(int* step, AdamScalars* sc, double lr,
                                                  double b1, double b2) {
  const int t = ++(*step);
  const double bc1 = 1.0 - pow(b1, (double)t);
  const double bc2 = 1.0 - pow(b2, (double)t);
  sc->step_size = (float)(lr / bc1);
  sc->bc2_sqrt = (float)sqrt(bc2);
}

}  // namespace stx

#endif  // STX_TAIL_H_

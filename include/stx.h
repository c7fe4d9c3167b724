/*
 * libstx — MI355X (gfx950 / CDNA4) kernels for the tupini07/StyleTransfer hot
 * path, behind a plain C ABI.  All pointers are DEVICE pointers to fp32 NCHW
 * contiguous tensors unless stated; `stream` is a hipStream_t (NULL = legacy
 * default stream).  Every entry point is asynchronous on `stream`, performs no
 * allocation and no host synchronisation, and returns 0 on success or a
 * non-zero STX_E_* / hipError_t code (message via stx_last_error_string()).
 * Kernels are graph-capturable.
 *
 * Reference interfaces replaced (all in /root/reference, tupini07/StyleTransfer):
 *   conv2d fwd/dgrad/wgrad  <- torchvision vgg19 `.features` Conv2d layers sliced in
 *                              stransfer/network.py:246-314 and the ImageTransformNet
 *                              Conv2d layers stransfer/network.py:468-481,525-609
 *   gram / style loss       <- StyleLoss.gram_matrix / forward  stransfer/network.py:92-123
 *   mse losses              <- ContentLoss.forward :155-164, FeatureReconstructionLoss.forward :186-201
 *   maxpool / relu          <- VGG MaxPool2d / ReLU(inplace=False) stransfer/network.py:270-271
 *   adam                    <- torch.optim.Adam via get_content_optimizer :403-409, get_optimizer :643-649
 *   instance norm           <- nn.InstanceNorm2d(affine=True) stransfer/network.py:474,483,531,...,600
 *   residual add            <- ResidualBlock.forward `out += residual` :502
 *   upsample nearest x2     <- nn.Upsample(mode='nearest', scale_factor=2) :580-581,592-593
 *   total variation         <- get_total_variation_regularization_loss :621-641
 *   temporal loss           <- VideoTransformNet.get_temporal_loss :885-903
 *   image conditioning      <- img_utils.image_loader_transform stransfer/img_utils.py:13-44
 *                              (COCO loader stransfer/dataset.py:141-197)
 */
#ifndef STX_H_
#define STX_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Every max|.| bound in this API ("amax": in_amax, w_amax, out_amax, p2_amax,
 * z_amax, stx_amax's out) is a group of STX_AMAX_SLOTS floats whose maximum is the
 * value; producers spread their atomics over the group, a zeroed group reads 0. */
#define STX_AMAX_SLOTS 32

#define STX_OK 0
#define STX_E_INVALID 1001   /* bad argument / unsupported shape */
#define STX_E_WORKSPACE 1002 /* workspace too small */

/* input-loader modes for stx_conv2d: how the virtual conv input is formed
 * from the physical tensor x (fused into the LDS halo load) */
#define STX_IN_RAW 0        /* v = x                                            */
#define STX_IN_RELU 1       /* v = max(x, 0)              (VGG ReLU, not in-place) */
#define STX_IN_RELU_POOL2 2 /* v = maxpool2x2(max(x,0))   (VGG ReLU + MaxPool2d) */
#define STX_IN_UPSAMPLE2 3  /* v = x[y/2][x/2]            (nn.Upsample nearest x2) */
#define STX_IN_DILATE2 4    /* v = x[y/2][x/2] at even y,x else 0 (stride-2 dgrad) */
/* A NaN in x under STX_IN_RELU / STX_IN_RELU_POOL2 (a NaN that reaches the GEMM makes every
 * output it touches NaN; one the loader's ReLU removes reads as 0, or in a pool window as
 * if it were absent), one line per loader:
 *   conv.hip (fp32 MFMA, every loader form)     fmaxf: NaN reads as 0
 *   wgrad.hip (fp32 weight gradient)            fmaxf: NaN reads as 0
 *   conv16.hip (fp16 hi/lo split)               integer max of the bit pattern: a NaN with
 *                                               the sign bit clear is kept (and wins its
 *                                               pool window), one with it set reads as 0
 *   convfew.hip, conv9.hip (few-channel / 9x9)  as conv16.hip
 *   wgrad16.hip                                 wgrad16_kernel as conv16.hip;
 *                                               wgrad16_lds_kernel fmaxf: NaN reads as 0
 * The split kernels also scale by in_amax, which a NaN input makes NaN (stx_amax).  The
 * stand-alone stx_relu_fwd / stx_maxpool2x2_fwd and the fused pool_out keep every NaN. */

typedef struct stx_conv_params {
  const float* x;     /* physical input [n][cin][h][w] */
  const float* wt;    /* prepped weights [cin_pad*ks*ks][cout_pad] (stx_conv_weight_prep);
                         may be NULL when wt16 selects the split path */
  const float* bias;  /* [cout] or NULL */
  float* y;           /* output [n][cout][ho][wo]; NULL with pool_out (split path, plain
                         epilogue): only pool_out is written */
  const float* mask;  /* NULL or [n][cout][ho][wo]: value *= (mask > 0)   (ReLU backward) */
  const float* aux;   /* NULL or [n][cout][ho][wo]: value += aux_scale*aux */
  float aux_scale;
  const float* acc_scale; /* NULL or device scalar: value = acc * (*acc_scale) first */
  int accumulate;     /* value += old y */
  int relu_out;       /* y = max(value, 0) */
  int n, cin, h, w;   /* physical input dims */
  int cout, ks, stride, pad;
  int in_mode;        /* STX_IN_* */
  int hv, wv;         /* virtual input dims (after the in_mode transform) */
  int ho, wo;         /* output dims */
  int cin_pad, cout_pad;
  long long wt_batch_stride; /* floats between per-image weight matrices (0 = shared) */
  /* optional fused second GEMM phase (Gram backward inside the data-gradient conv):
   * after the main K loop the mask is applied, then
   *   value += (*p2_scale) * sum_c A[n][c][co] * p2_z[n][c][oy][ox]
   * A = p2_wt + n*p2_wt_batch_stride, laid out [c (padded to cin_pad rule of a 1x1 conv)]
   * [cout_pad]; p2_z [n][p2_c][ho][wo].  p2_z == NULL disables it.  stride 1 only. */
  const float* p2_z;
  const float* p2_wt;
  const float* p2_scale;
  int p2_c;
  long long p2_wt_batch_stride;
  /* optional fused ReLU+MaxPool2d backward epilogue:
   *   value += unpool(up_dp)[co][oy][ox] * (up_z > 0)
   * with the 2x2 argmax (first max of relu(up_z), row-major) recomputed from up_z
   * [n][cout][ho][wo]; up_dp [n][cout][ho/2][wo/2].  up_dp == NULL disables it. */
  const float* up_dp;
  const float* up_z;
  /* fp16 hi/lo split path (3x3 stride-1 convs, cin >= 16, cout > 4): when wt16 is
   * non-NULL the conv runs on v_mfma_f32_32x32x16_f16 with both operands split as
   * s*v = hi + lo (fp16 each, s a per-tensor power of two) and the three products
   * hi*hi + hi*lo + lo*hi accumulated in fp32 (fp32-level accuracy).
   * wt16/w_amax come from stx_conv_weight_prep16; in_amax is a device scalar
   * >= max|x| over the physical input (stx_amax, or a producer's out_amax). */
  const void* wt16;
  const float* w_amax;
  const float* in_amax;
  /* optional: *out_amax = max(*out_amax, max|y|) over the values this call writes
   * (caller zeroes it first) — the next split conv's in_amax at no extra pass. */
  float* out_amax;
  /* optional fused VGG ReLU + MaxPool2d(2,2) output: pool_out [n][cout][ho/2][wo/2] =
   * maxpool(relu(y)) (torch floor mode), written beside y.  Split path (wt16) with
   * wo > 32 only; the next conv then reads it with STX_IN_RAW. */
  float* pool_out;
  /* split path only: device scalar >= max|p2_z| (required with p2_z and wt16; the
   * Gram-backward phase then also runs on the fp16 hi/lo split MFMA, A scaled per
   * block by its own max).  A 1x1 conv with per-image weights (the Gram backward
   * dz = s*A[n].z, stx_gram_bwd) given in_amax and wt16 = (void*)1 runs as that
   * phase alone on the split kernel (no ReLU mask allowed there). */
  const float* p2_amax;
  /* optional fused Gram partials of the output (StyleLoss.gram_matrix of a 64- or
   * 128-channel VGG tap, stransfer/network.py:92-108, computed where the tile is produced
   * instead of re-reading y): split path, stride 1, cout == 64 or 128, wo > 32, and the
   * plain epilogue (no mask / aux / accumulate / acc_scale / up_dp / p2_z / relu_out;
   * cout 128: raw or ReLU input).  Block t of image n writes sum over its output pixels
   * of y y^T (fp32, fp16 hi/lo MFMA with a block-local power-of-two scale) as U 64 x 64
   * tiles: tile u to gram_part + ((n * U + u) * T + t) * 4096, T = stx_conv_gram_tiles(p),
   * U = 1 (cout 64) or 3 (cout 128: tiles (0,0), (0,1), (1,1) of the 128 x 128 matrix,
   * diagonal tiles whole); stx_style_loss (parts) reduces them. */
  float* gram_part;
  /* with pool_out: pool_out = the 2x2 SUM of the output (no ReLU) and y is not written
   * -- the backward of nearest x2 upsampling (torch.nn.Upsample(scale_factor=2), the
   * ImageTransformNet's UpsampleConvLayer, stransfer/network.py:583-605) fused into the
   * data-gradient conv of the upsampled conv.  Split path, stride 1, wo > 32, even
   * ho / wo, plain epilogue only (no mask / aux / accumulate / acc_scale / up_dp / p2_z /
   * relu_out / gram_part / out_amax). */
  int pool_sum;
  /* optional with gram_part: per-group arrival counters, n * stx_conv_gram_groups(p)
   * uint32 words, zeroed once by the caller (every call leaves them zero again).  The
   * partials of tiles g*STX_GRAM_GROUP .. g*STX_GRAM_GROUP+7 of image n form group g;
   * the last block of a group to finish sums the group's partials in tile order and
   * writes that sum to gram_part + (n_total * T + n * NG + g) * 4096 (NG =
   * stx_conv_gram_groups(p)), so stx_style_loss (parts) reads NG sums per image
   * instead of T partials.  The per-tile slots then hold three of the four 32 x 32
   * blocks only (scratch); the gram_part slab needs (T + NG) * 4096 floats per image. */
  unsigned int* gram_cnt;
  /* optional with p2_z on the split path: device amax group >= max|s * A[n]| over every
   * image n (stx_gram_fin_job.coef_amax of the finalize that wrote A, times |p2_scale|
   * folded in by the kernel).  The Gram-backward phase then runs on the fp16 hi/lo
   * split MFMA with this precomputed scale instead of the fp32 MFMA. */
  const float* p2_wt_amax;
  /* optional with gram_part on a 128-channel tap (the content layer conv2_2,
   * stransfer/network.py:134-201): the content target ref [n][cout][ho][wo]; block t of
   * image n then also writes sum (y - ref)^2 and sum (relu y - relu ref)^2 over its
   * outputs to mse_parts[2 (n T + t) + 0 / 1] (n * T * 2 floats), which
   * stx_style_loss (mse_parts) reduces into the content / feature losses. */
  const float* mse_ref;
  float* mse_parts;
  /* optional with in_mode STX_IN_UPSAMPLE2 on the split path (wt16 / w_amax of the same
   * weights): the parity-class slab (stx_conv_weight_prep16_up).  The conv then runs as
   * four output-parity 2x2 convs over the un-upsampled input (64 x 8 output tiles of one
   * row parity per block); plain epilogue only (bias, relu_out, out_amax), wo > 32. */
  const void* wt16_up;
  /* unpool_out = 1 (split path, raw-input 3x3 stride-1 data gradient, cout C = 64 or 128,
   * wo % 32 == 0, ho % 4 == 0): the conv's result d (the gradient of a MaxPool2d(2,2)(ReLU
   * (.)) output, [n][C][ho][wo]) is not stored; y receives, at full resolution
   * [n][C][2ho][2wo],
   *   y[co][Y][X] = d[co][Y/2][X/2] * [(Y, X) is the first max of its 2x2 window of relu(z)]
   *                 * [z[co][Y][X] > 0]  +  s * sum_c A[n][c][co] z[c][Y][X]
   *                 (+ aux_scale * aux[co][Y][X] with aux, full resolution)
   * with z = up_z, A = p2_wt (p2_wt_batch_stride, pitch cout_pad = C), p2_c = C, s =
   * *p2_scale (or 1), p2_amax >= max|z| and p2_wt_amax >= max|A| -- the ReLU+MaxPool
   * backward and the Gram backward (+ the folded content term) of the pooled VGG tap
   * (stransfer/network.py:110-164 through :264-275) in the producing conv's epilogue, so d
   * never reaches HBM.  out_amax receives max|y|; no bias / mask / accumulate / relu_out /
   * pool / Gram outputs. */
  int unpool_out;
} stx_conv_params;

#define STX_GRAM_GROUP 8

int stx_version(void);
/* sizeof and the offset of the last member of each ABI struct, in this order:
 * stx_conv_params, stx_wprep_job, stx_loss_parts, stx_gram_fin_job, stx_in_pgrad_job,
 * stx_image_meta, stx_cin_job, stx_style_loss_params, stx_wgrad_params -- two values each,
 * min(n, count) written to out; returns the count.  Bindings check their mirrors against it. */
int stx_abi_layout(long long* out, int n);
const char* stx_last_error_string(void);
/* The ABI revision of this header (STX_ABI_VERSION): a host binding refuses a library of
 * another revision rather than pass arguments whose meaning changed (round 6:
 * stx_instnorm_bwd's second argument is beta, not y; 7: stx_conv_params.unpool_out;
 * 9: the guided Gram entry points; 10: stx_style_loss takes stx_style_loss_params; 11:
 * stx_conv2d_wgrad takes stx_wgrad_params).  The revision moves only when an existing
 * entry point or struct changes meaning; entry points that are merely added (the colour
 * control pair, the flow entry points below, stx_flow_compose) do not bump it -- a binding
 * finds a missing symbol at load. */
#define STX_ABI_VERSION 11
int stx_abi_version(void);

/* Padded GEMM dims the conv kernels expect for a (cin, cout, ks) conv. */
int stx_conv_weight_dims(int cin, int cout, int ks, int* cin_pad, int* cout_pad);

/* w [cout][cin][ks][ks] -> wt [cin_pad*ks*ks][cout_pad] (zero padded).
 * transpose=1 builds the data-gradient weights of the same layer instead:
 * wt'[co*ks*ks + kh*ks + kw][ci] = w[co][ci][ks-1-kh][ks-1-kw] with dims
 * (cin'=cout, cout'=cin) padded by stx_conv_weight_dims(cout, cin, ks). */
int stx_conv_weight_prep(const float* w, float* wt, int cout, int cin, int ks, int transpose,
                         void* stream);

/* fp16 hi/lo split weight slab for the wt16 path: bytes of the slab for GEMM dims
 * (cin', cout') = (cin, cout), or (cout, cin) for transpose=1, ks = 3. */
size_t stx_conv_weight16_bytes(int cin, int cout, int ks, int transpose);
/* w [cout][cin][3][3] -> split slab wt16 ([cin'/16][tap][hi,lo][cin' group of 8]
 * [cout' padded to 64][8] fp16, scaled by 2^(15-e), max|w| < 2^e) and *w_amax =
 * max|w| (device scalar).  transpose=1: the data-gradient weights (as
 * stx_conv_weight_prep). */
int stx_conv_weight_prep16(const float* w, void* wt16, float* w_amax, int cout, int cin, int ks,
                           int transpose, void* stream);
/* The data-gradient split slab of a composed weight, for a Gram-backward operator that
 * feeds a 3x3 conv's data gradient with nothing in between (VGG conv3_1: dZ5 = A5 Z5,
 * then dP4 = conv3_1^T(dZ5); stransfer/network.py:92-123 StyleLoss backward through
 * :264-314 the conv3_1 piece):  conv^T_w(A . z) = conv^T_{w'}(z) with
 *   w'[c][ci][kh][kw] = s * sum_co A[c*pitch + co] * w[co][ci][kh][kw]   (s = *scale or 1)
 * so the data gradient reads z directly and dZ = A z is never formed.  The identity as
 * written needs A symmetric, which the Gram-backward operator is (coef = c (G - T) with
 * the diagonal alpha term; G and T symmetric); for a general A the launch computes
 * conv^T_w(A^T . z).  A is one image's
 * [cout][pitch] operator (pitch >= cout; stx_style_loss's coef), a_amax an amax group
 * >= max|A| (the finalize's coef_amax), w [cout][cin][3][3] with w_amax >= max|w|.  One
 * launch writes the transposed split slab wtT16 (stx_conv_weight16_bytes(cin, cout, 3, 1)
 * bytes) at the power-of-two scale of the bound |s| * cout * max|A| * max|w| >= max|w'|,
 * and stores that bound into every slot of the group out_amax: the conv takes
 * wt16 = wtT16, w_amax = out_amax.  cout <= 256, cin % 4 == 0, w 16-byte aligned; fixed
 * summation order. */
int stx_conv_weight_compose16(const float* A, int pitch, const float* a_amax, const float* w,
                              const float* w_amax, int cout, int cin, const float* scale,
                              void* wtT16, float* out_amax, void* stream);
/* Both split slabs of one weight (forward and data gradient) and their shared w_amax in
 * two launches (one max pass, one conversion) -- a trained layer re-preps every step. */
int stx_conv_weight_prep16_pair(const float* w, void* wt16, void* wtT16, float* w_amax,
                                int cout, int cin, int ks, void* stream);
/* The parity-class split slab of a 3x3 conv that reads a nearest x2 upsampled input
 * (UpsampleConvLayer, stransfer/network.py:578-600): each output parity class (a, b) of
 * the conv over the upsampled image is a 2x2 conv over the input with summed weights
 * W'[a][b][ry][rx] (16 instead of 36 tap MACs per 2x2 output group).  w [cout][cin][3][3]
 * -> wt16_up (stx_conv_weight16up_bytes(cin, cout) bytes), *w_amax = max|w| (the slab is
 * split at 2^(13 - e), |W'| <= 4 max|w|); stx_conv_params.wt16_up takes it. */
size_t stx_conv_weight16up_bytes(int cin, int cout);
int stx_conv_weight_prep16_up(const float* w, void* wt16_up, float* w_amax, int cout, int cin,
                              void* stream);
/* Every slab of a trained network in two launches (one max|w| pass over the distinct
 * split-slab weights, one conversion pass over all jobs) instead of two launches per
 * slab: the per-step re-prep of ImageTransformNet's 14 conv weights after each Adam
 * update (stransfer/network.py:765 optimizer.step -> the next static_train closure).
 * kind STX_WPREP_F32: slab as stx_conv_weight_prep(w, slab, cout, cin, ks, transpose);
 * kind STX_WPREP_F16: as stx_conv_weight_prep16(w, slab, w_amax, ...) (ks = 3).  The
 * forward and data-gradient split slabs of one weight may share w_amax (computed
 * once).  `jobs` is a host array read at call time (graph-capturable). */
#define STX_WPREP_MAX 48
#define STX_WPREP_F32 0
#define STX_WPREP_F16 1
#define STX_WPREP_F16UP 2 /* the parity-class slab (stx_conv_weight_prep16_up), transpose 0 */
typedef struct stx_wprep_job {
  const float* w;
  void* slab;
  float* w_amax;
  int kind, cout, cin, ks, transpose;
  int pad_;
} stx_wprep_job;
int stx_conv_weight_prep_batch(const stx_wprep_job* jobs, int njobs, void* stream);
/* *out = max |x[i]| over n floats (device scalar; NaN propagates). */
int stx_amax(const float* x, long long n, float* out, void* stream);

/* Gram partials per image a stx_conv2d call with these params writes through
 * gram_part (its 256-pixel output tiles), or 0 when the fused Gram does not apply. */
int stx_conv_gram_tiles(const stx_conv_params* p);
/* Gram group sums per image written with gram_cnt (ceil(T / STX_GRAM_GROUP)), 0 when
 * the fused Gram does not apply. */
int stx_conv_gram_groups(const stx_conv_params* p);

/* Implicit-GEMM convolution on fp32 MFMA (v_mfma_f32_32x32x2_f32), fused input
 * transform (in_mode) and epilogue (bias, mask, aux, accumulate, relu). */
int stx_conv2d(const stx_conv_params* p, void* stream);

/* Weight gradient: dw[cout][cin][ks][ks] (+)= sum_{n,oy,ox} dy * xv  (xv = in_mode(x)).
 * Split-K partial slabs in ws (fp32), reduced in fixed order (deterministic).  The caller
 * describes the conv; the library picks the path from the dims alone: the first of FEW16,
 * F16, F16S2 that covers them, else F32. */
#define STX_WGRAD_NONE 0 /* unsupported: not ks 3 stride 1/2 or ks 9 stride 1, STX_IN_DILATE2,
                          * or ho / wo that do not follow from the dims */
/* Implicit GEMM on fp32 MFMA (wgrad.hip): every supported shape the paths below leave. */
#define STX_WGRAD_F32 1
/* 3x3 stride-1 pad-1 conv on the fp16 hi/lo split MFMA (wgrad16.hip; in_mode RAW / RELU /
 * UPSAMPLE2, wo % 16 == 0, cin and cout >= 16); the upsampled input runs in the parity
 * classes of stx_conv_weight_prep16_up. */
#define STX_WGRAD_F16 2
/* The 3x3 stride-2 pad-1 downsampling convs of ImageTransformNet (stransfer/network.py:
 * 528-533; replaces the autograd conv2d weight gradient of static_train :690-765) on the
 * split MFMA: raw input with h = 2 ho, w = 2 wo, wo % 16 == 0, cin / cout >= 16. */
#define STX_WGRAD_F16S2 3
/* dW of the ImageTransformNet 9x9 stride-1 pad-4 layers whose one side has 1..3 channels
 * and the other 32 (conv0 3->32, conv22 32->3; stransfer/network.py:525-527, 605-609) on
 * the split MFMA, raw input, w % 16 == 0 (wgrad9.hip): the 3-channel tensor is expanded
 * per tap row in LDS, the 32-channel one streamed. */
#define STX_WGRAD_FEW16 4
typedef struct stx_wgrad_params {
  const float* x;  /* [n][cin][h][w] */
  const float* dy; /* [n][cout][ho][wo] */
  float* dw;
  /* amax groups (>= max|x|, max|dy|); required iff the planned path is a split one (> F32),
   * which also needs x and dy 16-byte aligned */
  const float* x_amax;
  const float* dy_amax;
  void* ws; /* at least the planner's ws_bytes */
  size_t ws_bytes;
  int accumulate;
  int n, cin, h, w, cout, ks, stride, pad, in_mode, ho, wo;
  int no_split; /* 1: STX_WGRAD_F32 whatever the shape (the tests' fp32 comparison) */
} stx_wgrad_params;
/* The path (STX_WGRAD_*) stx_conv2d_wgrad takes for p and its workspace bytes (ws_bytes may
 * be NULL).  Reads only the dims, in_mode and no_split; needs no GPU. */
int stx_conv2d_wgrad_plan(const stx_wgrad_params* p, size_t* ws_bytes);
int stx_conv2d_wgrad(const stx_wgrad_params* p, void* stream);
/* db[c] (+)= sum_{n,p} dy[n][c][p]  (conv bias gradient) */
size_t stx_bias_grad_ws(int n, int c);
int stx_bias_grad(const float* dy, float* db, int n, int c, int hw, int accumulate,
                  void* ws, size_t ws_bytes, void* stream);

/* Gram: G[b] = F_b F_b^T * scale, F_b = z[b] viewed [c][hw].  Split-K MFMA +
 * deterministic reduction.  z_amax (optional device scalar >= max|z|, e.g. the
 * producing conv's out_amax): with it and hw % 8 == 0 the partials run on the fp16
 * hi/lo split MFMA (fp32-level accuracy), else on fp32 MFMA. */
size_t stx_gram_ws(int b, int c, int hw);
int stx_gram(const float* z, float* g, int b, int c, int hw, float scale,
             const float* z_amax, void* ws, size_t ws_bytes, void* stream);

/* Style loss forward + backward coefficients (StyleLoss.forward; stx_style_loss below):
 *   G = gram(z)/(c*hw);  loss = mean((G - T)^2) over b*c*c  -> *loss (device scalar)
 *   A[b] = weight*4/(b*c*c*c*hw) * (G[b]-T) + diag_alpha*I     (A is [b][cpad][cpad])
 * so that dz = A·z (+ aux) is d(weight*loss)/dz; g_out (optional) receives G.
 * cpad = stx_gram_coef_pitch(c).  ws: stx_gram_ws(b, c, hw). */
int stx_gram_coef_pitch(int c);
/* With loss == NULL stx_style_loss leaves its loss partials in ws: *nparts floats at
 * byte offset stx_style_loss_parts(b, c, hw, &nparts), loss = sum * 1/(b*c*c). */
size_t stx_style_loss_parts(int b, int c, int hw, int* nparts);
/* Deferred loss reductions in one launch (the 5 StyleLoss values of a forward, then
 * the weighted total of get_total_current_{style,content}_loss):
 *   losses[i] = inv[i] * sum(parts[i][0 .. nparts[i]))          i < k (fixed order)
 *   *total    = sum_i w[i] losses[i] + sum_j w[k+j] extra[j]    (if total != NULL)
 * extra: m device scalars (e.g. the content loss); w_host: k + m host floats. */
typedef struct stx_loss_parts {
  const float* parts[8];
  int nparts[8];
  float inv[8];
  int k;
} stx_loss_parts;
int stx_loss_finalize(const stx_loss_parts* lp, float* losses, const float* extra, int m,
                      const float* w_host, float* total, void* stream);
/* stx_conv_weight_compose16 (above) with up to two rider blocks beside the compose grid,
 * each doing what would otherwise be a one-block launch of its own in a Gatys iteration's
 * serial chain (the slab and out_amax are the bits of stx_conv_weight_compose16):
 *   lp != NULL:       stx_loss_finalize(lp, losses, extra, m, w_host, total) -- the same
 *                     values; the loss partials must be complete in stream order (the Gram
 *                     finalize ran before this call);
 *   step_dev != NULL: the first half of stx_adam_step_clear: ++*step_dev and the step's
 *                     bias-corrected scalars into adam_ws (stx_adam_ws() bytes), nothing
 *                     cleared; stx_adam_step_prepared then applies the update.
 * Either rider may be absent.  No block waits on another. */
int stx_conv_weight_compose16_tail(const float* A, int pitch, const float* a_amax, const float* w,
                                   const float* w_amax, int cout, int cin, const float* scale,
                                   void* wtT16, float* out_amax, const stx_loss_parts* lp,
                                   float* losses, const float* extra, int m, const float* w_host,
                                   float* total, int* step_dev, void* adam_ws, float lr,
                                   float beta1, float beta2, void* stream);
/* dz (+)= s * A[b]·z[b] (+ aux_scale*aux) — Gram backward as a 1x1 MFMA conv with
 * per-image weights; z viewed [b][c][h][w]; s = *acc_scale_dev (or 1 if NULL) */
int stx_gram_bwd(const float* coef, const float* z, float* dz, int b, int c, int h, int w,
                 const float* acc_scale_dev, const float* mask, const float* aux,
                 float aux_scale, int accumulate, void* stream);

/* Guided (region-weighted) Gram -- the spatial control of Gatys et al. 2017, "Controlling
 * Perceptual Factors in Neural Style Transfer".  R regions (1 <= R <= STX_GUIDE_MAX) with
 * non-negative pixel weights wts [R][hw] shared over the batch (the host normalises each
 * row to sum hw; w_max is a host float >= max wts):
 *   G[b][r]  = 1/(c hw) sum_p wts[r][p] z[b][:,p] z[b][:,p]^T       g_out [b][R][c][c] or NULL
 *   loss_r[r] = 1/(b c c) sum_{b,i,j} (G[b][r] - T[r])^2             target [R][c][c]
 *   A[b][r]  = weight lambda[r] 4/(b c^3 hw) (G[b][r] - T[r])        coef [b][R][cpad][cpad]
 * (cpad = stx_gram_coef_pitch(c); coef may be NULL; lambda: R host floats read at call
 * time).  With z_amax (an amax group >= max|z|), hw % 8 == 0 and 16-byte aligned z / wts
 * the partials run on the fp16 hi/lo split MFMA (A operand wts z at the power-of-two
 * scale of w_max max|z|, B operand z), else on the fp32 MFMA; split-K partials summed in
 * a fixed order.  R = 1 with all-ones weights is stx_style_loss's G, loss and A.
 * ws >= stx_guided_style_ws(b, c, hw, R) (0: unsupported dims). */
#define STX_GUIDE_MAX 4
size_t stx_guided_style_ws(int b, int c, int hw, int R);
int stx_guided_style_loss(const float* z, const float* wts, float w_max, const float* target,
                          float* g_out, float* coef, float* loss_r, int b, int c, int hw, int R,
                          const float* lambda, float weight, const float* z_amax, void* ws,
                          size_t ws_bytes, void* stream);
/* dz[b] (+)= s sum_r wts[r] o (A[b][r] z[b]),  s = *acc_scale_dev (or 1 if NULL): the
 * backward of the guided style loss in one pass over z whatever R is (z viewed
 * [b][c][h][w], c <= 512, coef as stx_guided_style_loss writes it).  With both amax groups
 * (z_amax >= max|z|, coef_amax >= max|coef|) the products run on the fp16 hi/lo split
 * MFMA, else on the fp32 MFMA.  accumulate = 1 adds onto dz. */
int stx_guided_gram_bwd(const float* coef, const float* z, const float* wts, float* dz, int b,
                        int c, int h, int w, int R, const float* acc_scale_dev, int accumulate,
                        const float* z_amax, const float* coef_amax, void* stream);

/* Colour control -- Gatys et al. 2017, "Controlling Perceptual Factors in Neural Style
 * Transfer", section 5 (the reference project has no such feature).
 *
 * stx_color_stats: the statistics colour matching needs (section 5.2, "colour histogram
 * matching": the style image's RGB mean and covariance are mapped onto the content
 * image's), and from which luminance mean / variance follow (section 5.1).  x
 * [n][3][h][w]; stats receives 9 doubles per image: mean[3], then the upper triangle
 * [rr, rg, rb, gg, gb, bb] of the population covariance E[x x^T] - mu mu^T.  fp64
 * accumulation, a fixed block count per image and fixed-order sums: bit-reproducible, and
 * image k's result does not depend on n.  ws >= stx_color_stats_ws(n, h, w) bytes, 16-byte
 * aligned (0: unsupported dims; n <= 65535).  16-byte loads when h w % 4 == 0 and x is
 * 16-byte aligned, scalar loads otherwise. */
size_t stx_color_stats_ws(int n, int h, int w);
int stx_color_stats(const float* x, double* stats, int n, int h, int w, void* ws,
                    size_t ws_bytes, void* stream);
/* stx_color_affine: a 3x3 colour transform per pixel over [n][3][h][w],
 *   out[c] = clamp_c( base[c] + sum_d M[c][d] (x[d] - base[d]) + b[c] )
 * evaluated as t[d] = x[d] - base[d];  v = fma(M[c][0], t[0], b[c]);  v = fma(M[c][1],
 * t[1], v);  v = fma(M[c][2], t[2], v);  out[c] = base[c] + v, then min(max(., lo[c]),
 * hi[c]) -- bit-stable.  It serves the recolouring of the style image (section 5.2: M =
 * Sigma_c^1/2 Sigma_s^-1/2, b = mu_c - M mu_s), the luminance image of section 5.1 (M's
 * rows all the luma weights) and the luminance merge that gives the stylised luminance
 * the content's chroma (section 5.1; base = the content image: YIQ^-1 maps Y to (1,1,1),
 * so replacing base's luminance by x's adds the luminance difference to every channel).
 * base may be NULL (reads as zeros); b may be NULL (zeros); lo / hi are per-channel clamp
 * bounds, both NULL for no clamp.  M [3][3] row-major, b, lo, hi are HOST arrays read
 * before the call returns and passed as kernel arguments (a captured graph bakes them
 * in).  out may alias x or base. */
int stx_color_affine(const float* x, const float* base, float* out, int n, int h, int w,
                     const float* M, const float* b, const float* lo, const float* hi,
                     void* stream);

/* Sum-of-squared-difference reductions (ContentLoss / FeatureReconstructionLoss):
 *   s = sum((f(a) - f(b))^2), f = relu if relu_inputs else identity
 *   mode 0: *out = s / n                        (F.mse_loss, mean)
 *   mode 1: out[0] = (s / n)^2 / n, out[1] = s / n   (FeatureReconstructionLoss)
 *   mode 2: both from one pass (16-B aligned a, b; relu_inputs ignored):
 *           out[0] = mean((a-b)^2), out[1] = mean((relu a - relu b)^2)^2 / n,
 *           out[2] = mean((relu a - relu b)^2)   (content + feature at conv2_2)
 * grad (optional, mode 0): grad = gscale * 2*(a-b)/n.
 * A NaN in a or b makes the plain sums NaN; the relu'd sums (relu_inputs, mode 2's
 * out[1] / out[2]) read it as 0 (fmaxf), as the fp32 conv loaders above do. */
size_t stx_mse_ws(long long n);
int stx_mse(const float* a, const float* b, long long n, int relu_inputs, int mode,
            float* out, float* grad, float gscale, void* ws, size_t ws_bytes, void* stream);
/* grad (+)= s0 * (*s1) * (*s2) * (f(a) - f(b)) [* (a>0) if relu]; s1/s2 device scalars or NULL */
int stx_diff_scale(const float* a, const float* b, float* grad, long long n, float s0,
                   const float* s1_dev, const float* s2_dev, int relu, int accumulate,
                   void* stream);
/* Deferred Gram finalizes: what one finalize launch does (G, coef, loss partials, the
 * content MSE sums), as stx_style_loss fills it with a non-NULL `defer`.
 * stx_gram_finalize_batch then runs up to STX_FIN_MAX such finalizes -- the five StyleLoss
 * taps of a forward -- in ONE launch, block for block the same arithmetic (bit-identical to
 * the immediate finalize).  The loss partials land where stx_style_loss_parts says; reduce
 * them with stx_loss_finalize. */
#define STX_FIN_MAX 8
typedef struct stx_gram_fin_job {
  const float* parts;      /* partial slabs [b][ntiles][nsplit][64][64] */
  float* g_out;            /* optional G */
  const float* target;
  float* coef;
  float* loss_parts;
  const float* mse_parts;  /* fused content pass (or NULL) */
  float* mse_out;
  long long t_bstride;
  double mse_n;
  float scale, cA, alpha;
  int c, nsplit, b, cpad, mse_nparts;
  float* coef_amax;        /* optional amax group (zeroed): >= max|coef| over the batch */
} stx_gram_fin_job;
/* The style loss of one VGG tap, from exactly one of two sources:
 *   z      features [b][c][hw]; the Gram partials are formed here (z_amax as for stx_gram)
 *   parts  [b][U][nparts][64][64] partials a conv epilogue wrote (stx_conv_params.gram_part;
 *          c <= 64: U = 1, c == 128: U = 3 tiles), summed in a fixed order
 * and then G, the loss and the backward operator as above.  With the content companion
 * (the content tap, stransfer/network.py:155-164, 186-201) mse_out[3] receives what
 * stx_mse(z, content, b*c*hw, 0, 2, mse_out, ...) writes: from `content` [b][c][hw] with
 * z (in the Gram's pass over z where its kernel allows, c = 128 on the split path, else a
 * separate pass), or from `mse_parts` with parts (stx_conv_params.mse_parts: b * nparts
 * pairs), finalized by the same launch.  content / mse_parts present iff mse_out is.
 * ws >= stx_gram_ws(b, c, hw), or stx_style_content_ws(b, c, hw) with `content`.
 * loss == NULL leaves the loss partials in ws (stx_style_loss_parts).  defer == NULL: the
 * finalize runs in this call; else only the partial kernel(s) (if any) run, *defer
 * describes the finalize for stx_gram_finalize_batch, and loss must be NULL.  Malformed
 * structs are refused before any launch. */
size_t stx_style_content_ws(int b, int c, int hw);
typedef struct stx_style_loss_params {
  const float* z;          /* source: features ... */
  const float* parts;      /* ... or precomputed partials, */
  int nparts;              /*     this many per tile */
  const float* z_amax;     /* optional, with z */
  const float* target;     /* [c][c], or [b][c][c] with target_batched */
  int target_batched;
  float* g_out;            /* optional G [b][c][c] */
  float* coef;             /* optional A [b][cpad][cpad] */
  float* loss;             /* optional device scalar */
  int b, c, hw;
  float weight, diag_alpha;
  const float* content;    /* content companion with z ... */
  const float* mse_parts;  /* ... or with parts */
  float* mse_out;
  void* ws;
  size_t ws_bytes;
  stx_gram_fin_job* defer;
} stx_style_loss_params;
int stx_style_loss(const stx_style_loss_params* p, void* stream);
int stx_gram_finalize_batch(const stx_gram_fin_job* jobs, int njobs, void* stream);

/* *out = sum_i w_host[i] * s[i]   (k <= 16 device scalars, fixed order) */
int stx_loss_combine(const float* s, int k, const float* w_host, float* out, void* stream);

/* Vector kernels of the on-device L-BFGS (StyleNetwork.train_gatys' optimiser,
 * stransfer/network.py:435; torch.optim.LBFGS semantics):
 *   stx_vec_reduce: r = dot(a,b) (op 0), sum|a| (op 1) or max|a| (op 2) over n floats
 *     (fixed-order two-stage reduction, ws >= stx_vec_ws()), then
 *     *out = (add ? *add : 0) + sgn * r * (mul ? *mul : 1)   (device scalars)
 *   stx_vec_axpby: y = alpha*x + b*y, alpha = a_dev ? a_sgn * (*a_dev) * a : a
 *   stx_scalar_op: s[k] = s[i] op s[j]  (0 div, 1 mul, 2 sub, 3 add, 4 1/s[i],
 *     5 min(s[j], 1/s[i])) on a device scalar array */
size_t stx_vec_ws(void);
int stx_vec_reduce(const float* a, const float* b, long long n, int op, float* out,
                   const float* mul, const float* add, float sgn, void* ws, size_t ws_bytes,
                   void* stream);
int stx_vec_axpby(float* y, const float* x, long long n, float a, const float* a_dev,
                  float a_sgn, float b, void* stream);
int stx_scalar_op(float* s, int op, int i, int j, int k, void* stream);

/* L-BFGS in the compact form (lbfgs.hip): torch.optim.LBFGS's search direction, step
 * size and parameter update without line search (StyleNetwork.train_gatys,
 * stransfer/network.py:435-456; torch/optim/lbfgs.py's two-loop recursion) in a fixed
 * launch sequence whatever the history length.
 *   hist   [2][m + 1][npad] floats (stx_lbfgs_hist_bytes): S slots then Y slots, a ring
 *          of m committed pairs + one candidate; npad = n rounded up to 1024
 *   state  stx_lbfgs_state_bytes(m) bytes, zeroed by the caller before the first call:
 *          pair order, R = [s_i.y_j], Y^T Y, H_diag, t, torch's n_iter
 *   prev_g npad floats (the previous gradient)
 *   scal   >= 16 device floats the host reads: 0 loss, 1 max|g|, 2 sum|g|, 3 g.d, 4 t,
 *          5 max|t d|, 6 stop flag (g.d > -tol_change: x not moved), 7 y.s, 8 pairs,
 *          9 n_iter, 10 H_diag
 * stx_lbfgs_grad_stats (after each closure evaluation): scal[0] = *loss (if loss),
 *   scal[1] = max|g|, scal[2] = sum|g|; zeroes clear[0 .. clear_n).
 * stx_lbfgs_direction (one torch loop iteration up to the next closure): n_iter += 1;
 *   y = g - prev_g, s = t_prev d_prev, accept when y.s > 1e-10 (H_diag = y.s / y.y); t =
 *   min(1, 1/sum|g|) * lr on the first iteration, else lr; d = -H g; g.d; x += t d unless
 *   g.d > -tol_change.  1 <= m <= 256; 16-byte aligned vectors. */
size_t stx_lbfgs_state_bytes(int m);
size_t stx_lbfgs_hist_bytes(long long n, int m);
size_t stx_lbfgs_ws(long long n, int m);
int stx_lbfgs_direction(float* x, const float* g, float* prev_g, float* hist, long long n, int m,
                        float lr, float tol_change, void* state, float* scal, void* ws,
                        size_t ws_bytes, void* stream);
int stx_lbfgs_grad_stats(const float* g, long long n, const float* loss, float* scal, float* clear,
                         int clear_n, void* ws, size_t ws_bytes, void* stream);

/* MaxPool2d(2,2) on (optionally relu'd) input; idx = flat y*w+x argmax per plane,
 * torch CPU semantics (first max in row-major window order; NaN propagates, with
 * relu_input too: the ReLU keeps a NaN, as torch's, and idx points at the window's last
 * NaN). idx may be NULL.  Floor mode: an odd trailing row / column is never pooled. */
int stx_maxpool2x2_fwd(const float* x, float* y, long long* idx, int nc, int h, int w,
                       int relu_input, void* stream);
/* dx = scatter(dy at idx)  (dx fully written, gather form) */
int stx_maxpool2x2_bwd(const float* dy, const long long* idx, float* dx, int nc, int h, int w,
                       void* stream);
/* dz = unpool(dp) * (z > 0): backward of ReLU + MaxPool2d(2,2) with the argmax
 * recomputed from z (dz fully written; z is the pre-ReLU tensor [nc][h][w]).  A NaN z
 * is not positive: dz = 0 there, as torch's backward gives (the argmax search ranks it
 * as 0). */
int stx_relupool_bwd(const float* dp, const float* z, float* dz, int nc, int h, int w,
                     void* stream);
/* y = x <= 0 ? +0 : x -- a NaN stays NaN, as torch.relu keeps it */
int stx_relu_fwd(const float* x, float* y, long long n, void* stream);
/* dx = dy * (y > 0): 0 at a NaN y, as torch's threshold backward */
int stx_relu_bwd(const float* dy, const float* y, float* dx, long long n, void* stream);

/* Adam (torch.optim.Adam semantics, in place).  Any 4-byte aligned buffers are accepted:
 * with p, g, m and v all 16-byte aligned the kernel moves 16 bytes per access, otherwise
 * one float (the two forms agree to rounding, not bit for bit).
 * step_dev: device int32 step counter, incremented on the device by every call so
 * a captured graph replays correctly.  ws: stx_adam_ws() bytes of device scratch. */
size_t stx_adam_ws(void);
int stx_adam_step(float* p, const float* g, float* m, float* v, long long n, float lr,
                  float beta1, float beta2, float eps, int* step_dev, void* ws, void* stream);
/* the same, and zeroes clear[0 .. clear_n) in the step-counter launch (the Gatys
 * engine's per-iteration amax groups, which are next produced by the following
 * iteration's forward): one launch fewer per iteration than a separate fill. */
int stx_adam_step_clear(float* p, const float* g, float* m, float* v, long long n, float lr,
                        float beta1, float beta2, float eps, int* step_dev, void* ws,
                        float* clear, int clear_n, void* stream);
/* the second half alone: the update with the scalars a prepare rider
 * (stx_conv_weight_compose16_tail) left in ws for this step, in one launch that also zeroes
 * clear[0 .. clear_n).  p, m and v end as stx_adam_step_clear leaves them. */
int stx_adam_step_prepared(float* p, const float* g, float* m, float* v, long long n, float beta1,
                           float beta2, float eps, const void* ws, float* clear, int clear_n,
                           void* stream);

/* InstanceNorm2d(affine) forward, per (n,c) plane over hw (biased var, eps):
 *   u = x (+ res);  y = (u-mean)*rstd*gamma + beta, formed as fma(u, gsc, sh) with
 *   gsc = gamma rstd, sh = fma(-mean, gsc, beta);  y = (y <= 0 ? +0 : y) if relu.
 * mean/rstd [n*c] saved for the backward (may be NULL).  out_amax (amax group, zeroed
 * by the caller, may be NULL) receives max|y| -- the next split conv's input scale.
 * x, res and y must be 16-byte aligned (STX_E_INVALID otherwise).
 * A NaN or Inf anywhere in a plane of u makes that plane's mean NaN (Inf for +-Inf
 * alone), its rstd, gsc and sh NaN and so every y of the plane, with relu too: the ReLU
 * keeps a NaN, as torch's and stx_relu_fwd (fmaxf(NaN, 0) = 0 would hand on a clean
 * zero plane with out_amax = 0), and out_amax then holds a NaN.  The other planes of the call
 * are untouched, bit for bit.  The 64^2 planes that share a block (n*c a multiple of 4,
 * from 1024 planes) have the bits of the same planes computed one per block. */
int stx_instnorm_fwd(const float* x, const float* res, const float* gamma, const float* beta,
                     float* y, float* mean, float* rstd, int n, int c, int hw, float eps,
                     int relu, float* out_amax, void* stream);
/* backward: dy = grad wrt y; beta = the forward's beta (NULL if none).  With relu the
 * mask y > 0 is recomputed from u = x (+ res), mean, rstd, gamma and beta exactly as the
 * forward formed y (y = fma(u, gsc, sh), gsc = gamma rstd, sh = fma(-mean, gsc, beta):
 * the same bits), so y itself is not read.  du = grad wrt u (= grad of x and of res).  dgamma/dbeta (may be NULL) (+)= sums over n (fixed order).  dbias_in
 * (may be NULL) (+)= sum_{n,p} du: the bias gradient of the conv that produced x
 * (stransfer/network.py:471-611, every Conv2d followed by InstanceNorm2d), so that
 * conv needs no separate bias-gradient pass.  out_amax (amax group or NULL) receives
 * max|du| -- the split dgrad/wgrad scale of du.
 * A NaN in dy of a plane (at an element the ReLU lets through) makes the plane's sums
 * NaN and so its whole du, its three partials, its channel of dgamma / dbeta / dbias_in
 * and out_amax; the other planes and channels are untouched, bit for bit.  A NaN (or
 * Inf) in x reaches the backward through the saved mean / rstd, both NaN: the recomputed
 * mask !(NaN > 0) zeroes g on the whole plane, but k = gamma rstd / hw is NaN and every
 * du of the plane is NaN, with and without relu (not 0, unlike stx_relu_bwd at a NaN y:
 * the plane has no finite statistics to differentiate through). */
size_t stx_instnorm_bwd_ws(int n, int c);
/* The parameter reductions of many stx_instnorm_bwd calls in one launch: each such
 * call ran with dgamma = dbeta = dbias_in = NULL into its own workspace `parts`
 * (>= stx_instnorm_bwd_ws(n, c) bytes, kept until this call); each job then writes /
 * accumulates its dgamma, dbeta, dbias_in (any may be NULL) with the same fixed-order
 * sums over n -- one launch per training step instead of one per InstanceNorm2d
 * layer (stransfer/network.py:474-600, 15 layers in ImageTransformNet). */
#define STX_PGRAD_MAX 32
typedef struct stx_in_pgrad_job {
  const float* parts;
  float* dgamma;
  float* dbeta;
  float* dbias_in;
  int n, c, accumulate, pad_;
} stx_in_pgrad_job;
int stx_instnorm_param_grads(const stx_in_pgrad_job* jobs, int njobs, void* stream);
int stx_instnorm_bwd(const float* dy, const float* beta, const float* x, const float* res,
                     const float* gamma, const float* mean, const float* rstd, float* du,
                     float* dgamma, float* dbeta, float* dbias_in, int n, int c, int hw, int relu,
                     int accumulate_params, float* out_amax, void* ws, size_t ws_bytes,
                     void* stream);

/* Conditional instance norm (Dumoulin et al., "A Learned Representation for Artistic
 * Style"): N styles share one network; only the IN affine rows are per style, tables
 * gtab / btab [S][c] per layer.  The IN kernels above index their affine vectors by
 * plane % c only, so a per-sample affine [n][c] is stx_instnorm_fwd/bwd called with
 * (n = 1, c = n*c) -- same kernel selection, speed and bits.  Two launches per step
 * serve every IN layer (one job each); mix [n][S] holds each sample's style weights
 * (a one-hot row selects a style, a convex row blends).
 *   stx_cin_mix:  gamma_n[k][ch] = sum_s mix[k][s] gtab[s][ch] (beta_n from btab), an
 *     fma chain from 0 with s ascending: a one-hot row reproduces the table row's bits.
 *     Needs gtab, btab, gamma_n, beta_n.
 *   stx_cin_param_grads:  from the layer's stx_instnorm_bwd partials `parts` [n*c][3]
 *     (that call ran with (1, n*c) and dgamma = dbeta = dbias_in = NULL into its own
 *     workspace),  dgtab[s][ch] (+)= sum_k mix[k][s] parts[k][ch][0],  dbtab likewise
 *     from [1],  dbias_in[ch] (+)= sum_k parts[k][ch][2];  k ascending, the order of
 *     stx_instnorm_param_grads (all samples on one style: that row has its sums' bits,
 *     the other rows get 0).  Needs parts; dgtab, dbtab, dbias_in may be NULL. */
#define STX_CIN_MAX 32
typedef struct stx_cin_job {
  const float* gtab;
  const float* btab; /* [S][c] style tables */
  float* gamma_n;
  float* beta_n;      /* mix: out [n][c] */
  const float* parts; /* grads: the layer's stx_instnorm_bwd partials [n*c][3] */
  float* dgtab;
  float* dbtab;    /* grads: [S][c], any may be NULL */
  float* dbias_in; /* grads: [c] (producing conv's bias), may be NULL */
  int c, accumulate;
} stx_cin_job;
int stx_cin_mix(const stx_cin_job* jobs, int njobs, const float* mix, int n, int S,
                void* stream);
int stx_cin_param_grads(const stx_cin_job* jobs, int njobs, const float* mix, int n, int S,
                        void* stream);

/* Adaptive instance normalisation (Huang & Belongie 2017, "Arbitrary Style Transfer in
 * Real-time with Adaptive Instance Normalization"): a style given at conversion time.
 * Planes are x [n][c][hw] fp32 with hw >= 2; statistics are per plane,
 *   mean = sum x / hw,   std = sqrt(sum (x - mean)^2 / (hw - 1) + eps)
 * (unbiased variance, eps inside the root: the paper's calc_mean_std, NOT the biased rstd
 * of stx_instnorm_fwd).  The deviations are taken about the computed mean, in a second pass
 * inside the block.  One block per plane and fixed-order reductions: bit-reproducible.
 * Every entry point below forms the statistics with the same code under the same kernel
 * selection (by hw, hw % 4 and the 16-byte alignment of x alone), so the same plane has the
 * same mean / std bits whichever of them computed it.  No alignment contract: an unaligned
 * x or an hw % 4 != 0 takes the loop kernels.  None of these allocates or synchronises;
 * arguments are checked before any launch (STX_E_INVALID; hw >= 2, hw <= 2^30, n c < 2^31).
 *
 * stx_chan_stats: mean, std [n][c] of x, or with relu_input of (x <= 0 ? +0 : x), which
 *   keeps a NaN as stx_relu_fwd does (a tap read from the conv output before its ReLU).
 *   A NaN or Inf in a plane makes that plane's mean and std NaN; no other plane is touched.
 *
 * stx_adain: style statistics smean, sstd [S][c], mix [n][S], strength alpha:
 *     M = sum_s mix[k][s] smean[s][ch],  G = sum_s mix[k][s] sstd[s][ch]   (fma chains from
 *         0, s ascending, as stx_cin_mix: a one-hot row reproduces the table row's bits)
 *     r = G / std,  a = fma(alpha, r, 1 - alpha),  b = alpha * fma(-r, mean, M)
 *     y = fma(x, a, b)
 *   alpha = 1 with a one-hot row is the paper's AdaIN; alpha = 0 gives a = 1, b = 0 and
 *   y = x in value; a convex row is the paper's style interpolation (the blend is linear in
 *   (smean, sstd)).  mean, std [n][c] (may be NULL) receive the content statistics, with
 *   stx_chan_stats' bits.  out_amax (amax group, zeroed by the caller, may be NULL) receives
 *   max|y|, the next split conv's input scale.  y may be x.  Planes of up to 65536 floats
 *   with hw % 4 == 0 and an aligned x are read once.
 *   A NaN or Inf in a plane of x, or a NaN in that plane's row of mix or channel of the
 *   tables, makes its mean, std and every y of the plane NaN (at alpha = 0 too: b is
 *   0 * NaN), and out_amax then holds a NaN; the other planes are untouched, bit for bit.
 *
 * stx_stats_loss: against targets tmean, tstd [n][c],
 *     out[1] = weight / (n c) * sum_{n,c} (mean - tmean)^2,  out[2] likewise of the stds,
 *     out[0] = out[1] + out[2];   *add_to += out[0] when add_to is given.
 *   The per-plane squares go to the workspace and one block sums them in a fixed order.
 *   mean, std [n][c] (may be NULL) are saved for the backward.  A NaN or Inf in any plane
 *   makes that plane's saved mean and std NaN and all of out NaN; the other planes' saved
 *   statistics are untouched, bit for bit.
 *
 * stx_stats_loss_bwd: from the saved mean, std,
 *     dx_i (+)= A + B (x_i - mean),  A = kk 2 (mean - tmean) / hw,
 *     B = kk 2 (std - tstd) / ((hw - 1) std),  kk = weight / (n c) * (*g_dev or 1),
 *   formed as fma(B, x_i - mean, A): one streaming pass, A and B once per block.  With
 *   accumulate the term is added to dx, and where the term is 0 the old value stays bit for
 *   bit (a tap's gradient joins the one arriving from deeper layers without another pass).
 *   out_amax (may be NULL) receives max|dx| as stored.  A plane whose saved statistics are
 *   NaN gets a NaN dx throughout; a NaN x_i alone (statistics given from elsewhere) makes
 *   that element NaN; the other planes are untouched, bit for bit. */
int stx_chan_stats(const float* x, float* mean, float* std_, int n, int c, int hw, float eps,
                   int relu_input, void* stream);
int stx_adain(const float* x, const float* smean, const float* sstd, const float* mix,
              float alpha, float* y, float* mean, float* std_, int n, int c, int hw, int S,
              float eps, float* out_amax, void* stream);
size_t stx_stats_loss_ws(int n, int c);
int stx_stats_loss(const float* x, const float* tmean, const float* tstd, int n, int c, int hw,
                   float eps, float weight, float* out, float* add_to, float* mean, float* std_,
                   void* ws, size_t ws_bytes, void* stream);
int stx_stats_loss_bwd(const float* x, const float* mean, const float* std_, const float* tmean,
                       const float* tstd, int n, int c, int hw, float weight, const float* g_dev,
                       float* dx, int accumulate, float* out_amax, void* stream);

/* nearest x2 upsample: y [nc][2h][2w];  backward dx[y][x] = sum of dy's 2x2 block */
int stx_upsample2x_fwd(const float* x, float* y, int nc, int h, int w, void* stream);
int stx_upsample2x_bwd(const float* dy, float* dx, int nc, int h, int w, void* stream);

/* Total variation, batch SUM (stransfer/network.py:621-641):
 *   *loss = factor*(sum|y[..,x]-y[..,x+1]| + sum|y[..,y,:]-y[..,y+1,:]|)
 *   grad (optional) = gscale * (*gscale_dev or 1) * d loss / dy */
size_t stx_tv_ws(int n, int c, int h, int w);
int stx_tv_loss(const float* y, float* loss, float* grad, float gscale, const float* gscale_dev,
                int n, int c, int h, int w, float factor, void* ws, size_t ws_bytes,
                void* stream);

/* Temporal loss of the video network (VideoTransformNet.get_temporal_loss,
 * stransfer/network.py:885-903), Frobenius norms over the whole batch:
 *   out[0] = ||y - y_old|| / (||x - x_old|| + 1) * weight,  out[1] = ||y - y_old||,
 *   out[2] = ||x - x_old||   (one streaming pass, fixed-order reduction)
 * Backward: grad (+)= (*g_dev or 1) * weight / ((out[2] + 1) * out[1]) * (y - y_old)
 * (0 where out[1] == 0, torch's norm backward); fwd = the forward's out.
 * All four tensors hold n floats, 16-byte aligned. */
size_t stx_temporal_loss_ws(void);
int stx_temporal_loss(const float* y, const float* y_old, const float* x, const float* x_old,
                      long long n, float weight, float* out, void* ws, size_t ws_bytes,
                      void* stream);
int stx_temporal_loss_bwd(const float* y, const float* y_old, long long n, const float* fwd,
                          float weight, const float* g_dev, float* grad, int accumulate,
                          void* stream);

/* Temporal consistency of optimisation-based video transfer (Ruder, Dosovitskiy & Brox 2016,
 * "Artistic Style Transfer for Videos").  Images and flows are NCHW fp32 with h, w >= 2; a
 * flow is [n][2][h][w], channel 0 the column displacement dx, channel 1 the row
 * displacement dy, in pixels.
 *
 * stx_flow_warp: out[b][k][i][j] = src[b][k] sampled bilinearly at y = i + flow[b][1][i][j],
 * x = j + flow[b][0][i][j] (fp32, one rounding each).
 *   valid = 0 <= y <= h-1 and 0 <= x <= w-1, compared on the fp32 coordinates as computed:
 *           a NaN or infinite coordinate is invalid.
 *   y0 = min(floor(y), h-2), y1 = y0 + 1, fy = y - y0 (likewise x); the taps' weights are
 *   (1-fy)(1-fx), (1-fy)fx, fy(1-fx), fy fx, computed once per pixel and reused over the c
 *   channels; the value is w00 a00 + w01 a01 + w10 a10 + w11 a11 as one product and three
 *   fmaf in that order (seven roundings at most: three on a weight, four in the sum).
 *   All four taps enter the sum, so a NaN tap makes the pixel NaN even under a zero weight.
 *   An invalid pixel reads no tap: out = fill[b][k][i][j] if fill is given, else +0.
 *   valid (optional) [n][h][w] receives 1.0f / 0.0f.  out must not overlap src; n <= 65535.
 *
 * stx_flow_consistency: cmask [n][h][w] = 1.0f where the pixel of frame t has a consistent
 * source in frame t-1, else 0.0f.  With w^ = bwd at the pixel and w~ = fwd warped by bwd
 * (stx_flow_warp's arithmetic), the pixel is
 *   occluded  if |w~ + w^|^2 > 0.01 (|w~|^2 + |w^|^2) + 0.5
 *   boundary  if |grad u^|^2 + |grad v^|^2 > 0.01 |w^|^2 + 0.002
 * (grad: central difference halved in the interior, one-sided and unhalved in the first
 * and last row and column), and cmask = valid and not occluded and not boundary.  A NaN on
 * either side of a comparison makes it false: a NaN in bwd at the pixel makes it invalid
 * (0), one in a neighbour's bwd or in a tap of fwd only silences the test it enters.
 *
 * stx_masked_mse: x, ref [n][c][hw], mask [n][hw] shared by the c channels:
 *   out[0] = weight / (n c hw) * sum over mask != 0 of (x - ref)^2
 *   grad (optional) = or += 2 weight / (n c hw) * (x - ref) where mask != 0
 * One streaming pass (512 blocks, fixed assignment) and a one-block finalize in a fixed
 * order: bit-reproducible.  The finalize also does *add_to += out[0] when add_to is given.
 * The mask selects: where mask == 0 nothing of x or ref reaches the loss or the gradient
 * (not a NaN either); grad is then written +0, or with accumulate left as it is, bit for
 * bit.  A NaN in the mask selects the pixel.  A NaN in x or ref under a set mask makes the
 * loss and that gradient element NaN.  Bases that are 16-byte aligned with hw % 4 == 0
 * take float4 accesses, anything else the scalar loop: the same values up to the order of
 * the per-thread sums.  n c hw < 2^31.
 *
 * stx_flow_compose: the per-frame set-up of the long-term consistency loss (their eq. 9 and
 * 10) in one launch.  prev, fwd, bwd are HOST arrays of count device pointers, 1 <= count
 * <= 4, nearest frame first: prev[q] [n][c][h][w] an earlier result, fwd[q] and bwd[q]
 * [n][2][h][w] the flows between that frame and this one (bwd[q] maps this frame onto it).
 * The arrays are read before the call returns and travel in the kernel's arguments: no
 * device table, capturable.  Per pixel, for q = 0 .. count-1 in order, stx_flow_consistency's
 * predicate is evaluated on (fwd[q], bwd[q]) (the same device function); the first q for
 * which it holds is selected and no later offset is looked at (it reads no flow, no tap):
 *   ref = init = stx_flow_warp's value of prev[q] along bwd[q], cmask = 1.0f, which = q.
 * If none holds: cmask = 0.0f, which = 255, ref = +0 and init = stx_flow_warp(prev[0],
 * bwd[0], fill).  With 0/1 masks the long-term masks max(c^j - sum_{k<j} c^k, 0) are
 * mutually exclusive, so sum_j stx_masked_mse(x, warp_j, c_long^j) with one weight equals
 * stx_masked_mse(x, ref, cmask).  At count = 1, (cmask, init) are stx_flow_consistency's and
 * stx_flow_warp(fill)'s bit for bit, and ref is stx_flow_warp's under the mask.  A NaN in
 * bwd[q] at the pixel makes offset q inconsistent there; one in prev[q] at a tap of a
 * selected pixel makes ref and init NaN, at an unselected offset it reaches nothing.
 * fill [n][c][h][w] is required; init and which [n][h][w] may be NULL.  ref, cmask, init
 * must not overlap an input or each other.
 *
 * None of these allocates or synchronises; arguments are checked before any launch. */
int stx_flow_compose(const float* const* prev, const float* const* fwd,
                     const float* const* bwd, int count, const float* fill, float* ref,
                     float* cmask, float* init, unsigned char* which, int n, int c, int h, int w,
                     void* stream);
int stx_flow_warp(const float* src, const float* flow, const float* fill, float* out,
                  float* valid, int n, int c, int h, int w, void* stream);
int stx_flow_consistency(const float* fwd, const float* bwd, float* cmask, int n, int h, int w,
                         void* stream);
size_t stx_masked_mse_ws(void);
int stx_masked_mse(const float* x, const float* ref, const float* mask, int n, int c, int hw,
                   float weight, float* out, float* add_to, float* grad, int accumulate,
                   void* ws, size_t ws_bytes, void* stream);

/* Image conditioning (img_utils.image_loader_transform, stransfer/img_utils.py:13-44)
 * of a batch of decoded 8-bit RGB images on the GPU: centre crop, Pillow-exact
 * BILINEAR resize to size x size (its 8-bit fixed-point two-pass resampler: output
 * bytes equal PIL's), ToTensor (/255) and (x - mean) / std -> out [b][3][size][size].
 * src: device buffer of packed HWC uint8 images; meta: device array of b entries;
 * coef: device int tables, per axis [out][2] bounds (first tap, taps) followed by
 * [out][k] coefficients, built with stx_resample_coeffs (host function: returns the
 * kernel size k, or with NULL outputs only the size query); mean/std: HOST arrays
 * of 3; tmp: device workspace holding every image's horizontally resampled rows
 * (max_rows = the largest y1 - y0; 0 when no image needs the horizontal pass). */
typedef struct {
  long long offset;        /* byte offset of the image in src */
  int h, w;                /* decoded size */
  int top, left;           /* centre-crop origin */
  int y0, y1;              /* crop rows read by the vertical pass */
  int resize_w, resize_h;  /* passes needed (0: the crop side already equals size) */
  int xcoef, ycoef;        /* int offsets of the two axis tables in coef */
  int xk, yk;              /* their kernel sizes */
  long long tmp_offset;    /* byte offset of this image's rows in tmp ([rows][size][3]) */
} stx_image_meta;
int stx_resample_coeffs(int in_size, int out_size, int* bounds, int* kk, int kk_stride);
int stx_image_condition(const void* src, const stx_image_meta* meta, int b, int max_rows,
                        const int* coef, int size, const float* mean, const float* std_,
                        float* out, void* tmp, size_t tmp_bytes, void* stream);

/* JPEG decode split between host and GPU: the host parses the markers and Huffman-decodes
 * the scan into quantised DCT coefficients, the GPU dequantises, runs libjpeg's "islow"
 * integer IDCT, upsamples the chroma ("fancy" triangle filter) and converts YCbCr to RGB,
 * into the packed HxWx3 uint8 layout stx_image_condition reads.  The output bytes equal
 * libjpeg's (and so Pillow's) exactly.
 *
 * The two host functions are plain C++ (no GPU is opened) and return an STX_JPEG_* status.
 * Decoded here: SOF0 / SOF1 (sequential Huffman), 8 bits, one interleaved scan, 1 component
 * or 3 (YCbCr) with 1x1 chroma and luma sampling 1x1, 2x1 or 2x2, restart intervals, any
 * 8-bit DQT / DHT.  Everything else -- progressive, arithmetic, lossless, 4 components, an
 * Adobe transform other than YCbCr, RGB component ids, 16-bit quantisation tables, other
 * samplings, several scans, bytes that are no JPEG -- is STX_JPEG_UNSUPPORTED.  A stream
 * that ends early, holds a bad Huffman code, a wrong or misplaced restart marker, a run
 * past coefficient 63, an undefined table or no EOI after the scan is STX_JPEG_CORRUPT.
 * Neither function reads past len or writes past coef_bytes.
 *
 * The info query fills a stx_jpeg_desc: size, components, sampling factors, the block grid
 * of each component padded to whole MCUs (bw x bh blocks) and coef_bytes =
 * sum_c bw[c] bh[c] 128.  The entropy decode writes the coefficients as int16 in natural
 * (row-major, de-zigzagged) order, component after component, each in block-raster order
 * over its padded grid, and one uint16[64] quantisation table per component (natural
 * order) to qtab [ncomp][64]; coef_bytes below the need is STX_JPEG_BAD_ARGS. */
#define STX_JPEG_OK 0
#define STX_JPEG_UNSUPPORTED 1
#define STX_JPEG_CORRUPT 2
#define STX_JPEG_BAD_ARGS 3
typedef struct {
  int status;              /* the STX_JPEG_* status the query returned */
  int h, w, ncomp;
  int hs[3], vs[3];        /* sampling factors (a lone component reports 1x1) */
  int bw[3], bh[3];        /* blocks per row / per column of the padded grid */
  int restart_interval;    /* MCUs between restart markers, 0: none */
  long long coef_bytes;
} stx_jpeg_desc;
int stx_jpeg_info(const void* data, size_t len, stx_jpeg_desc* info);
int stx_jpeg_entropy_decode(const void* data, size_t len, short* coef, size_t coef_bytes,
                            unsigned short* qtab);

/* The device stage for a batch.  jobs is a HOST array (read during the call, passed to the
 * kernels by value); coef_base, rgb_base and tmp are device buffers, 16-byte aligned.
 * Per job: a raw one copies h w 3 bytes from coef_base + coef_offset to rgb_base +
 * rgb_offset.  Otherwise (a) every 8x8 block is dequantised, inverse-transformed (columns
 * first, CONST_BITS 13, PASS1_BITS 2, descale by 11 then 18 with round-half-up) and written
 * as clamp(v + 128, 0, 255) to the component's plane in tmp ((8 bh) rows of (8 bw) bytes,
 * component after component from tmp_offset), then (b) each of the h x w pixels takes Y and
 * the chroma upsampled from planes cut to ceil(w / hmax) x ceil(h / vmax):
 *   2x1: even = (3 c + left + 1) >> 2, odd = (3 c + right + 2) >> 2, the first and last
 *        output of a row the sample itself;
 *   2x2: s = 3 c + the vertically nearer neighbour row (edge rows replicated), even =
 *        (3 s + s_left + 8) >> 4, odd = (3 s + s_right + 7) >> 4, first column (4 s + 8) >> 4,
 *        last (4 s + 7) >> 4;
 * and R = Y + ((91881 Cr' + 32768) >> 16), B = Y + ((116130 Cb' + 32768) >> 16),
 * G = Y + ((-22554 Cb' - 46802 Cr' + 32768) >> 16), Cb' = Cb - 128, Cr' = Cr - 128, clamped
 * to 0..255; one component writes Y three times.  int32 arithmetic that wraps: coefficients
 * no conforming encoder produces give unspecified pixels, never a fault.
 *
 * Checked before any launch (STX_E_INVALID): sizes 1..65535, ncomp, the sampling, bw / bh
 * equal to the padded grid of (h, w, hmax, vmax), offsets non-negative and 16-byte
 * aligned, every job's planes inside tmp_bytes (STX_E_WORKSPACE).  The caller guarantees
 * that the coefficient, table and pixel ranges lie inside coef_base and rgb_base.  Two
 * launches per 32 jobs; no allocation, no synchronisation.
 *
 * The layout query gives (size, last-member offset) of stx_jpeg_desc and stx_jpeg_job, as
 * stx_abi_layout does for the older structs. */
typedef struct {
  long long rgb_offset;    /* bytes: the h x w x 3 output in rgb_base */
  long long coef_offset;   /* bytes: component 0's blocks in coef_base, the others follow
                              (raw: the h w 3 pixels) */
  long long qtab_offset;   /* bytes: ncomp uint16[64] tables in coef_base */
  long long tmp_offset;    /* bytes: the component planes in tmp */
  int h, w;
  int ncomp;               /* 1 or 3 */
  int raw;                 /* non-zero: copy pixels through */
  int hmax, vmax;          /* luma sampling: 1x1, 2x1 or 2x2 */
  int bw[3], bh[3];        /* the padded block grids */
} stx_jpeg_job;
#define STX_JPEG_CHUNK 32  /* jobs per launch */
int stx_jpeg_decode_batch(const stx_jpeg_job* jobs, int njobs, const void* coef_base,
                          void* rgb_base, void* tmp, size_t tmp_bytes, void* stream);
int stx_jpeg_layout(long long* out, int n);

/* JPEG encode, the decode's mirror: the GPU converts RGB to YCbCr, downsamples the chroma,
 * runs libjpeg's "islow" integer forward DCT and quantises; the host only Huffman-codes.
 * The files equal what libjpeg (and so Pillow, optimize=False) writes, byte for byte.
 *
 * Host (plain C++, STX_JPEG_* status).  The quantisation tables of a quality: the Annex K
 * tables scaled as libjpeg does (quality clamped to 1..100, scale = q < 50 ? 5000 / q :
 * 200 - 2 q, entry = clamp((base scale + 50) / 100, 1, 255)) to qtab [2][64], natural order,
 * luma then chroma.  The bound is an upper limit of the file size, 0 for arguments the
 * encoder does not take.  The entropy encode writes a complete baseline JFIF file from
 * coefficients in exactly the layout stx_jpeg_entropy_decode writes (int16, natural order,
 * component after component, block raster over the MCU-padded grid) and qtab [ncomp][64]
 * (tables 1 and 2 must be equal): SOI, APP0 JFIF 1.01 (units 0, density 1x1), one 8-bit DQT
 * per table, SOF0 (ids 1 2 3, tq 0 1 1), DHT DC0 AC0 DC1 AC1 (the Annex K tables; one
 * component: DQT 0, DC0, AC0 only), SOS, the interleaved scan without restart markers, the
 * last byte padded with 1-bits, EOI.  ncomp 1, or 3 with luma sampling 1x1, 2x1 or 2x2.
 * STX_JPEG_BAD_ARGS, *len = 0 and nothing written past cap when cap is below the need,
 * coef_bytes below the grid, a DC difference outside +-2047, an AC value outside +-1023, a
 * table entry outside 1..255 or an unsupported sampling. */
int stx_jpeg_quant_tables(int quality, unsigned short* qtab);
size_t stx_jpeg_encode_bound(int h, int w, int ncomp, int hmax, int vmax);
int stx_jpeg_entropy_encode(const short* coef, size_t coef_bytes, int h, int w, int ncomp,
                            int hmax, int vmax, const unsigned short* qtab, void* out,
                            size_t cap, size_t* len);

/* The device stage of the encode for a batch; the conventions are stx_jpeg_decode_batch's
 * (host job array passed by value, STX_JPEG_CHUNK jobs per launch, everything checked
 * before any launch, no allocation, no synchronisation).  src_base, coef_base and tmp are
 * device buffers, 16-byte aligned.  A job's source is packed h x w x 3 (ncomp 1: h x w)
 * uint8, or (fp32 non-zero, ncomp 3) planar float [3][h][w] normalised with mean / std_:
 *   v = x * std_ + mean (two fp32 roundings, no fma) clamped to [0, 255],
 *   byte = min((int)(v * 255.0f), 255)
 * -- img_utils.to_pil's byte wherever v * 255 < 256; above that to_pil wraps through an
 * out-of-range float -> uint8 cast and this saturates (the one deliberate difference).
 * (a) Colour and downsampling, to planes in tmp ((8 bh) rows of (8 bw) bytes, component
 * after component from tmp_offset):
 *   Y  = (19595 R + 38470 G + 7471 B + 32768) >> 16
 *   Cb = (-11059 R - 21709 G + 32768 B + 8388608 + 32767) >> 16
 *   Cr = (32768 R - 27439 G - 5329 B + 8388608 + 32767) >> 16
 * source columns past w - 1 replicate column w - 1 and source rows past h - 1 row h - 1
 * inside a row group; chroma is downsampled 2x2 as (a00 + a01 + a10 + a11 + bias) >> 2 (bias
 * 1 on even output columns, 2 on odd) or 2x1 as (a0 + a1 + bias) >> 1 (bias 0 / 1), and the
 * downsampled rows past ceil(h / vmax) - 1 replicate that row.
 * (b) One thread per 8x8 block of the padded grid.  A block inside the component's real
 * extent (ceil(ceil(w hs / hmax) / 8) x ceil(ceil(h vs / vmax) / 8) blocks) runs jfdctint.c's
 * islow on sample - 128 (rows first, CONST_BITS 13, PASS1_BITS 2, DESCALE(x, n) =
 * (x + (1 << (n - 1))) >> n) and quantises a = (|c| + 4 q) / (8 q) with the sign restored.
 * A dummy block (outside the real extent) has zero AC and the quantised DC of the previous
 * block of its component in MCU order, formed from the sum of that block's samples.
 * Coefficients go to coef_base + coef_offset in the layout the entropy encode reads; the
 * two tables are read from coef_base + qtab_offset (uint16 [2][64], natural order).
 *
 * Checked before any launch (STX_E_INVALID): sizes 1..65535, ncomp, the sampling, fp32 only
 * with 3 components, bw / bh equal to the padded grid, offsets non-negative and 16-byte
 * aligned, the planes inside tmp_bytes (STX_E_WORKSPACE).  The caller guarantees the
 * source, table and coefficient ranges.  Two launches per 32 jobs.
 * The layout query gives (size, last-member offset) of stx_jpeg_enc_job. */
typedef struct {
  long long src_offset;    /* bytes: the source image in src_base */
  long long coef_offset;   /* bytes: component 0's blocks in coef_base, the others follow */
  long long qtab_offset;   /* bytes: uint16 [2][64] luma and chroma tables in coef_base */
  long long tmp_offset;    /* bytes: the component planes in tmp */
  int h, w;
  int ncomp;               /* 1 or 3 */
  int fp32;                /* non-zero: planar normalised float source */
  int hmax, vmax;          /* luma sampling: 1x1, 2x1 or 2x2 */
  int bw[3], bh[3];        /* the padded block grids */
  float mean[3], std_[3];  /* fp32 source: per-channel de-normalisation */
} stx_jpeg_enc_job;
int stx_jpeg_encode_batch(const stx_jpeg_enc_job* jobs, int njobs, const void* src_base,
                          void* coef_base, void* tmp, size_t tmp_bytes, void* stream);
int stx_jpeg_enc_layout(long long* out, int n);

/* fp32 separable resampling (scale control, Gatys et al. 2017 section 6: the pyramid levels
 * of a coarse-to-fine transfer): [nc][hi][wi] planes to [nc][ho][wo], antialiased, half-pixel
 * centres -- the semantics of torch.nn.functional.interpolate(mode = "bilinear" | "bicubic",
 * align_corners = False, antialias = True).
 *
 * Per axis, scale = in / out, s = max(scale, 1), radius 1 (triangle) or 2 (cubic, Keys
 * a = -0.5), support = radius s, and for output i the centre c = scale (i + 0.5):
 *   first = max(0, int(c - support + 0.5)),  end = min(in, int(c + support + 0.5)),
 *   w_j = f((j - c + 0.5) / s) for j in [first, end), divided by their sum
 * (fp64, rounded to fp32 once).
 *
 * stx_resample_plan (HOST function, needs no GPU) fills first[out], count[out] and
 * w[out][k] (zero padded) and returns the largest tap count, which k must be at least;
 * with first = count = w = NULL it only returns that count.  On a bad argument it returns
 * -STX_E_INVALID (a count can exceed any error code; the sign tells them apart).
 *
 * stx_resample2d: a horizontal pass into the workspace, then a vertical pass; the tables
 * are DEVICE copies of a plan's arrays (x: wi -> wo, y: hi -> ho).  An axis whose size does
 * not change is skipped and its tables may be NULL; an identity resize is an exact copy.
 * Each output is an fmaf chain over its taps in ascending order from w0 x0: bit-reproducible
 * and independent of nc.  y must not overlap x.  nc <= 65535, every side <= 4096. */
#define STX_FILTER_TRIANGLE 0
#define STX_FILTER_CUBIC 1
int stx_resample_plan(int in_size, int out_size, int filter, int* first, int* count, float* w,
                      int k);
size_t stx_resample2d_ws(int nc, int hi, int wi, int ho, int wo);
int stx_resample2d(const float* x, float* y, int nc, int hi, int wi, int ho, int wo,
                   const int* xfirst, const int* xcount, const float* xw, int xk,
                   const int* yfirst, const int* ycount, const float* yw, int yk, void* ws,
                   size_t ws_bytes, void* stream);

/* Dense optical flow between two conditioned frames (the input of the flow entry points
 * above): coarse-to-fine Horn-Schunck with warping, relaxed by Jacobi iterations.  For
 * frames A, B [n][3][h][w], h, w >= 2, the estimate f [n][2][h][w] (channel 0 = dx, 1 = dy,
 * in pixels) satisfies A(i, j) ~ B(i + f[1], j + f[0]): the flow that maps frame t onto
 * frame t-1 is the estimate of (frame t, frame t-1).  The method, which the entry points
 * below compose (video.FlowEstimator does; every fp32 expression is evaluated as written,
 * an fmaf where one is written and no other fusing):
 *
 * 1. Luma (stx_flow_luma), grey [n][h][w]: with R = fmaf(r, std[0], mean[0]), G, B likewise
 *    (mean, std_: HOST arrays of 3, as stx_image_condition's),
 *      g = 255 * fmaf(0.114, B, fmaf(0.587, G, 0.299 * R)).
 *
 * 2. Pyramid (stx_flow_pyramid, HOST function, needs no GPU): level 0 is (h, w); level l+1
 *    is (ceil(h_l / 2), ceil(w_l / 2)), added while min(h_l, w_l) div 2 >= min_side
 *    (min_side >= 2).  Fills hs[], ws[] (both or neither; min(levels, cap) entries) and
 *    returns the level count, -STX_E_INVALID on a bad argument.  A level's luma planes are
 *    the finer level's through stx_resample2d, STX_FILTER_TRIANGLE; the flow is zero on the
 *    coarsest level.
 *
 * 3. Linearise at the flow (u, v) = (flow[0], flow[1]) (stx_flow_linearize), per pixel:
 *      y = fminf(fmaxf(i + v, 0), h-1), x = fminf(fmaxf(j + u, 0), w-1)   (fp32)
 *    so that no bit pattern of a flow indexes outside the plane: fmaxf returns 0 for a NaN
 *    sum, which then samples row / column 0.  Taps and weights are stx_flow_warp's:
 *    y0 = min(floor(y), h-2), fy = y - y0, likewise x; w00 = (1-fy)(1-fx), w01 = (1-fy) fx,
 *    w10 = fy (1-fx), w11 = fy fx; a sampled plane P is
 *      S(P) = fmaf(w11, P11, fmaf(w10, P10, fmaf(w01, P01, w00 * P00))).
 *    With Bx[i][j] = 0.5 (B[i][min(j+1, w-1)] - B[i][max(j-1, 0)]) and By likewise along the
 *    rows (formed from the 4 x 4 neighbourhood of B around the taps, never stored):
 *      coef[0] = Ix = S(Bx), coef[1] = Iy = S(By),
 *      coef[2] = c = fmaf(Iy, v, fmaf(Ix, u, A - S(B))).
 *    coef is [n][3][h][w] and must not be flow.
 *
 * 4. Jacobi (stx_flow_jacobi): `iters` iterations from uv_in, both channels from the
 *    previous iterate.  With a2 = alpha * alpha, N, S, W, E the edge and NW, NE, SW, SE the
 *    corner neighbours of a plane, indices clamped to the plane (replicated edges):
 *      ubar = fmaf((NW + NE) + (SW + SE), 1/12, ((N + S) + (W + E)) * (1/6))
 *      ru   = 1 / fmaf(Ix, Ix, a2),  rv = 1 / fmaf(Iy, Iy, a2)      (IEEE division)
 *      u'   = fmaf(fmaf(-Iy, v, c), Ix, a2 * ubar) * ru
 *      v'   = fmaf(fmaf(-Ix, u, c), Iy, a2 * vbar) * rv
 *    (1/6 and 1/12 rounded to fp32).  fuse iterations run in one launch: a block relaxes a
 *    32 x 32 tile with a halo of STX_FLOW_JACOBI_MAXFUSE cells in LDS and writes the tile;
 *    every cell is computed by the same instructions whatever the fusion, so the result
 *    does not depend on fuse, bit for bit.  fuse = 0: the library's choice (MAXFUSE; all
 *    of iters where one tile covers the image); 1 <= fuse <= MAXFUSE: exactly that many
 *    per launch, the last launch the remainder.  With more than one launch the iterates
 *    alternate between uv_out and ws (stx_flow_jacobi_ws bytes); uv_in is never written.
 *    uv_out must not overlap uv_in, ws neither.  alpha > 0, iters >= 1.
 *
 * 5. Prolongation: both channels through stx_resample2d (triangle) to the finer level,
 *    then stx_flow_scale, in place: flow[0] *= sx, flow[1] *= sy with sx = (float)w_fine /
 *    (float)w_coarse, sy likewise in h.
 *
 * Per level, `warps` times: step 3 at the current flow, then step 4 from it.
 * None of these allocates or synchronises; arguments are checked before any launch.
 * n <= 65535, h w < 2^29. */
#define STX_FLOW_JACOBI_MAXFUSE 8
int stx_flow_pyramid(int h, int w, int min_side, int* hs, int* ws, int cap);
int stx_flow_luma(const float* img, float* grey, int n, int h, int w, const float* mean,
                  const float* std_, void* stream);
int stx_flow_linearize(const float* a, const float* b, const float* flow, float* coef, int n,
                       int h, int w, void* stream);
size_t stx_flow_jacobi_ws(int n, int h, int w);
int stx_flow_jacobi(const float* coef, const float* uv_in, float* uv_out, int n, int h, int w,
                    float alpha, int iters, int fuse, void* ws, size_t ws_bytes, void* stream);
int stx_flow_scale(float* flow, int n, int h, int w, float sx, float sy, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* STX_H_ */

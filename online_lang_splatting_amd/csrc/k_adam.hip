// k_adam.hip — one fused Adam step over every Gaussian parameter, fed by the flat gradient bucket.
//
// Caller side of the path.  The reference steps `torch.optim.Adam(param_groups, lr=0.0,
// eps=1e-15)` over seven parameter tensors (gaussian_splatting/scene/gaussian_model.py:393-440,
// utils/slam_backend.py:747-749): per tensor a chain of elementwise PyTorch kernels.  Here the bucket that
// the frame-sharded step all-reduces IS the gradient of all seven (row = [3 xyz | 3M sh | 1 opacity |
// 3 scale | 4 rotation | F language]), so one pass reads a row of gradient, parameters and both moments and
// writes parameters and moments back.  The arithmetic is torch.optim.Adam's single-tensor path, operation for
// operation (torch/optim/adam.py, _single_tensor_adam: lerp, mul/addcmul, sqrt / bias_correction2_sqrt + eps, addcdiv),
// every float32 operation rounded once: the UNFUSED sequence, equal bit for bit to its numpy restatement
// (tests/adam_ref.py, tests/test_gpu_adam.py).  torch's own CPU build departs from that sequence by the multiply-adds
// its kernels fuse (a quarter of the exp_avg elements differ in bits after three steps), so
// against torch.optim.Adam itself the match is to rounding, not to the bit.  Dense: a Gaussian with zero gradient
// still decays its moments and moves, exactly as in the reference — a "visible rows only" step would be cheaper but
// is a different optimiser.
//
// HBM-bound: 5 reads + 3 writes of P x width floats, all coalesced (consecutive threads = consecutive floats
// of the flat arrays; the parameter arrays are [P, k] slices addressed per (row, column)).
#include "olsr_device.h"
#include "olsr_kernels.h"

namespace olsr {

constexpr int ADAM_G = 64;  // Gaussians per block, as in k_accumulate.hip

// every scalar of the update, formed in double on the host and rounded to fp32 once (torch passes Python floats
// to lerp_ / mul_ / addcmul_ / addcdiv_, which round them to the tensor's dtype)
struct AdamScalars {
  float one_minus_beta1, beta2, one_minus_beta2, bias_correction2_sqrt, eps;
  float neg_step_xyz, neg_step_sh_dc, neg_step_sh_rest, neg_step_opacity, neg_step_scale, neg_step_rotation,
      neg_step_language;  // -(lr / bias_correction1)
};

// per-group bias corrections (olsr_adam_step_groups): the reference's optimiser counts a step per parameter group, and a group
// whose parameter was replaced in that iteration (reset_opacity, densification) skips it
struct AdamGroupScalars {
  float bias_correction2_sqrt[OLSR_ADAM_GROUPS];
  unsigned skip_mask;
};

// up to OLSR_ADAM_MAX_BUCKETS gradient buckets summed on the fly, in order: ((f0 + f1) + f2) + ... — what a sum of the lane
// buckets (frame_shard.FrameLanes) leaves, bit for bit, without writing it anywhere
struct AdamBuckets {
  const float* more[OLSR_ADAM_MAX_BUCKETS - 1];
  int n_more;
  // row masks (olsr_grad_bucket.row_mask: bit g clear = row g of that bucket is zero), or null = every row is read.
  // A block covers ADAM_G = 64 Gaussians = one mask word: rows a mask proves zero are not read at all (their gradient is the
  // +0.0 the row holds), the update itself stays dense — parameters and moments are those of the unmasked step bit for bit.
  const unsigned long long* mask0;
  const unsigned long long* mask_more[OLSR_ADAM_MAX_BUCKETS - 1];
};

// The isotropic regulariser of the mapping loss (utils/slam_backend.py:664-667):
//     loss_mapping += weight * |scaling - scaling.mean(dim=1)|.mean(),  scaling = exp(_scaling), weight = 10
// as a function of one Gaussian's own three scales (include/olsr.h restates the arithmetic).  x: the parameter values
// BEFORE the step; r: the gradient with respect to x; d: s_k - m.  A NaN scale is outside the contract: every comparison
// with it is false, so the row's sign terms are all zero — r is +-0 (NaN on the NaN element itself in raw mode) and the
// loss NaN.
struct AdamReg {
  float w9;  // (float)(weight / (9 P_total)), formed in double on the host
  int raw;   // the parameter is log(scale) (OLSR_ACT_SCALE_EXP)
};
__device__ __forceinline__ void isotropic_row(const float x[3], int raw, float w9, float r[3], float d[3]) {
  float s[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) s[k] = raw ? expf(x[k]) : x[k];
  const float m = ((s[0] + s[1]) + s[2]) / 3.0f;
  int sg[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    d[k] = s[k] - m;
    sg[k] = (d[k] > 0.f) - (d[k] < 0.f);
  }
  const int ssum = sg[0] + sg[1] + sg[2];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float rk = w9 * (float)(3 * sg[k] - ssum);
    if (raw) rk = rk * s[k];
    r[k] = rk;
  }
}

// GROUPS = false: one step count for every group (olsr_adam_step / _sum / _masked, unchanged); true: the per-group form, the
// same arithmetic with the group's own sqrt(bias_correction2) and a skip bit per group.
// REG (olsr_adam_step_groups_reg): the isotropic regulariser's gradient is added last to the gradient of every scale element.
// The loop below is element-parallel — the thread that writes scales[g][0] runs beside the threads that need its old value
// for the row's mean — so the block first forms r of its 64 Gaussians from the pre-step scales into LDS, behind a barrier,
// before any element of the block is written (blocks own disjoint Gaussians).
template <bool GROUPS, bool REG>
__global__ __launch_bounds__(256) void adam_step_kernel(int P, int M, int F, int width, const float* __restrict__ flat,
                                                        AdamBuckets extra,
                                                        float* __restrict__ means3D, float* __restrict__ shs,
                                                        float* __restrict__ opacities, float* __restrict__ scales,
                                                        float* __restrict__ rotations, float* __restrict__ language,
                                                        float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq,
                                                        AdamScalars hp, AdamGroupScalars gp, AdamReg reg) {
  const int g0 = blockIdx.x * ADAM_G;
  const int ng = min(ADAM_G, P - g0);
  __shared__ float s_reg[REG ? 3 * ADAM_G : 1];
  if constexpr (REG) {
    if (!((gp.skip_mask >> OLSR_ADAM_GROUP_SCALE) & 1u)) {   // (a skipped scale group takes no regulariser)
      if ((int)threadIdx.x < ng) {
        const size_t g = (size_t)(g0 + (int)threadIdx.x);
        const float x[3] = {scales[3 * g], scales[3 * g + 1], scales[3 * g + 2]};
        float r[3], d[3];
        isotropic_row(x, reg.raw, reg.w9, r, d);
#pragma unroll
        for (int k = 0; k < 3; ++k) s_reg[3 * threadIdx.x + k] = r[k];
      }
      __syncthreads();
    }
  }
  const int count = ng * width;
  const int sh_w = 3 * M;
  const float inv_w = 1.0f / (float)width;
  const size_t base = (size_t)g0 * width;
  static_assert(ADAM_G == 64, "one row-mask word per block");
  const unsigned long long w0 = extra.mask0 ? extra.mask0[blockIdx.x] : ~0ull;
  unsigned long long wm[OLSR_ADAM_MAX_BUCKETS - 1];
#pragma unroll
  for (int b = 0; b < OLSR_ADAM_MAX_BUCKETS - 1; ++b)
    wm[b] = (b < extra.n_more) ? (extra.mask_more[b] ? extra.mask_more[b][blockIdx.x] : ~0ull) : 0ull;
  for (int e = threadIdx.x; e < count; e += 256) {
    const int gl = (int)(((float)e + 0.5f) * inv_w);
    const int c = e - gl * width;
    const size_t g = (size_t)(g0 + gl);
    float* p;
    float neg_step;
    int group;
    if (c < 3) { p = means3D + 3 * g + c; neg_step = hp.neg_step_xyz; group = OLSR_ADAM_GROUP_XYZ; }
    else if (c < 3 + sh_w) {
      p = shs + g * sh_w + (c - 3);
      neg_step = (c < 6) ? hp.neg_step_sh_dc : hp.neg_step_sh_rest;
      group = (c < 6) ? OLSR_ADAM_GROUP_SH_DC : OLSR_ADAM_GROUP_SH_REST;
    }
    else if (c < 4 + sh_w) { p = opacities + g; neg_step = hp.neg_step_opacity; group = OLSR_ADAM_GROUP_OPACITY; }
    else if (c < 7 + sh_w) { p = scales + 3 * g + (c - 4 - sh_w); neg_step = hp.neg_step_scale; group = OLSR_ADAM_GROUP_SCALE; }
    else if (c < 11 + sh_w) { p = rotations + 4 * g + (c - 7 - sh_w); neg_step = hp.neg_step_rotation; group = OLSR_ADAM_GROUP_ROTATION; }
    else { p = language + g * F + (c - 11 - sh_w); neg_step = hp.neg_step_language; group = OLSR_ADAM_GROUP_LANGUAGE; }
    if (GROUPS && ((gp.skip_mask >> group) & 1u)) continue;
    const float bc2_sqrt = GROUPS ? gp.bias_correction2_sqrt[group] : hp.bias_correction2_sqrt;
    float grad = ((w0 >> gl) & 1ull) ? flat[base + e] : 0.0f;
#pragma unroll
    for (int b = 0; b < OLSR_ADAM_MAX_BUCKETS - 1; ++b)
      if ((wm[b] >> gl) & 1ull) grad += extra.more[b][base + e];
    if constexpr (REG)
      if (group == OLSR_ADAM_GROUP_SCALE) grad += s_reg[3 * gl + (c - 4 - sh_w)];
    float m = exp_avg[base + e], v = exp_avg_sq[base + e];
    m = m + (grad - m) * hp.one_minus_beta1;              // exp_avg.lerp_(grad, 1 - beta1)
    v = v * hp.beta2 + hp.one_minus_beta2 * grad * grad;  // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    const float denom = sqrtf(v) / bc2_sqrt + hp.eps;
    *p = *p + neg_step * (m / denom);                     // param.addcdiv_(exp_avg, denom, value=-step_size)
    exp_avg[base + e] = m;
    exp_avg_sq[base + e] = v;
  }
}

void launch_adam_step(int P, int M, int F, const olsr_adam_params& hp, const float* const* flats,
                      const unsigned long long* const* masks, int n_flats, float* means3D, float* shs, float* opacities, float* scales, float* rotations, float* language,
                      float* exp_avg, float* exp_avg_sq, hipStream_t st, const int32_t* group_step, unsigned skip_mask,
                      const olsr_adam_reg* reg) {
  if (P <= 0) return;
  const float* flat = flats[0];
  AdamBuckets extra{};
  extra.n_more = n_flats - 1;
  extra.mask0 = masks ? masks[0] : nullptr;
  for (int b = 1; b < n_flats; ++b) {
    extra.more[b - 1] = flats[b];
    extra.mask_more[b - 1] = masks ? masks[b] : nullptr;
  }
  const int width = 11 + 3 * M + F;
  // torch/optim/adam.py, _single_tensor_adam: Python-float (double) arithmetic for every scalar
  const double bc1 = 1.0 - pow(hp.beta1, (double)hp.step);
  const double bc2 = 1.0 - pow(hp.beta2, (double)hp.step);
  AdamScalars k;
  k.one_minus_beta1 = (float)(1.0 - hp.beta1);
  k.beta2 = (float)hp.beta2;
  k.one_minus_beta2 = (float)(1.0 - hp.beta2);
  k.bias_correction2_sqrt = (float)sqrt(bc2);
  k.eps = (float)hp.eps;
  k.neg_step_xyz = (float)(-(hp.lr_xyz / bc1));
  k.neg_step_sh_dc = (float)(-(hp.lr_sh_dc / bc1));
  k.neg_step_sh_rest = (float)(-(hp.lr_sh_rest / bc1));
  k.neg_step_opacity = (float)(-(hp.lr_opacity / bc1));
  k.neg_step_scale = (float)(-(hp.lr_scale / bc1));
  k.neg_step_rotation = (float)(-(hp.lr_rotation / bc1));
  k.neg_step_language = (float)(-(hp.lr_language / bc1));
  AdamGroupScalars gk{};
  if (!group_step) {
    adam_step_kernel<false, false><<<(P + ADAM_G - 1) / ADAM_G, 256, 0, st>>>(P, M, F, width, flat, extra, means3D, shs, opacities,
                                                                       scales, rotations, language, exp_avg, exp_avg_sq, k, gk, AdamReg{});
    return;
  }
  // per group: the same double arithmetic on the group's own step count (torch/optim/adam.py: step_t is per parameter)
  const double lrs[OLSR_ADAM_GROUPS] = {hp.lr_xyz, hp.lr_sh_dc, hp.lr_sh_rest, hp.lr_opacity, hp.lr_scale, hp.lr_rotation,
                                        hp.lr_language};
  float neg[OLSR_ADAM_GROUPS];
  for (int g = 0; g < OLSR_ADAM_GROUPS; ++g) {
    const int s = group_step[g] > 0 ? group_step[g] : 1;  // (a skipped group's count is not used)
    const double gbc1 = 1.0 - pow(hp.beta1, (double)s);
    const double gbc2 = 1.0 - pow(hp.beta2, (double)s);
    gk.bias_correction2_sqrt[g] = (float)sqrt(gbc2);
    neg[g] = (float)(-(lrs[g] / gbc1));
  }
  gk.skip_mask = skip_mask;
  k.neg_step_xyz = neg[OLSR_ADAM_GROUP_XYZ];
  k.neg_step_sh_dc = neg[OLSR_ADAM_GROUP_SH_DC];
  k.neg_step_sh_rest = neg[OLSR_ADAM_GROUP_SH_REST];
  k.neg_step_opacity = neg[OLSR_ADAM_GROUP_OPACITY];
  k.neg_step_scale = neg[OLSR_ADAM_GROUP_SCALE];
  k.neg_step_rotation = neg[OLSR_ADAM_GROUP_ROTATION];
  k.neg_step_language = neg[OLSR_ADAM_GROUP_LANGUAGE];
  if (reg && reg->isotropic_weight != 0.0) {
    const AdamReg rk{(float)(reg->isotropic_weight / (9.0 * (double)reg->P_total)), (reg->activations & OLSR_ACT_SCALE_EXP) ? 1 : 0};
    adam_step_kernel<true, true><<<(P + ADAM_G - 1) / ADAM_G, 256, 0, st>>>(P, M, F, width, flat, extra, means3D, shs, opacities,
                                                                            scales, rotations, language, exp_avg, exp_avg_sq, k, gk, rk);
    return;
  }
  adam_step_kernel<true, false><<<(P + ADAM_G - 1) / ADAM_G, 256, 0, st>>>(P, M, F, width, flat, extra, means3D, shs, opacities,
                                                                           scales, rotations, language, exp_avg, exp_avg_sq, k, gk, AdamReg{});
}

// olsr_isotropic_reg: the regulariser on its own — gradient rows and, in double, the loss.  A thread per Gaussian; a row's
// |d| are summed ((|d0| + |d1|) + |d2|), the rows of a wave by wave_sum, the four waves of a block in order, the blocks'
// partial sums by one more block (single_block_sum): a fixed order, the same bits on every run.
constexpr int ISO_T = 256;
__global__ __launch_bounds__(ISO_T) void isotropic_reg_kernel(int P, const float* __restrict__ scales, AdamReg reg,
                                                              float* __restrict__ grad, double* __restrict__ partials) {
  __shared__ double s_w[ISO_T / 64];
  const size_t g = (size_t)blockIdx.x * ISO_T + threadIdx.x;
  double a = 0.0;
  if (g < (size_t)P) {
    const float x[3] = {scales[3 * g], scales[3 * g + 1], scales[3 * g + 2]};
    float r[3], d[3];
    isotropic_row(x, reg.raw, reg.w9, r, d);
    if (grad) {
#pragma unroll
      for (int k = 0; k < 3; ++k) grad[3 * g + k] = r[k];
    }
    a = ((double)fabsf(d[0]) + (double)fabsf(d[1])) + (double)fabsf(d[2]);
  }
  if (!partials) return;   // (uniform over the launch)
  a = wave_sum(a);
  if (lane_id() == 0) s_w[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}
__global__ __launch_bounds__(ISO_T) void isotropic_loss_kernel(int nb, const double* __restrict__ partials, double scale,
                                                               double* __restrict__ loss) {
  __shared__ double s_w[ISO_T / 64];
  const double tot = single_block_sum<ISO_T / 64>(nb, partials, s_w);
  if (threadIdx.x == 0) *loss = scale * tot;
}

// the scratch: one partial sum per block
static double* isotropic_reg_carve(void* buf, int P, size_t& bytes) {
  Carver c(buf);
  double* partials = c.take<double>((size_t)((P + ISO_T - 1) / ISO_T));
  bytes = c.total();
  return partials;
}

size_t isotropic_reg_scratch_bytes(int P) {
  size_t bytes = 0;
  isotropic_reg_carve(nullptr, P > 0 ? P : 0, bytes);
  return bytes;
}

void launch_isotropic_reg(int P, const float* scales, int activations, double weight, float* grad, double* loss,
                          void* scratch, hipStream_t st) {
  const int nb = (P + ISO_T - 1) / ISO_T;
  const AdamReg rk{(float)(weight / (9.0 * (double)P)), (activations & OLSR_ACT_SCALE_EXP) ? 1 : 0};
  size_t bytes;
  double* partials = loss ? isotropic_reg_carve(scratch, P, bytes) : nullptr;
  isotropic_reg_kernel<<<nb, ISO_T, 0, st>>>(P, scales, rk, grad, partials);
  if (loss) isotropic_loss_kernel<<<1, ISO_T, 0, st>>>(nb, partials, weight / (3.0 * (double)P), loss);
}

}  // namespace olsr

// olsr_entries.hip — the C-ABI entries that check their arguments and make one launch: visibility, the Adam steps, the pose
// step, kNN, the stand-alone losses, gradient accumulation and buckets, the sparse exchange, map edits, keyframe seeding, the front end's frame step, the map's PLY record, the CLIP image tower, TSDF fusion, point-cloud metrics, the 2-D evaluation's query scoring.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "olsr_host.h"

using namespace olsr;

namespace {

// The checks and the launch of every Adam entry.  who: the entry's name in its messages, or nullptr for olsr_adam_step, whose
// one bucket is checked with the parameter arrays; params_error: what is wrong with the entry's own parameter struct, if
// anything.
int adam_entry(const char* who, int32_t P, int32_t M, int32_t F, const olsr_adam_params* hp, const char* params_error,
               int32_t n_flats, const float* const* flats, const uint64_t* const* row_masks, float* means3D, float* shs,
               float* opacities, float* scales, float* rotations, float* language, float* exp_avg, float* exp_avg_sq,
               void* hip_stream, const int32_t* group_step = nullptr, unsigned skip_mask = 0u,
               const olsr_adam_reg* reg = nullptr) {
  if (P < 0 || M < 0 || !supported_F(F)) return fail(OLSR_ERR_ARG, "P, M must be >= 0 and F one of 0, 3, 15, 16, 32");
  if (params_error) return fail(OLSR_ERR_ARG, params_error);
  if (who) {
    if (n_flats < 1 || n_flats > OLSR_ADAM_MAX_BUCKETS || !flats)
      return fail(OLSR_ERR_ARG, std::string(who) + ": between 1 and 8 gradient buckets");
    for (int b = 0; b < n_flats; ++b)
      if (!flats[b]) return fail(OLSR_ERR_ARG, std::string(who) + ": a gradient bucket is NULL");
  }
  if (P == 0) return OLSR_OK;
  if ((!who && !flats[0]) || !means3D || !opacities || !scales || !rotations || !exp_avg || !exp_avg_sq || (M > 0 && !shs) ||
      (F > 0 && !language))
    return fail(OLSR_ERR_ARG, std::string(who ? "" : "the bucket, ") + "every parameter array and both moment buffers are required");
  launch_adam_step(P, M, F, *hp, flats, reinterpret_cast<const unsigned long long* const*>(row_masks), n_flats, means3D, shs,
                   opacities, scales, rotations, language, exp_avg, exp_avg_sq, (hipStream_t)hip_stream, group_step, skip_mask,
                   reg);
  return launch_check(who ? who : "adam_step");
}

const char* adam_params_error(const olsr_adam_params* params) {
  return (!params || params->step < 1) ? "adam params are required and step must be >= 1" : nullptr;
}

// The segment tables of olsr_emd_cost / olsr_chamfer.  The offsets are read on the host — from device memory with one copy
// and a synchronisation of the stream, from host memory directly — and checked.  dev1 / dev2: what the kernels read, the
// caller's device pointers or, when the offsets arrived in host memory, the copies parked in the scratch.
struct CloudSegments {
  long long total1 = 0, total2 = 0;
  const int32_t *dev1 = nullptr, *dev2 = nullptr;
};
// reads and checks one table; on_device: where it lives
int cloud_offsets(const std::string& who, const char* name, int32_t B, const int32_t* off, int32_t max_n, hipStream_t st,
                  std::vector<int32_t>& h, bool* on_device) {
  h.resize((size_t)B + 1);
  hipPointerAttribute_t at;
  *on_device = hipPointerGetAttributes(&at, off) == hipSuccess && at.type == hipMemoryTypeDevice;
  (void)hipGetLastError();   // (a plain host pointer, or no device at all, is an error to the query)
  if (*on_device) {
    HIP_TRY(hipMemcpyAsync(h.data(), off, h.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  } else {
    std::memcpy(h.data(), off, h.size() * sizeof(int32_t));
  }
  if (h[0] < 0) return fail(OLSR_ERR_ARG, who + ": " + name + "[0] must be >= 0");
  int32_t longest = 0;
  for (int32_t b = 0; b < B; ++b) {
    if (h[b + 1] < h[b]) return fail(OLSR_ERR_ARG, who + ": " + name + " must be non-decreasing");
    longest = std::max(longest, h[b + 1] - h[b]);
  }
  if ((long long)h[B] >= (1ll << 31) / 3) return fail(OLSR_ERR_ARG, who + ": " + name + "[B] must be below 2^31 / 3");
  if (longest > max_n) return fail(OLSR_ERR_ARG, who + ": a segment of " + name + " is longer than its max_n");
  return OLSR_OK;
}
// the checks both entries share; scratch_offsets: emd_scratch_offsets or chamfer_scratch_offsets (the parking places are at
// the front of the scratch: they depend on B only).  Nothing is written before every check has passed.
int cloud_segments(const char* who_c, int32_t B, const int32_t* off1, const int32_t* off2, int32_t max_n1, int32_t max_n2,
                   const float* xyz1, const float* xyz2, bool outputs, bool per_point1, bool per_point2, void* scratch,
                   int32_t* (*scratch_offsets)(void*, int, long long, long long, int), hipStream_t st, CloudSegments* out) {
  const std::string who(who_c);
  if (B < 1 || B > OLSR_CLOUD_MAX_SEGMENTS) return fail(OLSR_ERR_ARG, who + ": B must be between 1 and 32767");
  if (!off1 || !off2) return fail(OLSR_ERR_ARG, who + ": off1 and off2 are required");
  if (max_n1 < 0 || max_n2 < 0) return fail(OLSR_ERR_ARG, who + ": max_n1 and max_n2 must be >= 0");
  if (!outputs) return fail(OLSR_ERR_ARG, who + ": every output is required");
  if (!scratch) return fail(OLSR_ERR_ARG, who + ": scratch is required");
  std::vector<int32_t> h[2];
  bool on_device[2];
  OLSR_TRY(cloud_offsets(who, "off1", B, off1, max_n1, st, h[0], &on_device[0]));
  OLSR_TRY(cloud_offsets(who, "off2", B, off2, max_n2, st, h[1], &on_device[1]));
  out->total1 = h[0][B];
  out->total2 = h[1][B];
  if ((out->total1 > 0 && !xyz1) || (out->total2 > 0 && !xyz2)) return fail(OLSR_ERR_ARG, who + ": xyz1 and xyz2 are required");
  // (per_point: the entry's per-point outputs of that cloud are all there; they may be NULL only for an empty cloud)
  if ((out->total1 > 0 && !per_point1) || (out->total2 > 0 && !per_point2)) return fail(OLSR_ERR_ARG, who + ": every output is required");
  const int32_t* given[2] = {off1, off2};
  const int32_t* dev[2];
  bool parked = false;
  for (int w = 0; w < 2; ++w) {
    dev[w] = given[w];
    if (on_device[w]) continue;
    int32_t* park = scratch_offsets(scratch, B, 0, 0, w);
    HIP_TRY(hipMemcpyAsync(park, h[w].data(), h[w].size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    dev[w] = park;
    parked = true;
  }
  if (parked) HIP_TRY(hipStreamSynchronize(st));   // h goes away
  out->dev1 = dev[0];
  out->dev2 = dev[1];
  return OLSR_OK;
}

// what is wrong with the sizes of olsr_mask_smooth / olsr_query_eval, if anything
const char* query_eval_size_error(int32_t P, int32_t H, int32_t W) {
  if (P < 1 || P > OLSR_QUERY_EVAL_MAX_PLANES) return "P must be between 1 and 65535";
  if (H < 2 || W < 2) return "H and W must be >= 2 (the reference's window is empty below that)";
  if (H > OLSR_QUERY_EVAL_MAX_EXTENT || W > OLSR_QUERY_EVAL_MAX_EXTENT || (int64_t)H * (int64_t)W > (int64_t)0x7FFFFFFF)
    return "H and W must be <= 2^20 and H * W must fit an int32";
  return nullptr;
}

}  // namespace

extern "C" {

int olsr_mark_visible(int32_t P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                      uint8_t* present, void* hip_stream) {
  (void)projmatrix;  // the reference computes p_hom and discards it (CR/auxiliary.h:149-151)
  if (P < 0) return fail(OLSR_ERR_ARG, "P must be >= 0");
  if (P == 0) return OLSR_OK;
  if (!means3D || !viewmatrix || !present) return fail(OLSR_ERR_ARG, "means3D, viewmatrix and present are required");
  launch_mark_visible(P, means3D, viewmatrix, present, (hipStream_t)hip_stream);
  return launch_check("mark_visible");
}

int olsr_adam_step(int32_t P, int32_t M, int32_t F, const olsr_adam_params* params, const float* flat, float* means3D,
                   float* shs, float* opacities, float* scales, float* rotations, float* language, float* exp_avg,
                   float* exp_avg_sq, void* hip_stream) {
  const float* one[1] = {flat};
  return adam_entry(nullptr, P, M, F, params, adam_params_error(params), 1, one, nullptr, means3D, shs, opacities, scales,
                    rotations, language, exp_avg, exp_avg_sq, hip_stream);
}

int olsr_adam_step_sum(int32_t P, int32_t M, int32_t F, const olsr_adam_params* params, int32_t n_flats,
                       const float* const* flats, float* means3D, float* shs, float* opacities, float* scales,
                       float* rotations, float* language, float* exp_avg, float* exp_avg_sq, void* hip_stream) {
  return olsr_adam_step_masked(P, M, F, params, n_flats, flats, nullptr, means3D, shs, opacities, scales, rotations, language,
                               exp_avg, exp_avg_sq, hip_stream);
}

int olsr_adam_step_masked(int32_t P, int32_t M, int32_t F, const olsr_adam_params* params, int32_t n_flats,
                          const float* const* flats, const uint64_t* const* row_masks, float* means3D, float* shs,
                          float* opacities, float* scales, float* rotations, float* language, float* exp_avg,
                          float* exp_avg_sq, void* hip_stream) {
  return adam_entry("adam_step_sum", P, M, F, params, adam_params_error(params), n_flats, flats, row_masks, means3D, shs,
                    opacities, scales, rotations, language, exp_avg, exp_avg_sq, hip_stream);
}

int olsr_adam_step_groups(int32_t P, int32_t M, int32_t F, const olsr_adam_group_params* params, int32_t n_flats,
                          const float* const* flats, const uint64_t* const* row_masks, float* means3D, float* shs,
                          float* opacities, float* scales, float* rotations, float* language, float* exp_avg,
                          float* exp_avg_sq, void* hip_stream) {
  return olsr_adam_step_groups_reg(P, M, F, params, n_flats, flats, row_masks, means3D, shs, opacities, scales, rotations,
                                   language, exp_avg, exp_avg_sq, nullptr, hip_stream);
}

int olsr_adam_step_groups_reg(int32_t P, int32_t M, int32_t F, const olsr_adam_group_params* params, int32_t n_flats,
                              const float* const* flats, const uint64_t* const* row_masks, float* means3D, float* shs,
                              float* opacities, float* scales, float* rotations, float* language, float* exp_avg,
                              float* exp_avg_sq, const olsr_adam_reg* reg, void* hip_stream) {
  const char* params_error = params ? nullptr : "adam group params are required";
  for (int g = 0; params && g < OLSR_ADAM_GROUPS; ++g)
    if (!((params->skip_mask >> g) & 1) && params->group_step[g] < 1)
      params_error = "adam_step_groups: the step count of every group that steps must be >= 1";
  if (reg && reg->isotropic_weight != 0.0) {
    if (!std::isfinite(reg->isotropic_weight)) params_error = "adam_step_groups_reg: isotropic_weight must be finite";
    if (reg->activations & ~7) params_error = "adam_step_groups_reg: activations outside OLSR_ACT_*";
    if (reg->P_total < P || reg->P_total < 1) params_error = "adam_step_groups_reg: P_total must be >= P and >= 1";
  }
  return adam_entry("adam_step_groups", P, M, F, params ? &params->base : nullptr, params_error, n_flats, flats, row_masks,
                    means3D, shs, opacities, scales, rotations, language, exp_avg, exp_avg_sq, hip_stream,
                    params ? params->group_step : nullptr, params ? (unsigned)params->skip_mask : 0u, reg);
}

size_t olsr_isotropic_reg_scratch_bytes(int32_t P) { return isotropic_reg_scratch_bytes(P); }

int olsr_isotropic_reg(int32_t P, const float* scales, int32_t activations, double weight, float* grad, double* loss,
                       void* scratch, void* hip_stream) {
  if (P < 0) return fail(OLSR_ERR_ARG, "isotropic_reg: P must be >= 0");
  if (activations & ~7) return fail(OLSR_ERR_ARG, "isotropic_reg: activations outside OLSR_ACT_*");
  if (!std::isfinite(weight)) return fail(OLSR_ERR_ARG, "isotropic_reg: weight must be finite");
  if (loss && !scratch) return fail(OLSR_ERR_ARG, "isotropic_reg: the loss needs scratch");
  if (P > 0 && !scales) return fail(OLSR_ERR_ARG, "isotropic_reg: scales are required");
  if (P == 0) {   // (the mean over no element: the loss is written as 0)
    if (loss) HIP_TRY(hipMemsetAsync(loss, 0, sizeof(double), (hipStream_t)hip_stream));
    return OLSR_OK;
  }
  if (!grad && !loss) return OLSR_OK;
  launch_isotropic_reg(P, scales, activations, weight, grad, loss, scratch, (hipStream_t)hip_stream);
  return launch_check("isotropic_reg");
}

int olsr_window_pose_step(const olsr_pose_params* params, int32_t V, const int32_t* flags, const float* dL_dtau_sum,
                          const float* dL_dexposure, const float* projection_matrix, float* state, int32_t* status,
                          const int32_t* frame_status, void* hip_stream) {
  if (V < 1 || V > OLSR_WINDOW_MAX_VIEWS) return fail(OLSR_ERR_ARG, "window_pose_step: V must be between 1 and 32");
  if (!params || !flags || !projection_matrix || !state || !status)
    return fail(OLSR_ERR_ARG, "window_pose_step: pose params, flags, projection_matrix, state and status are required");
  for (int v = 0; v < V; ++v) {
    if (flags[v] & ~(OLSR_WINDOW_OPT_POSE | OLSR_WINDOW_OPT_EXPOSURE))
      return fail(OLSR_ERR_ARG, "window_pose_step: unknown flag bits");
    if ((flags[v] & OLSR_WINDOW_OPT_POSE) && !dL_dtau_sum)
      return fail(OLSR_ERR_ARG, "window_pose_step: a view optimises its pose but dL_dtau_sum is NULL");
    if ((flags[v] & OLSR_WINDOW_OPT_EXPOSURE) && !dL_dexposure)
      return fail(OLSR_ERR_ARG, "window_pose_step: a view optimises its exposure but dL_dexposure is NULL");
  }
  launch_window_pose_step(*params, V, flags, dL_dtau_sum, dL_dexposure, projection_matrix, state, status, frame_status,
                          (hipStream_t)hip_stream);
  return launch_check("window_pose_step");
}

int olsr_pose_step(const olsr_pose_params* params, const float* dL_dtau_sum, const float* dL_dexposure,
                   const float* projection_matrix, float* state, int32_t* status, void* hip_stream) {
  return olsr_pose_step_gated(params, dL_dtau_sum, dL_dexposure, projection_matrix, state, status, nullptr, hip_stream);
}

int olsr_pose_step_gated(const olsr_pose_params* params, const float* dL_dtau_sum, const float* dL_dexposure,
                         const float* projection_matrix, float* state, int32_t* status, const int32_t* frame_status,
                         void* hip_stream) {
  if (!params || !projection_matrix || !state || !status)
    return fail(OLSR_ERR_ARG, "pose params, projection_matrix, state and status are required");
  // (step <= 0 with a gradient: the step count is status[1] + 1, kept on the device — see include/olsr.h)
  if (!dL_dtau_sum && dL_dexposure) return fail(OLSR_ERR_ARG, "an exposure gradient needs a pose gradient (one optimiser step)");
  launch_pose_step(*params, dL_dtau_sum, dL_dexposure, projection_matrix, state, status, frame_status,
                   (hipStream_t)hip_stream);
  return launch_check("pose_step");
}

size_t olsr_knn_scratch_bytes(int32_t P) { return knn_scratch_bytes(P); }

int olsr_knn_mean_dist2(int32_t P, const float* points, float* mean_dist2, void* scratch, void* hip_stream) {
  if (P < 0) return fail(OLSR_ERR_ARG, "P must be >= 0");
  if (P == 0) return OLSR_OK;
  if (!points || !mean_dist2 || !scratch) return fail(OLSR_ERR_ARG, "points, mean_dist2 and scratch are required");
  launch_knn(P, points, mean_dist2, scratch, (hipStream_t)hip_stream);
  return launch_check("knn");
}

size_t olsr_mapping_loss_scratch_bytes(int32_t width, int32_t height) {
  size_t bytes = 0;
  loss_partials_carve(nullptr, (size_t)loss_blocks(width > 0 ? width : 0, height > 0 ? height : 0), bytes);
  return bytes;
}

int olsr_mapping_loss(const olsr_loss_params* params, const float* image, const float* depth, const float* language,
                      const float* gt_image, const float* gt_depth, const float* gt_language, const float* exposure,
                      float* dL_dimage, float* dL_ddepth, float* dL_dlanguage, float* loss, float* dL_dexposure,
                      void* scratch, void* hip_stream) {
  if (!params) return fail(OLSR_ERR_ARG, "loss params are NULL");
  const olsr_loss_params& p = *params;
  if (p.width <= 0 || p.height <= 0) return fail(OLSR_ERR_ARG, "image size must be positive");
  if (!supported_F(p.F)) return fail(OLSR_ERR_ARG, "F (language channels) must be one of 0, 3, 15, 16, 32");
  if (!image || !depth || !gt_image || !gt_depth || !dL_dimage || !dL_ddepth || !loss || !scratch)
    return fail(OLSR_ERR_ARG, "image, depth, their targets, their gradient outputs, loss and scratch are required");
  if (p.F > 0 && (!language || !dL_dlanguage)) return fail(OLSR_ERR_ARG, "language and dL_dlanguage are required when F > 0");
  if (p.F > 0 && gt_language && (p.lang_width <= 0 || p.lang_height <= 0))
    return fail(OLSR_ERR_ARG, "the language target size must be positive");
  hipStream_t st = (hipStream_t)hip_stream;
  size_t bytes;
  float* partials = loss_partials_carve(scratch, (size_t)loss_blocks(p.width, p.height), bytes);
  launch_mapping_loss(p, image, depth, language, gt_image, gt_depth, p.F > 0 ? gt_language : nullptr, exposure, nullptr,
                      nullptr, false, dL_dimage, dL_ddepth, dL_dlanguage, loss, dL_dexposure, partials, st);
  return launch_check("mapping_loss");
}

int olsr_tracking_loss(const olsr_loss_params* params, const float* image, const float* depth, const float* opacity,
                       const float* gt_image, const float* gt_depth, const float* grad_mask, const float* exposure,
                       float* dL_dimage, float* dL_ddepth, float* loss, float* dL_dexposure, void* scratch,
                       void* hip_stream) {
  if (!params) return fail(OLSR_ERR_ARG, "loss params are NULL");
  const olsr_loss_params& p = *params;
  if (p.width <= 0 || p.height <= 0) return fail(OLSR_ERR_ARG, "image size must be positive");
  if (!image || !depth || !opacity || !gt_image || !gt_depth || !dL_dimage || !dL_ddepth || !loss || !scratch)
    return fail(OLSR_ERR_ARG, "image, depth, opacity, their targets, the gradient outputs, loss and scratch are required");
  hipStream_t st = (hipStream_t)hip_stream;
  size_t bytes;
  float* partials = loss_partials_carve(scratch, (size_t)loss_blocks(p.width, p.height), bytes);
  launch_mapping_loss(p, image, depth, nullptr, gt_image, gt_depth, nullptr, exposure, opacity, grad_mask, true, dL_dimage,
                      dL_ddepth, nullptr, loss, dL_dexposure, partials, st);
  return launch_check("tracking_loss");
}

size_t olsr_refinement_loss_scratch_bytes(int32_t width, int32_t height) {
  return refinement_loss_scratch_bytes(width, height);
}

int olsr_refinement_loss(int32_t width, int32_t height, float lambda_dssim, const float* image, const float* gt_image,
                         float* dL_dimage, float* loss, void* scratch, void* hip_stream) {
  if (width <= 0 || height <= 0) return fail(OLSR_ERR_ARG, "image size must be positive");
  if (width > 65535 * 32 || height > 65535 * 16) return fail(OLSR_ERR_ARG, "image size beyond 65535 tiles");
  if (!image || !gt_image || !loss || !scratch) return fail(OLSR_ERR_ARG, "image, gt_image, loss and scratch are required");
  launch_refinement_loss(width, height, lambda_dssim, image, gt_image, dL_dimage, loss, scratch, (hipStream_t)hip_stream);
  return launch_check("refinement_loss");
}

size_t olsr_lang_ae_scratch_bytes(int32_t N) { return lang_ae_scratch_bytes(N); }

static bool lang_ae_layout_ok(int32_t layout) {
  return layout == OLSR_LANG_AE_CODES_ROWS || layout == OLSR_LANG_AE_CODES_CHANNELS;
}

int olsr_lang_ae_train_step(const olsr_lang_ae_params* p, int32_t N, const float* features, float* params, float* exp_avg,
                            float* exp_avg_sq, int32_t* step_dev, float* loss, float* codes, float* grad_out, void* scratch,
                            void* hip_stream) {
  if (!p) return fail(OLSR_ERR_ARG, "lang_ae_train_step: the parameter struct is NULL");
  if (p->in_dim != OLSR_LANG_AE_IN || p->hidden_dim != OLSR_LANG_AE_HIDDEN || p->code_dim != OLSR_LANG_AE_CODE)
    return fail(OLSR_ERR_ARG, "lang_ae_train_step: the sizes 32 / 24 / 15 are compiled in");
  if (N <= 0) return fail(OLSR_ERR_ARG, "lang_ae_train_step: N must be positive");
  if (!lang_ae_layout_ok(p->code_layout)) return fail(OLSR_ERR_ARG, "lang_ae_train_step: unknown code layout");
  if (!features || !params || !exp_avg || !exp_avg_sq || !loss || !scratch)
    return fail(OLSR_ERR_ARG, "lang_ae_train_step: features, params, both moments, loss and scratch are required");
  if (p->step <= 0 && !step_dev) return fail(OLSR_ERR_ARG, "lang_ae_train_step: step <= 0 needs the device step counter");
  launch_lang_ae_train_step(*p, N, features, params, exp_avg, exp_avg_sq, step_dev, loss, codes, grad_out, scratch,
                            (hipStream_t)hip_stream);
  return launch_check("lang_ae_train_step");
}

int olsr_lang_ae_encode(int32_t N, const float* features, const float* params, int32_t code_layout, float* codes,
                        void* hip_stream) {
  if (N <= 0) return fail(OLSR_ERR_ARG, "lang_ae_encode: N must be positive");
  if (!lang_ae_layout_ok(code_layout)) return fail(OLSR_ERR_ARG, "lang_ae_encode: unknown code layout");
  if (!features || !params || !codes) return fail(OLSR_ERR_ARG, "lang_ae_encode: features, params and codes are required");
  launch_lang_ae_encode(N, features, params, code_layout, codes, (hipStream_t)hip_stream);
  return launch_check("lang_ae_encode");
}

int olsr_lang_ae_decode(int32_t N, const float* codes, const float* params, int32_t code_layout, float* recon,
                        void* hip_stream) {
  if (N <= 0) return fail(OLSR_ERR_ARG, "lang_ae_decode: N must be positive");
  if (!lang_ae_layout_ok(code_layout)) return fail(OLSR_ERR_ARG, "lang_ae_decode: unknown code layout");
  if (!codes || !params || !recon) return fail(OLSR_ERR_ARG, "lang_ae_decode: codes, params and recon are required");
  launch_lang_ae_decode(N, codes, params, code_layout, recon, (hipStream_t)hip_stream);
  return launch_check("lang_ae_decode");
}

// the layer widths a caller names against the ones compiled in
static bool widths_built(int32_t n_widths, const int32_t* widths, std::initializer_list<int32_t> built) {
  return n_widths == (int32_t)built.size() && std::equal(built.begin(), built.end(), widths);
}

// what is wrong with the sizes of a language query apart from its width list, or nullptr
static const char* lang_query_sizes_error(const olsr_lang_query_params* p) {
  if (p->K < 1 || p->K > OLSR_LANG_QUERY_MAX_PHRASES) return "K must be between 1 and 64";
  if (p->n_pos < 0 || p->n_labels < 0 || p->n_pos + p->n_labels > p->K) return "n_pos and n_labels must be >= 0 and sum to at most K";
  if (p->in_width < 1 || p->in_height < 1 || p->dec_width < 1 || p->dec_height < 1 || p->out_width < 1 || p->out_height < 1)
    return "every width and height must be positive";
  if ((int64_t)p->in_width * p->in_height > (1 << 28) || (int64_t)p->dec_width * p->dec_height > (1 << 28) ||
      (int64_t)p->out_width * p->out_height > (1 << 28))
    return "a map has at most 2^28 pixels";
  if (p->flags & ~(OLSR_LANG_QUERY_WANT_MASK | OLSR_LANG_QUERY_WANT_LABELS)) return "flags holds unknown OLSR_LANG_QUERY_* bits";
  return nullptr;
}

// what is wrong with the sizes of a language query, or nullptr
static const char* lang_query_params_error(const olsr_lang_query_params* p) {
  if (!p) return "the parameter struct is NULL";
  if (!widths_built(p->n_widths, p->widths, {OLSR_LANG_AE_IN, 192, 256, 384, 512, OLSR_LANG_QUERY_FEATURE_DIM}))
    return "this build decodes the layer widths {32, 192, 256, 384, 512, 768} only";
  return lang_query_sizes_error(p);
}

size_t olsr_lang_query_scratch_bytes(const olsr_lang_query_params* p) {
  return (!p || p->out_width < 1 || p->out_height < 1) ? ALIGN : lang_query_scratch_bytes(*p);
}

int olsr_lang_query_sims(const olsr_lang_query_params* p, const float* codes, const float* online_params,
                         const float* decoder_params, const float* phrases, float* sims, void* hip_stream) {
  if (const char* e = lang_query_params_error(p)) return fail(OLSR_ERR_ARG, std::string("lang_query_sims: ") + e);
  if (!codes || !online_params || !decoder_params || !phrases || !sims)
    return fail(OLSR_ERR_ARG, "lang_query_sims: codes, both parameter arrays, phrases and sims are required");
  if (((uintptr_t)decoder_params & 15u) || ((uintptr_t)phrases & 15u))
    return fail(OLSR_ERR_ARG, "lang_query_sims: decoder_params and phrases must be 16-byte aligned");
  return launch_check("lang_query_sims", launch_lang_query_sims(*p, codes, online_params, decoder_params, phrases, sims,
                                                                (hipStream_t)hip_stream));
}

int olsr_lang_query_relevancy(const olsr_lang_query_params* p, const float* sims, float* relevancy, float* smoothed,
                              float* blended, float* score, int32_t* coord, float* minmax, uint8_t* mask, int32_t* labels,
                              void* scratch, void* hip_stream) {
  if (const char* e = lang_query_params_error(p)) return fail(OLSR_ERR_ARG, std::string("lang_query_relevancy: ") + e);
  if (p->K - p->n_pos - p->n_labels < 1) return fail(OLSR_ERR_ARG, "lang_query_relevancy: at least one negative phrase is required");
  const bool want_mask = p->flags & OLSR_LANG_QUERY_WANT_MASK, want_labels = p->flags & OLSR_LANG_QUERY_WANT_LABELS;
  if (p->n_pos < 1 && !want_labels) return fail(OLSR_ERR_ARG, "lang_query_relevancy: nothing to do without positives or labels");
  if (want_labels && p->n_labels < 1) return fail(OLSR_ERR_ARG, "lang_query_relevancy: the label map needs n_labels >= 1");
  if (!(p->thresh == p->thresh)) return fail(OLSR_ERR_ARG, "lang_query_relevancy: thresh is NaN");
  if (!sims) return fail(OLSR_ERR_ARG, "lang_query_relevancy: sims is required");
  if (p->n_pos > 0 && (!relevancy || !smoothed || !blended || !score || !coord || !minmax || !scratch))
    return fail(OLSR_ERR_ARG, "lang_query_relevancy: relevancy, smoothed, blended, score, coord, minmax and scratch are required");
  if (want_mask && (!mask || p->n_pos < 1)) return fail(OLSR_ERR_ARG, "lang_query_relevancy: the mask needs its array and a positive");
  if (want_labels && !labels) return fail(OLSR_ERR_ARG, "lang_query_relevancy: the label map needs its array");
  launch_lang_query_relevancy(*p, sims, relevancy, smoothed, blended, score, coord, minmax, want_mask ? mask : nullptr,
                              want_labels ? labels : nullptr, scratch, (hipStream_t)hip_stream);
  return launch_check("lang_query_relevancy");
}

// what is wrong with a call of one of the two encoders apart from its width list, or nullptr; missing: the entry's own
// complaint about its arrays (or nullptr), which goes between the sizes and the alignment
extern "C++" template <typename P>
static const char* lang_encoder_call_error(const P* p, int32_t N, const float* encoder_params, const char* missing) {
  if (N < 1) return "N must be positive";
  if (p->in_layout != OLSR_LANG_ENCODER_IN_ROWS && p->in_layout != OLSR_LANG_ENCODER_IN_CHANNELS) return "unknown input layout";
  if (!lang_ae_layout_ok(p->code_layout)) return "unknown code layout";
  if (p->in_layout == OLSR_LANG_ENCODER_IN_CHANNELS && p->plane_stride < (int64_t)N)
    return "plane_stride must be at least N in the channel layout";
  if (!(p->bn_eps > 0.0)) return "bn_eps must be positive";
  if (missing) return missing;
  if ((uintptr_t)encoder_params & 15u) return "encoder_params must be 16-byte aligned";
  return nullptr;
}

int olsr_lang_encoder_encode(const olsr_lang_encoder_params* p, int32_t N, const float* features768, const float* encoder_params,
                             const float* online_params, float* features32, float* codes, void* hip_stream) {
  if (!p) return fail(OLSR_ERR_ARG, "lang_encoder_encode: the parameter struct is NULL");
  if (!widths_built(p->n_widths, p->widths, {OLSR_LANG_QUERY_FEATURE_DIM, 512, 256, 128, 64, OLSR_LANG_AE_IN}))
    return fail(OLSR_ERR_ARG, "lang_encoder_encode: this build encodes the layer widths {768, 512, 256, 128, 64, 32} only");
  const char* missing = !features768 || !encoder_params ? "features768 and encoder_params are required"
                        : !features32 && !codes         ? "features32 and codes are both NULL"
                        : codes && !online_params       ? "codes need online_params"
                                                        : nullptr;
  if (const char* e = lang_encoder_call_error(p, N, encoder_params, missing))
    return fail(OLSR_ERR_ARG, std::string("lang_encoder_encode: ") + e);
  return launch_check("lang_encoder_encode", launch_lang_encoder(*p, N, features768, encoder_params, online_params,
                                                                 features32, codes, (hipStream_t)hip_stream));
}

// ---- the single-stage chain (include/olsr_single_stage.h)
int olsr_ss_encoder_encode(const olsr_ss_encoder_params* p, int32_t N, const float* features768, const float* encoder_params,
                           float* codes, void* hip_stream) {
  if (!p) return fail(OLSR_ERR_ARG, "ss_encoder_encode: the parameter struct is NULL");
  if (!widths_built(p->n_widths, p->widths, {OLSR_LANG_QUERY_FEATURE_DIM, 384, 192, 96, 48, 24, OLSR_LANG_AE_CODE}))
    return fail(OLSR_ERR_ARG, "ss_encoder_encode: this entry encodes the layer widths {768, 384, 192, 96, 48, 24, 15} only");
  const char* missing = !features768 || !encoder_params || !codes ? "features768, encoder_params and codes are required" : nullptr;
  if (const char* e = lang_encoder_call_error(p, N, encoder_params, missing))
    return fail(OLSR_ERR_ARG, std::string("ss_encoder_encode: ") + e);
  return launch_check("ss_encoder_encode", launch_ss_encoder(*p, N, features768, encoder_params, codes, (hipStream_t)hip_stream));
}

int olsr_ss_query_sims(const olsr_lang_query_params* p, const float* codes, const float* decoder_params, const float* phrases,
                       float* sims, void* hip_stream) {
  if (!p) return fail(OLSR_ERR_ARG, "ss_query_sims: the parameter struct is NULL");
  if (!widths_built(p->n_widths, p->widths, {OLSR_LANG_AE_CODE, 24, 48, 96, 192, 384, 384, OLSR_LANG_QUERY_FEATURE_DIM}))
    return fail(OLSR_ERR_ARG, "ss_query_sims: this entry decodes the layer widths {15, 24, 48, 96, 192, 384, 384, 768} only");
  if (const char* e = lang_query_sizes_error(p)) return fail(OLSR_ERR_ARG, std::string("ss_query_sims: ") + e);
  if (!codes || !decoder_params || !phrases || !sims)
    return fail(OLSR_ERR_ARG, "ss_query_sims: codes, decoder_params, phrases and sims are required");
  if (((uintptr_t)decoder_params & 15u) || ((uintptr_t)phrases & 15u))
    return fail(OLSR_ERR_ARG, "ss_query_sims: decoder_params and phrases must be 16-byte aligned");
  return launch_check("ss_query_sims", launch_ss_query_sims(*p, codes, decoder_params, phrases, sims, (hipStream_t)hip_stream));
}

size_t olsr_hr_net_workspace_bytes(int32_t h, int32_t w, int32_t h3, int32_t w3, int32_t h2, int32_t w2) {
  if (h < 1 || w < 1 || h3 < 1 || w3 < 1 || h2 < 1 || w2 < 1) return 0;
  return hr_net_workspace_bytes(h, w);  // f3 and f2 are sampled in place: their sizes add nothing
}

int olsr_hr_net_forward(const olsr_hr_net_params* p, const float* fv, const float* f3, const float* f2, const float* packed_params,
                        void* workspace, float* out, void* hip_stream) {
  if (!p) return fail(OLSR_ERR_ARG, "hr_net_forward: the parameter struct is NULL");
  if (p->c_fv != 768 || p->c_f3 != 384 || p->c_f2 != 192 || p->c_out != 768)
    return fail(OLSR_ERR_ARG, "hr_net_forward: this build has the channel widths fv 768, f3 384, f2 192, out 768 only");
  if (p->h < 1 || p->w < 1 || p->h3 < 1 || p->w3 < 1 || p->h2 < 1 || p->w2 < 1)
    return fail(OLSR_ERR_ARG, "hr_net_forward: every size must be positive");
  const int64_t n = (int64_t)p->h * p->w, n3 = (int64_t)p->h3 * p->w3, n2 = (int64_t)p->h2 * p->w2, lim = (int64_t)1 << 31;
  if (p->fv_stride < n || p->f3_stride < n3 || p->f2_stride < n2 || p->out_stride < 64 * n)
    return fail(OLSR_ERR_ARG, "hr_net_forward: a plane stride is smaller than its plane");
  if (p->fv_stride >= lim / 768 || p->f3_stride >= lim / 384 || p->f2_stride >= lim / 192 || p->out_stride >= lim / 768)
    return fail(OLSR_ERR_ARG, "hr_net_forward: channels x plane stride must stay below 2^31 elements");
  if (!(p->bn_eps > 0.0)) return fail(OLSR_ERR_ARG, "hr_net_forward: bn_eps must be positive");
  if (p->launches >> OLSR_HR_NET_LAUNCHES) return fail(OLSR_ERR_ARG, "hr_net_forward: launches names a launch that does not exist");
  if (!fv || !f3 || !f2 || !packed_params || !workspace || !out)
    return fail(OLSR_ERR_ARG, "hr_net_forward: fv, f3, f2, packed_params, workspace and out are required");
  if (((uintptr_t)packed_params | (uintptr_t)workspace) & 15u)
    return fail(OLSR_ERR_ARG, "hr_net_forward: packed_params and workspace must be 16-byte aligned");
  if (p->workspace_bytes < (uint64_t)hr_net_workspace_bytes(p->h, p->w))
    return fail(OLSR_ERR_ARG, "hr_net_forward: the workspace is smaller than olsr_hr_net_workspace_bytes");
  launch_hr_net(*p, fv, f3, f2, packed_params, (float*)workspace, out, (hipStream_t)hip_stream);
  return launch_check("hr_net_forward");
}

int olsr_accumulate_gradients(int32_t P, int32_t M, int32_t F, int32_t assign, const float* dL_dmeans3D,
                              const float* dL_dsh,
                              const float* dL_dopacity, const float* dL_dscales, const float* dL_drotations,
                              const float* dL_dlanguage, const float* dL_dmeans2D, const int32_t* radii, float* flat,
                              float* densify, int32_t* max_radii, void* hip_stream) {
  if (P < 0 || M < 0 || F < 0) return fail(OLSR_ERR_ARG, "P, M, F must be >= 0");
  if (P == 0) return OLSR_OK;
  if (!dL_dmeans3D || !dL_dopacity || !dL_dscales || !dL_drotations || !dL_dmeans2D || !radii || !flat || !densify ||
      !max_radii || (M > 0 && !dL_dsh) || (F > 0 && !dL_dlanguage))
    return fail(OLSR_ERR_ARG, "gradient, radii and accumulator pointers must not be NULL");
  launch_accumulate(P, M, F, assign != 0, dL_dmeans3D, dL_dsh, dL_dopacity, dL_dscales, dL_drotations, dL_dlanguage, dL_dmeans2D,
                    radii, flat, densify, max_radii, (hipStream_t)hip_stream);
  return launch_check("accumulate");
}

int olsr_bucket_add(int32_t P, int32_t width, float* dst_flat, float* dst_densify, int32_t* dst_max_radii,
                    uint64_t* dst_row_mask, const float* src_flat, const float* src_densify, const int32_t* src_max_radii,
                    const uint64_t* src_row_mask, void* hip_stream) {
  if (P < 0 || width <= 0) return fail(OLSR_ERR_ARG, "P must be >= 0, width > 0");
  if (P == 0) return OLSR_OK;
  if (!dst_flat || !dst_densify || !dst_max_radii || !src_flat || !src_densify || !src_max_radii)
    return fail(OLSR_ERR_ARG, "bucket_add: flat, densify and max_radii of both buckets are required");
  launch_bucket_add(P, width, dst_flat, src_flat, reinterpret_cast<unsigned long long*>(dst_row_mask),
                    reinterpret_cast<const unsigned long long*>(src_row_mask), dst_densify, src_densify, dst_max_radii,
                    src_max_radii, (hipStream_t)hip_stream);
  return launch_check("bucket_add");
}

int olsr_sparse_exchange_mask(int32_t P, int32_t width, const float* flat, const uint64_t* row_mask, const int32_t* max_radii,
                              int32_t* imax, void* hip_stream) {
  if (P < 0 || width <= 0) return fail(OLSR_ERR_ARG, "P must be >= 0, width > 0");
  if (P == 0) return OLSR_OK;
  if (!flat || !max_radii || !imax) return fail(OLSR_ERR_ARG, "flat, max_radii and imax must not be NULL");
  launch_exchange_mask(P, width, flat, reinterpret_cast<const unsigned long long*>(row_mask), max_radii, imax,
                       (hipStream_t)hip_stream);
  return launch_check("sparse exchange (mask)");
}

int64_t olsr_sparse_exchange_scratch_ints(int32_t P) { return P <= 0 ? 0 : ((int64_t)P + 1023) / 1024; }

int olsr_sparse_exchange_pack(int32_t P, int32_t width, int32_t capacity, const float* flat, const int32_t* imax,
                              int32_t* max_radii, uint64_t* row_mask, const float* densify, int32_t* idx, float* fsum,
                              int32_t* scratch, int32_t* status_dev, void* hip_stream) {
  if (P < 0 || width <= 0 || capacity <= 0) return fail(OLSR_ERR_ARG, "P must be >= 0, width and capacity > 0");
  if (P == 0) return OLSR_OK;
  if (!flat || !imax || !max_radii || !densify || !scratch || !status_dev || ((idx == nullptr) != (fsum == nullptr)))
    return fail(OLSR_ERR_ARG, "sparse exchange (pack): only row_mask may be NULL, or idx and fsum together (count only)");
  launch_exchange_pack(P, width, capacity, flat, imax, max_radii, reinterpret_cast<unsigned long long*>(row_mask), densify, idx,
                       fsum, scratch, status_dev, (hipStream_t)hip_stream);
  return launch_check("sparse exchange (pack)");
}

int olsr_sparse_exchange_unpack(int32_t P, int32_t width, int32_t capacity, const int32_t* idx, const float* fsum, float* flat,
                                float* densify, void* hip_stream) {
  if (P < 0 || width <= 0 || capacity <= 0) return fail(OLSR_ERR_ARG, "P must be >= 0, width and capacity > 0");
  if (P == 0) return OLSR_OK;
  if (!idx || !fsum || !flat || !densify) return fail(OLSR_ERR_ARG, "sparse exchange (unpack): pointers must not be NULL");
  launch_exchange_unpack(P, width, capacity, idx, fsum, flat, densify, (hipStream_t)hip_stream);
  return launch_check("sparse exchange (unpack)");
}

size_t olsr_map_edit_scratch_bytes(int32_t P) { return map_edit_scratch_bytes(P); }

static bool map_buffers_complete(const olsr_map_buffers* b, int32_t M, int32_t F) {
  return b && b->means3D && b->opacities && b->scales && b->rotations && (M == 0 || b->shs) && (F == 0 || b->language) &&
         b->exp_avg && b->exp_avg_sq && b->kf_id && b->n_obs && b->stats && b->max_radii;
}

int olsr_map_edit_plan(int32_t P, const olsr_map_edit_params* params, const olsr_map_buffers* src, const uint8_t* drop_mask,
                       void* scratch, int32_t* status, void* hip_stream) {
  if (P < 0 || !params || !src || !scratch || !status) return fail(OLSR_ERR_ARG, "map_edit_plan: P >= 0, params, src, scratch and status are required");
  if (params->mode != OLSR_MAP_EDIT_DENSIFY && params->mode != OLSR_MAP_EDIT_MASK) return fail(OLSR_ERR_ARG, "map_edit_plan: unknown mode");
  if (params->n_append < 0) return fail(OLSR_ERR_ARG, "map_edit_plan: n_append must be >= 0");
  if (params->mode == OLSR_MAP_EDIT_DENSIFY && params->n_append != 0)
    return fail(OLSR_ERR_ARG, "map_edit_plan: densify mode appends nothing");
  if (P > 0 && params->mode == OLSR_MAP_EDIT_DENSIFY && (!src->stats || !src->scales || !src->opacities))
    return fail(OLSR_ERR_ARG, "map_edit_plan: densify mode reads stats, scales and opacities");
  launch_map_edit_plan(P, *params, *src, drop_mask, scratch, status, (hipStream_t)hip_stream);
  return launch_check("map_edit_plan");
}

int olsr_map_edit_apply(int32_t P, int32_t M, int32_t F, const olsr_map_edit_params* params, const olsr_map_buffers* src,
                        const float* z, const olsr_map_buffers* append, const void* scratch, const int32_t* status,
                        int32_t P_new, int32_t dst_capacity, const olsr_map_buffers* dst, int32_t* src_index,
                        void* hip_stream) {
  if (P < 0 || M < 0 || !supported_F(F) || !params || !scratch || !status)
    return fail(OLSR_ERR_ARG, "map_edit_apply: P, M >= 0, F one of 0, 3, 15, 16, 32; params, scratch and status are required");
  if (P_new > dst_capacity) return fail(OLSR_ERR_CAPACITY, "map_edit_apply: P_new exceeds the destination's capacity");
  if (P_new == 0) return OLSR_OK;
  if (!map_buffers_complete(dst, M, F) || !src_index) return fail(OLSR_ERR_ARG, "map_edit_apply: every destination buffer is required");
  if (P > 0 && !map_buffers_complete(src, M, F)) return fail(OLSR_ERR_ARG, "map_edit_apply: every source buffer is required");
  if (P > 0 && params->mode == OLSR_MAP_EDIT_DENSIFY && !z) return fail(OLSR_ERR_ARG, "map_edit_apply: densify mode needs z [P,2,3]");
  if (params->n_append > 0 && (!append || !append->means3D || !append->opacities || !append->scales || !append->rotations ||
                               (M > 0 && !append->shs)))
    return fail(OLSR_ERR_ARG, "map_edit_apply: the appended rows need means3D, shs, opacities, scales and rotations");
  launch_map_edit_apply(P, M, F, *params, *src, z, append, scratch, status, dst_capacity, *dst, src_index,
                        (hipStream_t)hip_stream);
  return launch_check("map_edit_apply");
}

size_t olsr_keyframe_seed_scratch_bytes(int32_t W, int32_t H) { return keyframe_seed_scratch_bytes(W, H); }

// what is wrong with the parameters of a keyframe seeding, if anything
static const char* keyframe_seed_params_error(const olsr_keyframe_seed_params* p) {
  if (!p) return "params are required";
  if (p->W <= 0 || p->H <= 0) return "W and H must be > 0";
  if (p->downsample <= 0) return "downsample must be > 0";
  const int64_t N = (int64_t)p->W * (int64_t)p->H;
  if (N > (int64_t)0x7FFFFFFF) return "W * H must fit an int32";
  if (p->plane_stride < N) return "plane_stride must be >= W * H";
  if (p->M < 1) return "M must be >= 1";
  if ((int64_t)p->capacity < N / p->downsample) return "capacity must be >= W * H / downsample";
  if (!(p->fx > 0.0) || !(p->fy > 0.0) || !std::isfinite(p->fx) || !std::isfinite(p->fy)) return "fx and fy must be finite and > 0";
  if (!(p->depth_trunc > 0.0f)) return "depth_trunc must be > 0";
  return nullptr;
}

int olsr_keyframe_seed_plan(const olsr_keyframe_seed_params* p, const float* image, const float* depth, const float* exposure,
                            const float* w2c, const olsr_map_buffers* rows, int32_t* pix_index, void* scratch,
                            int32_t* status, float* aux, void* hip_stream) {
  if (const char* e = keyframe_seed_params_error(p)) return fail(OLSR_ERR_ARG, std::string("keyframe_seed_plan: ") + e);
  if (!image || !depth || !w2c || !rows || !pix_index || !scratch || !status || !aux)
    return fail(OLSR_ERR_ARG, "keyframe_seed_plan: image, depth, w2c, rows, pix_index, scratch, status and aux are required");
  if (!rows->means3D || !rows->shs || !rows->opacities || !rows->scales || !rows->rotations)
    return fail(OLSR_ERR_ARG, "keyframe_seed_plan: the staging rows need means3D, shs, opacities, scales and rotations");
  return launch_check("keyframe_seed_plan", launch_keyframe_seed_plan(*p, image, depth, exposure, w2c, *rows, pix_index,
                                                                      scratch, status, aux, (hipStream_t)hip_stream));
}

int olsr_keyframe_seed_finish(const olsr_keyframe_seed_params* p, int32_t n, const olsr_map_buffers* rows, const float* aux,
                              void* scratch, void* knn_scratch, void* hip_stream) {
  if (const char* e = keyframe_seed_params_error(p)) return fail(OLSR_ERR_ARG, std::string("keyframe_seed_finish: ") + e);
  if (n < 0 || n > p->capacity || (int64_t)n > (int64_t)p->W * p->H)
    return fail(OLSR_ERR_ARG, "keyframe_seed_finish: n must lie in 0 ... min(capacity, W * H)");
  if (!rows || !aux || !scratch) return fail(OLSR_ERR_ARG, "keyframe_seed_finish: rows, aux and scratch are required");
  if (!rows->means3D || !rows->scales) return fail(OLSR_ERR_ARG, "keyframe_seed_finish: the staging rows need means3D and scales");
  if (n < 4) return OLSR_OK;   // no three neighbours: nothing is written, the caller appends nothing
  if (!knn_scratch) return fail(OLSR_ERR_ARG, "keyframe_seed_finish: knn_scratch is required");
  launch_keyframe_seed_finish(*p, n, *rows, aux, scratch, knn_scratch, (hipStream_t)hip_stream);
  return launch_check("keyframe_seed_finish");
}

size_t olsr_frontend_scratch_bytes(int64_t n) { return frontend_scratch_bytes(n); }

int olsr_grad_mask(int32_t W, int32_t H, int64_t plane_stride, int32_t mode, float edge_threshold, const float* image,
                   float* mask, void* scratch, void* hip_stream) {
  if (W <= 0 || H <= 0) return fail(OLSR_ERR_ARG, "grad_mask: W and H must be > 0");
  const int64_t N = (int64_t)W * (int64_t)H;
  if (N > (int64_t)0x7FFFFFFF) return fail(OLSR_ERR_ARG, "grad_mask: W * H must fit an int32");
  if (plane_stride < N) return fail(OLSR_ERR_ARG, "grad_mask: plane_stride must be >= W * H");
  if (!image || !mask) return fail(OLSR_ERR_ARG, "grad_mask: image and mask are required");
  if (mode == OLSR_GRAD_MASK_BLOCKS) {
    if (W < 32 || H < 32) return fail(OLSR_ERR_ARG, "grad_mask: block mode needs W and H >= 32");
    const int64_t bh = H / 32, bw = W / 32;
    if (bh * bw > OLSR_GRAD_MASK_MAX_BLOCK_PIXELS || (bh + 3) * (bw + 2) * (int64_t)sizeof(float) > 65536)
      return fail(OLSR_ERR_ARG, "grad_mask: an image block may hold 8192 pixels and (H / 32 + 3) (W / 32 + 2) floats 64 KiB at most");
  } else if (mode == OLSR_GRAD_MASK_GLOBAL) {
    if (W < 2 || H < 2) return fail(OLSR_ERR_ARG, "grad_mask: W and H must be >= 2");
    if (!scratch) return fail(OLSR_ERR_ARG, "grad_mask: global mode needs scratch");
  } else {
    return fail(OLSR_ERR_ARG, "grad_mask: mode must be OLSR_GRAD_MASK_BLOCKS or OLSR_GRAD_MASK_GLOBAL");
  }
  return launch_check("grad_mask", launch_grad_mask(W, H, plane_stride, mode, edge_threshold, image, mask, scratch,
                                                    (hipStream_t)hip_stream));
}

int olsr_median_depth(int64_t N, const float* depth, const float* opacity, const uint8_t* mask, void* scratch, float* median,
                      int32_t* count, void* hip_stream) {
  if (N <= 0 || N > (int64_t)0x7FFFFFFF) return fail(OLSR_ERR_ARG, "median_depth: N must lie in 1 ... 2^31 - 1");
  if (!depth || !opacity || !scratch || !median || !count)
    return fail(OLSR_ERR_ARG, "median_depth: depth, opacity, scratch, median and count are required");
  return launch_check("median_depth", launch_median_depth(N, depth, opacity, mask, scratch, median, count, (hipStream_t)hip_stream));
}

int olsr_covisibility(int64_t P, const int32_t* n_touched, const olsr_covis_views* views, uint8_t* cur_out, int64_t* counts,
                      void* hip_stream) {
  if (P <= 0 || P > (int64_t)0x7FFFFFFF) return fail(OLSR_ERR_ARG, "covisibility: P must lie in 1 ... 2^31 - 1");
  if (!n_touched || !views || !counts) return fail(OLSR_ERR_ARG, "covisibility: n_touched, views and counts are required");
  if (views->K < 0 || views->K > OLSR_COVIS_MAX_VIEWS) return fail(OLSR_ERR_ARG, "covisibility: K must lie in 0 ... 16");
  for (int k = 0; k < views->K; ++k)
    if (!views->vis[k]) return fail(OLSR_ERR_ARG, "covisibility: a keyframe visibility is NULL");
  return launch_check("covisibility", launch_covisibility(P, n_touched, *views, cur_out, counts, (hipStream_t)hip_stream));
}

int olsr_keyframe_decide(const olsr_keyframe_decide_params* p, const int64_t* counts, const float* median,
                         const float* cur_pose, const float* kf_poses, void* record, void* hip_stream) {
  if (!p) return fail(OLSR_ERR_ARG, "keyframe_decide: params are required");
  if (p->window_len < 0 || p->window_len > OLSR_COVIS_MAX_VIEWS)
    return fail(OLSR_ERR_ARG, "keyframe_decide: window_len must lie in 0 ... 16");
  if (p->window_size < 1) return fail(OLSR_ERR_ARG, "keyframe_decide: window_size must be >= 1");
  if (!counts || !median || !cur_pose || !record || (p->window_len > 0 && !kf_poses))
    return fail(OLSR_ERR_ARG, "keyframe_decide: counts, median, cur_pose, record and (window_len > 0) kf_poses are required");
  launch_keyframe_decide(*p, counts, median, cur_pose, kf_poses, record, (hipStream_t)hip_stream);
  return launch_check("keyframe_decide");
}

// ---- a frame's ingest (include/olsr_frame_ingest.h)
int olsr_frame_ingest(const olsr_frame_ingest_params* p, const uint8_t* rgb, const void* depth, float* image, float* depth_out,
                      void* hip_stream) {
  if (!p) return fail(OLSR_ERR_ARG, "frame_ingest: params are required");
  if (p->W <= 0 || p->H <= 0) return fail(OLSR_ERR_ARG, "frame_ingest: W and H must be > 0");
  const int64_t N = (int64_t)p->W * (int64_t)p->H;
  if (N > (int64_t)0x7FFFFFFF) return fail(OLSR_ERR_ARG, "frame_ingest: W * H must fit an int32");
  if (p->plane_stride < N) return fail(OLSR_ERR_ARG, "frame_ingest: plane_stride must be >= W * H");
  if (p->depth_type != OLSR_INGEST_DEPTH_U16 && p->depth_type != OLSR_INGEST_DEPTH_F32)
    return fail(OLSR_ERR_ARG, "frame_ingest: depth_type must be OLSR_INGEST_DEPTH_U16 or OLSR_INGEST_DEPTH_F32");
  if (!(p->depth_scale > 0.0) || !std::isfinite(p->depth_scale))
    return fail(OLSR_ERR_ARG, "frame_ingest: depth_scale must be finite and > 0");
  if (!rgb || !depth || !image || !depth_out)
    return fail(OLSR_ERR_ARG, "frame_ingest: rgb, depth, image and depth_out are required");
  const uintptr_t depth_align = p->depth_type == OLSR_INGEST_DEPTH_U16 ? 2 : 4;
  if ((uintptr_t)depth % depth_align || (uintptr_t)image % 4 || (uintptr_t)depth_out % 4)
    return fail(OLSR_ERR_ARG, "frame_ingest: depth must be aligned to its element size, image and depth_out to 4 bytes");
  launch_frame_ingest(*p, rgb, depth, image, depth_out, (hipStream_t)hip_stream);
  return launch_check("frame_ingest");
}

// ---- the map <-> the point_cloud.ply record array (include/olsr_map_io.h)
// what is wrong with the sizes of a record, if anything
static const char* map_ply_sizes_error(int32_t M, int32_t F) {
  if (M != 1 && M != 4 && M != 9 && M != 16) return "M must be a perfect square in 1 ... 16";
  if (F < 0 || F > OLSR_MAP_PLY_MAX_F) return "F must lie in 0 ... 32";
  return nullptr;
}

// what is wrong with the parameter arrays of a map that an entry reads or writes, if anything
static const char* map_ply_buffers_error(const olsr_map_buffers* b, int32_t F) {
  if (!b) return "the map's buffers are required";
  if (!b->means3D || !b->shs || !b->opacities || !b->scales || !b->rotations || (F > 0 && !b->language))
    return "means3D, shs, opacities, scales, rotations and (F > 0) language are required";
  if (((uintptr_t)b->means3D | (uintptr_t)b->shs | (uintptr_t)b->opacities | (uintptr_t)b->scales | (uintptr_t)b->rotations |
       (uintptr_t)b->language) % 4)
    return "every array must be aligned to 4 bytes";
  return nullptr;
}

int olsr_map_ply_width(int32_t M, int32_t F) {
  if (const char* e = map_ply_sizes_error(M, F)) return fail(OLSR_ERR_ARG, std::string("map_ply_width: ") + e);
  return 14 + 3 * M + F;
}

int olsr_map_ply_pack(int32_t P, int32_t M, int32_t F, const olsr_map_buffers* src, float* rows, void* hip_stream) {
  if (const char* e = map_ply_sizes_error(M, F)) return fail(OLSR_ERR_ARG, std::string("map_ply_pack: ") + e);
  if (P < 0) return fail(OLSR_ERR_ARG, "map_ply_pack: P must be >= 0");
  if (P == 0) return OLSR_OK;
  if (const char* e = map_ply_buffers_error(src, F)) return fail(OLSR_ERR_ARG, std::string("map_ply_pack: ") + e);
  if (!rows || (uintptr_t)rows % 4) return fail(OLSR_ERR_ARG, "map_ply_pack: rows is required, aligned to 4 bytes");
  launch_map_ply_pack(P, M, F, *src, rows, (hipStream_t)hip_stream);
  return launch_check("map_ply_pack");
}

int olsr_map_ply_unpack(int32_t P, int32_t M, int32_t F, int32_t n_cols, const int32_t* col, const float* rows,
                        const olsr_map_buffers* dst, void* hip_stream) {
  if (const char* e = map_ply_sizes_error(M, F)) return fail(OLSR_ERR_ARG, std::string("map_ply_unpack: ") + e);
  if (P < 0) return fail(OLSR_ERR_ARG, "map_ply_unpack: P must be >= 0");
  if (n_cols < 1 || n_cols > OLSR_MAP_PLY_MAX_COLS)
    return fail(OLSR_ERR_ARG, "map_ply_unpack: n_cols must lie in 1 ... OLSR_MAP_PLY_MAX_COLS");
  if (!col) return fail(OLSR_ERR_ARG, "map_ply_unpack: col is required");
  const int width = 14 + 3 * M + F, lang0 = 6 + 3 * M;
  for (int j = 0; j < width; ++j) {
    if (col[j] >= n_cols || col[j] < -1) return fail(OLSR_ERR_ARG, "map_ply_unpack: a col[j] lies outside -1 ... n_cols - 1");
    // (a normal is never stored: its entry is not read)
    if (col[j] == -1 && !(j >= 3 && j < 6) && !(j >= lang0 && j < lang0 + F))
      return fail(OLSR_ERR_ARG, "map_ply_unpack: only a normal or a language channel may be absent (col[j] = -1)");
  }
  if (P == 0) return OLSR_OK;
  if (const char* e = map_ply_buffers_error(dst, F)) return fail(OLSR_ERR_ARG, std::string("map_ply_unpack: ") + e);
  if (!rows || (uintptr_t)rows % 4) return fail(OLSR_ERR_ARG, "map_ply_unpack: rows is required, aligned to 4 bytes");
  launch_map_ply_unpack(P, M, F, n_cols, col, rows, *dst, (hipStream_t)hip_stream);
  return launch_check("map_ply_unpack");
}

// ---- the CLIP ConvNeXt image tower (include/olsr_clip_trunk.h)
static const char* convnext_block_sizes_error(int64_t C, int64_t h, int64_t w) {
  if (C < 64 || C % 64 != 0 || C > OLSR_CLIP_TRUNK_MAX_DIM) return "C must be a multiple of 64 in 64 ... 4096";
  if (h < 1 || w < 1) return "h and w must be >= 1";
  if (h > 0x7FFFFFFF / w || h * w > 0x7FFFFFFF / (4 * C)) return "4 C h w must stay below 2^31";
  return nullptr;
}

size_t olsr_convnext_block_workspace_bytes(int32_t C, int32_t h, int32_t w) {
  return convnext_block_sizes_error(C, h, w) ? 0 : convnext_block_workspace_bytes(C, h, w);
}

int olsr_convnext_block(const olsr_convnext_block_params* p, const float* x, const float* block_params, float* y,
                        void* workspace, void* hip_stream) {
  if (!p) return fail(OLSR_ERR_ARG, "convnext_block: the parameter struct is NULL");
  if (const char* e = convnext_block_sizes_error(p->C, p->h, p->w)) return fail(OLSR_ERR_ARG, std::string("convnext_block: ") + e);
  if (!(p->ln_eps > 0.0) || !std::isfinite(p->ln_eps)) return fail(OLSR_ERR_ARG, "convnext_block: ln_eps must be positive");
  if (!x || !block_params || !y || !workspace)
    return fail(OLSR_ERR_ARG, "convnext_block: x, block_params, y and workspace are required");
  if ((uintptr_t)block_params % 16 || (uintptr_t)workspace % 16 || (uintptr_t)x % 4 || (uintptr_t)y % 4)
    return fail(OLSR_ERR_ARG, "convnext_block: block_params and workspace must be 16-byte aligned, x and y 4-byte aligned");
  if (p->workspace_bytes < (uint64_t)convnext_block_workspace_bytes(p->C, p->h, p->w))
    return fail(OLSR_ERR_ARG, "convnext_block: the workspace is smaller than olsr_convnext_block_workspace_bytes");
  return launch_check("convnext_block",
                      launch_convnext_block(*p, x, block_params, y, (float*)workspace, (hipStream_t)hip_stream));
}

// what is wrong with a tower's configuration, if anything (launches, ln_eps and the workspace are the forward's own checks)
static const char* clip_trunk_config_error(const olsr_clip_trunk_params* p) {
  if (!p) return "the parameter struct is NULL";
  for (int i = 0; i < 4; ++i) {
    if (p->dims[i] < 64 || p->dims[i] % 64 != 0 || p->dims[i] > OLSR_CLIP_TRUNK_MAX_DIM)
      return "every dim must be a multiple of 64 in 64 ... 4096";
    if (p->depths[i] < 1 || p->depths[i] > OLSR_CLIP_TRUNK_MAX_LAUNCHES) return "every depth must lie in 1 ... 128";
  }
  if (p->embed_dim < 16 || p->embed_dim % 16 != 0 || p->embed_dim > OLSR_CLIP_TRUNK_MAX_DIM)
    return "embed_dim must be a multiple of 16 in 16 ... 4096";
  if (p->R < 32 || p->R % 32 != 0 || p->R > 4096) return "R must be a multiple of 32 in 32 ... 4096";
  if (p->H < 1 || p->W < 1 || (int64_t)p->H * p->W > (int64_t)0x7FFFFFFF / 3) return "H, W must be >= 1 and 3 H W below 2^31";
  if (clip_trunk_launches(*p) > OLSR_CLIP_TRUNK_MAX_LAUNCHES) return "the depths need more launches than the mask holds";
  for (int i = 0; i < 4; ++i) {
    const int64_t side = p->R >> (2 + i);
    if (side * side > (int64_t)0x7FFFFFFF / (4 * (int64_t)p->dims[i])) return "a stage's hidden map must stay below 2^31 elements";
  }
  for (int c = 0; c < 3; ++c)
    if (!std::isfinite(p->mean[c]) || !std::isfinite(p->std[c]) || p->std[c] == 0.0f) return "mean must be finite, std finite and not 0";
  return nullptr;
}

size_t olsr_clip_trunk_workspace_bytes(const olsr_clip_trunk_params* p) {
  return clip_trunk_config_error(p) ? 0 : clip_trunk_workspace_bytes(*p);
}

size_t olsr_clip_trunk_packed_floats(const olsr_clip_trunk_params* p) {
  return clip_trunk_config_error(p) ? 0 : (size_t)clip_trunk_packed_floats(*p);
}

int32_t olsr_clip_trunk_launches(const olsr_clip_trunk_params* p) {
  return clip_trunk_config_error(p) ? 0 : (int32_t)clip_trunk_launches(*p);
}

int olsr_clip_trunk_forward(const olsr_clip_trunk_params* p, const float* image, const float* packed_params, float* res2,
                            float* res3, float* clip_vis_dense, void* workspace, void* hip_stream) {
  if (const char* e = clip_trunk_config_error(p)) return fail(OLSR_ERR_ARG, std::string("clip_trunk_forward: ") + e);
  if (!(p->ln_eps > 0.0) || !std::isfinite(p->ln_eps)) return fail(OLSR_ERR_ARG, "clip_trunk_forward: ln_eps must be positive");
  const int n = (int)clip_trunk_launches(*p);
  for (int k = n; k < OLSR_CLIP_TRUNK_MAX_LAUNCHES; ++k)
    if ((p->launches[k >> 6] >> (k & 63)) & 1u) return fail(OLSR_ERR_ARG, "clip_trunk_forward: launches names a launch that does not exist");
  if (!image || !packed_params || !res2 || !res3 || !clip_vis_dense || !workspace)
    return fail(OLSR_ERR_ARG, "clip_trunk_forward: image, packed_params, res2, res3, clip_vis_dense and workspace are required");
  if ((uintptr_t)packed_params % 16 || (uintptr_t)workspace % 16)
    return fail(OLSR_ERR_ARG, "clip_trunk_forward: packed_params and workspace must be 16-byte aligned");
  if ((uintptr_t)image % 4 || (uintptr_t)res2 % 4 || (uintptr_t)res3 % 4 || (uintptr_t)clip_vis_dense % 4)
    return fail(OLSR_ERR_ARG, "clip_trunk_forward: image, res2, res3 and clip_vis_dense must be 4-byte aligned");
  if (p->workspace_bytes < (uint64_t)clip_trunk_workspace_bytes(*p))
    return fail(OLSR_ERR_ARG, "clip_trunk_forward: the workspace is smaller than olsr_clip_trunk_workspace_bytes");
  return launch_check("clip_trunk_forward", launch_clip_trunk(*p, image, packed_params, res2, res3, clip_vis_dense,
                                                              (float*)workspace, (hipStream_t)hip_stream));
}

// what is wrong with a TSDF volume, if anything (surface: the extraction's tighter size limit)
static const char* tsdf_volume_error(const olsr_tsdf_volume* v, bool surface) {
  if (!v) return "volume is required";
  if (v->X < 1 || v->Y < 1 || v->Z < 1) return "volume: X, Y, Z must be >= 1";
  const int64_t limit = surface ? (((int64_t)1 << 31) - 1) / 3 : ((int64_t)1 << 31) - 1;
  if ((int64_t)v->X * v->Y > limit || (int64_t)v->X * v->Y * v->Z > limit)
    return surface ? "volume: 3 X Y Z must be below 2^31" : "volume: X Y Z must be below 2^31";
  if (v->feat_mode == OLSR_TSDF_FEAT_PACKED_RGB) {
    if (v->F != 1) return "volume: F must be 1 with OLSR_TSDF_FEAT_PACKED_RGB";
  } else if (v->feat_mode != OLSR_TSDF_FEAT_FLOAT) {
    return "volume: unknown feat_mode";
  } else if (!supported_F(v->F)) {
    return "volume: F must be one of 0, 3, 15, 16, 32";
  }
  if (!(v->voxel_size > 0.0f) || !(v->trunc_margin > 0.0f)) return "volume: voxel_size and trunc_margin must be > 0";
  if (!v->tsdf || !v->weight || (v->F > 0 && !v->feat)) return "volume: tsdf, weight and (F > 0) feat are required";
  return nullptr;
}

int olsr_tsdf_init(const olsr_tsdf_volume* volume, void* hip_stream) {
  if (const char* e = tsdf_volume_error(volume, false)) return fail(OLSR_ERR_ARG, std::string("tsdf_init: ") + e);
  launch_tsdf_init(*volume, (hipStream_t)hip_stream);
  return launch_check("tsdf_init");
}

int olsr_tsdf_integrate(const olsr_tsdf_volume* volume, int32_t n_views, const olsr_tsdf_view* views, void* hip_stream) {
  if (const char* e = tsdf_volume_error(volume, false)) return fail(OLSR_ERR_ARG, std::string("tsdf_integrate: ") + e);
  if (n_views < 1 || n_views > OLSR_TSDF_MAX_VIEWS || !views)
    return fail(OLSR_ERR_ARG, "tsdf_integrate: between 1 and 16 views");
  for (int v = 0; v < n_views; ++v) {
    const olsr_tsdf_view& c = views[v];
    if (c.H < 1 || c.W < 1 || (int64_t)c.H * c.W > (((int64_t)1 << 31) - 1) / 32)
      return fail(OLSR_ERR_ARG, "tsdf_integrate: a view's H, W must be >= 1 and 32 H W below 2^31");
    if (!c.depth || (volume->F > 0 && !c.feat)) return fail(OLSR_ERR_ARG, "tsdf_integrate: a view's depth and (F > 0) feat are required");
    if (c.feat_layout != OLSR_TSDF_IMAGE_CHANNELS && c.feat_layout != OLSR_TSDF_IMAGE_ROWS)
      return fail(OLSR_ERR_ARG, "tsdf_integrate: unknown feat_layout");
  }
  launch_tsdf_integrate(*volume, n_views, views, (hipStream_t)hip_stream);
  return launch_check("tsdf_integrate");
}

size_t olsr_tsdf_surface_scratch_bytes(int32_t X, int32_t Y, int32_t Z) { return tsdf_surface_scratch_bytes(X, Y, Z); }

int olsr_tsdf_surface_plan(const olsr_tsdf_volume* volume, float min_weight, void* scratch, int32_t* status, void* hip_stream) {
  if (const char* e = tsdf_volume_error(volume, true)) return fail(OLSR_ERR_ARG, std::string("tsdf_surface_plan: ") + e);
  if (!scratch || !status) return fail(OLSR_ERR_ARG, "tsdf_surface_plan: scratch and status are required");
  launch_tsdf_surface_plan(*volume, min_weight, scratch, status, (hipStream_t)hip_stream);
  return launch_check("tsdf_surface_plan");
}

int olsr_tsdf_surface_emit(const olsr_tsdf_volume* volume, float min_weight, const void* scratch, int32_t capacity,
                           float* points, float* feats, int32_t* voxel_index, void* hip_stream) {
  if (const char* e = tsdf_volume_error(volume, true)) return fail(OLSR_ERR_ARG, std::string("tsdf_surface_emit: ") + e);
  if (capacity < 0 || !scratch) return fail(OLSR_ERR_ARG, "tsdf_surface_emit: scratch and capacity >= 0 are required");
  if (capacity == 0) return OLSR_OK;
  if (!points || (volume->F > 0 && !feats)) return fail(OLSR_ERR_ARG, "tsdf_surface_emit: points and (F > 0) feats are required");
  launch_tsdf_surface_emit(*volume, min_weight, scratch, capacity, points, volume->F > 0 ? feats : nullptr, voxel_index,
                           (hipStream_t)hip_stream);
  return launch_check("tsdf_surface_emit");
}

size_t olsr_tsdf_mesh_scratch_bytes(int32_t X, int32_t Y, int32_t Z) { return tsdf_mesh_scratch_bytes(X, Y, Z); }

int olsr_tsdf_mesh_plan(const olsr_tsdf_volume* volume, float min_weight, void* scratch, int32_t* status, void* hip_stream) {
  if (const char* e = tsdf_volume_error(volume, true)) return fail(OLSR_ERR_ARG, std::string("tsdf_mesh_plan: ") + e);
  if (!scratch || !status) return fail(OLSR_ERR_ARG, "tsdf_mesh_plan: scratch and status are required");
  launch_tsdf_mesh_plan(*volume, min_weight, scratch, status, (hipStream_t)hip_stream);
  return launch_check("tsdf_mesh_plan");
}

int olsr_tsdf_mesh_emit(const olsr_tsdf_volume* volume, float min_weight, const void* scratch, int32_t vert_capacity,
                        int32_t face_capacity, float* points, float* normals, float* feats, int32_t* voxel_index, int32_t* faces,
                        void* hip_stream) {
  if (const char* e = tsdf_volume_error(volume, true)) return fail(OLSR_ERR_ARG, std::string("tsdf_mesh_emit: ") + e);
  if (vert_capacity < 0 || face_capacity < 0 || !scratch)
    return fail(OLSR_ERR_ARG, "tsdf_mesh_emit: scratch, vert_capacity >= 0 and face_capacity >= 0 are required");
  if (face_capacity > INT32_MAX / 3) return fail(OLSR_ERR_ARG, "tsdf_mesh_emit: 3 face_capacity must be below 2^31");
  if (vert_capacity == 0 && face_capacity == 0) return OLSR_OK;
  if (vert_capacity > 0 && (!points || !normals || (volume->F > 0 && !feats)))
    return fail(OLSR_ERR_ARG, "tsdf_mesh_emit: points, normals and (F > 0) feats are required");
  if (face_capacity > 0 && !faces) return fail(OLSR_ERR_ARG, "tsdf_mesh_emit: faces is required");
  (void)min_weight;  // (the plan's words hold what it decided)
  launch_tsdf_mesh_emit(*volume, scratch, vert_capacity, face_capacity, points, normals, volume->F > 0 ? feats : nullptr,
                        voxel_index, faces, (hipStream_t)hip_stream);
  return launch_check("tsdf_mesh_emit");
}

size_t olsr_emd_scratch_bytes(int32_t B, int64_t total1, int64_t total2) { return emd_scratch_bytes(B, total1, total2); }

int olsr_emd_cost(int32_t B, const int32_t* off1, const int32_t* off2, int32_t max_n1, int32_t max_n2, const float* xyz1,
                  const float* xyz2, double* cost, float* residual, int32_t* valid, void* scratch, void* hip_stream) {
  CloudSegments seg;
  OLSR_TRY(cloud_segments("emd_cost", B, off1, off2, max_n1, max_n2, xyz1, xyz2, cost && valid, true, true, scratch,
                          emd_scratch_offsets, (hipStream_t)hip_stream, &seg));
  launch_emd_cost(B, seg.dev1, seg.dev2, seg.total1, seg.total2, max_n1, max_n2, xyz1, xyz2, cost, residual, valid, scratch,
                  (hipStream_t)hip_stream);
  return launch_check("emd_cost");
}

size_t olsr_chamfer_scratch_bytes(int32_t B, int64_t total1, int64_t total2) {
  return chamfer_scratch_bytes(B, total1, total2);
}

int olsr_chamfer(int32_t B, const int32_t* off1, const int32_t* off2, int32_t max_n1, int32_t max_n2, const float* xyz1,
                 const float* xyz2, float* min_d2_1, int32_t* nn_1, float* min_d2_2, int32_t* nn_2, double* mean,
                 int32_t* valid, void* scratch, void* hip_stream) {
  CloudSegments seg;
  OLSR_TRY(cloud_segments("chamfer", B, off1, off2, max_n1, max_n2, xyz1, xyz2, mean && valid, min_d2_1 && nn_1,
                          min_d2_2 && nn_2, scratch,
                          chamfer_scratch_offsets, (hipStream_t)hip_stream, &seg));
  launch_chamfer(B, seg.dev1, seg.dev2, seg.total1, seg.total2, max_n1, max_n2, xyz1, xyz2, min_d2_1, nn_1, min_d2_2, nn_2,
                 mean, valid, scratch, (hipStream_t)hip_stream);
  return launch_check("chamfer");
}

int olsr_mask_smooth(int32_t P, int32_t H, int32_t W, const uint8_t* mask_in, uint8_t* mask_out, void* hip_stream) {
  if (const char* e = query_eval_size_error(P, H, W)) return fail(OLSR_ERR_ARG, std::string("mask_smooth: ") + e);
  if (!mask_in || !mask_out) return fail(OLSR_ERR_ARG, "mask_smooth: mask_in and mask_out are required");
  if (mask_in == mask_out) return fail(OLSR_ERR_ARG, "mask_smooth: mask_out must not be mask_in (a tile reads its neighbours' pixels)");
  launch_mask_smooth(P, H, W, mask_in, mask_out, (hipStream_t)hip_stream);
  return launch_check("mask_smooth");
}

size_t olsr_query_eval_scratch_bytes(int32_t P, int32_t H, int32_t W) {
  return query_eval_size_error(P, H, W) ? ALIGN : query_eval_scratch_bytes(P, H, W);
}

int olsr_query_eval(int32_t P, int32_t H, int32_t W, const uint8_t* mask, const float* smoothed, const float* score,
                    const uint8_t* gt_mask, const float* boxes, const int32_t* box_offsets, int32_t* result,
                    uint8_t* mask_smoothed, void* scratch, void* hip_stream) {
  const hipStream_t st = (hipStream_t)hip_stream;
  if (const char* e = query_eval_size_error(P, H, W)) return fail(OLSR_ERR_ARG, std::string("query_eval: ") + e);
  if (!mask || !smoothed || !score || !gt_mask) return fail(OLSR_ERR_ARG, "query_eval: mask, smoothed, score and gt_mask are required");
  if (!box_offsets) return fail(OLSR_ERR_ARG, "query_eval: box_offsets is required");
  if (!result || !scratch) return fail(OLSR_ERR_ARG, "query_eval: result and scratch are required");
  if (mask_smoothed == mask) return fail(OLSR_ERR_ARG, "query_eval: mask_smoothed must not be mask (a tile reads its neighbours' pixels)");
  std::vector<int32_t> h;
  bool on_device;
  OLSR_TRY(cloud_offsets("query_eval", "box_offsets", P, box_offsets, 0x7FFFFFFF, st, h, &on_device));
  if (h[P] > 0 && !boxes) return fail(OLSR_ERR_ARG, "query_eval: boxes is required when box_offsets lists any");
  const int32_t* dev = box_offsets;
  if (!on_device) {
    int32_t* park = query_eval_scratch_offsets(scratch, P, H, W);
    HIP_TRY(hipMemcpyAsync(park, h.data(), h.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));   // h goes away
    dev = park;
  }
  launch_query_eval(P, H, W, mask, smoothed, score, gt_mask, boxes, dev, result, mask_smoothed, scratch, st);
  return launch_check("query_eval");
}

size_t olsr_image_psnr_scratch_bytes(void) { return image_psnr_scratch_bytes(); }

int olsr_image_psnr(int32_t C, int32_t H, int32_t W, const float* image, const float* gt, double* out, void* scratch,
                    void* hip_stream) {
  if (C < 1 || H < 1 || W < 1) return fail(OLSR_ERR_ARG, "image_psnr: C, H and W must be >= 1");
  const int64_t n = (int64_t)C * (int64_t)H * (int64_t)W;
  if (n > (int64_t)0x7FFFFFFF) return fail(OLSR_ERR_ARG, "image_psnr: C * H * W must fit an int32");
  if (!image || !gt || !out || !scratch) return fail(OLSR_ERR_ARG, "image_psnr: image, gt, out and scratch are required");
  launch_image_psnr(n, image, gt, out, scratch, (hipStream_t)hip_stream);
  return launch_check("image_psnr");
}

}  // extern "C"

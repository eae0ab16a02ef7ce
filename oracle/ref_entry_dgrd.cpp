// ref_entry_dgrd.cpp — a C ABI over the disentangled reference rasteriser's own entry points, built on the host.
// TEST INFRASTRUCTURE ONLY.
//
// Compiled by oracle/ref_build.py together with DGR-D's cuda_rasterizer sources (copied, not committed; DGR-D =
// submodules/diff-gaussian-rasterization-disentangle-optim) and the execution model of oracle/ref_shim/.  It drives
// CudaRasterizer::LanguageRasterizer of DGR-D exactly as DGR-D's torch binding does: buffers through the four resize
// callbacks (geometry, binning, binning_lang, image), zero-filled outputs, language_M = 0.  A Gaussian carries two
// opacity / scale / rotation (or 3D covariance) sets: the first arrives in `s`, the second in `s2`, of which only
// opacities, scales, rotations and cov3D_precomp are read.  F == NUM_LANGUAGE_CHANNELS of this build.
//
// Symbols are refd_*, so that a library of this family can sit in one process beside those of ref_entry.cpp.
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <tuple>
#include <vector>

#include <cuda_runtime.h>
#define GLM_FORCE_CUDA
#include <glm/glm.hpp>

#include "auxiliary.h"
#include "backward.h"
#include "config.h"
#include "rasterizer.h"
#include "rasterizer_impl.h"

#include "olsr.h"

namespace {

struct RefState {
  int P = 0, F = 0, W = 0, H = 0, R = 0, R_lang = 0;
  // DGR-D leaves the rows of culled Gaussians unwritten: every chunk is zeroed before the call
  std::vector<char> geom, binning, binning_lang, img;
};

std::function<char*(size_t)> resizer(std::vector<char>& v) {
  return [&v](size_t n) {
    v.assign(n, 0);
    return v.data();
  };
}

bool check_scene(const olsr_scene* s, const olsr_scene* s2) {
  if (!s || !s2 || s->P <= 0 || s->width <= 0 || s->height <= 0) return false;
  if (s->tile != BLOCK_X || BLOCK_X != BLOCK_Y) return false;
  if (s->F != NUM_LANGUAGE_CHANNELS || s->language_precomp == nullptr) return false;
  if ((s->shs == nullptr) == (s->colors_precomp == nullptr)) return false;
  for (const olsr_scene* t : {s, s2}) {
    const bool has_sr = t->scales != nullptr && t->rotations != nullptr;
    if (has_sr == (t->cov3D_precomp != nullptr)) return false;
  }
  return true;
}

bool same_shape(const RefState& st, const olsr_scene* s) {
  return st.P == s->P && st.F == s->F && st.W == s->width && st.H == s->height;
}

void zero(float* p, size_t n) { std::fill(p, p + n, 0.f); }

}  // namespace

extern "C" {

int refd_tile() { return BLOCK_X; }
int refd_language_channels() { return NUM_LANGUAGE_CHANNELS; }

void* refd_create() { return new RefState(); }
void refd_destroy(void* h) { delete (RefState*)h; }

int refd_forward(void* h, const olsr_scene* s, const olsr_scene* s2, float* out_color, float* out_language, float* out_depth,
                 float* out_opacity, float* out_opacity_lang, int32_t* radii, int32_t* radii_lang, int32_t* n_touched,
                 int32_t* n_touched_lang, int32_t* num_rendered, int32_t* num_rendered_lang) {
  if (!h || !check_scene(s, s2)) return OLSR_ERR_ARG;
  RefState& st = *(RefState*)h;
  const int P = s->P, W = s->width, H = s->height, F = s->F;
  st.P = P; st.F = F; st.W = W; st.H = H;
  const size_t N = (size_t)W * H;
  zero(out_color, 3 * N);
  zero(out_language, (size_t)F * N);
  zero(out_depth, N);
  zero(out_opacity, N);
  zero(out_opacity_lang, N);
  for (int32_t* p : {radii, radii_lang, n_touched, n_touched_lang}) std::fill(p, p + P, 0);
  try {
    std::tie(st.R, st.R_lang) = CudaRasterizer::LanguageRasterizer::forward(
        resizer(st.geom), resizer(st.binning), resizer(st.binning_lang), resizer(st.img), P, s->D, s->M, 0, s->background, W,
        H, s->means3D, s->shs, s->colors_precomp, s->language_precomp, s->opacities, s2->opacities, s->scales, s2->scales,
        s->scale_modifier, s->rotations, s2->rotations, s->cov3D_precomp, s2->cov3D_precomp, s->viewmatrix, s->projmatrix,
        s->cam_pos, s->tan_fovx, s->tan_fovy, s->prefiltered != 0, out_color, out_language, out_depth, out_opacity,
        out_opacity_lang, radii, radii_lang, n_touched, n_touched_lang, s->debug != 0);
  } catch (const std::exception&) {
    return OLSR_ERR_ARG;
  }
  *num_rendered = st.R;
  *num_rendered_lang = st.R_lang;
  return OLSR_OK;
}

// Every output of DGR-D's backward.  dL_dout_depth may be NULL: the binding always passes a tensor, zeros then.
int refd_backward(void* h, const olsr_scene* s, const olsr_scene* s2, const int32_t* radii, const int32_t* radii_lang,
                  const float* dL_dout_color, const float* dL_dout_language, const float* dL_dout_depth, float* dL_dmeans2D,
                  float* dL_dconic, float* dL_dconic_lang, float* dL_dopacity, float* dL_dopacity_lang, float* dL_dcolors,
                  float* dL_dlanguage, float* dL_ddepths, float* dL_dmeans3D, float* dL_dcov3D, float* dL_dcov3D_lang,
                  float* dL_dsh, float* dL_dscales, float* dL_dscales_lang, float* dL_drotations, float* dL_drotations_lang,
                  float* dL_dtau) {
  if (!h || !check_scene(s, s2) || !s->projmatrix_raw) return OLSR_ERR_ARG;
  RefState& st = *(RefState*)h;
  if (!same_shape(st, s)) return OLSR_ERR_ARG;
  const size_t P = s->P, F = s->F, M = s->M, N = (size_t)s->width * s->height;
  // torch::zeros for every gradient, as the binding allocates them
  zero(dL_dmeans2D, 3 * P);
  zero(dL_dconic, 4 * P);
  zero(dL_dconic_lang, 4 * P);
  zero(dL_dopacity, P);
  zero(dL_dopacity_lang, P);
  zero(dL_dcolors, 3 * P);
  zero(dL_dlanguage, F * P);
  zero(dL_ddepths, P);
  zero(dL_dmeans3D, 3 * P);
  zero(dL_dcov3D, 6 * P);
  zero(dL_dcov3D_lang, 6 * P);
  if (M > 0) zero(dL_dsh, 3 * M * P);
  zero(dL_dscales, 3 * P);
  zero(dL_dscales_lang, 3 * P);
  zero(dL_drotations, 4 * P);
  zero(dL_drotations_lang, 4 * P);
  zero(dL_dtau, 6 * P);
  std::vector<float> no_depth;
  if (!dL_dout_depth) {
    no_depth.assign(N, 0.f);
    dL_dout_depth = no_depth.data();
  }
  CudaRasterizer::LanguageRasterizer::backward(
      (int)P, s->D, (int)M, 0, st.R, st.R_lang, s->background, s->width, s->height, s->means3D, s->shs, s->colors_precomp,
      s->language_precomp, s->scales, s2->scales, s->scale_modifier, s->rotations, s2->rotations, s->cov3D_precomp,
      s2->cov3D_precomp, s->viewmatrix, s->projmatrix, s->projmatrix_raw, s->cam_pos, s->tan_fovx, s->tan_fovy, radii,
      radii_lang, st.geom.data(), st.binning.data(), st.binning_lang.data(), st.img.data(), dL_dout_color, dL_dout_language,
      dL_dout_depth, dL_dmeans2D, dL_dconic, dL_dconic_lang, dL_dopacity, dL_dopacity_lang, dL_dcolors, dL_dlanguage,
      dL_ddepths, dL_dmeans3D, dL_dcov3D, dL_dcov3D_lang, dL_dsh, dL_dscales, dL_dscales_lang, dL_drotations,
      dL_drotations_lang, dL_dtau, s->debug != 0);
  return OLSR_OK;
}

// The per-Gaussian half alone: DGR-D's computeCov2DCUDA, computeCov2DCUDA_no_tau and language_preprocessCUDA
// (BACKWARD::language_preprocess launches exactly these three), on composite-level gradients that the CALLER provides.
int refd_backward_chain(void* h, const olsr_scene* s, const olsr_scene* s2, const int32_t* radii, const int32_t* radii_lang,
                        const float* dL_dmeans2D_in, const float* dL_dconic_in, const float* dL_dconic_lang_in,
                        const float* dL_dcolors_in, const float* dL_ddepths_in, float* dL_dmeans3D, float* dL_dcov3D,
                        float* dL_dcov3D_lang, float* dL_dsh, float* dL_dscales, float* dL_dscales_lang, float* dL_drotations,
                        float* dL_drotations_lang, float* dL_dtau) {
  if (!h || !check_scene(s, s2) || !s->projmatrix_raw) return OLSR_ERR_ARG;
  RefState& st = *(RefState*)h;
  if (!same_shape(st, s)) return OLSR_ERR_ARG;
  const size_t P = s->P, F = s->F, M = s->M;
  zero(dL_dmeans3D, 3 * P);
  zero(dL_dcov3D, 6 * P);
  zero(dL_dcov3D_lang, 6 * P);
  if (M > 0) zero(dL_dsh, 3 * M * P);
  zero(dL_dscales, 3 * P);
  zero(dL_dscales_lang, 3 * P);
  zero(dL_drotations, 4 * P);
  zero(dL_drotations_lang, 4 * P);
  zero(dL_dtau, 6 * P);
  // the chain's inputs it is declared to write (dL_dcolor, dL_dlanguage, dL_ddepth are non-const there) are copies
  std::vector<float> colors(dL_dcolors_in, dL_dcolors_in + 3 * P), depths(dL_ddepths_in, dL_ddepths_in + P);
  std::vector<float> language(F * P, 0.f);
  char* p = st.geom.data();
  const auto g = CudaRasterizer::LanguageGeometryState::fromChunk(p, P);
  const float focal_y = s->height / (2.0f * s->tan_fovy);
  const float focal_x = s->width / (2.0f * s->tan_fovx);
  const float* cov3D_ptr = s->cov3D_precomp ? s->cov3D_precomp : g.cov3D;
  const float* cov3D_ptr_lang = s2->cov3D_precomp ? s2->cov3D_precomp : g.cov3D_lang;
  BACKWARD::language_preprocess(
      (int)P, s->D, (int)M, 0, (const float3*)s->means3D, radii, radii_lang, s->shs, g.clamped, (const glm::vec3*)s->scales,
      (const glm::vec3*)s2->scales, (const glm::vec4*)s->rotations, (const glm::vec4*)s2->rotations, s->scale_modifier,
      cov3D_ptr, cov3D_ptr_lang, s->viewmatrix, s->projmatrix, s->projmatrix_raw, focal_x, focal_y, s->tan_fovx, s->tan_fovy,
      (const glm::vec3*)s->cam_pos, (const float3*)dL_dmeans2D_in, dL_dconic_in, dL_dconic_lang_in, (glm::vec3*)dL_dmeans3D,
      colors.data(), language.data(), depths.data(), dL_dcov3D, dL_dcov3D_lang, dL_dsh, (glm::vec3*)dL_dscales,
      (glm::vec3*)dL_dscales_lang, (glm::vec4*)dL_drotations, (glm::vec4*)dL_drotations_lang, dL_dtau);
  return OLSR_OK;
}

// State inspection by name; the second set's fields carry the suffix _lang.  Returns the element count; copies into dst
// if non-NULL.
int64_t refd_get_field(void* h, const char* name, void* dst) {
  RefState& st = *(RefState*)h;
  auto cp = [&](const void* src, size_t n, size_t esz) -> int64_t {
    if (dst && n) std::memcpy(dst, src, n * esz);
    return (int64_t)n;
  };
  const size_t P = st.P, N = (size_t)st.W * st.H;
  const size_t tiles = (size_t)((st.W + BLOCK_X - 1) / BLOCK_X) * ((st.H + BLOCK_Y - 1) / BLOCK_Y);
  char* gp = st.geom.data();
  const auto g = CudaRasterizer::LanguageGeometryState::fromChunk(gp, P);
  char* bp = st.binning.data();
  const auto b = CudaRasterizer::BinningState::fromChunk(bp, st.R);
  char* bp2 = st.binning_lang.data();
  const auto b2 = CudaRasterizer::BinningState::fromChunk(bp2, st.R_lang);
  char* ip = st.img.data();
  const auto im = CudaRasterizer::LanguageImageState::fromChunk(ip, N);
  auto is = [&](const char* n) { return !std::strcmp(name, n); };
  if (is("depths")) return cp(g.depths, P, 4);
  if (is("means2D")) return cp(g.means2D, 2 * P, 4);
  if (is("cov3D")) return cp(g.cov3D, 6 * P, 4);
  if (is("cov3D_lang")) return cp(g.cov3D_lang, 6 * P, 4);
  if (is("conic_opacity")) return cp(g.conic_opacity, 4 * P, 4);
  if (is("conic_opacity_lang")) return cp(g.conic_opacity_lang, 4 * P, 4);
  if (is("rgb")) return cp(g.rgb, 3 * P, 4);
  if (is("clamped")) return cp(g.clamped, 3 * P, 1);
  if (is("tiles_touched")) return cp(g.tiles_touched, P, 4);
  if (is("tiles_touched_lang")) return cp(g.tiles_touched_lang, P, 4);
  if (is("point_offsets")) return cp(g.point_offsets, P, 4);
  if (is("point_offsets_lang")) return cp(g.point_offsets_lang, P, 4);
  if (is("point_list")) return cp(b.point_list, st.R, 4);
  if (is("point_list_lang")) return cp(b2.point_list, st.R_lang, 4);
  if (is("keys")) return cp(b.point_list_keys, st.R, 8);
  if (is("keys_lang")) return cp(b2.point_list_keys, st.R_lang, 8);
  if (is("ranges")) return cp(im.ranges, 2 * tiles, 4);
  if (is("ranges_lang")) return cp(im.ranges_lang, 2 * tiles, 4);
  if (is("final_T")) return cp(im.accum_alpha, N, 4);
  if (is("final_T_lang")) return cp(im.accum_alpha_lang, N, 4);
  if (is("n_contrib")) return cp(im.n_contrib, N, 4);
  if (is("n_contrib_lang")) return cp(im.n_contrib_lang, N, 4);
  return -1;
}

}  // extern "C"

// ref_entry.cpp — a C ABI over the reference rasteriser's own entry points, built on the host.  TEST INFRASTRUCTURE ONLY.
//
// Compiled by oracle/ref_build.py together with the reference's cuda_rasterizer sources (copied, not committed) and the
// execution model of oracle/ref_shim/.  Everything below drives CudaRasterizer::Rasterizer (no language, F == 0) and
// CudaRasterizer::LanguageRasterizer (F == NUM_LANGUAGE_CHANNELS of this build) exactly as the reference's torch binding
// does: buffers through the three resize callbacks, zero-filled outputs, language_M = 0.  Key building, the sort, the tile
// ranges and the carving of the state buffers are therefore the reference's own code as well.
//
// The functions mirror oracle.cpp's (oracle_forward, oracle_backward, oracle_backward_chain, oracle_get_field), so that
// oracle/oracle_ref.py can present this library with the surface of oracle/oracle_C.py.
#include <cstdint>
#include <cstring>
#include <stdexcept>
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
  int P = 0, F = 0, W = 0, H = 0, R = 0;
  std::vector<char> geom, binning, img;
  std::vector<int> n_touched;
};

std::function<char*(size_t)> resizer(std::vector<char>& v) {
  return [&v](size_t n) {
    v.assign(n, 0);
    return v.data();
  };
}

bool check_scene(const olsr_scene* s) {
  if (!s || s->P <= 0 || s->width <= 0 || s->height <= 0) return false;
  if (s->tile != BLOCK_X || BLOCK_X != BLOCK_Y) return false;
  if (s->F != 0 && s->F != NUM_LANGUAGE_CHANNELS) return false;
  if ((s->shs == nullptr) == (s->colors_precomp == nullptr)) return false;
  const bool has_sr = s->scales != nullptr && s->rotations != nullptr;
  if (has_sr == (s->cov3D_precomp != nullptr)) return false;
  if (s->F > 0 && s->language_precomp == nullptr) return false;
  return true;
}

// the per-Gaussian fields both geometry states share, whichever of the two carved the buffer
struct GeomView {
  const float* depths;
  const bool* clamped;
  const float2* means2D;
  const float* cov3D;
  const float4* conic_opacity;
  const float* rgb;
  const uint32_t* point_offsets;
  const uint32_t* tiles_touched;
};

GeomView geom_view(RefState& st) {
  char* p = st.geom.data();
  if (st.F > 0) {
    auto g = CudaRasterizer::LanguageGeometryState::fromChunk(p, st.P);
    return {g.depths, g.clamped, g.means2D, g.cov3D, g.conic_opacity, g.rgb, g.point_offsets, g.tiles_touched};
  }
  auto g = CudaRasterizer::GeometryState::fromChunk(p, st.P);
  return {g.depths, g.clamped, g.means2D, g.cov3D, g.conic_opacity, g.rgb, g.point_offsets, g.tiles_touched};
}

}  // namespace

extern "C" {

int ref_tile() { return BLOCK_X; }
int ref_language_channels() { return NUM_LANGUAGE_CHANNELS; }
const char* ref_variant() {
#ifdef REF_LIBM_EXP
  return "libm_exp";
#else
  return "default";
#endif
}

void* ref_create() { return new RefState(); }
void ref_destroy(void* h) { delete (RefState*)h; }

int ref_forward(void* h, const olsr_scene* s, float* out_color, float* out_language, float* out_depth, float* out_opacity,
                int32_t* radii, int32_t* n_touched, int32_t* num_rendered) {
  if (!h || !check_scene(s)) return OLSR_ERR_ARG;
  RefState& st = *(RefState*)h;
  const int P = s->P, W = s->width, H = s->height, F = s->F;
  st.P = P; st.F = F; st.W = W; st.H = H;
  const size_t N = (size_t)W * H;
  std::fill(out_color, out_color + 3 * N, 0.f);
  if (F > 0) std::fill(out_language, out_language + (size_t)F * N, 0.f);
  std::fill(out_depth, out_depth + N, 0.f);
  std::fill(out_opacity, out_opacity + N, 0.f);
  std::fill(radii, radii + P, 0);
  std::fill(n_touched, n_touched + P, 0);
  try {
    if (F > 0)
      st.R = CudaRasterizer::LanguageRasterizer::forward(
          resizer(st.geom), resizer(st.binning), resizer(st.img), P, s->D, s->M, 0, s->background, W, H, s->means3D, s->shs,
          s->colors_precomp, s->language_precomp, s->opacities, s->scales, s->scale_modifier, s->rotations, s->cov3D_precomp,
          s->viewmatrix, s->projmatrix, s->cam_pos, s->tan_fovx, s->tan_fovy, s->prefiltered != 0, out_color, out_language,
          out_depth, out_opacity, radii, n_touched, s->debug != 0);
    else
      st.R = CudaRasterizer::Rasterizer::forward(
          resizer(st.geom), resizer(st.binning), resizer(st.img), P, s->D, s->M, s->background, W, H, s->means3D, s->shs,
          s->colors_precomp, s->opacities, s->scales, s->scale_modifier, s->rotations, s->cov3D_precomp, s->viewmatrix,
          s->projmatrix, s->cam_pos, s->tan_fovx, s->tan_fovy, s->prefiltered != 0, out_color, out_depth, out_opacity, radii,
          n_touched, s->debug != 0);
  } catch (const std::exception&) {
    return OLSR_ERR_ARG;
  }
  st.n_touched.assign(n_touched, n_touched + P);
  *num_rendered = st.R;
  return OLSR_OK;
}

int ref_backward(void* h, const olsr_scene* s, const int32_t* radii, const float* dL_dout_color,
                 const float* dL_dout_language, const float* dL_dout_depth, float* dL_dmeans2D, float* dL_dconic,
                 float* dL_dopacity, float* dL_dcolors, float* dL_dlanguage, float* dL_ddepths, float* dL_dmeans3D,
                 float* dL_dcov3D, float* dL_dsh, float* dL_dscales, float* dL_drotations, float* dL_dtau) {
  if (!h || !check_scene(s) || !s->projmatrix_raw) return OLSR_ERR_ARG;
  RefState& st = *(RefState*)h;
  const int P = s->P, F = s->F, M = s->M;
  if (st.P != P || st.F != F || st.W != s->width || st.H != s->height) return OLSR_ERR_ARG;
  // torch::zeros for every gradient, as the binding allocates them
  std::fill(dL_dmeans2D, dL_dmeans2D + (size_t)3 * P, 0.f);
  std::fill(dL_dconic, dL_dconic + (size_t)4 * P, 0.f);
  std::fill(dL_dopacity, dL_dopacity + P, 0.f);
  std::fill(dL_dcolors, dL_dcolors + (size_t)3 * P, 0.f);
  if (F > 0) std::fill(dL_dlanguage, dL_dlanguage + (size_t)F * P, 0.f);
  std::fill(dL_ddepths, dL_ddepths + P, 0.f);
  std::fill(dL_dmeans3D, dL_dmeans3D + (size_t)3 * P, 0.f);
  std::fill(dL_dcov3D, dL_dcov3D + (size_t)6 * P, 0.f);
  if (M > 0) std::fill(dL_dsh, dL_dsh + (size_t)3 * M * P, 0.f);
  std::fill(dL_dscales, dL_dscales + (size_t)3 * P, 0.f);
  std::fill(dL_drotations, dL_drotations + (size_t)4 * P, 0.f);
  std::fill(dL_dtau, dL_dtau + (size_t)6 * P, 0.f);
  if (F > 0)
    CudaRasterizer::LanguageRasterizer::backward(
        P, s->D, M, 0, st.R, s->background, s->width, s->height, s->means3D, s->shs, s->colors_precomp, s->language_precomp,
        s->scales, s->scale_modifier, s->rotations, s->cov3D_precomp, s->viewmatrix, s->projmatrix, s->projmatrix_raw,
        s->cam_pos, s->tan_fovx, s->tan_fovy, radii, st.geom.data(), st.binning.data(), st.img.data(), dL_dout_color,
        dL_dout_language, dL_dout_depth, dL_dmeans2D, dL_dconic, dL_dopacity, dL_dcolors, dL_dlanguage, dL_ddepths,
        dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations, dL_dtau, s->debug != 0);
  else
    CudaRasterizer::Rasterizer::backward(
        P, s->D, M, st.R, s->background, s->width, s->height, s->means3D, s->shs, s->colors_precomp, s->scales,
        s->scale_modifier, s->rotations, s->cov3D_precomp, s->viewmatrix, s->projmatrix, s->projmatrix_raw, s->cam_pos,
        s->tan_fovx, s->tan_fovy, radii, st.geom.data(), st.binning.data(), st.img.data(), dL_dout_color, dL_dout_depth,
        dL_dmeans2D, dL_dconic, dL_dopacity, dL_dcolors, dL_ddepths, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales,
        dL_drotations, dL_dtau, s->debug != 0);
  return OLSR_OK;
}

// The per-Gaussian half of the backward alone: the reference's computeCov2DCUDA, then its preprocessCUDA /
// language_preprocessCUDA (BACKWARD::preprocess / BACKWARD::language_preprocess launch exactly these two), on
// composite-level gradients that the CALLER provides.  Arguments as oracle_backward_chain.
int ref_backward_chain(void* h, const olsr_scene* s, const int32_t* radii, const float* dL_dmeans2D_in,
                       const float* dL_dconic_in, const float* dL_dcolors_in, const float* dL_ddepths_in,
                       float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscales, float* dL_drotations,
                       float* dL_dtau) {
  if (!h || !check_scene(s) || !s->projmatrix_raw) return OLSR_ERR_ARG;
  RefState& st = *(RefState*)h;
  const int P = s->P, F = s->F, M = s->M;
  if (st.P != P || st.F != F || st.W != s->width || st.H != s->height) return OLSR_ERR_ARG;
  std::fill(dL_dmeans3D, dL_dmeans3D + (size_t)3 * P, 0.f);
  std::fill(dL_dcov3D, dL_dcov3D + (size_t)6 * P, 0.f);
  if (M > 0) std::fill(dL_dsh, dL_dsh + (size_t)3 * M * P, 0.f);
  std::fill(dL_dscales, dL_dscales + (size_t)3 * P, 0.f);
  std::fill(dL_drotations, dL_drotations + (size_t)4 * P, 0.f);
  std::fill(dL_dtau, dL_dtau + (size_t)6 * P, 0.f);
  // the chain's inputs it is declared to write (dL_dcolor, dL_ddepth, dL_dlanguage are non-const there) are copies
  std::vector<float> colors(dL_dcolors_in, dL_dcolors_in + (size_t)3 * P), depths(dL_ddepths_in, dL_ddepths_in + P);
  std::vector<float> language((size_t)(F > 0 ? F : 1) * P, 0.f);
  const GeomView g = geom_view(st);
  const float focal_y = s->height / (2.0f * s->tan_fovy);
  const float focal_x = s->width / (2.0f * s->tan_fovx);
  const float* cov3D_ptr = s->cov3D_precomp ? s->cov3D_precomp : g.cov3D;
  if (F > 0)
    BACKWARD::language_preprocess(
        P, s->D, M, 0, (const float3*)s->means3D, radii, s->shs, g.clamped, (const glm::vec3*)s->scales,
        (const glm::vec4*)s->rotations, s->scale_modifier, cov3D_ptr, s->viewmatrix, s->projmatrix, s->projmatrix_raw, focal_x,
        focal_y, s->tan_fovx, s->tan_fovy, (const glm::vec3*)s->cam_pos, (const float3*)dL_dmeans2D_in, dL_dconic_in,
        (glm::vec3*)dL_dmeans3D, colors.data(), language.data(), depths.data(), dL_dcov3D, dL_dsh, (glm::vec3*)dL_dscales,
        (glm::vec4*)dL_drotations, dL_dtau);
  else
    BACKWARD::preprocess(
        P, s->D, M, (const float3*)s->means3D, radii, s->shs, g.clamped, (const glm::vec3*)s->scales,
        (const glm::vec4*)s->rotations, s->scale_modifier, cov3D_ptr, s->viewmatrix, s->projmatrix, s->projmatrix_raw, focal_x,
        focal_y, s->tan_fovx, s->tan_fovy, (const glm::vec3*)s->cam_pos, (const float3*)dL_dmeans2D_in, dL_dconic_in,
        (glm::vec3*)dL_dmeans3D, colors.data(), depths.data(), dL_dcov3D, dL_dsh, (glm::vec3*)dL_dscales,
        (glm::vec4*)dL_drotations, dL_dtau);
  return OLSR_OK;
}

int ref_mark_visible(int32_t P, const float* means3D, const float* viewmatrix, const float* projmatrix, uint8_t* present) {
  static_assert(sizeof(bool) == 1, "present is a bool array");
  if (P > 0)
    CudaRasterizer::Rasterizer::markVisible(P, (float*)means3D, (float*)viewmatrix, (float*)projmatrix, (bool*)present);
  return OLSR_OK;
}

// State inspection with oracle_get_field's names and layouts.  Returns the element count; copies into dst if non-NULL.
int64_t ref_get_field(void* h, const char* name, void* dst) {
  RefState& st = *(RefState*)h;
  auto cp = [&](const void* src, size_t n, size_t esz) -> int64_t {
    if (dst && n) std::memcpy(dst, src, n * esz);
    return (int64_t)n;
  };
  const size_t P = st.P, R = st.R, N = (size_t)st.W * st.H;
  const size_t tiles = (size_t)((st.W + BLOCK_X - 1) / BLOCK_X) * ((st.H + BLOCK_Y - 1) / BLOCK_Y);
  const GeomView g = geom_view(st);
  char* bp = st.binning.data();
  const auto b = CudaRasterizer::BinningState::fromChunk(bp, R);
  char* ip = st.img.data();
  const auto im = CudaRasterizer::ImageState::fromChunk(ip, N);
  if (!std::strcmp(name, "depths")) return cp(g.depths, P, 4);
  if (!std::strcmp(name, "means2D")) return cp(g.means2D, 2 * P, 4);
  if (!std::strcmp(name, "cov3D")) return cp(g.cov3D, 6 * P, 4);
  if (!std::strcmp(name, "conic_opacity")) return cp(g.conic_opacity, 4 * P, 4);
  if (!std::strcmp(name, "rgb")) return cp(g.rgb, 3 * P, 4);
  if (!std::strcmp(name, "clamped")) return cp(g.clamped, 3 * P, 1);
  if (!std::strcmp(name, "tiles_touched")) return cp(g.tiles_touched, P, 4);
  if (!std::strcmp(name, "point_offsets")) return cp(g.point_offsets, P, 4);
  if (!std::strcmp(name, "point_list")) return cp(b.point_list, R, 4);
  if (!std::strcmp(name, "keys")) return cp(b.point_list_keys, R, 8);
  if (!std::strcmp(name, "ranges")) return cp(im.ranges, 2 * tiles, 4);
  if (!std::strcmp(name, "final_T")) return cp(im.accum_alpha, N, 4);
  if (!std::strcmp(name, "n_contrib")) return cp(im.n_contrib, N, 4);
  return -1;
}

}  // extern "C"

// olsr_api.hip — the C-ABI of include/olsr.h: argument checking, state-buffer carving and
// the launch sequence of the forward and backward passes.  (The entries that make a single launch are in olsr_entries.hip,
// the host state of the synchronising entry in olsr_dropin.hip, diagnostics in olsr_diag.hip.)
//
// Counterpart of CR/rasterizer_impl.cu:216-756 (orchestration) and of the torch glue in
// DGR/rasterize_points.cu (allocation), minus everything torch: the caller owns memory.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "olsr_device.h"
#include "olsr_host.h"

using namespace olsr;

namespace {
thread_local std::string g_err;
}

int olsr::fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

namespace {

int check_scene(const olsr_scene* s, bool backward) {
  if (!s) return fail(OLSR_ERR_ARG, "scene is NULL");
  if (s->P < 0) return fail(OLSR_ERR_ARG, "P must be >= 0");
  if (s->width <= 0 || s->height <= 0) return fail(OLSR_ERR_ARG, "image size must be positive");
  // (tile coordinates travel as 16-bit fields of the emission record)
  if (s->width > 65535 * 15 || s->height > 65535 * 15) return fail(OLSR_ERR_ARG, "image size beyond 65535 tiles");
  if (s->tile != 15 && s->tile != 16) return fail(OLSR_ERR_ARG, "tile must be 15 or 16");
  if (!backward && s->binning != OLSR_BINNING_RECT && s->binning != OLSR_BINNING_ELLIPSE)
    return fail(OLSR_ERR_ARG, "binning must be OLSR_BINNING_RECT or OLSR_BINNING_ELLIPSE");
  if (!supported_F(s->F)) return fail(OLSR_ERR_ARG, "F (language channels) must be one of 0, 3, 15, 16, 32");
  if (s->D < 0 || s->D > 3) return fail(OLSR_ERR_ARG, "SH degree must be 0..3");
  if (s->P == 0) return OLSR_OK;
  if (!s->means3D || !s->background || !s->viewmatrix || !s->projmatrix || !s->cam_pos)
    return fail(OLSR_ERR_ARG, "means3D, background, viewmatrix, projmatrix and cam_pos are required");
  if (!backward && !s->opacities) return fail(OLSR_ERR_ARG, "opacities are required");
  if (s->flags & ~(OLSR_FLAG_SIGNED_EMPTY_RADII | OLSR_FLAG_FWD_ACCUM_MFMA | OLSR_FLAG_FWD_ACCUM_WEIGHT | OLSR_FLAG_FRAMES_IN_FLIGHT)) return fail(OLSR_ERR_ARG, "flags holds unknown OLSR_FLAG_* bits");
  if (s->activations & ~(OLSR_ACT_OPACITY_SIGMOID | OLSR_ACT_SCALE_EXP | OLSR_ACT_ROTATION_NORMALIZE))
    return fail(OLSR_ERR_ARG, "activations holds unknown OLSR_ACT_* bits");
  if (backward && (s->activations & OLSR_ACT_OPACITY_SIGMOID) && !s->opacities)
    return fail(OLSR_ERR_ARG, "a raw (pre-sigmoid) opacity is needed by backward as well");
  if ((s->activations & (OLSR_ACT_SCALE_EXP | OLSR_ACT_ROTATION_NORMALIZE)) && s->cov3D_precomp)
    return fail(OLSR_ERR_ARG, "scale / rotation activations make no sense with a precomputed 3D covariance");
  if ((s->shs == nullptr) == (s->colors_precomp == nullptr))
    return fail(OLSR_ERR_ARG, "Please provide excatly one of either SHs or precomputed colors!");
  const bool has_sr = s->scales != nullptr && s->rotations != nullptr;
  const bool any_sr = s->scales != nullptr || s->rotations != nullptr;
  if ((!has_sr && !s->cov3D_precomp) || (any_sr && s->cov3D_precomp))
    return fail(OLSR_ERR_ARG, "Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!");
  if (s->shs && (s->M < (s->D + 1) * (s->D + 1))) return fail(OLSR_ERR_ARG, "shs holds fewer coefficients than the degree needs");
  if (s->F > 0 && !s->language_precomp) return fail(OLSR_ERR_ARG, "language_precomp is required when F > 0");
  if (backward && !s->projmatrix_raw) return fail(OLSR_ERR_ARG, "projmatrix_raw is required by backward");
  if (s->backward_row_capacity < 0) return fail(OLSR_ERR_ARG, "backward_row_capacity must be >= 0");
  if (s->backward_row_capacity > 0 && s->bwd_mode != OLSR_BWD_REFERENCE && s->bwd_mode != OLSR_BWD_EXACT)
    return fail(OLSR_ERR_ARG, "backward_row_capacity needs a valid bwd_mode in the forward as well");
  return OLSR_OK;
}

FrameDims frame_dims(const olsr_scene& s) {
  FrameDims d;
  d.W = s.width;
  d.H = s.height;
  d.tile = s.tile;
  d.gx = tiles_along(s.width, s.tile);
  d.gy = tiles_along(s.height, s.tile);
  d.ntiles = d.gx * d.gy;
  d.focal_y = s.height / (2.0f * s.tan_fovy);  // CR/rasterizer_impl.cu:394-395
  d.focal_x = s.width / (2.0f * s.tan_fovx);
  return d;
}

int tile_bits(int ntiles) {
  int bits = 1;
  while ((1LL << bits) < (long long)ntiles) ++bits;
  return bits;
}
// where the tile sort leaves its result: 0 = (key_a, src), 1 = (key_b, val_b)
int tile_sort_where(int ntiles) { return ((tile_bits(ntiles) + 7) / 8) & 1; }

// One forward, as its entry describes it.  The binning buffer is either the caller's (sync-free entries: bin_buf holds
// `capacity` instances, the count stays on the device) or comes from bin_alloc once the host knows the count (olsr_forward).
struct ForwardCall {
  void* geom_buf = nullptr;
  void* img_buf = nullptr;
  void* bin_buf = nullptr;
  int64_t capacity = 0;
  olsr_alloc_fn bin_alloc = nullptr;  // non-null: the synchronising entry
  void* bin_user = nullptr;
  float *out_color = nullptr, *out_language = nullptr, *out_depth = nullptr, *out_opacity = nullptr;
  int32_t *radii = nullptr, *n_touched = nullptr;
  int32_t* num_rendered_host = nullptr;  // (synchronising entry)
  int32_t* num_rendered_dev = nullptr;   // (sync-free entries)
  uint32_t* tile_order_inout = nullptr;
  const olsr_loss_fusion* loss = nullptr;  // the loss in the composite's epilogue (olsr_forward_async_loss)
  uint32_t* view_hints = nullptr;          // the stream's per-view tile orders (synchronising entry; olsr_dropin.hip)
  hipStream_t st = nullptr;
};

// forces the multi-kernel radix passes (the fallback of sorts too large for the fused ones), so that both paths can be
// tested at any size
bool force_legacy_sort() { return sort_knobs().legacy.load(std::memory_order_relaxed) != 0; }

int forward_impl(const olsr_scene& s, const ForwardCall& c) {
  const hipStream_t st = c.st;
  const FrameDims d = frame_dims(s);
  const size_t N = (size_t)d.W * d.H;
  const GeometryState g = GeometryState::carve(c.geom_buf, (size_t)s.P, grad_row(s.F));
  const ImageState im = ImageState::carve(c.img_buf, N, (size_t)d.ntiles);
  mark("begin", st);

  if (!(c.loss && c.loss->skip_images) &&
      (!c.out_color || !c.out_depth || !c.out_opacity || (s.F > 0 && !c.out_language)))
    return fail(OLSR_ERR_ARG, "output image pointers must not be NULL");
  if (s.P > 0 && (!c.radii || !c.n_touched)) return fail(OLSR_ERR_ARG, "radii and n_touched must not be NULL");

  if (s.P <= 0) {  // nothing below runs: leave a consistent empty state behind
    HIP_TRY(hipMemsetAsync(g.counters, 0, sizeof(int32_t) * CNT_WORDS, st));
    HIP_TRY(hipMemsetAsync(im.ranges, 0, sizeof(uint32_t) * 2 * (size_t)d.ntiles, st));
    HIP_TRY(hipMemsetAsync(im.live_rows, 0, sizeof(uint32_t) * 4, st));
  }

  const bool legacy = force_legacy_sort();
  const bool sync_mode = c.bin_alloc != nullptr;
  int64_t n_host = 0;
  uint32_t* carry = nullptr;  // the caller's carried depth order, when this frame uses it
  uint32_t* order = nullptr;  // where the depth order lies when neither g.depth_order nor the carried array holds it
  const int32_t* n_order_dev = nullptr;  // its length on the device when the sort compacted its input (else: P)
  if (s.P > 0) {
    launch_preprocess(s, d, g, c.radii, c.n_touched, st);  // also zeroes the geometry buffer's synchronisation words
    STAGE(s, "preprocess", st);
    // digit totals of the four depth passes in one read of the keys + the frame's counters (instances emitted,
    // the reference's num_rendered, overflow against the capacity), tile ranges reset to "empty"
    FusedHouse house{g.part_rect, g.part_count, (s.P + 255) / 256, sync_mode ? 0x7FFFFFFFLL : (long long)c.capacity,
                     g.counters, c.num_rendered_dev, im.ranges, 2 * d.ntiles, nullptr, 0, im.live_rows,
                     c.view_hints, s.viewmatrix};  // (the synchronising entry: this frame's slot among the stream's per-view orders)
    if (sync_mode) OLSR_TRY(pinned_count_arm(house));
    SortBuffers sb{g.key_a, g.key_b, g.val_a, g.val_b, g.radix_table, g.scan_partials};
    const bool in_flight = (s.flags & OLSR_FLAG_FRAMES_IN_FLIGHT) != 0;
    // Carried depth order (include/olsr.h): two launches of independent workgroups repair the order the previous frame of this
    // view left in the caller's array; the sort below is enqueued behind them in any case and does its work only when the
    // repair says it could not prove the result (carry_miss != 0) — the lists never depend on what the array held.
    carry = (!sync_mode && !legacy && fused_sort_applicable(s.P, 32)) ? s.depth_order_carry : nullptr;
    const uint32_t* run_if = carry ? g.carry_miss : nullptr;
    if (carry)
      launch_order_repair(s.P, carry, g.key_a, g.key_b, g.val_b, g.tiles_touched, g.carry_totals, g.carry_miss, in_flight, st);
    if (!legacy && small_depth_sort_applicable(s.P, carry != nullptr)) {
      // at most 8 192 Gaussians: histogram, bookkeeping and all four passes in ONE launch of one workgroup (k_sort.hip)
      launch_small_depth_sort(g.key_a, s.P, carry ? carry : g.depth_order, g.tiles_touched, g.emit_status, &house, run_if, st);
      STAGE(s, "depth_sort", st);
    } else {
    const SortPlan depth_plan = sort_plan(s.P, false, 85, in_flight);
    const bool fused_depth = !legacy && fused_sort_applicable(s.P, 32);
    // Visible-set compaction (k_sort.hip): without a carried order — whose domain is every Gaussian — the histogram kernel
    // hands the passes only the Gaussians that emit instances, (key, index) densely in key_b / val_b; the order they leave,
    // n_order = counters[CNT_SORTED] entries long, goes to the backward's (idle) per-Gaussian scratch: the emission uses the
    // sort's own buffers for its rank lists.
    const bool compacted = fused_depth && carry == nullptr && depth_sort_compaction_applicable(s.P);
    SortCompaction cmp{g.tiles_touched, g.part_vis, g.key_b, g.val_b, &g.counters[CNT_SORTED]};
    launch_sort_hist(g.key_a, s.P, nullptr, 32, g.sort_hist, &house, depth_plan.threads, st, run_if, compacted ? &cmp : nullptr);
    // (the last pass also leaves the instance total of every block of 1024 depth ranks behind, for the emission)
    if (fused_depth) {
      // compacted: (key, index) pairs out of key_b / val_b, n_order of them, the order to `order`; else values = Gaussian
      // indices: the first pass takes them from the position (preprocess writes no index array), the order to val_a or `carry`
      const SortBuffers sbc{g.key_b, g.key_a, g.val_b, g.val_a, g.radix_table, g.scan_partials};
      if (compacted) {
        order = reinterpret_cast<uint32_t*>(g.gacc);
        n_order_dev = &g.counters[CNT_SORTED];
      }
      launch_sort_fused(compacted ? sbc : sb, depth_plan, s.P, n_order_dev, 32, !compacted, g.sort_hist, g.sort_status,
                        g.tickets + GT_DEPTH_PASS, nullptr, nullptr, g.tiles_touched, g.emit_status, &g.counters[CNT_SYNC_ERROR],
                        sort_knobs().fault.load(std::memory_order_relaxed) & 1, st, compacted ? order : carry, run_if);
    } else {
      launch_radix_sort(sb, s.P, nullptr, 32, true, st);
      launch_emit_totals(g.depth_order, s.P, g.tiles_touched, g.emit_status, st);
    }
    STAGE(s, "depth_sort", st);
    }
  }

  void* bin_buf = nullptr;
  if (!sync_mode) {
    n_host = c.capacity;
    bin_buf = c.bin_buf;
  } else {
    int32_t R = 0;
    if (s.P > 0) OLSR_TRY(pinned_count_wait(st, &R));
    n_host = R;
    if (c.num_rendered_host) *c.num_rendered_host = R;
    bin_buf = c.bin_alloc(c.bin_user, olsr_binning_bytes(R, s.F));
    if (!bin_buf) return fail(OLSR_ERR_ALLOC, "binning allocation callback returned NULL");
  }
  const BinningState b = BinningState::carve(bin_buf, (size_t)n_host);
  const int32_t* n_dev = &g.counters[CNT_INSTANCES_EFF];

  if (s.P > 0) {
    const int tbits = tile_bits(d.ntiles);
    int tpasses = 0;
    const int tdb = fused_sort_digit_bits(tbits, &tpasses);
    const bool fused_tiles = !legacy && fused_sort_applicable(n_host, tbits);
    // (with depth cut-offs a steady-state frame keeps a fraction of the instances its capacity was sized for — config 3: a
    //  quarter —, and a pass is bound by the latency of its fattest block: plan the chunks for that, the uncut first frame of a
    //  sequence pays a few rounds more)
    const bool cut_mode = !sync_mode && s.tile_depth_cut != nullptr && s.binning == OLSR_BINNING_ELLIPSE;
    const SortPlan tile_plan = sort_plan(n_host, /*n_is_capacity=*/!sync_mode, cut_mode ? 25 : 85,
                                         (s.flags & OLSR_FLAG_FRAMES_IN_FLIGHT) != 0);
    // synchronisation words of the binning buffer that this frame uses (zeroed by the emission kernel)
    const int64_t bin_sync_words =
        (b.tile_status - b.sync_words) +
        (fused_tiles ? ((int64_t)tpasses * tile_plan.nblk * ((int64_t)1 << tdb) + 1) / 2 : 0);  // 16-bit words
    launch_emit(s, d, g, b, bin_sync_words, n_host, carry ? carry : (order ? order : g.depth_order),
                carry ? g.carry_totals : nullptr, carry ? g.carry_miss : nullptr, n_order_dev, st);
    STAGE(s, "emit", st);
    if (n_host > 0) {
      // arrange the value ping-pong so that the last pass always lands in b.src
      const bool odd = tile_sort_where(d.ntiles) != 0;
      SortBuffers sb{b.key_a, b.key_b, odd ? b.val_b : b.src, odd ? b.src : b.val_b, b.radix_table, b.scan_partials};
      if (fused_tiles) {
        launch_sort_hist(b.key_a, n_host, n_dev, tbits, b.tile_hist, nullptr, tile_plan.threads, st);
        // the first pass also clears the liveness flags, the last one derives the tile ranges
        launch_sort_fused(sb, tile_plan, n_host, n_dev, tbits, true, b.tile_hist, b.tile_status, b.tickets + BT_TILE_PASS, b.flags,
                          im.ranges, nullptr, nullptr, &g.counters[CNT_SYNC_ERROR],
                          sort_knobs().fault.load(std::memory_order_relaxed) & 2, st);
      } else {
        const int where = launch_radix_sort(sb, n_host, n_dev, tbits, true, st);
        launch_tile_ranges(where ? b.key_b : b.key_a, n_host, n_dev, im.ranges, b.flags, st);
      }
      STAGE(s, "tile_sort", st);
    }
  }
  ForwardTail tail;
  uint32_t* tile_order_inout = c.tile_order_inout;
  if (sync_mode) OLSR_TRY(rows_ring_post(st, tail));  // the drop-in entry: the frame's gradient-row counts for the matching backward
  if (c.view_hints != nullptr && s.P > 0) {  // (the synchronising entry; the slot was picked by the depth sort's histogram kernel)
    tail.hint_slot = c.view_hints;
    tile_order_inout = c.view_hints + HINT_HDR;
  }
  // the caller announced its backward's row capacity: the forward's last launch compacts the rows as well (include/olsr.h)
  if (s.backward_row_capacity > 0 && s.P > 0 && bin_buf != nullptr) tail.compact_rows_n = n_host;
  stamp(st, 0);
  launch_render_forward(s, d, g, b, im, c.out_color, c.out_language, c.out_depth, c.out_opacity, c.n_touched, tile_order_inout,
                        c.num_rendered_dev, (s.P > 0) ? c.loss : nullptr, tail, st);
  stamp(st, 1);
  STAGE(s, "render_forward", st);

  if (c.num_rendered_dev && s.P == 0) HIP_TRY(hipMemsetAsync(c.num_rendered_dev, 0, 2 * sizeof(int32_t), st));
  return OLSR_OK;
}

}  // namespace

extern "C" {

const char* olsr_last_error(void) { return g_err.c_str(); }

const char* olsr_version(void) { return "olsr 0.1 (gfx950)"; }

size_t olsr_geometry_bytes(int32_t P, int32_t F) {
  size_t bytes = 0;
  GeometryState::carve(nullptr, (size_t)(P > 0 ? P : 0), grad_row(supported_F(F) ? F : 0), &bytes);
  return bytes;
}

size_t olsr_image_bytes(int32_t width, int32_t height, int32_t tile) {
  size_t bytes = 0;
  ImageState::carve(nullptr, (size_t)width * (size_t)height, tile_count(width, height, tile), &bytes);
  return bytes;
}

size_t olsr_binning_bytes(int64_t num_rendered, int32_t F) {
  (void)F;
  size_t bytes = 0;
  BinningState::carve(nullptr, (size_t)(num_rendered > 0 ? num_rendered : 0), &bytes);
  return bytes;
}

size_t olsr_backward_scratch_bytes(int64_t rows, int32_t F) {
  return align_up((size_t)(rows > 0 ? rows : 0) * (size_t)grad_row(supported_F(F) ? F : 0) * sizeof(float)) + 2 * ALIGN;
}

size_t olsr_fused_loss_scratch_bytes(int32_t width, int32_t height, int32_t tile) {
  if (width <= 0 || height <= 0 || (tile != 15 && tile != 16)) return 0;
  size_t bytes = 0;
  loss_partials_carve(nullptr, tile_count(width, height, tile), bytes);
  return bytes;
}

int olsr_forward(const olsr_scene* scene, olsr_alloc_fn geometry_alloc, void* geometry_user,
                 olsr_alloc_fn binning_alloc, void* binning_user, olsr_alloc_fn image_alloc, void* image_user,
                 float* out_color, float* out_language, float* out_depth, float* out_opacity, int32_t* radii,
                 int32_t* n_touched, int32_t* num_rendered, void* hip_stream) {
  OLSR_TRY(check_scene(scene, false));
  if (!geometry_alloc || !binning_alloc || !image_alloc) return fail(OLSR_ERR_ARG, "allocation callbacks are required");
  // (before the allocation callbacks run: a call that fails for an EARLIER frame's error must not have resized the caller's
  //  buffers — ADVICE round 4)
  OLSR_TRY(sticky_sync_error_check((hipStream_t)hip_stream));
  ForwardCall c;
  c.st = (hipStream_t)hip_stream;
  c.geom_buf = geometry_alloc(geometry_user, olsr_geometry_bytes(scene->P, scene->F));
  if (!c.geom_buf) return fail(OLSR_ERR_ALLOC, "geometry allocation callback returned NULL");
  c.img_buf = image_alloc(image_user, olsr_image_bytes(scene->width, scene->height, scene->tile));
  if (!c.img_buf) return fail(OLSR_ERR_ALLOC, "image allocation callback returned NULL");
  c.bin_alloc = binning_alloc;
  c.bin_user = binning_user;
  if (num_rendered) *num_rendered = 0;
  c.num_rendered_host = num_rendered;
  olsr_scene sc = *scene;
  sc.tile_depth_cut = nullptr;  // (per-tile depth cut-offs belong to the sync-free entries: their verdict is a device status word)
  sc.depth_order_carry = nullptr;  // (a caller-owned array: the reference-shaped entry has no place for one)
  c.out_color = out_color, c.out_language = out_language, c.out_depth = out_depth, c.out_opacity = out_opacity;
  c.radii = radii, c.n_touched = n_touched;
  c.view_hints = order_hint_of((int)tile_count(scene->width, scene->height, scene->tile), c.st);
  return forward_impl(sc, c);
}

int olsr_forward_async(const olsr_scene* scene, void* geometry_buffer, void* binning_buffer, int64_t capacity,
                       void* image_buffer, float* out_color, float* out_language, float* out_depth, float* out_opacity,
                       int32_t* radii, int32_t* n_touched, int32_t* num_rendered_dev, uint32_t* tile_order_inout,
                       void* hip_stream) {
  return olsr_forward_async_loss(scene, geometry_buffer, binning_buffer, capacity, image_buffer, out_color, out_language,
                                 out_depth, out_opacity, radii, n_touched, num_rendered_dev, tile_order_inout, nullptr,
                                 hip_stream);
}

int olsr_forward_async_loss(const olsr_scene* scene, void* geometry_buffer, void* binning_buffer, int64_t capacity,
                            void* image_buffer, float* out_color, float* out_language, float* out_depth,
                            float* out_opacity, int32_t* radii, int32_t* n_touched, int32_t* num_rendered_dev,
                            uint32_t* tile_order_inout, const olsr_loss_fusion* loss, void* hip_stream) {
  OLSR_TRY(check_scene(scene, false));
  if (!geometry_buffer || !binning_buffer || !image_buffer || capacity < 0)
    return fail(OLSR_ERR_ARG, "state buffers and a non-negative capacity are required");
  olsr_loss_fusion lf;
  if (!loss) {  // olsr_forward_async
    if (scene->tile_depth_cut && scene->binning == OLSR_BINNING_ELLIPSE &&
        (scene->flags & (OLSR_FLAG_FWD_ACCUM_MFMA | OLSR_FLAG_FWD_ACCUM_WEIGHT)))
      return fail(OLSR_ERR_ARG, "tile_depth_cut: only with the default forward accumulation");
  } else {
    const olsr_loss_params& lp = loss->params;
    if (lp.width != scene->width || lp.height != scene->height)
      return fail(OLSR_ERR_ARG, "fused loss: params.width / height must equal the scene's");
    if (scene->flags & (OLSR_FLAG_FWD_ACCUM_MFMA | OLSR_FLAG_FWD_ACCUM_WEIGHT))
      return fail(OLSR_ERR_ARG, "fused loss: only with the default forward accumulation");
    if (!loss->gt_image || !loss->gt_depth || !loss->dL_dimage || !loss->dL_ddepth || !loss->loss || !loss->scratch)
      return fail(OLSR_ERR_ARG, "fused loss: gt_image, gt_depth, dL_dimage, dL_ddepth, loss and scratch are required");
    const bool lang_term = !loss->tracking && lp.F > 0 && loss->gt_language != nullptr;
    if (lang_term && (lp.F != scene->F || !loss->dL_dlanguage || lp.lang_width <= 0 || lp.lang_height <= 0))
      return fail(OLSR_ERR_ARG, "fused loss: a language term needs params.F == scene F, dL_dlanguage and the target's size");
    if (scene->tile_depth_cut && scene->binning == OLSR_BINNING_ELLIPSE && !loss->tracking)
      return fail(OLSR_ERR_ARG, "tile_depth_cut: with a fused loss only for the tracking loss (a mapping step sums views; a view "
                                "whose frame missed would change the sum)");
    if (scene->P <= 0)  // nothing is rendered (the images are the background): the stand-alone kernels define this case
      return fail(OLSR_ERR_ARG, "fused loss: P must be > 0 (use olsr_mapping_loss / olsr_tracking_loss on an empty render)");
    lf = *loss;
    size_t bytes;
    lf.scratch = loss_partials_carve(loss->scratch, tile_count(scene->width, scene->height, scene->tile), bytes);
  }
  ForwardCall c;
  c.st = (hipStream_t)hip_stream;
  c.geom_buf = geometry_buffer, c.img_buf = image_buffer, c.bin_buf = binning_buffer, c.capacity = capacity;
  c.out_color = out_color, c.out_language = out_language, c.out_depth = out_depth, c.out_opacity = out_opacity;
  c.radii = radii, c.n_touched = n_touched;
  c.num_rendered_dev = num_rendered_dev;
  c.tile_order_inout = tile_order_inout;
  c.loss = loss ? &lf : nullptr;
  return forward_impl(*scene, c);
}

int olsr_backward(const olsr_scene* scene, const int32_t* radii, void* geometry_buffer, int32_t num_rendered,
                  void* binning_buffer, const void* image_buffer, olsr_alloc_fn scratch_alloc, void* scratch_user,
                  int32_t rows_token, void* scratch, int64_t scratch_rows, const float* dL_dout_color,
                  const float* dL_dout_language, const float* dL_dout_depth, float* dL_dmeans2D, float* dL_dconic,
                  float* dL_dopacity, float* dL_dcolors, float* dL_dlanguage, float* dL_ddepths, float* dL_dmeans3D,
                  float* dL_dcov3D, float* dL_dsh, float* dL_dscales, float* dL_drotations, float* dL_dtau,
                  float* dL_dtau_sum, const olsr_grad_bucket* bucket, int32_t* status_dev, void* hip_stream) {
  OLSR_TRY(check_scene(scene, true));
  const olsr_scene& s = *scene;
  hipStream_t st = (hipStream_t)hip_stream;
  if (s.bwd_mode != OLSR_BWD_REFERENCE && s.bwd_mode != OLSR_BWD_EXACT)
    return fail(OLSR_ERR_ARG, "bwd_mode must be OLSR_BWD_REFERENCE or OLSR_BWD_EXACT");
  OLSR_TRY(sticky_sync_error_check(st));
  mark("begin", st);
  if (s.P == 0) {
    if (dL_dtau_sum) HIP_TRY(hipMemsetAsync(dL_dtau_sum, 0, 6 * sizeof(float), st));
    if (status_dev) HIP_TRY(hipMemsetAsync(status_dev, 0, 2 * sizeof(int32_t), st));
    return OLSR_OK;
  }
  if (!radii || !geometry_buffer || !binning_buffer || !image_buffer || num_rendered < 0)
    return fail(OLSR_ERR_ARG, "radii, the three state buffers and num_rendered (>= 0) are required");
  if (!scratch_alloc && (!scratch || scratch_rows < 0))
    return fail(OLSR_ERR_ARG, "either a scratch allocation callback or a scratch buffer with its row capacity is required");
  if (!dL_dout_color) return fail(OLSR_ERR_ARG, "dL_dout_color must not be NULL");
  // A NULL language / depth cotangent means "the loss does not depend on that image" (what autograd hands the
  // reference's backward as None -> zeros, DGR/diff_gaussian_rasterization/__init__.py:296-345; the tracking loss has
  // no language term, utils/slam_utils.py:92-121).  Without a language cotangent the RGB instantiation of the composite
  // backward runs on the language forward's state: D - A == 0 and the rank-0 language row == 0, so every gradient
  // equals what zero-filled cotangents give, and dL_dlanguage is written as zeros.
  const int F_rows = (s.F > 0 && !dL_dout_language) ? 0 : s.F;
  if (bucket) {
    if (!bucket->flat || !bucket->densify || !bucket->max_radii)
      return fail(OLSR_ERR_ARG, "bucket.flat, bucket.densify and bucket.max_radii must not be NULL");
  } else if (!dL_dtau_sum && (!dL_dmeans2D || !dL_dopacity || !dL_dcolors || (s.F > 0 && !dL_dlanguage) ||
                              !dL_dmeans3D || !dL_dcov3D || (s.M > 0 && !dL_dsh) || !dL_dscales || !dL_drotations ||
                              !dL_dtau)) {
    return fail(OLSR_ERR_ARG, "gradient outputs must not be NULL (unless a gradient bucket or dL_dtau_sum is given)");
  }
  const FrameDims d = frame_dims(s);
  const GeometryState g = GeometryState::carve(geometry_buffer, (size_t)s.P, grad_row(s.F));
  const ImageState im = ImageState::carve(const_cast<void*>(image_buffer), (size_t)d.W * d.H, (size_t)d.ntiles);
  const BinningState b = BinningState::carve(binning_buffer, (size_t)num_rendered);
  const bool packed_ref15 = (s.bwd_mode == OLSR_BWD_REFERENCE && s.tile == 15);
  const bool rows_compacted = s.backward_row_capacity > 0;
  if (rows_compacted && (scratch_alloc || scratch_rows != s.backward_row_capacity))
    return fail(OLSR_ERR_ARG, "backward_row_capacity: the backward needs a caller-owned scratch of exactly that many rows");

  // one backward whose partial-gradient rows go to `buf`, which holds `capacity` rows
  auto launch = [&](void* buf, int64_t capacity) -> int {
    // compact the partial-gradient rows: one row per (instance, slot) pair the forward blended — unless the forward did
    // (olsr_scene.backward_row_capacity: rowbase, CNT_LIVE_ROWS and CNT_ROW_OVERFLOW are in place, the backward's last kernel
    // copies them to status_dev)
    if (!rows_compacted) {
      launch_row_compaction(b.flags, num_rendered, &g.counters[CNT_INSTANCES_EFF], packed_ref15, b.rowbase, b.row_status,
                            b.tickets + BT_ROWS, capacity, g.counters, status_dev, st);
      STAGE(s, "row_compaction", st);
    }
    float* rows = align_ptr<float>(buf);

    stamp(st, 2);
    if (s.bwd_mode == OLSR_BWD_REFERENCE)
      launch_render_backward_reference(s, F_rows, d, g, b, im, dL_dout_color, dL_dout_language, dL_dout_depth, rows, st);
    else
      launch_render_backward_exact(s, F_rows, d, g, b, im, dL_dout_color, dL_dout_language, dL_dout_depth, rows, st);
    stamp(st, 3);
    STAGE(s, "render_backward", st);
    GradOut o{dL_dmeans2D, dL_dconic, dL_dopacity, dL_dcolors, dL_dlanguage, dL_ddepths, dL_dmeans3D,
              dL_dcov3D,   dL_dsh,    dL_dscales,  dL_drotations, dL_dtau,    dL_dtau_sum};
    if (bucket) {
      o.bucket_flat = bucket->flat;
      o.bucket_densify = bucket->densify;
      o.bucket_max_radii = bucket->max_radii;
      o.bucket_assign = bucket->assign;
      o.bucket_row_mask = reinterpret_cast<unsigned long long*>(bucket->row_mask);
    }
    o.status_dev = status_dev;
    o.status_rows = rows_compacted;
    // (a caller that passes status_dev reads the report there; one that does not — the reference-shaped bindings — gets it
    //  from the library's next call)
    o.sticky_error = status_dev ? nullptr : sticky_sync_error_dev(st);
    launch_preprocess_backward(s, F_rows, d, g, b, rows, radii, o, g.tau_partials, st);
    STAGE(s, "preprocess_backward", st);
    return OLSR_OK;
  };
  if (!scratch_alloc) return launch(scratch, scratch_rows);

  // The drop-in policy (include/olsr.h).  A training loop reaches its backward while the forward is still executing; waiting
  // for the posted count and only then launching left the GPU idle between the forward's last kernel and the backward's first
  // (13 us per frame at config 3).  So: the count if it is there; else a guess, launched at once and verified while the GPU
  // works; a guess that was too small (that backward wrote zeros and said so) is followed by an exact second backward on the
  // same stream, which overwrites every output.
  const int packed = packed_ref15 ? 1 : 0;
  const int64_t bound = (int64_t)num_rendered * (packed ? 2 : 4);
  auto alloc_and_launch = [&](int64_t nrows) -> int {
    void* buf = scratch_alloc(scratch_user, olsr_backward_scratch_bytes(nrows, s.F));
    if (!buf) return fail(OLSR_ERR_ALLOC, "backward scratch allocation callback returned NULL");
    return launch(buf, nrows);
  };
  int64_t nrows = olsr_live_rows(rows_token, packed);
  bool guessed = false;
  if (nrows < 0 || nrows > bound) {
    const float ratio = g_rows_ratio[packed].load(std::memory_order_relaxed);
    if (olsr_live_rows_overwritten(rows_token)) {
      nrows = bound;  // (the slot belongs to a later forward: no count will ever arrive — no guess, no wait, no second backward)
    } else if (rows_token > 0 && ratio > 0.f && num_rendered > 0 &&
               olsr_backward_scratch_bytes(bound, s.F) > ROWS_WAIT_BYTES) {
      // (rounded up to a multiple of 128 Ki rows — 14 MB at F = 15: a size that changed a little from frame to frame, with the
      //  decaying ratio, made the caching allocator cut a new block every frame, and every few frames that is a hipMalloc)
      nrows = (int64_t)(1.5 * (double)ratio * num_rendered) + 65536;
      nrows = std::min<int64_t>(bound, (nrows + 131071) / 131072 * 131072);
      guessed = true;
    } else {
      nrows = olsr_backward_rows(rows_token, packed, num_rendered, s.F);  // (waits when the bound would cost more than 64 MB)
    }
  }
  OLSR_TRY(alloc_and_launch(nrows));
  int64_t exact = (nrows < bound || bound == 0) ? nrows : -1;
  if (guessed) {
    exact = olsr_live_rows_wait(rows_token, packed, 20000);
    if (exact < 0 || exact > nrows) {
      g_rows_redos.fetch_add(1, std::memory_order_relaxed);
      OLSR_TRY(alloc_and_launch((exact < 0 || exact > bound) ? bound : exact));
    }
  }
  if (exact >= 0 && num_rendered > 0) {
    // a slowly decaying maximum: the views of a mapping window differ in rows per instance (the arc views of the benchmark
    // by 60 %), and a guess sized from the lightest of them would be redone for every heavier one
    const float now = (float)exact / (float)num_rendered;
    const float old = g_rows_ratio[packed].load(std::memory_order_relaxed);
    g_rows_ratio[packed].store(std::max(now, 0.9f * old + 0.1f * now), std::memory_order_relaxed);
  }
  return OLSR_OK;
}

// (a test instrument, kept beside the backward whose checks and state carving it shares)
int olsr_debug_backward_ordered(const olsr_scene* scene, const void* geometry_buffer, int32_t num_rendered,
                                const void* binning_buffer, const void* image_buffer, const float* dL_dout_color,
                                const float* dL_dout_language, const float* dL_dout_depth, void* scratch, float* dL_dmeans2D,
                                float* dL_dconic, float* dL_dopacity, float* dL_dcolors, float* dL_dlanguage,
                                float* dL_ddepths, int32_t condition, void* hip_stream) {
  OLSR_TRY(check_scene(scene, true));
  const olsr_scene& s = *scene;
  if (s.bwd_mode != OLSR_BWD_REFERENCE && s.bwd_mode != OLSR_BWD_EXACT)
    return fail(OLSR_ERR_ARG, "bwd_mode must be OLSR_BWD_REFERENCE or OLSR_BWD_EXACT");
  if (s.P <= 0) return OLSR_OK;
  if (!geometry_buffer || !binning_buffer || !image_buffer || num_rendered < 0 || !scratch || !dL_dout_color || !dL_dmeans2D ||
      !dL_dconic || !dL_dopacity || !dL_dcolors || !dL_ddepths || (s.F > 0 && !dL_dlanguage))
    return fail(OLSR_ERR_ARG, "ordered backward: state buffers, scratch, dL_dout_color and the six outputs are required");
  const FrameDims d = frame_dims(s);
  const GeometryState g = GeometryState::carve(const_cast<void*>(geometry_buffer), (size_t)s.P, grad_row(s.F));
  const ImageState im = ImageState::carve(const_cast<void*>(image_buffer), (size_t)d.W * d.H, (size_t)d.ntiles);
  const BinningState b = BinningState::carve(const_cast<void*>(binning_buffer), (size_t)num_rendered);
  size_t bytes;
  const OrderedBwdScratch sc = OrderedBwdScratch::carve(scratch, (size_t)num_rendered, grad_row(s.F), bytes);
  launch_render_backward_ordered(s, d, g, b, im, num_rendered, dL_dout_color, dL_dout_language, dL_dout_depth, sc.rows, sc.used,
                                 dL_dmeans2D, dL_dconic, dL_dopacity, dL_dcolors, dL_dlanguage, dL_ddepths, condition != 0,
                                 (hipStream_t)hip_stream);
  return launch_check("ordered backward");
}

}  // extern "C"

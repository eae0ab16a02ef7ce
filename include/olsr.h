/*
 * olsr.h — C-ABI of the MI355X-native language-Gaussian rasterizer ("olsr").
 *
 * This is the drop-in boundary for the one hot path of rpng/online_lang_splatting:
 * the differentiable tile rasterizer behind `diff_gaussian_rasterization`.
 * Every entry point takes plain device pointers, sizes and a HIP stream handle
 * (no torch types).  The reference interface each entry point replaces is cited
 * as file:line relative to
 *   DGR = /root/reference/submodules/diff-gaussian-rasterization
 *   CR  = DGR/cuda_rasterizer
 *
 * Conventions (identical to the reference):
 *   - all float arrays are fp32, row-major, contiguous, resident on the GPU;
 *   - viewmatrix / projmatrix / projmatrix_raw are the 16 floats the Python caller
 *     holds (i.e. the transposes W2C^T, (P*W2C)^T, P^T) — column-major to the kernels;
 *   - opacities are post-sigmoid, scales post-exp, rotations are NOT re-normalised (unless
 *     scene->activations says the arrays are raw, see OLSR_ACT_*);
 *   - outputs are fully overwritten by the library (the caller need not zero them).
 *
 * Error behaviour: every function returns OLSR_OK (0) or a negative code and
 * records a message retrievable with olsr_last_error() (thread-local).
 *
 * Contents: the rasterizer itself (olsr_forward, olsr_forward_async, olsr_backward, olsr_mark_visible and
 * their size / introspection / profiling helpers — SURVEY.md section 8 rows a-e), then the callers and
 * data either side of it (rows f1-f3): olsr_mapping_loss, olsr_tracking_loss, olsr_pose_step, olsr_window_pose_step,
 * olsr_accumulate_gradients, olsr_sparse_exchange_mask / _pack / _unpack, olsr_adam_step (and its per-group form
 * olsr_adam_step_groups, olsr_adam_step_groups_reg with olsr_isotropic_reg), olsr_map_edit_plan / _apply (densify, prune, extend on the device), olsr_knn_mean_dist2,
 * olsr_keyframe_seed_plan / _finish (a keyframe's new Gaussians from its RGB-D image), olsr_grad_mask, olsr_median_depth,
 * olsr_covisibility and olsr_keyframe_decide (the front end's frame step around the tracking loop).
 * Three groups of entries of the same library are declared in headers of their own, which include this one:
 * olsr_single_stage.h (the single-stage language chain), olsr_frame_ingest.h (a frame's ingest ahead of the frame step) and
 * olsr_map_io.h (the map as the reference's PLY record, packed and unpacked on the device).
 */
#ifndef OLSR_H_INCLUDED
#define OLSR_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OLSR_OK 0
#define OLSR_ERR_ARG (-1)      /* bad argument (shape / exclusivity / unsupported F, tile) */
#define OLSR_ERR_DEVICE (-2)   /* HIP runtime error (message holds hipGetErrorString) */
#define OLSR_ERR_ALLOC (-3)    /* allocation callback returned NULL */
#define OLSR_ERR_CAPACITY (-4) /* async mode: instance count exceeded caller capacity */

/* Device-side status words of the sync-free entries (num_rendered_dev[1] of olsr_forward_async, status_dev[1] of
 * olsr_backward):  0 = fine;  1 = capacity overflow (instances resp. gradient rows; nothing rendered / zero gradients);
 * 2 = synchronisation error: a block of the frame's radix passes or of the row compaction waited for a predecessor's counts
 * until its spin bound ran out — the frame's synchronisation words were overwritten from outside mid-frame.  The library
 * never hangs on that and never writes out of bounds, but the tile lists are garbage: the forward's images must not be used,
 * the backward writes zero gradients.  For olsr_forward and for an olsr_backward without status_dev (the reference-shaped
 * bindings) the frame's last kernel raises a flag in mapped host memory and the FIRST olsr_forward / olsr_backward ON THE
 * SAME DEVICE AND STREAM after the GPU got there returns OLSR_ERR_DEVICE (once), the way an asynchronous HIP error surfaces
 * (round 6: the flag is keyed by device and stream — up to 63 pairs, further ones share one word —, so a broken frame on one
 * stream does not fail healthy calls on another). */
#define OLSR_STATUS_OK 0
#define OLSR_STATUS_OVERFLOW 1
#define OLSR_STATUS_SYNC_ERROR 2

/* Backward flavour.  REFERENCE reproduces what the shipped CUDA computes with its
 * 15x15 tiles (CR/config.h:17-18): the 225-lane tree reduction of
 * CR/backward.cu:684-702 keeps 128 of 225 pixel ranks, language gradients come from
 * tile rank 0 only (CR/backward.cu:1137,1194-1197) and the language recursion is not
 * skip-guarded (CR/backward.cu:1127-1139).  EXACT is the true gradient.
 * Both modes are tolerance-level, not bit-level, restatements of the reference's backward: the value path is re-associated
 * (running form of the behind-colour recursion, dot form of the language recursion, a wave-level reduction tree instead of
 * the shared-memory tree + float atomics), so gradients agree with the reference's arithmetic to the north-star tolerance
 * (>= 99.99 % of the elements of every tensor within 1e-4), not bit for bit; recursion-only visits are skipped while a
 * wave's last_alpha is still zero, which presumes finite features and cotangents (0 * x == 0). */
#define OLSR_BWD_REFERENCE 0
#define OLSR_BWD_EXACT 1

/* Allocation callback: must return a device pointer to >= nbytes (256-byte aligned),
 * valid until the matching backward has run.  Mirrors the std::function<char*(size_t)>
 * resize functionals of CR/rasterizer.h:34-36 and DGR/rasterize_points.cu:27-33. */
typedef void *(*olsr_alloc_fn)(void *user, size_t nbytes);

/* Scratch buffers.  Wherever an entry takes a `scratch` pointer sized by an olsr_*_scratch_bytes function, the pointer may
 * have any alignment: the library rounds it up to 256 bytes and lays its arrays out behind that, and the sizing function
 * reserves the slack.  The contents need not survive the call unless the entry says so (a plan's scratch is read by its
 * emit, apply or finish).  One buffer is not of this kind: olsr_hr_net_forward's workspace must be 16-byte aligned. */

/* Caller-side activations folded into the kernels.  The reference applies
 * sigmoid / exp / normalize in PyTorch before every render (GaussianModel.get_opacity / get_scaling /
 * get_rotation, gaussian_splatting/scene/gaussian_model.py:95-105) and autograd chains back through them.
 * With a bit set, the corresponding array holds the RAW parameter, preprocess applies
 *   opacity = 1 / (1 + exp(-x))      scale = exp(x)      rotation = q / max(|q|, 1e-12)
 * and the backward returns the gradient with respect to the RAW parameter (dL_dopacity, dL_dscales,
 * dL_drotations and the bucket rows).  With a raw opacity the backward needs scene->opacities too. */
#define OLSR_ACT_OPACITY_SIGMOID 1
#define OLSR_ACT_SCALE_EXP 2
#define OLSR_ACT_ROTATION_NORMALIZE 4

/* olsr_scene.flags.
 *   OLSR_FLAG_SIGNED_EMPTY_RADII  (forward) a Gaussian inside the frustum whose bounding square covers no tile gets
 *       radii[i] = -radius instead of 0 (it still emits nothing, and n_touched stays 0).  The disentangled rasterizer
 *       (DGR-D = submodules/diff-gaussian-rasterization-disentangle-optim) needs it: its
 *       preprocess writes BOTH radii of a Gaussian as soon as ONE of its two covariance sets covers a tile
 *       (DGR-D/cuda_rasterizer/forward.cu:391-431), so the caller that composes the two passes must know the radius of
 *       the set that covered none.  A backward must be given max(radii, 0). */
#define OLSR_FLAG_SIGNED_EMPTY_RADII 1
/*   OLSR_FLAG_ORACLE_KEEP_ZERO_DET  (forward; the CPU oracle only - the library rejects it as an unknown bit) a Gaussian
 *       whose float32 2D covariance has determinant a c - b b == 0 is NOT dropped: it goes on with the conic 1 / 0 gives
 *       (+inf, -+inf or NaN, +inf) and the radius its eigenvalues give.  DGR-D's preprocess does that to a covariance set
 *       whenever the Gaussian's OTHER set has a non-zero determinant (DGR-D/cuda_rasterizer/forward.cu:356-366);
 *       tests/dgrd_oracle.py composes the rule.  Thin needles close to the camera reach it: with a footprint variance of
 *       1e7 px^2 and more, a c and b b round to the same float although 0.3 was added to the diagonal. */
#define OLSR_FLAG_ORACLE_KEEP_ZERO_DET 0x100
/*   OLSR_FLAG_FWD_ACCUM_MFMA  (forward) the per-pixel feature accumulation C += f alpha T of the forward composite — a dense
 *       [64 pixels x K entries] x [K x (4 + F) channels] contraction per wave — runs on the matrix cores
 *       (v_mfma_f32_16x16x4_f32: exact fp32, a k-ordered fma chain) instead of the vector ALU.  Every decision (alpha
 *       floor, saturation, n_touched, the backward's liveness flags) stays on the vector ALU and is unchanged, so
 *       final_T / n_contrib / radii / n_touched are bit-identical; the images are rounded as fma(alpha T, f, C) where the
 *       reference's source order (CR/forward.cu:479-484) gives fma(f alpha, T, C): equal to ~1e-7 relative, not bit for
 *       bit.  Non-finite features then poison the 16-pixel block instead of the blending pixels only. */
#define OLSR_FLAG_FWD_ACCUM_MFMA 2
/*   OLSR_FLAG_FWD_ACCUM_WEIGHT  (forward) the same rounding as the MFMA variant on the vector ALU: w = alpha T once per pixel,
 *       then one fma(w, f, C) per channel instead of the reference's mul + fma (half the lane operations of the
 *       accumulation).  Decisions unchanged and bit-identical; images to ~1e-7 relative of the reference's rounding. */
#define OLSR_FLAG_FWD_ACCUM_WEIGHT 4
/*   OLSR_FLAG_FRAMES_IN_FLIGHT  (forward; round 5) the caller keeps SEVERAL frames in flight on several HIP streams (the views of
 *       a mapping iteration, a benchmark's lanes).  One composite kernel fills the chip, and the workgroup dispatcher keeps
 *       feeding it while it has workgroups left: a 1024-thread workgroup of ANOTHER frame's radix sort needs sixteen free wave
 *       slots on one CU and gets them only in the composite's tail, so the frames' dependent binning chains stalled behind each
 *       other's composites (kernel trace, four frames in flight: radix passes of 15 us stretched to 147 us, no composite
 *       executing during 26 % of the wall time).  With the flag the histogram and pass kernels of this frame run as four-wave
 *       workgroups with sixteen keys per thread, which are placed sooner: + 2 % frames/s with four frames in flight at config 3
 *       (2 304 -> 2 350, K = 60) — and - 11 % with ONE frame in flight (the depth sort 69 -> 108 us), which is why it is a
 *       statement about the caller and not the default.  Lists, images and gradients are bit-identical either way. */
#define OLSR_FLAG_FRAMES_IN_FLIGHT 8

/* How Gaussians are binned into tiles.
 *   OLSR_BINNING_RECT     every tile of the reference's bounding square (getRect, CR/auxiliary.h:46-56):
 *                         instance lists, num_rendered and n_contrib equal the reference's bit for bit.
 *   OLSR_BINNING_ELLIPSE  only the tiles that the ellipse alpha >= 1/255 can reach (a subset of the
 *                         square, same order).  The dropped (tile, Gaussian) pairs blend no pixel in the
 *                         forward and are whole-tile skips in the backward, so every image, radii,
 *                         n_touched and every gradient is unchanged; num_rendered and the state buffers'
 *                         list positions (n_contrib) count the kept pairs. */
#define OLSR_BINNING_RECT 0
#define OLSR_BINNING_ELLIPSE 1

/* Per-call scene description shared by forward and backward.
 * Replaces the positional argument lists of
 *   CudaRasterizer::Rasterizer::forward / backward           CR/rasterizer.h:33-104
 *   CudaRasterizer::LanguageRasterizer::forward / backward   CR/rasterizer.h:115-197
 * F == 0 selects the RGB-only rasterizer (GaussianRasterizer), F > 0 the language one. */
typedef struct olsr_scene {
  int32_t P;           /* number of Gaussians */
  int32_t D;           /* active SH degree 0..3 */
  int32_t M;           /* SH coefficients per channel in `shs` (0 when shs == NULL) */
  int32_t F;           /* language channels: 0, 3, 15, 16 or 32 */
  int32_t width;
  int32_t height;
  int32_t tile;        /* logical tile edge in pixels: 15 (reference, CR/config.h) or 16 */
  int32_t prefiltered; /* CR/auxiliary.h:154-161 */
  int32_t debug;       /* synchronise + check after every stage (CR/auxiliary.h:166-173) */
  int32_t bwd_mode;    /* OLSR_BWD_REFERENCE or OLSR_BWD_EXACT (used by backward only) */
  float tan_fovx;
  float tan_fovy;
  float scale_modifier;
  int32_t binning;     /* OLSR_BINNING_RECT or OLSR_BINNING_ELLIPSE (used by forward only) */
  const float *background;       /* [3] */
  const float *means3D;          /* [P,3] */
  const float *shs;              /* [P,M,3] or NULL */
  const float *colors_precomp;   /* [P,3] or NULL (exactly one of shs / colors_precomp) */
  const float *language_precomp; /* [P,F]; required when F > 0 (CR/rasterizer_impl.cu:500-502) */
  const float *opacities;        /* [P] */
  const float *scales;           /* [P,3] or NULL */
  const float *rotations;        /* [P,4] or NULL */
  const float *cov3D_precomp;    /* [P,6] or NULL (exactly one of scales+rotations / cov3D) */
  const float *viewmatrix;       /* [16] */
  const float *projmatrix;       /* [16] */
  const float *projmatrix_raw;   /* [16] (backward only; may be NULL in forward) */
  const float *cam_pos;          /* [3] */
  int32_t activations; /* OLSR_ACT_* bit mask: which parameter arrays are RAW (pre-activation); 0 = the
                        * reference's calling convention (already activated) */
  int32_t flags;       /* OLSR_FLAG_* bit mask, 0 = the reference's behaviour */
  float *tile_depth_cut; /* NULL (the default), or device float[2 x tiles], in/out — see "Per-tile depth cut-offs" below.
                          * Used by olsr_forward_async / olsr_forward_async_loss only. */
  int64_t backward_row_capacity; /* 0 (the default), or — for a caller that owns a fixed backward scratch — its row capacity
                          * (`scratch_rows` of the olsr_backward that will follow, with this bwd_mode and tile).  The forward's last
                          * launch then also compacts the backward's rows (which depend on the forward alone), and an
                          * olsr_backward given a scene with the same non-zero value skips its own compaction launch: one launch
                          * and ~8 us less per frame.  Both calls must see the same value, bwd_mode and tile; the backward
                          * verifies scratch_rows == backward_row_capacity (OLSR_ERR_ARG) and needs scratch_alloc == NULL. */
  uint32_t *depth_order_carry; /* NULL (the default), or device uint32[P], in/out — see "Carried depth order" below.  Used by
                          * olsr_forward_async / olsr_forward_async_loss only. */
} olsr_scene;

/* Carried depth order (round 6; a performance hint for SEQUENCES of nearly identical views of the same Gaussians: the ~100
 * dependent tracking iterations of a frame, utils/slam_frontend.py:163-277, and the ~150 mapping iterations over one window of
 * keyframes, utils/slam_backend.py:499-670 — one array per VIEW).  The depth sort (hist + four radix passes: five dependent
 * launches, ~70 us whatever it sorts) orders the P Gaussians by (depth bits, index); between two iterations of such a loop
 * the pose or the parameters move by a step of the optimiser and the order changes only locally.  With
 * scene->depth_order_carry the forward REPAIRS the order the previous forward left in the array instead of sorting from
 * scratch: two launches of independent workgroups (no look-back, no ticket) merge-sort windows of 2048 ranks of the old
 * order under the new keys, first aligned, then offset by half a window, which is a complete sort whenever no Gaussian moved
 * by more than 1024 ranks; the second launch proves the result — every adjacent pair of (depth bits, index) strictly
 * ascending, which also proves that the array is a permutation — and otherwise raises a device-side flag that makes the
 * radix passes, which are enqueued behind the repair in any case, run instead of returning at once.  The lists are therefore
 * ALWAYS the reference's, bit for bit, whatever the array held on entry (zeros, another view's order, garbage: the frame then
 * simply pays for both); on exit the array holds this frame's order.  Sort keys are defined for all P Gaussians (the view-space
 * depth also for Gaussians outside the frustum, a monotone function of it behind the near plane), so that the order is a
 * property of the pose and not of what is visible.  olsr_forward (the synchronising entry) ignores the field, and so do
 * sorts that take the multi-kernel passes (more than 67 M Gaussians).
 * An array holds the order of exactly ONE frame in flight: a forward reads and rewrites it from its repair to its emission,
 * so two frames that may overlap on the device (different streams, OLSR_FLAG_FRAMES_IN_FLIGHT lanes) need an array each —
 * sharing one gives the reader an order that nothing has proved.  The emission reads the array with 16-byte loads: allocate it
 * 16-byte aligned.  A frame that contains a Gaussian whose sort key is 0xFFFFFFFF (view-depth bits all ones: a NaN with every
 * payload bit set, e.g. positions in memory filled with 0xFF) ALWAYS takes the radix passes: that key is the repair's padding,
 * and a proof that cannot tell a Gaussian from padding is not accepted. */

/* Per-tile depth cut-offs (round 4; an opt-in for SEQUENCES of nearly identical views: the ~100 tracking iterations of a
 * frame).  The forward composite reads a tile's depth-sorted list only until every pixel of the tile is saturated — at config 3
 * that is 14 % of the instances; the rest is emitted, tile-sorted and compacted for nothing.  With scene->tile_depth_cut
 * (device float[2 x tiles]: [0, tiles) the cut-offs in force, in/out — initialise with +infinity = no cut; [tiles, 2 tiles)
 * library scratch) the forward drops every Gaussian that lies behind the cut-off of EVERY tile its footprint reaches, and
 * leaves behind, per tile, the cut-off for the NEXT frame: 1.1 x the depth of the entry at which the tile saturated (+ 0.01),
 * +infinity if it did not saturate, then the largest of the tile's 3 x 3 neighbourhood (a depth edge may move into the tile).
 * A tile's list is complete up to its cut-off depth, so the result is EXACT — bit-identical images, radii and n_touched,
 * gradients equal up to the order of their per-Gaussian sums; num_rendered counts the kept instances — whenever every tile
 * saturated at an entry in front of its cut-off.  If one did not (the view or the scene moved too much) the frame is flagged
 * OLSR_STATUS_CUT_MISS in num_rendered_dev[1]: its images and gradients may lack contributions in that tile, and the caller
 * re-renders.  The array has been updated by then: a tile that did not saturate at all carries +infinity again (and so do
 * its neighbours, through the 3 x 3 maximum); a tile that saturated, but BEHIND its cut-off, carries the finite
 * 1.1 x (the depth it saturated at) + 0.01 — taken from a list that may have had holes, hence possibly still too near: such a
 * tile can miss once more and converges from below, every miss moving its cut-off outwards.  Exact tile binning
 * only (OLSR_BINNING_ELLIPSE; ignored with OLSR_BINNING_RECT), default forward accumulation only, and with a fused loss only
 * the tracking loss (OLSR_ERR_ARG otherwise); olsr_forward (the synchronising entry) ignores the field.
 * Without a host read-back: olsr_backward on the state buffers of a CUT_MISS frame writes zero gradients (status_dev[1] = 3),
 * and olsr_pose_step_gated given that frame's num_rendered_dev takes no step — an iteration whose frame missed is a no-op on
 * the device, and the k-th COUNTED step sees the pose the k-th step of the loop without cut-offs sees.  A missed iteration
 * still consumes one of a caller's fixed budget of iterations (the reference's tracking_itr_num): a caller that wants the
 * same NUMBER of optimiser steps iterates until status[1] of olsr_pose_step_gated (steps done, on the device) has reached
 * it — slam_iterations.TrackingLoop.run(steps) does, reading the count back every few iterations. */
#define OLSR_STATUS_CUT_MISS 3

/* Sizes of the three opaque state buffers (bytes).  Replace
 * CudaRasterizer::required<GeometryState|ImageState|BinningState>, CR/rasterizer_impl.h:84-90. */
size_t olsr_geometry_bytes(int32_t P, int32_t F);
size_t olsr_image_bytes(int32_t width, int32_t height, int32_t tile);
size_t olsr_binning_bytes(int64_t num_rendered, int32_t F);

/* Forward.  Replaces RasterizeGaussiansCUDA / RasterizeLanguageGaussiansCUDA ->
 * Rasterizer::forward / LanguageRasterizer::forward
 * (DGR/rasterize_points.cu:35-123,125-241; CR/rasterizer_impl.cu:216-362,364-525).
 * The three callbacks are invoked once each (geometry, image, then — after the
 * instance count is known, one host sync like CR/rasterizer_impl.cu:454-455 —
 * binning).  Outputs: out_color[3,H,W], out_language[F,H,W] (ignored when F == 0),
 * out_depth[H,W], out_opacity[H,W], radii[P] (int32), n_touched[P] (int32).
 * *num_rendered receives R, the number of (Gaussian, tile) instances. */
/* Non-finite Gaussians ("Non-finite inputs"; tests/test_gpu_nonfinite.py).  No input value can make a
 * kernel index out of bounds: every float that becomes a tile, a row or a count is converted saturating (NaN -> 0) and
 * clamped.  A Gaussian whose mean, scale, rotation or covariance is NaN or overflows to a NaN eigenvalue has radius 0 and
 * holds NO instance (the reference counts one uninitialised list slot for it: undefined there, culled here); radii[] is 0
 * for it.  A radius saturates at 2^31 - 1.  An opacity <= 0 is listed and never blended; a NaN opacity blends alpha = 0.99
 * wherever power <= 0, as in the reference.  A non-finite colour or language value makes exactly the pixels that blend it
 * non-finite.  A NaN conic (the covariance of a scale of 1e10 or more has overflowed) blends alpha = 0.99 in every pixel
 * of its rect, the reference's min(0.99f, opacity * exp(NaN)).  The outputs
 * are the reference's, bit for bit, NaN where it has NaN. */
/* Process-wide state olsr_forward keeps (results never depend on it; tested): per (device, stream, tile count) the
 * heaviest-first tile orders of up to 16 VIEWS the stream has rendered (launch-order hints: a one-wave kernel in front of the
 * composite picks the stored view matrix nearest to this frame's, else recycles the least recently used slot — the
 * reference's mapping loop renders its window of keyframes in turn on one stream; 16 x tiles x 4 bytes, stream-ordered
 * allocation, at most 64 keys with least-recently-used eviction, never freed otherwise); a ring of 256 mapped host slots for the gradient-row counts
 * (olsr_live_rows); two mapped host words per calling thread for the instance count (leaked at thread exit by design: a
 * thread_local destructor could run after the HIP runtime's teardown). */
int olsr_forward(const olsr_scene *scene,
                 olsr_alloc_fn geometry_alloc, void *geometry_user,
                 olsr_alloc_fn binning_alloc, void *binning_user,
                 olsr_alloc_fn image_alloc, void *image_user,
                 float *out_color, float *out_language, float *out_depth, float *out_opacity,
                 int32_t *radii, int32_t *n_touched,
                 int32_t *num_rendered, void *hip_stream);

/* Forward without a host sync: the caller provides all three buffers, the binning
 * buffer sized for `capacity` instances (olsr_binning_bytes(capacity, F)).  R stays on
 * the device; `num_rendered_dev` (device int32[2]) receives {R, status}: OLSR_STATUS_OK, _OVERFLOW
 * (nothing is rendered when R > capacity) or _SYNC_ERROR.  This is the entry the
 * benchmark and the frame-sharded trainer use; it has no reference counterpart
 * (SURVEY.md §7 step 8).
 *
 * tile_order_inout (device uint32[tiles], may be NULL): launch-order hint.  On entry it must hold a
 * permutation of [0, tiles) in which, inside each eighth of the range (one XCD's share), tiles are
 * sorted by expected work, heaviest first — the identity is fine for a first frame; on exit it holds
 * exactly that order measured on THIS frame.  Consecutive frames of a SLAM sequence (and the ~100
 * tracking iterations per frame) see nearly the same per-tile load, so feeding the array back lets the
 * forward composite start its stragglers first.  The result never depends on the order. */
int olsr_forward_async(const olsr_scene *scene,
                       void *geometry_buffer, void *binning_buffer, int64_t capacity,
                       void *image_buffer,
                       float *out_color, float *out_language, float *out_depth, float *out_opacity,
                       int32_t *radii, int32_t *n_touched,
                       int32_t *num_rendered_dev, uint32_t *tile_order_inout, void *hip_stream);

/* Backward.  Replaces RasterizeGaussiansBackwardCUDA / RasterizeLanguageGaussiansBackwardCUDA ->
 * Rasterizer::backward / LanguageRasterizer::backward
 * (DGR/rasterize_points.cu:243-331,333-455; CR/rasterizer_impl.cu:529-636,638-756).
 * `num_rendered` is the R returned by olsr_forward — or, for buffers filled by
 * olsr_forward_async, the `capacity` that call was given (it fixes the carving of the
 * binning buffer).
 *
 * Scratch.  The composite backward writes one partial-gradient row per (instance, 64-pixel
 * slot) pair that the forward actually blended; the per-Gaussian reduction then sums them in a
 * fixed order (this replaces the reference's float atomicAdd, CR/backward.cu:1176-1198, and
 * makes the gradients bit-reproducible).  The number of such pairs, L <= 4 R, is known on the
 * device after the forward.  Two ways to provide the row buffer, neither of which synchronises the stream:
 *   - scratch_alloc != NULL (the drop-in bindings, behind an olsr_forward): the library picks a row count and asks the
 *     callback for olsr_backward_scratch_bytes(rows, F) bytes.  rows_token is olsr_last_forward_token() taken right after
 *     the matching olsr_forward (0: none).  The rows are, first that applies: the count that forward posted
 *     (olsr_live_rows); the bound — 2 rows per instance in the reference mode of 15x15 tiles, else 4 — when the token's
 *     slot already belongs to a later forward (olsr_live_rows_overwritten); when the bound would cost more than 64 MB and
 *     an earlier call verified a ratio of rows per instance, a GUESS of 1.5 x ratio x num_rendered + 65536, rounded up to
 *     a multiple of 128 Ki rows; else olsr_backward_rows.  A guessed backward is launched at once, then the library waits
 *     up to 20 ms for the exact count; if the guess was too small (that backward wrote zeros) it calls the callback a
 *     SECOND time, with the exact size, and launches an exact backward on the same stream, which overwrites every output.
 *     Every exact count updates the process-wide ratio, a slowly decaying maximum: max(now, 0.9 old + 0.1 now)
 *     (olsr_debug_rows_ratio).  The callback is not called under a library lock.  A second call may release the first
 *     buffer while the first backward still reads it: the caller's allocator must hand that memory only to work ordered
 *     behind it on hip_stream, as a stream-ordered caching allocator (PyTorch's) does.
 *   - scratch_alloc == NULL: `scratch` holds olsr_backward_scratch_bytes(scratch_rows, F) bytes;
 *     rows_token is ignored.  If L > scratch_rows nothing is written and the overflow is reported
 *     through status_dev.
 * status_dev (device int32[2], may be NULL) receives {L, status}: OLSR_STATUS_OK / _OVERFLOW / _SYNC_ERROR.
 *
 * Cotangents.  dL_dout_color[3,H,W] is required.  dL_dout_language[F,H,W] and dL_dout_depth[H,W] may be NULL: "the loss
 * does not depend on that image" — what autograd hands the reference's backward as None and PyTorch turns into zeros
 * (DGR/diff_gaussian_rasterization/__init__.py:296-345).  The front end's tracking loss has no language term
 * (utils/slam_utils.py:92-121): without a language cotangent the RGB instantiation of the composite backward runs on the
 * language forward's state (the language terms of dL_dalpha vanish identically), every gradient equals what a zero-filled
 * cotangent gives, and dL_dlanguage / the bucket's language columns are written as zeros.
 *
 * Gradient outputs, all fully overwritten:
 *   dL_dmeans2D[P,3]  dL_dcolors[P,3]  dL_dlanguage[P,F]  dL_dopacity[P]
 *   dL_dmeans3D[P,3]  dL_dcov3D[P,6]   dL_dsh[P,M,3]      dL_dscales[P,3]
 *   dL_drotations[P,4]  dL_dtau[P,6]
 * dL_dconic[P,4] and dL_ddepths[P] are the reference's internal buffers
 * (DGR/rasterize_points.cu:390-391); they may be NULL.  The geometry and binning buffers carry
 * scratch regions the backward writes (the reference passes them as char* too).
 * dL_dtau_sum[6] (may be NULL) receives the sum over P that the Python layer computes at
 * DGR/diff_gaussian_rasterization/__init__.py:383-385.
 *
 * bucket (may be NULL): additionally write (assign != 0) or add (assign == 0) this view's gradients
 * straight into the flat all-reduce buffer and the densification statistics described at
 * olsr_accumulate_gradients — the same result as calling that function afterwards, without the
 * round trip through the separate arrays.  With a bucket, every per-Gaussian output above may be
 * NULL and is then not written (a mapping step only consumes the bucket and dL_dtau_sum).  Likewise with
 * dL_dtau_sum alone: tracking (utils/slam_frontend.py) optimises only the camera pose, so a pose-only backward
 * passes NULL for every per-Gaussian array. */
typedef struct olsr_grad_bucket {
  float *flat;        /* [P][3 xyz | 3M sh | 1 opacity | 3 scale | 4 rotation | F language] */
  float *densify;     /* [P][2]  {sum of ||dL_dmeans2D.xy|| over views, number of views that saw it} */
  int32_t *max_radii; /* [P] */
  int32_t assign;     /* 1: first view of a step (overwrite), 0: add */
  int32_t _pad0;
  uint64_t *row_mask; /* NULL, or device uint64[ceil(P / 64)], in/out: bit g is set when row g of `flat` MAY be non-zero.
                       * Saturation leaves ~98 % of a view's Gaussians without gradient (config 3), and an overwrite that
                       * rewrites their zero rows is 150 MB of stores per view for nothing: with a mask, assign != 0 writes
                       * only the rows that have a gradient now or whose bit was set (those are zeroed), and leaves the mask =
                       * rows with a gradient now; assign == 0 ORs the rows it adds to into the mask.  The result in `flat`
                       * is the same, bit for bit, provided the mask covers every non-zero row when the call is made: start
                       * with all ones (= unknown: the first overwrite is dense), and set it to all ones again after writing
                       * `flat` by any other means (a collective, olsr_accumulate_gradients, a sum of buckets).  `densify` and
                       * `max_radii` are always written for every Gaussian. */
} olsr_grad_bucket;
size_t olsr_backward_scratch_bytes(int64_t rows, int32_t F);
/* Exact scratch rows for the backward of an olsr_forward (the synchronising entry) without a synchronisation.  The
 * forward's last kernel posts the frame's gradient-row counts into mapped host memory; olsr_last_forward_token() names the
 * olsr_forward this thread issued last, olsr_live_rows(token, packed) returns that frame's row count — `packed` != 0: the
 * reference-mode backward of 15x15 tiles (one row per packed survivor wave), else one row per 64-pixel slot — or -1 while
 * the forward has not finished or after 256 later forwards of the thread reused the slot: size the scratch by the bound
 * (2 resp. 4 rows per instance) then.  No reference counterpart (its backward accumulates with atomics). */
int32_t olsr_last_forward_token(void);
int64_t olsr_live_rows(int32_t token, int32_t packed_survivor_waves);
/* The same, for a caller that runs ahead of the GPU (a training loop reaches its backward while the forward is still
 * executing): waits — polling the mapped word, the GPU is busy with the forward meanwhile — until the forward has posted
 * its counts, at most timeout_us microseconds, and not at all when the slot already belongs to a later forward.
 * Returns the row count or -1 (then size by the bound).  olsr_backward_rows calls it when the bound would cost more than
 * 64 MB of scratch (OLSR_ROWS_WAIT_US, read once at load, default 5000; 0: never wait). */
int64_t olsr_live_rows_wait(int32_t token, int32_t packed_survivor_waves, int32_t timeout_us);
/* 1 when the ring slot of `token` already belongs to a LATER forward (more than 255 forwards were issued before this
 * backward): the count will never be readable, so a caller sizes its scratch by the bound at once instead of guessing and
 * then waiting for a count that cannot arrive. */
int32_t olsr_live_rows_overwritten(int32_t token);
/* The last step of the drop-in olsr_backward's choice of rows (scratch_alloc != NULL), when it does not guess: the posted
 * count of (token, R instances, F), waited for when the bound would cost more than 64 MB, else the bound. */
int64_t olsr_backward_rows(int32_t token, int32_t packed_survivor_waves, int64_t num_rendered, int32_t F);
/* Non-finite Gaussians in the backward ("Non-finite inputs").  A culled Gaussian (radius 0) has zero
 * gradients.  A row the reference has finite stays finite and within the usual tolerance; a row it has NaN or infinite is NaN
 * or infinite element by element (OLSR_BWD_EXACT) — with two deviations, both towards "assumes finite values": (1) a
 * Gaussian no pixel blended skips the per-Gaussian chain and gets exact zeros where the reference multiplies a zero by its NaN
 * covariance; (2) in OLSR_BWD_REFERENCE the skipped recursion-only visits leave some rows finite that the reference has NaN.
 * A caller that must not step on NaNs masks non-finite rows itself. */
int olsr_backward(const olsr_scene *scene, const int32_t *radii,
                  void *geometry_buffer, int32_t num_rendered,
                  void *binning_buffer, const void *image_buffer,
                  olsr_alloc_fn scratch_alloc, void *scratch_user, int32_t rows_token,
                  void *scratch, int64_t scratch_rows,
                  const float *dL_dout_color, const float *dL_dout_language,
                  const float *dL_dout_depth,
                  float *dL_dmeans2D, float *dL_dconic, float *dL_dopacity,
                  float *dL_dcolors, float *dL_dlanguage, float *dL_ddepths,
                  float *dL_dmeans3D, float *dL_dcov3D, float *dL_dsh,
                  float *dL_dscales, float *dL_drotations, float *dL_dtau,
                  float *dL_dtau_sum, const olsr_grad_bucket *bucket,
                  int32_t *status_dev, void *hip_stream);

/* ---- optimiser step on the gradient bucket -------------------------------
 * One fused Adam step over all Gaussian parameters, fed by the flat bucket olsr_backward / the all-reduce
 * produced: replaces `self.gaussians.optimizer.step()` — torch.optim.Adam(param_groups, lr=0.0, eps=1e-15) over
 * xyz, f_dc, f_rest, opacity, scaling, rotation, f_language (gaussian_splatting/scene/gaussian_model.py:393-440,
 * utils/slam_backend.py:747-749) — with the same arithmetic (torch/optim/adam.py, single-tensor path, no
 * amsgrad / weight decay) and the same DENSE semantics (rows with zero gradient decay their moments and
 * move).  `step` is the 1-based step count AFTER the increment.  shs is [P,M,3] (k = 0: f_dc, k >= 1:
 * f_rest); parameter arrays hold whatever the caller optimises (raw parameters with scene.activations).
 * exp_avg / exp_avg_sq: [P, 11 + 3M + F] in bucket layout, zero before the first step. */
typedef struct olsr_adam_params {
  /* doubles, like the Python floats torch.optim.Adam holds: every scalar the update uses (1 - beta1, 1 - beta2,
   * the bias corrections, step_size = lr / bias_correction1, sqrt(bias_correction2)) is formed in double on the
   * host and rounded to fp32 once, exactly where torch rounds it */
  double lr_xyz, lr_sh_dc, lr_sh_rest, lr_opacity, lr_scale, lr_rotation, lr_language;
  double beta1, beta2, eps; /* 0.9, 0.999, 1e-15 in the reference */
  int32_t step;
  int32_t _pad0;
} olsr_adam_params;
int olsr_adam_step(int32_t P, int32_t M, int32_t F, const olsr_adam_params *params, const float *flat,
                   float *means3D, float *shs, float *opacities, float *scales, float *rotations,
                   float *language, float *exp_avg, float *exp_avg_sq, void *hip_stream);

/* The same step fed by SEVERAL buckets (1 <= n_flats <= 8, `flats` a host array of device pointers): the gradient of a row
 * is ((flats[0] + flats[1]) + flats[2]) + ... — exactly what adding the buckets into flats[0] first would leave, without
 * the read-modify-write passes over P x width floats (a caller that renders a step's views on several HIP streams keeps one
 * bucket per stream: frame_shard.FrameLanes). */
int olsr_adam_step_sum(int32_t P, int32_t M, int32_t F, const olsr_adam_params *params, int32_t n_flats,
                       const float *const *flats, float *means3D, float *shs, float *opacities, float *scales,
                       float *rotations, float *language, float *exp_avg, float *exp_avg_sq, void *hip_stream);

/* The same step for buckets that carry a row mask (olsr_grad_bucket.row_mask; round 5): row_masks[b] (host array of device
 * pointers, an entry or the array itself may be NULL = "every row may be non-zero") names the rows of flats[b] that may hold
 * a gradient; a row whose bit is clear is NOT READ — its gradient is the +0.0 the row holds by the mask's invariant.  The
 * update stays dense (every parameter and both moments of every row are read and written): parameters and moments equal
 * olsr_adam_step_sum's — torch.optim.Adam's — bit for bit.  What goes is the read of known-zero gradient rows: on a surface
 * map a view leaves 20 % of the rows live, on the i.i.d. volume of SURVEY 8(d) 2 %.  P must start at a multiple of 64 rows
 * of the masks (a block of the kernel owns one mask word). */
int olsr_adam_step_masked(int32_t P, int32_t M, int32_t F, const olsr_adam_params *params, int32_t n_flats,
                          const float *const *flats, const uint64_t *const *row_masks, float *means3D, float *shs,
                          float *opacities, float *scales, float *rotations, float *language, float *exp_avg,
                          float *exp_avg_sq, void *hip_stream);

/* dst bucket += src bucket — the sum of the per-stream buckets of a step before its exchange (what autograd's `.grad +=`
 * over the views of BackEnd.map does, utils/slam_backend.py:510-670) — reading and writing only the gradient rows that
 * src_row_mask says may be non-zero (NULL: all of them); dst_row_mask (may be NULL) |= src_row_mask.  densify (SUM) and
 * max_radii (MAX) are combined for every Gaussian.  Same bits as a dense dst += src (a row left alone is dst + 0.0). */
int olsr_bucket_add(int32_t P, int32_t width, float *dst_flat, float *dst_densify, int32_t *dst_max_radii,
                    uint64_t *dst_row_mask, const float *src_flat, const float *src_densify, const int32_t *src_max_radii,
                    const uint64_t *src_row_mask, void *hip_stream);

/* Per-group step counts (the reference's optimiser keeps one `step` per parameter group, and two of its map edits make
 * groups skip a step: gaussian_model.py replace_tensor_to_optimizer / densification_postfix replace parameters, whose `grad`
 * is then None in that iteration's optimizer.step()).  group_step[g] is group g's 1-based step count AFTER its increment,
 * g = OLSR_ADAM_GROUP_*; a group whose bit is set in skip_mask is not touched at all (parameters and moments unchanged).
 * The other fields of `base` are used as in olsr_adam_step (base.step is ignored).  With every group_step equal to s and
 * skip_mask 0 the result equals olsr_adam_step_masked with step s, bit for bit. */
#define OLSR_ADAM_GROUP_XYZ 0
#define OLSR_ADAM_GROUP_SH_DC 1
#define OLSR_ADAM_GROUP_SH_REST 2
#define OLSR_ADAM_GROUP_OPACITY 3
#define OLSR_ADAM_GROUP_SCALE 4
#define OLSR_ADAM_GROUP_ROTATION 5
#define OLSR_ADAM_GROUP_LANGUAGE 6
#define OLSR_ADAM_GROUPS 7
typedef struct olsr_adam_group_params {
  olsr_adam_params base;
  int32_t group_step[OLSR_ADAM_GROUPS];
  int32_t skip_mask;
} olsr_adam_group_params;
int olsr_adam_step_groups(int32_t P, int32_t M, int32_t F, const olsr_adam_group_params *params, int32_t n_flats,
                          const float *const *flats, const uint64_t *const *row_masks, float *means3D, float *shs,
                          float *opacities, float *scales, float *rotations, float *language, float *exp_avg,
                          float *exp_avg_sq, void *hip_stream);

/* ---- the isotropic regulariser of the mapping loss (csrc/k_adam.hip) -------------------------------------------------
 * The reference adds `10 * |scaling - scaling.mean(dim=1)|.mean()` to every mapping iteration's loss
 * (utils/slam_backend.py:664-667, scaling = exp(_scaling)); autograd then adds its gradient to _scaling.grad.  It is a
 * function of a Gaussian's own three scales, so the Adam step that already owns the row forms it itself
 * (olsr_adam_step_groups_reg: no extra pass); olsr_isotropic_reg is the same statement on its own, with the loss value.
 * Arithmetic, float32 unless stated, for row g with the parameter values x_k read BEFORE the step:
 *   s_k  = (activations & OLSR_ACT_SCALE_EXP) ? expf(x_k) : x_k          (the expf of the preprocess kernel)
 *   m    = ((s_0 + s_1) + s_2) / 3.0f,   d_k = s_k - m,   sg_k = (d_k > 0) - (d_k < 0)
 *   q_k  = 3 sg_k - (sg_0 + sg_1 + sg_2)                                  (an integer, |q| <= 4)
 *   w9   = (float)(weight / (9.0 * P_total))                              (formed in double on the host)
 *   r_k  = w9 * (float)q_k, once more times s_k when the parameter is raw — autograd's weight / (3 P) (sg_k - mean_j sg_j)
 *          through exp
 *   loss = weight / (3 P) * sum |d_k|: the sum in double in a fixed order (a row ((|d_0| + |d_1|) + |d_2|), rows per wave,
 *          waves per block, blocks), the same bits on every run.
 * A NaN scale is outside the contract: every comparison with it is false, so its row's r is +-0 (NaN on the NaN element
 * itself in raw mode) and the loss is NaN.
 *   grad     device float[P,3] (assigned) or NULL;  loss  device double[1] or NULL;  scratch: olsr_isotropic_reg_scratch_bytes(P),
 *            needed with loss.  P_total of the standalone entry is P.  OLSR_ERR_ARG: P < 0, NULL scales, activations outside
 *            OLSR_ACT_*, loss without scratch. */
size_t olsr_isotropic_reg_scratch_bytes(int32_t P);
int olsr_isotropic_reg(int32_t P, const float *scales, int32_t activations, double weight, float *grad, double *loss,
                       void *scratch, void *hip_stream);
/* olsr_adam_step_groups with the regulariser inside: the gradient of a scale element is (((f0 + f1) + ...) + r_k), the
 * regulariser added last — the bits of olsr_adam_step_groups fed one EXTRA bucket that holds olsr_isotropic_reg's gradient
 * in its scale columns and +0.0 elsewhere.  A clear row-mask bit still skips that row's bucket reads, not r_k; a skipped
 * scale group takes no regulariser.  P_total >= P (OLSR_ERR_ARG otherwise) keeps the 1 / P of the whole map when a row
 * range is stepped.  reg == NULL or isotropic_weight == 0: olsr_adam_step_groups itself, bit for bit. */
typedef struct olsr_adam_reg {
  double isotropic_weight; /* 10 in the reference */
  int32_t activations;     /* OLSR_ACT_* of the scene: OLSR_ACT_SCALE_EXP = `scales` holds log(scale) */
  int32_t P_total;
} olsr_adam_reg;
int olsr_adam_step_groups_reg(int32_t P, int32_t M, int32_t F, const olsr_adam_group_params *params, int32_t n_flats,
                              const float *const *flats, const uint64_t *const *row_masks, float *means3D, float *shs,
                              float *opacities, float *scales, float *rotations, float *language, float *exp_avg,
                              float *exp_avg_sq, const olsr_adam_reg *reg, void *hip_stream);

/* ---- map edits: densify, prune and extend the Gaussian map on the fused buffers (csrc/k_map_edit.hip) --------------
 * One primitive behind GaussianModel.densify_and_prune / prune_points / extend_from_pcd
 * (gaussian_splatting/scene/gaussian_model.py:718-961), in two launches around ONE host read:
 *   olsr_map_edit_plan   classifies every source row (keep / clone / split / drop), counts the output segments per block and
 *                        prefixes the counts over the blocks; status[0] = P_new (the caller reads it back to size the
 *                        destination: the edit's one host synchronisation);
 *   olsr_map_edit_apply  reads every source row once and writes the destination buffers out of place.
 * Output order is the reference's: [kept originals | kept clones | kept split children k = 0 | k = 1 | appended rows],
 * each segment in source order.  No atomics on data: two runs on the same inputs give the same bits.
 * Densify mode (OLSR_MAP_EDIT_DENSIFY; src->stats = {xyz_gradient_accum, denom}): g = accum / denom, 0/0 -> 0;
 * smax = max(exp(scaling)); clone: g >= max_grad and smax <= clone_max_scale (percent_dense * extent); split:
 * g >= max_grad and smax > clone_max_scale (N = 2 children; child k of source row j uses z[j, k, 0:3]:
 * xyz = build_rotation(q) (std * z) + xyz with std = exp(scaling), scaling = log(exp(scaling) / 1.6), other fields raw
 * copies); then every candidate row is dropped when sigmoid(opacity) < min_opacity, or — screen_size_term != 0 —
 * max(exp(scaling)) > big_scale (0.1 * extent).  The reference's max_radii2D > max_screen_size term never fires: its
 * densification_postfix has zeroed max_radii2D just before (:847-849).  Moments: kept originals keep theirs, new rows start
 * at zero; accumulators (stats, max_radii) are zeroed for EVERY row.
 * Mask mode (OLSR_MAP_EDIT_MASK): row j is dropped when drop_mask[j] != 0 (NULL: none); moments and accumulators follow the
 * kept rows (prune_points).  n_append > 0 appends that many rows from `append` (means3D, shs, opacities, scales, rotations;
 * language zero, kf_id = append_kf_id, n_obs 0, moments zero) and zeroes every row's accumulators (extend_from_pcd).
 * src_index[i] = the source row destination row i came from, or -(k + 1) for appended row k.
 * Scratch: olsr_map_edit_scratch_bytes(P); status: int32[8] = {P_new, kept originals, kept clones, kept children per k,
 * appended, 0, 0, 0}.  dst buffers hold dst_capacity rows; rows past dst_capacity are never written (OLSR_ERR_CAPACITY
 * from apply when P_new exceeds it - the status is read on the host first). */
#define OLSR_MAP_EDIT_DENSIFY 0
#define OLSR_MAP_EDIT_MASK 1
typedef struct olsr_map_buffers {
  float *means3D, *shs, *opacities, *scales, *rotations, *language; /* [P,3] [P,M,3] [P] [P,3] [P,4] [P,F] */
  float *exp_avg, *exp_avg_sq;                                      /* [P, 11 + 3M + F], bucket layout */
  int32_t *kf_id, *n_obs;                                           /* [P] */
  float *stats;                                                     /* [P,2] {xyz_gradient_accum, denom} */
  int32_t *max_radii;                                               /* [P] */
} olsr_map_buffers;
typedef struct olsr_map_edit_params {
  int32_t mode, n_append, append_kf_id, screen_size_term;
  float max_grad, min_opacity, clone_max_scale, big_scale; /* fp32, as torch compares a float tensor with a Python float */
} olsr_map_edit_params;
size_t olsr_map_edit_scratch_bytes(int32_t P);
int olsr_map_edit_plan(int32_t P, const olsr_map_edit_params *params, const olsr_map_buffers *src, const uint8_t *drop_mask,
                       void *scratch, int32_t *status, void *hip_stream);
int olsr_map_edit_apply(int32_t P, int32_t M, int32_t F, const olsr_map_edit_params *params, const olsr_map_buffers *src,
                        const float *z, const olsr_map_buffers *append, const void *scratch, const int32_t *status,
                        int32_t P_new, int32_t dst_capacity, const olsr_map_buffers *dst, int32_t *src_index,
                        void *hip_stream);

/* ---- the reference's other native dependency ----------------------------
 * mean_dist2[i] = mean of the squared distances from point i to its 3 nearest neighbours (FLT_MAX counts
 * for a missing neighbour when P < 4).  Replaces simple_knn._C.distCUDA2 -> SimpleKNN::knn
 * (submodules/simple-knn/spatial.cu:15-26, simple_knn.cu:185-221), used to initialise Gaussian scales
 * (gaussian_splatting/scene/gaussian_model.py:256-263).  points[P,3], mean_dist2[P], scratch of
 * olsr_knn_scratch_bytes(P) bytes; everything stays on the device (the reference copies the bounding box
 * to the host twice). */
size_t olsr_knn_scratch_bytes(int32_t P);
int olsr_knn_mean_dist2(int32_t P, const float *points, float *mean_dist2, void *scratch, void *hip_stream);

/* ---- keyframe seeding: the rows of a keyframe's new Gaussians from its RGB-D image (csrc/k_keyframe_seed.hip) ----------
 * Replaces FrontEnd.add_new_keyframe (utils/slam_frontend.py:106-132) + BackEnd.add_next_kf (utils/slam_backend.py:187-202)
 * -> GaussianModel.extend_from_pcd_seq -> create_pcd_from_image / create_pcd_from_image_and_depth
 * (gaussian_splatting/scene/gaussian_model.py:135-281), which copy image and depth to the host, go through Open3D
 * (create_from_color_and_depth, create_from_rgbd_image, random_down_sample), take np.median(depth) on the host and copy the
 * points back for distCUDA2.  Here: plan (dependent launches, no host read, no atomics on data — the radix histograms are
 * integer atomics, order-independent), ONE host read of status[1] = n_keep by the caller, finish.
 *
 * olsr_keyframe_seed_plan, with i = v W + u the pixel index, image [3,H,W] (planes plane_stride floats apart), depth [H,W]:
 *  1. validity   rgb_ok = ((r + g) + b) > rgb_boundary_threshold on the raw image; d' = rgb_ok ? depth : 0; a pixel is VALID
 *                iff 0 < d' < depth_trunc in float32 (NaN, negative and +inf depths are invalid).  status[0] = n_valid.
 *  2. median     of d' over ALL W H pixels, zeros included (np.median(depth), gaussian_model.py:204), by a radix select on the
 *                float bits: odd count -> the middle element, even count -> fl32(fl32(a + b) / 2) of the two middle ones.
 *                DEVIATION: a non-finite or negative d' counts as 0 (numpy would return NaN).
 *                point size ps = adaptive_pointsize ? (float) min(0.05, point_size * (double) median) : (float) point_size —
 *                the product in double, narrowed once, as numpy 1.x (the reference's environment) evaluates
 *                python_float * np.float32.  aux = {median, ps, 0, 0}.
 *  3. sample     n_keep = (int32)((double) n_valid * (1.0 / downsample)) (the count rule of Open3D's random_down_sample as
 *                this project states it); status[1] = n_keep.  Pixel i has the key fmix32(i ^ (seed * 0x9E3779B9)), fmix32 =
 *                murmur3's finaliser (x ^= x >> 16; x *= 0x85EBCA6B; x ^= x >> 13; x *= 0xC2B2AE35; x ^= x >> 16, mod 2^32):
 *                a bijection, so no two pixels tie.  Kept: the n_keep valid pixels with the smallest keys, emitted in PIXEL
 *                ORDER; pix_index[k] = i.  DEVIATION: Open3D's shuffle (and its order of the sample) is not reproduced.
 *  4. colour     c = clamp(exp(a) img + b, 0, 1) in float32 — the library's pinned exp, product and sum rounded separately —
 *                or img itself when exposure == NULL; byte = (uint8)(c * 255) (truncation); colour = (float) byte / 255.0f;
 *                shs[k, 0, :] = (colour - 0.5f) / (float) 0.28209479177387814 (RGB2SH), shs[k, 1:, :] = 0.
 *  5. position   in double, as Open3D back-projects: z = d', x = (u - cx) z / fx, y = (v - cy) z / fy; world = Rt (p - t) with
 *                R, t the float32 entries of w2c (row-major world-to-camera) widened to double, component k =
 *                (R0k q0 + R1k q1) + R2k q2, q = p - t, no FMA contraction; narrowed to float32 once (the reference's
 *                .float()).  DEVIATION: the reference inverts the 4x4 in Eigen; Rt (p - t) is the contract here.
 *  6. constants  rotations (1, 0, 0, 0), opacities 0.0f = inverse_sigmoid(0.5).
 * olsr_keyframe_seed_finish(n = status[1]): olsr_knn_mean_dist2 over the n new points alone, then
 * scales[k, 0:3] = logf(sqrtf(max(d2, 1e-7f) * ps)).  DEVIATION: with n < 4 distCUDA2 has no three neighbours; finish then
 * returns OLSR_OK and writes nothing, and the caller appends nothing.
 * The monocular branch of the reference (random synthetic depth, gaussian_model.py:163-169) is not part of this entry.
 * rows: staging of `capacity` rows (means3D, shs [capacity, M, 3], opacities, scales, rotations; the other members are not
 * read); capacity >= (W H) / downsample always holds n_keep, so the caller sizes it without a host read.  scratch:
 * olsr_keyframe_seed_scratch_bytes(W, H), the same buffer for plan and finish; knn_scratch: olsr_knn_scratch_bytes(n).
 * OLSR_ERR_ARG before anything touches the device: a NULL pointer (exposure excepted); W, H or downsample <= 0;
 * plane_stride < W H; capacity < W H / downsample; M < 1; fx or fy not finite or not positive; depth_trunc <= 0;
 * finish: n < 0 or n > capacity. */
typedef struct olsr_keyframe_seed_params {
  int32_t W, H;                 /* image size */
  int64_t plane_stride;         /* floats between the three colour planes */
  int32_t M;                    /* SH coefficients per channel, (max_sh_degree + 1)^2 */
  int32_t downsample;           /* pcd_downsample or pcd_downsample_init: the caller chooses */
  uint32_t seed;                /* seed of the sampling hash */
  int32_t _pad0;
  double fx, fy, cx, cy;        /* intrinsics */
  float rgb_boundary_threshold; /* rgb-validity threshold */
  float depth_trunc;            /* the reference passes 100 */
  double point_size;            /* configured point size */
  int32_t adaptive_pointsize;   /* 0 or 1 */
  int32_t capacity;             /* rows the staging buffers (and pix_index) hold */
} olsr_keyframe_seed_params;
size_t olsr_keyframe_seed_scratch_bytes(int32_t W, int32_t H);
int olsr_keyframe_seed_plan(const olsr_keyframe_seed_params *p, const float *image, const float *depth,
                            const float *exposure /* device float[2] {a, b} or NULL */,
                            const float *w2c /* device float[16], row-major world-to-camera */, const olsr_map_buffers *rows,
                            int32_t *pix_index /* [capacity] */, void *scratch, int32_t *status /* int32[8] */,
                            float *aux /* float[4] {median, point_size, 0, 0} */, void *hip_stream);
int olsr_keyframe_seed_finish(const olsr_keyframe_seed_params *p, int32_t n, const olsr_map_buffers *rows, const float *aux,
                              void *scratch, void *knn_scratch, void *hip_stream);

/* ---- front end: the frame step around the tracking loop (csrc/k_frontend.hip) ------------------------------------------
 * What the reference's front end does once per frame in PyTorch ops with host reads (utils/slam_frontend.py:577-676): the
 * tracking mask (Camera.compute_grad_mask, utils/camera_utils.py:123-152), the median depth after tracking (get_median_depth,
 * utils/slam_utils.py:168-179) and the keyframe test with the window policy (is_keyframe / add_to_window and the small-window
 * rule, utils/slam_frontend.py:279-430, 633-645).  No float atomics; the radix histograms and the counts are integer atomics,
 * order-independent: two runs give the same bits.  "Lower median" below is the element of rank (n - 1) / 2 in ascending order,
 * which is what torch.median returns.  Every entry returns OLSR_ERR_ARG before anything touches the device for a NULL required
 * pointer, a size <= 0, a size above 2^31 - 1, and what its own paragraph lists.
 *
 * olsr_grad_mask: image [3,H,W] (planes plane_stride floats apart, no alignment requirement) -> mask [H,W] float.
 * Float32 statements, every operation rounded once (correctly rounded divide and sqrt, no FMA), in this order:
 *   gray = ((r + g) + b) / 3.0f;  p = gray reflect-padded by 1 (index -1 -> 1, index n -> n - 2)
 *   gv = (1/32) (((3 p[y-1,x-1] + 10 p[y-1,x]) + 3 p[y-1,x+1]) - ((3 p[y+1,x-1] + 10 p[y+1,x]) + 3 p[y+1,x+1]))
 *   gh = (1/32) (((3 p[y-1,x-1] + 10 p[y,x-1]) + 3 p[y+1,x-1]) - ((3 p[y-1,x+1] + 10 p[y,x+1]) + 3 p[y+1,x+1]))
 *   ok = all nine padded neighbours satisfy |p| > 0.01f;  I = ok ? sqrtf(gv gv + gh gh) : 0
 * OLSR_GRAD_MASK_BLOCKS (the reference's `replica` branch): bh = H / 32, bw = W / 32; for r, c < 32 the block
 *   [r bh, (r+1) bh) x [c bw, (c+1) bw) takes the lower median med of its intensities, th = med * edge_threshold, and each of
 *   its pixels becomes (I > th && !(1.0f <= th)) ? 1 : 0 — the second term is the reference's two sequential masked writes,
 *   which zero everything when th >= 1.  Pixels outside the 32 x 32 blocks keep the RAW INTENSITY I, as the reference leaves
 *   them.  One launch, a workgroup per block, no scratch (scratch may be NULL).  OLSR_ERR_ARG: H or W < 32; a block of more
 *   than 8192 pixels (a 4K frame has 8040), or one whose (bh + 3) (bw + 2) floats exceed 64 KiB of LDS.
 * OLSR_GRAD_MASK_GLOBAL (every other dataset): mask = I > med_all * edge_threshold as 0 / 1 floats, med_all the lower median
 *   of all W H intensities (radix select on the float bits).  scratch: olsr_frontend_scratch_bytes(W H).  OLSR_ERR_ARG: H or
 *   W < 2 (reflect padding), scratch NULL.
 * Both: OLSR_ERR_ARG for plane_stride < W H and an unknown mode.  An image with NaN or infinite values is outside the contract
 * (the reference propagates NaN through its median).
 *
 * olsr_median_depth: get_median_depth(depth, opacity, mask) over N pixels.  A pixel is valid when depth > 0 && opacity > 0.95f
 * && (mask == NULL || mask[i] != 0), mask uint8; a NaN depth is invalid (NaN > 0 is false), +inf is valid, as in the reference.
 * median (device float[1]) = the lower median of the valid depths, count (device int32[1]) = how many there are.
 * DEVIATION: with no valid pixel the reference raises; here the median is NaN and the count 0.  return_std is not built
 * (nothing in the reference calls it).  scratch: olsr_frontend_scratch_bytes(N).
 *
 * olsr_covisibility: cur[i] = n_touched[i] > 0 over P Gaussians against K <= 16 keyframe visibilities (uint8 [P] each, nonzero
 * = visible; window position 0 = the last keyframe).  counts (device int64[OLSR_COVIS_COUNTS]): counts[0] = |cur|,
 * counts[1 + 2k] = |cur & vis_k|, counts[2 + 2k] = |vis_k|, the rest 0.  cur_out (uint8 [P] or NULL) receives cur — the new
 * keyframe's occ_aware_visibility entry.  One pass over the K + 1 arrays.  OLSR_ERR_ARG: K outside 0 ... 16, vis[k] NULL, k < K.
 *
 * olsr_keyframe_decide: one wave; reads counts and the median word on the device, the tracked pose cur_pose (float[16],
 * row-major world-to-camera, last row 0 0 0 1) and the K = window_len keyframe poses [K][16], and writes one record for the
 * host: int32[8] followed by float[OLSR_KEYFRAME_RECORD_FLOATS].  The reference's logic, statement for statement:
 *   t(A, B) = translation of A B^-1 = R_A c_B + t_A with c_B = -(R_B^-1 t_B), in double from the float32 entries: R^-1 =
 *     cofactors * (1 / det), det = (r00 c00 + r01 c01) + r02 c02, sums left to right, no FMA; t narrowed to float32 once;
 *     |t| = sqrtf((t0 t0 + t1 t1) + t2 t2) in float32.
 *   dist = |t(cur, kf_0)|;  ratio_u = (float) inter_0 / (float) (|cur| + |vis_0| - inter_0)  (torch's int / int)
 *   is_kf = (ratio_u < kf_overlap && dist > kf_min_translation * median) || dist > kf_translation * median  (float32 products)
 *   create = is_kf;  if (window_len < window_size) create = check_time && ratio_u < kf_overlap;
 *   if (single_thread) create = check_time && create.
 * Window policy on [cur] + window (window position k is position k + 1 there, so "positions >= 2" are k >= 1):
 *   cut_k = (float) inter_k / (float) min(|cur|, |vis_k|); the LAST k >= 1 with cut_k <= kf_cutoff is removed (removed_a).
 *   If K + 1 - (one removed) > window_size: score_i = (double) sqrtf(|t(kf_i, cur)|) * sum over the remaining j >= 1, j != i,
 *   ascending, of 1.0 / (double) (|t(kf_i, kf_j)| + 1e-6f), in double; the remaining i >= 1 with the largest score is removed
 *   (removed_b; the first maximum wins, np.argmax).  Both removals can happen in one call.  They are computed whether or not
 *   create is set; the caller commits them only when it is.  A union or minimum of 0 gives NaN, and every comparison with NaN
 *   is false, as in torch.  K = 0: dist and ratio_u are NaN, is_kf = 0.  DEVIATION: with nothing left to score the reference's
 *   np.argmax raises; here nothing is removed.
 * record int32: {create, removals, removed_a (-1: none), removed_b (-1: none), is_kf, |cur|, inter_0, |vis_0|};
 * record float: {dist, median, ratio_u, 0, cut_k [16], (float) score_k [16], 0 ...} (NaN where not computed).  The record has
 * 40 floats, not 24: K = 16 needs 4 + 2 * 16.
 * OLSR_ERR_ARG: window_len outside 0 ... 16, window_size < 1, kf_poses NULL with window_len > 0. */
#define OLSR_GRAD_MASK_BLOCKS 0
#define OLSR_GRAD_MASK_GLOBAL 1
#define OLSR_GRAD_MASK_MAX_BLOCK_PIXELS 8192
#define OLSR_COVIS_MAX_VIEWS 16
#define OLSR_COVIS_COUNTS 33            /* 1 + 2 * OLSR_COVIS_MAX_VIEWS */
#define OLSR_KEYFRAME_RECORD_FLOATS 40
#define OLSR_KEYFRAME_RECORD_BYTES 192  /* int32[8] + float[40] */
typedef struct olsr_covis_views {
  int32_t K;                                 /* keyframes in the window, 0 ... 16 */
  int32_t _pad0;
  const uint8_t *vis[OLSR_COVIS_MAX_VIEWS];  /* device uint8 [P] each; entries from K on are not read */
} olsr_covis_views;
typedef struct olsr_keyframe_decide_params {
  int32_t window_len;    /* K: keyframes in the window now */
  int32_t window_size;   /* Training.window_size */
  int32_t check_time;    /* (cur_frame_idx - last_keyframe_idx) >= kf_interval */
  int32_t single_thread;
  float kf_translation, kf_min_translation, kf_overlap, kf_cutoff;
} olsr_keyframe_decide_params;
size_t olsr_frontend_scratch_bytes(int64_t n);
int olsr_grad_mask(int32_t W, int32_t H, int64_t plane_stride, int32_t mode, float edge_threshold, const float *image,
                   float *mask, void *scratch, void *hip_stream);
int olsr_median_depth(int64_t N, const float *depth, const float *opacity, const uint8_t *mask /* or NULL */, void *scratch,
                      float *median, int32_t *count, void *hip_stream);
int olsr_covisibility(int64_t P, const int32_t *n_touched, const olsr_covis_views *views, uint8_t *cur_out /* or NULL */,
                      int64_t *counts, void *hip_stream);
int olsr_keyframe_decide(const olsr_keyframe_decide_params *p, const int64_t *counts, const float *median,
                         const float *cur_pose, const float *kf_poses, void *record, void *hip_stream);

/* ---- caller side of the path -----------------------------------------
 * Mapping loss of one view and its gradient with respect to the rendered images, in one pass over the
 * pixels.  Replaces, with their autograd backward,
 *   get_loss_mapping / get_loss_mapping_rgbd                        utils/slam_utils.py:124-165
 *   F.interpolate(gt_lang_feat, size=(H, W), mode='bilinear', align_corners=False)
 *   l1_loss(language_feat, gt_lang_feat_resize), lamda_lang weighting   utils/slam_backend.py:579-597
 *                                                        gaussian_splatting/utils/loss_utils.py:21-22
 *   loss = alpha * mean|m_rgb * (exp(a) * image + b) - m_rgb * gt_image|
 *        + (1 - alpha) * mean|m_d * depth - m_d * gt_depth|
 *        + lamda_lang * mean|language - resize(gt_language)|
 * with m_rgb = (sum_c gt_image > rgb_boundary_threshold), m_d = (gt_depth > 0.01), means over all
 * elements of the respective tensor.  The outputs dL_dimage[3,H,W], dL_ddepth[1,H,W] and
 * dL_dlanguage[F,H,W] are exactly the cotangents olsr_backward consumes, so the rendered images
 * make one round trip instead of the ~20 elementwise kernels of the PyTorch formulation.
 *   exposure      device float[2] {exposure_a, exposure_b}, or NULL / initialization != 0 for a = b = 0
 *   gt_language   [F, lang_height, lang_width] or NULL (no language term; dL_dlanguage zero-filled)
 *   loss          device float[4]: {total, rgb term, depth term, language term} (each already weighted)
 *   dL_dexposure  device float[2] {dL/da, dL/db} or NULL
 *   scratch       olsr_mapping_loss_scratch_bytes(width, height) bytes */
typedef struct olsr_loss_params {
  int32_t width, height;
  int32_t F;                       /* language channels (0: none) */
  int32_t lang_width, lang_height; /* size of gt_language (192 x 192 in the reference) */
  int32_t initialization;          /* != 0: skip the exposure transform (get_loss_mapping, :125-126) */
  float alpha;                     /* config["Training"]["alpha"], default 0.95 */
  float rgb_boundary_threshold;    /* config["Training"]["rgb_boundary_threshold"] */
  float lamda_lang;                /* BackEnd.lamda_lang (1.0), utils/slam_backend.py:80 */
  float one_minus_alpha;           /* the depth term's weight, (float)(1.0 - alpha) formed from the caller's DOUBLE alpha as the
                                      reference forms it (a Python double meeting a float32 tensor); 0: the library uses
                                      1.f - alpha, which carries the float alpha's own rounding alpha / (1 - alpha) times
                                      enlarged (3 ulp of the weight at 0.95) */
} olsr_loss_params;
size_t olsr_mapping_loss_scratch_bytes(int32_t width, int32_t height);
int olsr_mapping_loss(const olsr_loss_params *params, const float *image, const float *depth,
                      const float *language, const float *gt_image, const float *gt_depth,
                      const float *gt_language, const float *exposure,
                      float *dL_dimage, float *dL_ddepth, float *dL_dlanguage,
                      float *loss, float *dL_dexposure, void *scratch, void *hip_stream);

/* ---- the loss in the forward composite's epilogue ------------------------------------------
 * olsr_forward_async with olsr_mapping_loss / olsr_tracking_loss evaluated where the composite kernel still holds every
 * pixel's colour, depth, language features and transmittance in registers (the equivalent of CR/forward.cu:490-512): the
 * kernel writes the cotangents olsr_backward consumes (dL_dimage, dL_ddepth, dL_dlanguage) next to — or, with skip_images,
 * instead of — the images, and one partial sum per tile that a one-block kernel turns into loss[4] / dL_dexposure[2].
 * The rendered images make NO round trip: the separate loss kernel re-reads 4 (4 + F) bytes per pixel and writes as many.
 * Same arithmetic per pixel as the two stand-alone entries (shared source, csrc/olsr_loss_device.h): the cotangents are
 * bit-identical to theirs, the loss differs in the summation order only (per-tile instead of per-256-pixel partials).
 *   params        width / height must equal the scene's; params.F: language channels of the loss term — the scene's F, or 0
 *                 for "no language term" (then dL_dlanguage is not written: hand olsr_backward a NULL language cotangent)
 *   tracking      0: the mapping loss;  != 0: the tracking loss (opacity-weighted, grad_mask; params.F is ignored)
 *   skip_images   != 0: out_color / out_language / out_depth / out_opacity are not written and may be NULL
 *   gt_language   [F, lang_height, lang_width] or NULL (no language term)
 *   scratch       olsr_fused_loss_scratch_bytes(width, height, tile) bytes
 * Every normaliser of these losses is the pixel count (means over all elements): nothing has to be precomputed per keyframe.
 * Supported with the default forward accumulation (not with OLSR_FLAG_FWD_ACCUM_MFMA / _WEIGHT). */
typedef struct olsr_loss_fusion {
  olsr_loss_params params;
  int32_t tracking;
  int32_t skip_images;
  const float *gt_image;    /* [3,H,W] */
  const float *gt_depth;    /* [H,W] */
  const float *gt_language; /* [F,lang_height,lang_width] or NULL */
  const float *exposure;    /* device float[2] or NULL */
  const float *grad_mask;   /* [H,W] float or NULL (tracking only) */
  float *dL_dimage;         /* [3,H,W] */
  float *dL_ddepth;         /* [H,W] */
  float *dL_dlanguage;      /* [F,H,W]; required when a language term is evaluated */
  float *loss;              /* device float[4] {total, rgb, depth, language} */
  float *dL_dexposure;      /* device float[2] or NULL */
  void *scratch;
} olsr_loss_fusion;
size_t olsr_fused_loss_scratch_bytes(int32_t width, int32_t height, int32_t tile);
int olsr_forward_async_loss(const olsr_scene *scene,
                            void *geometry_buffer, void *binning_buffer, int64_t capacity,
                            void *image_buffer,
                            float *out_color, float *out_language, float *out_depth, float *out_opacity,
                            int32_t *radii, int32_t *n_touched,
                            int32_t *num_rendered_dev, uint32_t *tile_order_inout,
                            const olsr_loss_fusion *loss, void *hip_stream);

/* Tracking loss of one view (front end: the pose is optimised, the Gaussians are fixed) and its image cotangents.
 * Replaces get_loss_tracking / get_loss_tracking_rgb / get_loss_tracking_rgbd (utils/slam_utils.py:92-121):
 *   loss = alpha * mean(opacity * |m * (exp(a) * image + b) - m * gt_image|)
 *        + (1 - alpha) * mean|dm * depth - dm * gt_depth|
 * m = (sum_c gt_image > rgb_boundary_threshold) * grad_mask (grad_mask[H,W] float, NULL = all ones),
 * dm = (gt_depth > 0.01) * (opacity > 0.95).  params->F, lang_* and lamda_lang are ignored.
 * loss = device float[4] {total, rgb term, depth term, 0}.  No gradient is produced for `opacity`: the
 * rasterizer's autograd function discards the cotangent of its opacity output
 * (DGR/diff_gaussian_rasterization/__init__.py:333-343), so the reference's backward drops it as well.
 * Same scratch as olsr_mapping_loss.  Follow with olsr_backward in pose-only mode (dL_dtau_sum alone). */
int olsr_tracking_loss(const olsr_loss_params *params, const float *image, const float *depth,
                       const float *opacity, const float *gt_image, const float *gt_depth,
                       const float *grad_mask, const float *exposure,
                       float *dL_dimage, float *dL_ddepth, float *loss, float *dL_dexposure,
                       void *scratch, void *hip_stream);

/* ---- colour refinement (third loop of the back end, utils/slam_backend.py:769-819) --------------------------------------
 * loss = (1 - lambda_dssim) * mean|image - gt_image| + lambda_dssim * (1 - SSIM(image, gt_image)) and its gradient with
 * respect to `image`.  Replaces l1_loss and ssim (gaussian_splatting/utils/loss_utils.py:21-22, 42-101: 11-tap Gaussian
 * window, sigma 1.5, normalised in float32, zero padding of 5 without renormalised borders, per channel, C1 = 0.01^2,
 * C2 = 0.03^2, mean over all 3 H W elements) with their autograd backward: five grouped 11 x 11 convolutions and ~20
 * elementwise kernels become two launches (one when no gradient is asked for, plus a one-block reduction).  SSIM is also
 * the reference's evaluation metric (utils/eval_utils.py:174): pass dL_dimage = NULL for the values alone.
 *   image, gt_image   device float[3,H,W]; any H, W >= 1; gt_image is a constant
 *   dL_dimage         device float[3,H,W], fully overwritten, or NULL; a tie image == gt_image contributes 0 to the L1 part
 *   loss              device float[4]: {total, (1 - lambda) L1, lambda (1 - SSIM), SSIM}; deterministic sums, no host read
 *   scratch           olsr_refinement_loss_scratch_bytes(width, height) bytes (three intermediate [3,H,W] planes) */
size_t olsr_refinement_loss_scratch_bytes(int32_t width, int32_t height);
int olsr_refinement_loss(int32_t width, int32_t height, float lambda_dssim,
                         const float *image, const float *gt_image, float *dL_dimage, float *loss,
                         void *scratch, void *hip_stream);

/* ---- the online language autoencoder (back end, utils/slam_backend.py:266-323) ------------------------------------------
 * BackEnd.train_online_autoencoder trains EncoderDecoderOnline (language/autoencoder/model.py:314-354) on a keyframe's
 * N x 32 language feature rows and hands the codes back as the keyframe's language target (viewpoint.gt_lang_feat, :562-576):
 *   encode(x) = z / |z|,  z = W2 relu(W1 x + b1) + b2        32 -> 24 -> 15
 *   decode(c) = y / |y|,  y = W4 relu(W3 c + b3) + b4        15 -> 24 -> 32
 *   loss = mean_{N 32}|r - x| + 0.6 (1 - mean_N cos(r, x)),  r = decode(encode(x)),  cos = F.cosine_similarity(dim=1, eps=1e-8)
 * followed by autograd's backward and torch.optim.Adam.step (defaults: betas 0.9 / 0.999, eps 1e-8, no weight decay) — several
 * dozen launches of microsecond kernels and a loss.item() host read in the reference, two launches here (one more for codes of
 * the updated parameters), no host read, no atomics: a step is bit-reproducible.  Neither norm has an epsilon, as in the
 * reference: a row whose z or y is exactly zero gives NaN there and here.  relu'(0) = 0 and sgn(0) = 0, as autograd has them.
 * The sizes 32 / 24 / 15 are compiled in; params->in_dim / hidden_dim / code_dim must name them (anything else: OLSR_ERR_ARG).
 *   params        device float[2351], state_dict order: encoder.0.weight [24,32], encoder.0.bias [24], encoder.2.weight [15,24],
 *                 encoder.2.bias [15], decoder.0.weight [24,15], decoder.0.bias [24], decoder.2.weight [32,24], decoder.2.bias [32]
 *   exp_avg, exp_avg_sq   device float[2351], Adam's moments in the same order; zero before the first step
 *   features      device float[N,32] rows, a constant
 *   step_dev      device int32[1], the number of steps done; every call adds one.  params->step is the 1-based Adam step count
 *                 of this call; step <= 0: the count is step_dev[0] kept on the device (required then), so that a loop of steps is
 *                 enqueued without a synchronisation or replayed from a HIP graph; zero it to restart the optimiser
 *   loss          device float[4]: {total, L1 term, 0.6 (1 - mean cos) term, mean cos}, of the parameters BEFORE the update
 *   codes         device float[N,15] (OLSR_LANG_AE_CODES_ROWS) or [15,N] (OLSR_LANG_AE_CODES_CHANNELS: low_dim.T.view(15,h,w),
 *                 the language target olsr_mapping_loss reads, without a transpose pass) of the parameters BEFORE the update, or
 *                 NULL; follow with olsr_lang_ae_encode for the codes of the updated parameters (the reference's viz=True)
 *   grad_out      device float[2351] or NULL: the gradient Adam was given (a test instrument)
 *   scratch       olsr_lang_ae_scratch_bytes(N) bytes: per 256 rows one float32 partial gradient; they are added in double */
#define OLSR_LANG_AE_IN 32
#define OLSR_LANG_AE_HIDDEN 24
#define OLSR_LANG_AE_CODE 15
#define OLSR_LANG_AE_PARAMS 2351
#define OLSR_LANG_AE_CODES_ROWS 0
#define OLSR_LANG_AE_CODES_CHANNELS 1
typedef struct olsr_lang_ae_params {
  double lr;                 /* the reference: 1e-3 during initialisation, 1e-4 in map(); its scheduler is never stepped */
  double beta1, beta2, eps;  /* 0.9, 0.999, 1e-8 */
  int32_t step;
  int32_t code_layout;       /* OLSR_LANG_AE_CODES_* (checked even when codes is NULL) */
  int32_t in_dim, hidden_dim, code_dim;
  int32_t _pad0;
} olsr_lang_ae_params;
size_t olsr_lang_ae_scratch_bytes(int32_t N);
int olsr_lang_ae_train_step(const olsr_lang_ae_params *params_struct, int32_t N, const float *features,
                            float *params, float *exp_avg, float *exp_avg_sq, int32_t *step_dev,
                            float *loss, float *codes, float *grad_out, void *scratch, void *hip_stream);
/* codes = encode(features) and recon [N,32] = decode(codes), one launch each; code_layout as above, N >= 1. */
int olsr_lang_ae_encode(int32_t N, const float *features, const float *params, int32_t code_layout,
                        float *codes, void *hip_stream);
int olsr_lang_ae_decode(int32_t N, const float *codes, const float *params, int32_t code_layout,
                        float *recon, void *hip_stream);

/* ---- open-vocabulary text queries on a rendered language map (eval/evaluate_onlinelangslam.py:266-287) -------------------
 * The reference answers "where is the table?" from a rendered 15-channel code map with
 *   codes -> model_online.decode (15 -> 24 -> 32, the decoder half of olsr_lang_ae_*) -> AutoencoderMLP.decode (32 -> 192 ->
 *   256 -> 384 -> 512 -> 768, ReLU between layers, x / |x|) -> embed @ phrases.T -> softmax(10 [s_pos, s_neg])[0], smallest
 *   over the canonical negatives (eval/openclip_encoder.py:44-107) -> 30 x 30 mean (cv2.filter2D defaults) -> max point, mask
 * in torch ops that write the [N,768] feature image (2.5 GB at 1200 x 680).  Here stage A, olsr_lang_query_sims, goes from the
 * codes to the K similarities of every pixel in one launch on the fp32 matrix cores and stores nothing wider than K per pixel;
 * stage B, olsr_lang_query_relevancy, goes from the similarities to every per-phrase output on the device, without a host read
 * and without atomics: both are bit-reproducible.  Arithmetic is float32 (v_mfma_f32_16x16x4_f32 is a k-ordered fmaf chain),
 * norms and window sums are accumulated in double.
 *   widths        the layer widths of the general decoder, input first.  This build has kernels for the two-stage chain
 *                 {32, 192, 256, 384, 512, 768} behind the online decoder; any other list is OLSR_ERR_ARG (the single-stage
 *                 decoder {15, 24, 48, 96, 192, 384, 384, 768} has an entry of its own in olsr_single_stage.h, whose
 *                 similarities olsr_lang_query_relevancy takes as they are)
 *   phrases       device float[K,768], unit rows, 16-byte aligned: [n_pos positives | n_labels labels | negatives], 1 <= K <= 64
 *   codes         device float[15,in_height,in_width], channel-major: what the rasteriser returns.  When (dec_width,
 *                 dec_height) differs they are resampled first, as F.interpolate(mode="bilinear", align_corners=False) (:270)
 *   online_params device float[2351], the layout of olsr_lang_ae_* (its decoder half is read)
 *   decoder_params device float[745536], 16-byte aligned: AutoencoderMLP.decoder in state_dict order (decoder.0.weight [192,32],
 *                 decoder.0.bias [192], decoder.2.weight [256,192], ... decoder.8.bias [768])
 *   sims          device float[K,dec_height,dec_width]: <decode(codes) , phrase>
 * olsr_lang_query_relevancy reads sims and writes at (out_width, out_height); when that differs from the decode size the
 * similarity planes are up-sampled bilinearly first (the dot product is linear, so this is the reference's up-sampling of the
 * 768-channel features at :274 followed by the product).
 *   relevancy     float[n_pos,H,W]: get_relevancy + get_max_across' [..., 0:1]
 *   smoothed      float[n_pos,H,W]: the 30 x 30 mean (correlation, anchor (15,15): window -15 .. +14, border reflect-101)
 *   blended       float[n_pos,H,W]: 0.5 (smoothed + relevancy)
 *   score         float[n_pos]: max of smoothed;  coord int32[n_pos,2]: its (x, y), the first in row-major order among equals
 *   minmax        float[n_pos,2]: min and max of blended
 *   mask          uint8[n_pos,H,W] or NULL (required with OLSR_LANG_QUERY_WANT_MASK): clip(2 (b - min) / (max - min + 1e-9) - 1,
 *                 0, 1) > thresh (:146-152)
 *   labels        int32[H,W] or NULL (required with OLSR_LANG_QUERY_WANT_LABELS, which needs n_labels >= 1): get_semantic_map,
 *                 the argmax over label and negative similarities, an index >= n_labels written as -1
 *   scratch       olsr_lang_query_scratch_bytes(params) bytes: 16 bytes per positive and 32 x 32 output tile
 * n_pos = 0 (labels only) is allowed in olsr_lang_query_relevancy; at least one negative is required there. */
#define OLSR_LANG_QUERY_MAX_LAYERS 8
#define OLSR_LANG_QUERY_MAX_PHRASES 64
#define OLSR_LANG_QUERY_FEATURE_DIM 768
#define OLSR_LANG_QUERY_DECODER_PARAMS 745536
#define OLSR_LANG_QUERY_WANT_MASK 1u
#define OLSR_LANG_QUERY_WANT_LABELS 2u
typedef struct olsr_lang_query_params {
  int32_t n_widths;
  int32_t widths[OLSR_LANG_QUERY_MAX_LAYERS];
  int32_t K, n_pos, n_labels;
  int32_t in_width, in_height;    /* the code map */
  int32_t dec_width, dec_height;  /* the size the decoder runs at (the reference's evaluation: 480 x 640) */
  int32_t out_width, out_height;  /* the size of every output of olsr_lang_query_relevancy */
  float thresh;                   /* the reference: mask_thresh = 0.4 */
  uint32_t flags;                 /* OLSR_LANG_QUERY_WANT_* */
} olsr_lang_query_params;
size_t olsr_lang_query_scratch_bytes(const olsr_lang_query_params *params);
int olsr_lang_query_sims(const olsr_lang_query_params *params, const float *codes, const float *online_params,
                         const float *decoder_params, const float *phrases, float *sims, void *hip_stream);
int olsr_lang_query_relevancy(const olsr_lang_query_params *params, const float *sims, float *relevancy,
                              float *smoothed, float *blended, float *score, int32_t *coord, float *minmax,
                              uint8_t *mask, int32_t *labels, void *scratch, void *hip_stream);

/* ---- the general language encoder 768 -> 32 (utils/slam_backend.py:556-559 and :392-395) ---------------------------------
 * The reference turns a keyframe's CLIP map clip_viz_dense [1,768,h,w] into the rows the online autoencoder trains on with
 *   clip_viz_dense.permute(0,2,3,1).view(-1,768) -> auto_model.encode  (AutoencoderMLP.encode, language/autoencoder/model.py:
 *   15-56: Linear 768 -> 512, then three times BatchNorm1d / ReLU / Linear down to 256 -> 128 -> 64 -> 32, then x / |x|)
 * in torch ops: about 15 launches, a permuted copy of the map and every intermediate written and read again.  The module is in
 * eval() there (:142), so a BatchNorm1d is its running statistics.  Here one launch, the mirror of olsr_lang_query_sims:
 *   h1 = W0 x + b0;   h(k+1) = W(k) relu(bn(k)(h(k))) + b(k), k = 1..4;   features32 = h5 / |h5|
 *   bn(h) = alpha h + beta per channel, alpha = weight / sqrt(running_var + bn_eps), beta = bias - running_mean alpha, both
 *   computed in double and rounded once, applied as one fmaf in the producing layer's epilogue (never folded into weights)
 * Every product is float32 on v_mfma_f32_16x16x4_f32 (a fixed fmaf chain per output), ReLU is fmaxf(., 0) with a NaN kept
 * (torch's ReLU: a NaN input row gives a NaN output row), |h5|^2 is accumulated in double, and the norm has no epsilon: a row
 * whose h5 is exactly zero gives NaN, as in the reference.  No atomics: a call is bit-reproducible, a pixel's result does not
 * depend on the other pixels, and both input layouts give the same bits.
 *   widths          the layer widths, input first.  This build has a kernel for the two-stage chain {768, 512, 256, 128, 64, 32};
 *                   any other list (the single-stage {768, 384, 192, 96, 48, 24, 15} included) is OLSR_ERR_ARG: that chain's
 *                   encoder is a separate entry, declared in olsr_single_stage.h
 *   features768     device float, N >= 1 pixels.  OLSR_LANG_ENCODER_IN_CHANNELS: [768] planes of N pixels, plane_stride >= N
 *                   elements apart — a [1,768,h,w] tensor, or one item of a batch, read in place; no alignment is assumed and
 *                   nothing beyond pixel N - 1 of a plane is read.  OLSR_LANG_ENCODER_IN_ROWS: [N,768] (plane_stride unused)
 *   encoder_params  device float[572128], 16-byte aligned: AutoencoderMLP.encoder in state_dict order without
 *                   num_batches_tracked: encoder.0.weight [512,768], encoder.0.bias [512], encoder.1.{weight, bias,
 *                   running_mean, running_var} [512], encoder.3.weight [256,512], encoder.3.bias, encoder.4.*, encoder.6.*,
 *                   encoder.7.*, encoder.9.*, encoder.10.*, encoder.12.weight [32,64], encoder.12.bias [32]
 *   features32      device float[N,32] rows or NULL: what olsr_lang_ae_train_step takes, the back end's coco_lang_feat
 *   online_params, codes   both or neither, codes only with online_params: device float[2351] (the layout of olsr_lang_ae_*) and
 *                   float[N,15] or [15,N] (code_layout, OLSR_LANG_AE_CODES_*).  The epilogue then also runs the online encoder
 *                   32 -> 24 -> 15 on each pixel's unit row; the codes equal olsr_lang_ae_encode(features32) bit for bit
 * features32 and codes must not both be NULL. */
#define OLSR_LANG_ENCODER_PARAMS 572128 /* 568288 Linear + 3840 BatchNorm */
#define OLSR_LANG_ENCODER_IN_ROWS 0
#define OLSR_LANG_ENCODER_IN_CHANNELS 1
typedef struct olsr_lang_encoder_params {
  int32_t n_widths;
  int32_t widths[8];
  int32_t in_layout;     /* OLSR_LANG_ENCODER_IN_* */
  int32_t code_layout;   /* OLSR_LANG_AE_CODES_* (checked even when codes is NULL) */
  int64_t plane_stride;  /* elements between two channel planes (channel layout) */
  double bn_eps;         /* BatchNorm1d's eps: 1e-5 */
} olsr_lang_encoder_params;
int olsr_lang_encoder_encode(const olsr_lang_encoder_params *params, int32_t N, const float *features768,
                             const float *encoder_params, const float *online_params, float *features32,
                             float *codes, void *hip_stream);

/* ---- the high-resolution language feature net (language/supervisedNet.py:6-109, utils/slam_backend.py:547-555) ------------
 * The stage between the CLIP backbone and olsr_lang_encoder_encode: HighResLanguageFeatureNet in eval() turns the backbone's
 * maps fv = clip_vis_dense [768,h,w], f3 = res3 [384,h3,w3] and f2 = res2 [192,h2,w2] into the [768,8h,8w] map the encoder
 * reads.  Forward only, exact float32 on v_mfma_f32_16x16x4_f32, thirteen launches of one implicit-GEMM convolution kernel:
 *    0 initial_conv     3x3 768 -> 512, BN, ReLU                                    [512,h,w]
 *    1 upsample1        ConvTranspose2d(4, 2, 1) 512 -> 512, BN, ReLU               [512,2h,2w]
 *    2 fusion1 align    bilinear(f3 -> 2h x 2w, align_corners = False), 1x1 384 -> 512
 *    3 fusion1 fusion   3x3 over (upsample1 | align) 1024 -> 512, BN, ReLU  = fused
 *    4 fusion1 att.0    3x3 512 -> 512, BN, ReLU
 *    5 fusion1 att.3    1x1 512 -> 512, fused * sigmoid(.) + fused (one fmaf)
 *    6 upsample2        ConvTranspose2d 512 -> 256, BN, ReLU                        [256,4h,4w]
 *    7..10 fusion2      as 2..5 with f2 (192) and 256 channels
 *   11 upsample3        ConvTranspose2d 256 -> 128, BN, ReLU                        [128,8h,8w]
 *   12 final_conv       1x1 128 -> 768                                              [768,8h,8w]
 * The resize is sampled while the 1x1's input is staged and the concatenation is two sources walked one after the other along
 * K: neither copy exists.  A ConvTranspose2d runs as its four output parities, each a 2x2 convolution.  BatchNorm2d is its
 * running statistics, alpha = weight / sqrt(running_var + bn_eps), beta = bias - running_mean alpha, folded in double and
 * rounded once in the producing launch's epilogue, applied as relu(fmaf(alpha, conv + bias, beta)); ReLU keeps a NaN.  The K
 * order of every output is fixed (chunks of 32 input channels in order, the taps in order inside a chunk), there are no
 * atomics and no split K: a value depends on its own receptive field only and a call is bit-reproducible.
 *   fv, f3, f2      device float, channel planes of h w (h3 w3, h2 w2) contiguous pixels, *_stride >= that many elements apart:
 *                   a [1,C,.,.] tensor or one item of a batch, read in place; no alignment is assumed and nothing beyond a
 *                   plane's last pixel is read.  channels x stride must stay below 2^31.
 *   packed_params   device float[OLSR_HR_NET_PARAMS], 16-byte aligned.  The module's layers in the order of the list above,
 *                   each as   weight: taps x [out][in]  |  bias [out]  |  BatchNorm weight, bias, running_mean, running_var
 *                   [4][out] (the six layers that have one)   with the weight regrouped so that a tap's [out][in] slab is
 *                   contiguous: Conv2d's [out,in,kh,kw] as slab kh * kw_count + kw, ConvTranspose2d's [in,out,4,4] as slab
 *                   4 ky + kx, transposed to [out][in].  The fusion layers' in runs over the concatenation (high | low).
 *   workspace       device, 16-byte aligned, olsr_hr_net_workspace_bytes bytes: the intermediates.  The library allocates
 *                   nothing.  workspace_bytes in the struct is what the caller provides.
 *   out             device float [768] planes of 8h x 8w pixels, out_stride >= 64 h w elements apart
 *   launches        0: all thirteen.  Otherwise bit k selects launch k of the list (for timing single launches; the others'
 *                   outputs are whatever the workspace holds).
 * Enqueues on hip_stream, reads nothing back and does not synchronise. */
#define OLSR_HR_NET_PARAMS 19890816
#define OLSR_HR_NET_LAUNCHES 13
typedef struct olsr_hr_net_params {
  int32_t h, w, h3, w3, h2, w2;           /* the sizes of fv, f3, f2 */
  int32_t c_fv, c_f3, c_f2, c_out;        /* this build: 768, 384, 192, 768 */
  uint32_t launches;
  int32_t _pad0;
  int64_t fv_stride, f3_stride, f2_stride, out_stride; /* elements between two channel planes */
  double bn_eps;                          /* BatchNorm2d's eps: 1e-5 */
  uint64_t workspace_bytes;
} olsr_hr_net_params;
size_t olsr_hr_net_workspace_bytes(int32_t h, int32_t w, int32_t h3, int32_t w3, int32_t h2, int32_t w2); /* 0: bad sizes */
int olsr_hr_net_forward(const olsr_hr_net_params *params, const float *fv, const float *f3, const float *f2,
                        const float *packed_params, void *workspace, float *out, void *hip_stream);

/* ---- TSDF fusion of depth and language maps into a 3-D map (tsdf-fusion/fusion.py, fusion2.py, fusion3.py) ---------------
 * The reference's 3-D evaluation fuses, per keyframe, a depth image and a feature image (packed 8-bit colour in fusion.py, 3
 * float channels in fusion2.py, 15 in fusion3.py) into a truncated signed distance volume with one CUDA launch per frame, 16
 * image uploads per frame and 15 separate feature volumes, and takes the surface points and the mesh of that volume from
 * skimage's marching cubes on the host.  Here the volume stays on the device:
 *   tsdf   float[X,Y,Z] (z fastest), 1 where nothing was observed;  weight float[X,Y,Z], 0 there
 *   feat   OLSR_TSDF_FEAT_FLOAT: float[F,X,Y,Z], planar (the running mean of every channel; F = 0: geometry only, feat unused)
 *          OLSR_TSDF_FEAT_PACKED_RGB: float[X,Y,Z], one float b * 65536 + g * 256 + r per voxel as in fusion.py (F must be 1)
 * olsr_tsdf_init fills tsdf with 1 and weight and feat with 0 (one launch).
 * olsr_tsdf_integrate fuses 1 <= n_views <= OLSR_TSDF_MAX_VIEWS views in ONE launch.  A thread owns a voxel, applies the views
 * in index order, loads the voxel's state at the first view that reaches it, keeps it in registers, and stores it once: the
 * result equals n_views single-view calls bit for bit, the volume is read and written once per batch instead of once per
 * view, and a voxel that no view reaches is never written.  Per voxel and view the expressions and their order are those of
 * the reference kernel (fusion.py:93-139, fusion3.py:181-290) in float32, without FMA contraction and with IEEE division:
 *   pt = origin + voxel * voxel_size;  tmp = pt - pose[:,3];  cam = pose[:,:3]^T tmp (three-term sums left to right);
 *   pixel = roundf(fx * (cam_x / cam_z) + cx), roundf(fy * (cam_y / cam_z) + cy);  skip outside the image, at depth == 0 and
 *   at depth - cam_z < -trunc_margin;  dist = fminf(1, (depth - cam_z) / trunc_margin);  w_new = w_old + obs_weight;
 *   tsdf = (tsdf * w_old + obs_weight * dist) / w_new;  feat_c = (feat_c * w_old + obs_weight * new_c) / w_new, or for the packed
 *   colour the floor / round / min statements of fusion.py:128-139 (roundf: half away from zero).
 * Divergences from the reference kernel, on purpose:
 *   - voxel coordinates are integer quotients and remainders of the linear index, exact at any size (the reference divides
 *     (float)voxel_idx, which is wrong above 2^24 voxels);
 *   - the index bound is idx < X*Y*Z (the reference's `voxel_idx > N` lets idx == N through);
 *   - a voxel with !(cam_z > 0) is skipped (the reference kernel skips only cam_z < 0 and converts a NaN or infinite pixel
 *     coordinate to int at cam_z == 0; its CPU path tests pix_z > 0);
 *   - the rounded pixel coordinate is range-checked as a float, then converted (no undefined float -> int conversion);
 *   - rounding is roundf as in the reference kernel, where its CPU path rounds half to even (np.round);
 *   - a view may carry an opacity plane: a pixel with opacity < min_opacity counts as invalid depth (rendered maps have pixels
 *     no Gaussian covers; the reference fuses sensor depth, where 0 marks them).
 * olsr_tsdf_view (passed by value in the kernel arguments, 128 bytes):
 *   fx, fy, cx, cy  the pinhole intrinsics;  pose  camera-to-world, row-major [4,4];  obs_weight as in the reference
 *   depth         device float[H,W]
 *   feat          device float: OLSR_TSDF_IMAGE_CHANNELS [F,H,W] (what the rasteriser returns) or OLSR_TSDF_IMAGE_ROWS [H,W,F];
 *                 packed mode: float[H,W] of b * 65536 + g * 256 + r;  NULL only with F = 0
 *   opacity       device float[H,W] or NULL
 * olsr_tsdf_surface_plan / olsr_tsdf_surface_emit extract the surface point cloud: plan counts, per voxel, the grid edges it
 * owns that cross zero, prefixes the per-block counts in block order (no atomics: the output order is deterministic) and
 * writes status[0] = N; the caller reads those 4 bytes, allocates, and emit writes the points.
 *   - the edge from voxel v to v + e_a (a = x, y, z; inside the grid) is owned by v and crosses when (t0 < 0) != (t1 < 0);
 *     with min_weight > 0 both ends must also have weight >= min_weight (0, the default, is the reference, where an
 *     unobserved voxel counts as +1);
 *   - pos = v + e_a * (t0 / (t0 - t1)) in float32;  point = pos * voxel_size + origin (two roundings);
 *   - its features are those of the voxel rintf(pos) (the reference's np.round(verts).astype(int)); packed mode emits r, g, b;
 *   - order: voxel linear index, then axis.
 *   points float[N,3];  feats float[N,F] (packed: [N,3]; F = 0: may be NULL);  voxel_index int32[N] or NULL: the owner's linear index
 * These are the edge vertices of marching cubes at level 0, and the vertices of the mesh below.
 * olsr_tsdf_mesh_plan / olsr_tsdf_mesh_emit extract the surface as a triangle mesh, by the same pattern (count, prefix in block
 * order, emit; no atomics, deterministic order, one host read): plan writes status = {n_verts, n_faces, 0, 0} (n_faces clamped
 * to 2^31 - 1), the caller reads those, allocates, and emit writes the mesh.
 *   - the vertices are olsr_tsdf_surface_emit's: same rule, same order, same bits of points, feats and voxel_index;
 *   - a cube is owned by its lowest voxel v (x + 1 < X, y + 1 < Y, z + 1 < Z); its configuration has bit c set when the corner
 *     v + (c & 1, c >> 1 & 1, c >> 2 & 1) has tsdf < 0 (a NaN is not negative); with min_weight > 0 a cube is triangulated only
 *     when all eight corners have weight >= min_weight;
 *   - its triangles come from a generated table (csrc/olsr_mc_table.h, scripts/gen_mc_table.py states the rule: marching squares
 *     on every face, a face whose signs alternate cuts its two negative corners off separately, the closed loops fanned).  Two
 *     cubes that share a face draw the same segments on it, so the mesh is closed away from the volume's boundary and from
 *     cubes left out by min_weight.  No interior vertices and no asymptotic decider (Lewiner's variant, which skimage uses, has
 *     both): no parity with skimage's faces, vertex order or winding is claimed;
 *   - faces int32[M,3] index the vertex list, in cube linear order (z fastest), then table order; a face (i, j, k) is wound so
 *     that cross(v_j - v_i, v_k - v_i) points to the positive-distance (free-space) side;
 *   - normals float[N,3], per vertex: g(v) = the gradient of tsdf by central differences 0.5f * (t[+1] - t[-1]), one-sided
 *     (t[+1] - t[0], t[0] - t[-1]) on the grid's border and 0 along an axis of one voxel;  n = g0 + (g1 - g0) * mu at the edge's two
 *     voxels with the vertex's mu = t0 / (t0 - t1);  normal = n / sqrtf(nx * nx + ny * ny + nz * nz) (summed left to right), (0, 0, 0)
 *     where that length is 0.  It points to free space, like the winding.  float32 without contraction: a numpy restatement
 *     gives the same bits;
 *   - emit writes vertices below vert_capacity and faces below face_capacity only; its min_weight is the plan's (the plan's
 *     scratch holds what it decided).  3 * face_capacity must fit an int32: OLSR_ERR_ARG otherwise.
 *   scratch: olsr_tsdf_mesh_scratch_bytes: 4 bytes per voxel and four 32-bit words per block of 256 voxels.
 * Limits: X * Y * Z < 2^31 for integrate and init, 3 * X * Y * Z < 2^31 for the extraction. */
#define OLSR_TSDF_MAX_VIEWS 16
#define OLSR_TSDF_FEAT_FLOAT 0
#define OLSR_TSDF_FEAT_PACKED_RGB 1
#define OLSR_TSDF_IMAGE_CHANNELS 0
#define OLSR_TSDF_IMAGE_ROWS 1
typedef struct olsr_tsdf_volume {
  int32_t X, Y, Z;
  int32_t F;             /* OLSR_TSDF_FEAT_FLOAT: 0, 3, 15, 16 or 32; OLSR_TSDF_FEAT_PACKED_RGB: 1 */
  int32_t feat_mode;     /* OLSR_TSDF_FEAT_* */
  float voxel_size, trunc_margin;
  float origin[3];
  float *tsdf, *weight, *feat;
} olsr_tsdf_volume;
typedef struct olsr_tsdf_view {
  float fx, fy, cx, cy;
  float pose[16];
  float obs_weight;
  float min_opacity;
  int32_t H, W;
  int32_t feat_layout;   /* OLSR_TSDF_IMAGE_* */
  int32_t _pad0;
  const float *depth, *feat, *opacity;
} olsr_tsdf_view;
int olsr_tsdf_init(const olsr_tsdf_volume *volume, void *hip_stream);
int olsr_tsdf_integrate(const olsr_tsdf_volume *volume, int32_t n_views, const olsr_tsdf_view *views, void *hip_stream);
size_t olsr_tsdf_surface_scratch_bytes(int32_t X, int32_t Y, int32_t Z);
int olsr_tsdf_surface_plan(const olsr_tsdf_volume *volume, float min_weight, void *scratch, int32_t *status /* [2] = {N, 0} */,
                           void *hip_stream);
int olsr_tsdf_surface_emit(const olsr_tsdf_volume *volume, float min_weight, const void *scratch, int32_t capacity,
                           float *points, float *feats, int32_t *voxel_index, void *hip_stream);
size_t olsr_tsdf_mesh_scratch_bytes(int32_t X, int32_t Y, int32_t Z);
int olsr_tsdf_mesh_plan(const olsr_tsdf_volume *volume, float min_weight, void *scratch, int32_t *status /* [4] */,
                        void *hip_stream);
int olsr_tsdf_mesh_emit(const olsr_tsdf_volume *volume, float min_weight, const void *scratch, int32_t vert_capacity,
                        int32_t face_capacity, float *points, float *normals, float *feats, int32_t *voxel_index,
                        int32_t *faces /* [M,3] */, void *hip_stream);

/* ---- point-cloud metrics: approximate earth mover's distance and Chamfer distance (the reference's 3-D evaluation) ----------
 * The two numbers tsdf-fusion/3d_evaluation_and_visualize_langslam_dim15.py:396-423 reports per queried class, for ragged
 * batches of cloud pairs (one pair per class) in the same launches.
 *   B             1 <= B <= OLSR_CLOUD_MAX_SEGMENTS pairs ("segments")
 *   off1, off2    int32[B+1], non-decreasing, off[0] >= 0: segment b of cloud 1 is rows off1[b] .. off1[b+1]-1 of xyz1 (n_b
 *                 points), likewise cloud 2 (m_b points).  total = off[B] < 2^31 / 3.  Device memory or host memory, each table
 *                 on its own.  The tables are checked on the host before anything is launched: device tables
 *                 cost one 4 (B + 1)-byte read and a synchronisation of the stream, host tables one small upload into the scratch.
 *   max_n1/2      at least the longest segment of the cloud (sizes the grid); a longer segment is OLSR_ERR_ARG
 *   xyz1, xyz2    device float[total,3], packed
 *   scratch       device, olsr_*_scratch_bytes(B, off1[B], off2[B]) bytes.  EMD: per point 8 (the row's cost, double) + 12 (remain x 2, ratio) + 3 x 16 x 4 (cloud 1; 16 x 4
 *                 for cloud 2) bytes of partial sums: O(n + m), no match matrix.  Chamfer: 16 x 8 bytes per point.
 * An empty segment on either side is legal: its outputs are NaN (nn: -1), valid[b] = 0.  Non-finite coordinates make that
 * segment's outputs unspecified and touch no other segment.  A segment's outputs depend on its own points only, bit for bit:
 * the batch equals B single calls, and a repeated call repeats its bits (fixed-order sums, no floating-point atomics).
 *
 * olsr_emd_cost: PyTorchEMD's approxmatch + matchcost (tsdf-fusion/PyTorchEMD/cuda/emd_kernel.cu) without the match matrix.
 * With d_kl = (dx dx + dy dy) + dz dz (squared), multiL, multiR = (1, n / m) if n >= m else (m / n, 1) in integer division,
 * remainL = multiL, remainR = multiR, for j = 7 .. -2 (level = -4^j, 0 at j = -2) and e_kl = exp(level d_kl):
 *   1. ratioL[k] = remainL[k] / (1e-9 + sum_l e_kl remainR[l])
 *   2. sumr[l] = (sum_k e_kl ratioL[k]) remainR[l];  ratioR[l] = min(remainR[l] / (sumr[l] + 1e-9), 1) remainR[l];
 *      remainR[l] = max(0, remainR[l] - sumr[l])
 *   3. w_kl = e_kl ratioL[k] ratioR[l];  cost += sum_kl d_kl w_kl;  remainL[k] = max(0, remainL[k] - sum_l w_kl)
 * in float32; exp is the hardware's 2^x on (level log2 e) d, as the reference uses __expf.  Sums over the other cloud are
 * float32 partials over at most 16 chunks of it, added in chunk order; d w is summed in float32 per row, chunk and level and
 * in double over those.  cost[b] is sum d w, NOT divided by n (the reference's earth_mover_distance divides by n afterwards).
 *   residual      float[B,2] or NULL: sum remainL, sum remainR after the last level — the mass the approximate matching left
 *                 unassigned, which the reference drops silently
 * 23 launches for any B and any sizes (1 + 1 + 2 per level + 1), nothing read back in between.  No backward: the evaluation's
 * copy of emd.py saves nothing for one either.
 *
 * olsr_chamfer: per point the squared distance to its nearest point of the other cloud of its segment (d as above, not
 * contracted) and that point's segment-local index, the lowest index on ties; mean[b] = {mean over cloud 1 of sqrt(min_d2_1),
 * mean over cloud 2 of sqrt(min_d2_2)} in double — chamfer_distance's 'x_to_y' and 'y_to_x' with x = cloud 1; 'bi' is their
 * sum.  Brute force, n m pairs per segment; two launches. */
#define OLSR_CLOUD_MAX_SEGMENTS 32767
size_t olsr_emd_scratch_bytes(int32_t B, int64_t total1, int64_t total2);
int olsr_emd_cost(int32_t B, const int32_t *off1, const int32_t *off2, int32_t max_n1, int32_t max_n2,
                  const float *xyz1, const float *xyz2, double *cost /*[B], sum d w, undivided*/,
                  float *residual /*[B,2] = sum remainL, sum remainR after the last level; may be NULL*/,
                  int32_t *valid /*[B]*/, void *scratch, void *hip_stream);
size_t olsr_chamfer_scratch_bytes(int32_t B, int64_t total1, int64_t total2);
int olsr_chamfer(int32_t B, const int32_t *off1, const int32_t *off2, int32_t max_n1, int32_t max_n2,
                 const float *xyz1, const float *xyz2, float *min_d2_1, int32_t *nn_1, float *min_d2_2, int32_t *nn_2,
                 double *mean /*[B,2]: x->y, y->x*/, int32_t *valid, void *scratch, void *hip_stream);

/* ---- scoring text queries: mask smoothing, IoU, localisation, masked PSNR (the reference's 2-D evaluation) ----------------
 * What eval/evaluate_onlinelangslam.py does with the maps olsr_lang_query_relevancy returns, up to the counts its two reported
 * figures (mean IoU, localisation accuracy) are formed from, and the masked PSNR of utils/eval_utils.py:171-173.  Everything but
 * the PSNR is integer arithmetic without atomics: the results are exact and the same on every run.  One head only: the online
 * pipeline has one level, so the reference's choice among heads (:165-172, :208) has nothing to choose from.
 *
 * olsr_mask_smooth: `smooth` of eval/utils.py:47-56, a 7 x 7 majority vote, in one launch.
 *   mask_in       device uint8[P,H,W], read as it lies: no alignment of planes or rows is assumed.  A byte != 0 counts as 1
 *   mask_out      device uint8[P,H,W] of 0 / 1, out of place (mask_out == mask_in is OLSR_ERR_ARG; overlapping is undefined)
 * For pixel (i, j) the window is rows max(0, i-3) .. min(i+4, H-1) - 1 and columns max(0, j-3) .. min(j+4, W-1) - 1: the
 * reference's slice, its quirk kept — the upper bound is clamped to H-1 / W-1, so the last row and the last column never
 * enter any window.  out = 1 iff 2 * ones > area of that window; a tie gives 0, as np.argmax(np.bincount(.)) takes the first
 * maximum.  Deviations: H < 2 or W < 2 is OLSR_ERR_ARG where the reference raises on the empty window; a mask that is not
 * binary is binarised first, where the reference would vote over the byte values.  1 <= P <= 65535, H, W <= 2^20,
 * H W < 2^31.
 *
 * olsr_query_eval: the same pass with the counts of :160-161 and :203-223 in its epilogue, then one launch that adds the
 * workgroups' partial counts per phrase.  Nothing is read back; the caller reads 16 P bytes.
 *   mask          device uint8[P,H,W]: the mask BEFORE smoothing, as olsr_lang_query_relevancy wrote it
 *   smoothed      device float[P,H,W] and score float[P] (its maximum), as olsr_lang_query_relevancy wrote them
 *   gt_mask       device uint8[P,H,W]: the annotated masks, already at the map's size (the reference's cv2.resize of the
 *                 annotation, :157, stays with the caller); != 0 counts as set
 *   boxes         device float[B,4] = (x1, y1, x2, y2) in pixels of the map, or NULL if there is none
 *   box_offsets   int32[P+1], non-decreasing from >= 0: phrase p owns boxes box_offsets[p] .. box_offsets[p+1] - 1, possibly
 *                 none.  Host or device memory, checked on the host before anything is launched (a device table costs one
 *                 small read and a synchronisation of the stream, a host table one small upload into the scratch)
 *   result        device int32[P,4] = {intersection, union, n_max, hit}: the counts of gt & s and gt | s with s the smoothed
 *                 mask (IoU = intersection / union; 0 / 0 is the reference's NaN and left to the caller); the number of
 *                 pixels with smoothed == score[p]; 1 iff any of THOSE pixels (x = column, y = row) lies in any of the
 *                 phrase's boxes, min(x1,x2) <= x <= max(x1,x2) and likewise y, bounds included.  Every pixel that attains
 *                 the maximum is tested, as the reference does — olsr_lang_query_relevancy's coord is only the first of
 *                 them.  No box: hit = 0.  A NaN score: n_max = 0, hit = 0
 *   mask_smoothed device uint8[P,H,W] or NULL: the smoothed masks, if wanted (never mask itself)
 *   scratch       device, olsr_query_eval_scratch_bytes(P, H, W) bytes: 16 bytes per phrase and 64 x 64 tile
 *
 * olsr_image_psnr: image, gt device float[C,H,W] (C H W < 2^31) -> out double[2] = {sum of (clamp(image, 0, 1) - gt)^2 over the
 * ELEMENTS with gt > 0, their number} — image[mask] with mask = gt_image > 0 is per element in the reference, not per pixel.
 * The difference is float32 as the reference's, its square and the sums are double in an order that depends on C H W alone.
 * The caller forms mse = sum / count and 20 log10(1 / sqrt(mse)); a count of 0 gives the reference's NaN.  Two launches.
 *   scratch       device, olsr_image_psnr_scratch_bytes() bytes */
#define OLSR_QUERY_EVAL_MAX_PLANES 65535
#define OLSR_QUERY_EVAL_MAX_EXTENT 1048576
int olsr_mask_smooth(int32_t P, int32_t H, int32_t W, const uint8_t *mask_in, uint8_t *mask_out, void *hip_stream);
size_t olsr_query_eval_scratch_bytes(int32_t P, int32_t H, int32_t W);
int olsr_query_eval(int32_t P, int32_t H, int32_t W, const uint8_t *mask, const float *smoothed, const float *score,
                    const uint8_t *gt_mask, const float *boxes, const int32_t *box_offsets,
                    int32_t *result /*[P,4]*/, uint8_t *mask_smoothed /*may be NULL*/, void *scratch, void *hip_stream);
size_t olsr_image_psnr_scratch_bytes(void);
int olsr_image_psnr(int32_t C, int32_t H, int32_t W, const float *image, const float *gt, double *out /*[2]*/,
                    void *scratch, void *hip_stream);

/* ---- one tracking iteration's pose update (the front end) ----------------------
 * Replaces, per iteration of the reference's tracking loop (utils/slam_frontend.py:216-243),
 *   pose_optimizer.step()           torch.optim.Adam over cam_rot_delta (lr config Training.lr.cam_rot_delta = 0.003),
 *                                   cam_trans_delta (0.001), exposure_a / exposure_b (0.01); eps 1e-8, betas (0.9, 0.999)
 *   converged = update_pose(cam)    utils/pose_utils.py:79-97: tau = [cam_trans_delta | cam_rot_delta],
 *                                   new_w2c = SE3_exp(tau) @ T_w2c (:61-76), converged = |tau| < 1e-4, deltas zeroed
 * and the camera properties the next render reads (utils/camera_utils.py:103-117): world_view_transform = W2C^T,
 * full_proj_transform = world_view_transform @ projection_matrix, camera_center = world_view_transform^-1 [3, :3]
 * — one launch instead of ~40 one-element PyTorch kernels and a host read-back between two dependent renders.
 * Tolerance: Adam, SE3_exp and the convergence test follow the reference operation for operation; the view matrix is formed
 * directly as W2C^T, where the reference's Camera goes through getWorld2View2 (gaussian_splatting/utils/graphics_utils.py:
 * 33-46), which inverts [R|t] twice, and update_pose re-reads R and T from that.  T_w2c and the matrices therefore agree with
 * the reference to fp32 rounding per iteration (tests/test_gpu_pose.py holds them to 5e-7 x the iteration number), not
 * bit for bit.
 *   dL_dtau_sum   device float[6] = [rho | theta] as olsr_backward leaves it (rho: gradient of cam_trans_delta,
 *                 theta: of cam_rot_delta), or NULL: no step, only the matrices of the current pose are (re)derived
 *   dL_dexposure  device float[2] from olsr_tracking_loss, or NULL (exposure not optimised)
 *   projection_matrix  device float[16], the P^T the callers hold (Camera.projection_matrix)
 *   state         device float[80], all zero before the first call except T_w2c:
 *                 [0,16) T_w2c row-major (in/out) | [16,32) world_view_transform | [32,48) full_proj_transform |
 *                 [48,51) camera_center | [52,58) exp_avg of tau | [58,64) exp_avg_sq | [64,70) tau this step applied |
 *                 [70,72) exposure a, b (in/out) | [72,74) their exp_avg | [74,76) exp_avg_sq
 *   status        device int32[2]: {converged flag of this step, steps done}
 * params->step is the 1-based Adam step count of this call; step <= 0: the count is status[1] + 1, kept on the device (the
 * launch is then the same every iteration and can be replayed from a HIP graph; reset status to restart the optimiser). */
typedef struct olsr_pose_params {
  double lr_rot, lr_trans, lr_exposure;
  double beta1, beta2, eps;  /* torch.optim.Adam defaults in the reference: 0.9, 0.999, 1e-8 */
  double converged_threshold; /* 1e-4 */
  int32_t step;
  int32_t _pad0;
} olsr_pose_params;
int olsr_pose_step(const olsr_pose_params *params, const float *dL_dtau_sum, const float *dL_dexposure,
                   const float *projection_matrix, float *state, int32_t *status, void *hip_stream);
/* olsr_pose_step, skipped on the device when the frame its gradient came from was not usable:
 *   frame_status  device int32[2], the num_rendered_dev of that frame's olsr_forward_async[_loss] (or NULL: always step).
 * frame_status[1] != 0 (OLSR_STATUS_OVERFLOW / SYNC_ERROR / CUT_MISS): no optimiser step — state [0,16) and [52,76) and
 * status[1] keep their values, status[0] = 0 — only the matrices are re-derived, as with dL_dtau_sum == NULL. */
int olsr_pose_step_gated(const olsr_pose_params *params, const float *dL_dtau_sum, const float *dL_dexposure,
                         const float *projection_matrix, float *state, int32_t *status, const int32_t *frame_status,
                         void *hip_stream);

/* ---- mapping's bundle adjustment: every window keyframe's pose and exposure step in ONE launch ----------------------
 * The reference's back end builds one torch.optim.Adam (`keyframe_optimizers`, utils/slam_backend.py:933-980) at every new
 * keyframe: cam_rot_delta / cam_trans_delta of the first `pose_window` window keyframes at HALF the tracking rates,
 * exposure_a / exposure_b of every window keyframe at 0.01, nothing for frame 0; after each mapping iteration's backward
 * it runs keyframe_optimizers.step() and update_pose(viewpoint) for those first views (:756-765).  Here: one wave per view,
 * the launch shape depends on V only.  state [V,80] and status [V,2] in olsr_pose_step's layout, projection_matrix shared.
 * params->step > 0 is one host-side count for all views; <= 0 uses each view's own status[v][1] + 1.  Per view v, flags[v]:
 *   POSE | EXPOSURE  the bits of olsr_pose_step_gated(params, dL_dtau_sum + 6 v, dL_dexposure + 2 v, projection_matrix,
 *                    state + 80 v, status + 2 v, frame_status ? frame_status + 2 v : NULL)
 *   POSE             the same call with dL_dexposure == NULL
 *   EXPOSURE         (a window keyframe beyond pose_window) only words 70..75 change, by the same Adam arithmetic; words
 *                    0..15 and 52..69 keep their bits; the matrices are re-derived; status[v][0] = 0, status[v][1] += 1
 *   0                (frame 0, rehearsal views) as dL_dtau_sum == NULL: only the re-derived matrices are written, no count
 * frame_status[2 v + 1] != 0 gates view v alone, as in the single call.  A view's flags must not change between resets of
 * its state and status: the step count is shared by its groups, so a group that joined late would run on the bias
 * corrections of the others' count (the reference builds a fresh optimiser instead: KeyframeWindow.rebuild).
 * OLSR_ERR_ARG before any launch: V outside 1 ... OLSR_WINDOW_MAX_VIEWS, unknown flag bits, NULL params, flags, state, status
 * or projection_matrix, a NULL gradient array that some flag needs. */
#define OLSR_WINDOW_MAX_VIEWS 32
#define OLSR_WINDOW_OPT_POSE 1
#define OLSR_WINDOW_OPT_EXPOSURE 2
int olsr_window_pose_step(const olsr_pose_params *params, int32_t V, const int32_t *flags /* host int32[V] */,
                          const float *dL_dtau_sum /* device [V,6] */, const float *dL_dexposure /* device [V,2] */,
                          const float *projection_matrix /* device [16], shared */, float *state /* device [V,80] */,
                          int32_t *status /* device [V,2] */, const int32_t *frame_status /* device [V,2] or NULL */,
                          void *hip_stream);

/* Adds one view's per-Gaussian gradients into the flat fp32 buffer
 *   flat[P][3 xyz | 3M sh | 1 opacity | 3 scale | 4 rotation | F language]
 * that a frame-sharded trainer all-reduces once per optimisation step, and updates the
 * densification statistics densify[P][2] += {||dL_dmeans2D.xy||, 1} for visible Gaussians and
 * max_radii[P] = max(max_radii, radii).  With assign != 0 the accumulators are overwritten
 * instead (first view of a step; saves zero-filling them).  No reference counterpart in native code: it is what
 * autograd's `.grad +=` over the views of BackEnd.map (utils/slam_backend.py:510-670) and
 * GaussianModel.add_densification_stats (gaussian_splatting/scene/gaussian_model.py:965-969) do
 * with separate PyTorch kernels. */
int olsr_accumulate_gradients(int32_t P, int32_t M, int32_t F, int32_t assign,
                              const float *dL_dmeans3D,
                              const float *dL_dsh, const float *dL_dopacity,
                              const float *dL_dscales, const float *dL_drotations,
                              const float *dL_dlanguage, const float *dL_dmeans2D,
                              const int32_t *radii, float *flat, float *densify,
                              int32_t *max_radii, void *hip_stream);

/* ---- the capacity-bound sparse exchange of the bucket (SURVEY.md section 8, rows e and f2) ---------------------------
 * Saturation leaves ~2 % of a view's Gaussians with a gradient row (config 3: 9 471 of 500 000), so a frame-sharded
 * step exchanges the UNION of the ranks' non-zero rows instead of the whole bucket — without a host synchronisation,
 * so that several frames stay in flight.  The caller issues two collectives (RCCL through torch.distributed, or any
 * other all-reduce) and these three calls around them, all on one stream:
 *   olsr_sparse_exchange_mask    imax[0..P) = 1 where row g of `flat` holds a non-zero element (only rows whose bit
 *                                of row_mask is set are looked at; row_mask may be NULL = look at every row),
 *                                imax[P..2P) = max_radii
 *   -- all-reduce MAX over imax (int32[2P]): the union of the rows, and the reduced radii --
 *   olsr_sparse_exchange_pack    max_radii <- imax[P..2P); row_mask (if given) <- the union; the union's rows, in
 *                                ascending row order, are copied into fsum[slot][width] for slot < capacity, unused
 *                                slots are zero-filled, idx[slot] = the row (P for an unused slot);
 *                                fsum[capacity * width ..) <- densify[P][2]; status_dev = {rows in the union,
 *                                1 if they did not fit};  scratch: olsr_sparse_exchange_scratch_ints(P) int32.
 *                                With idx == fsum == NULL nothing is packed: the call only counts (status_dev, max_radii
 *                                and row_mask as above) — for a caller that reads the count back and sizes the packed
 *                                buffer exactly (FrameShardedStep's "sparse" exchange, one host synchronisation per step)
 *   -- all-reduce SUM over fsum (fp32[capacity * width + 2P]) --
 *   olsr_sparse_exchange_unpack  flat[idx[slot]] <- fsum[slot], densify <- the tail
 * The bucket then holds what a dense all-reduce of {flat, densify} (SUM) and max_radii (MAX) would have left, bit for
 * bit, provided the union fitted; on overflow only the first `capacity` rows of the union were exchanged and the
 * caller must repeat the step with a larger capacity or densely (the contract of an instance overflow).  `width` is
 * the bucket's row width 11 + 3M + F.  No reference counterpart: the reference is single-GPU and autograd's `.grad`
 * accumulates the views of BackEnd.map (utils/slam_backend.py:510-670) in one process. */
int olsr_sparse_exchange_mask(int32_t P, int32_t width, const float *flat, const uint64_t *row_mask,
                              const int32_t *max_radii, int32_t *imax, void *hip_stream);
int64_t olsr_sparse_exchange_scratch_ints(int32_t P);
int olsr_sparse_exchange_pack(int32_t P, int32_t width, int32_t capacity, const float *flat, const int32_t *imax,
                              int32_t *max_radii, uint64_t *row_mask, const float *densify, int32_t *idx,
                              float *fsum, int32_t *scratch, int32_t *status_dev, void *hip_stream);
int olsr_sparse_exchange_unpack(int32_t P, int32_t width, int32_t capacity, const int32_t *idx, const float *fsum,
                                float *flat, float *densify, void *hip_stream);

/* Near-plane visibility test.  Replaces markVisible / checkFrustum
 * (DGR/rasterize_points.cu:457-476; CR/rasterizer_impl.cu:54-66,141-153).
 * present[P] is one byte per Gaussian (bool). */
int olsr_mark_visible(int32_t P, const float *means3D, const float *viewmatrix,
                      const float *projmatrix, uint8_t *present, void *hip_stream);

/* Introspection of the opaque state for stage-by-stage parity tests and for the
 * benchmark's byte model.  Each returns a device pointer inside the given buffer
 * (or NULL for an unknown name).  Names: geometry — "depths" f32[P], "means2D"
 * f32[P,2], "cov3D" f32[P,6], "conic_opacity" f32[P,4], "rgb" f32[P,3], "clamped"
 * u8[P,3], "tiles_touched" u32[P], "depth_order" u32[P]; binning — "src" u32[R]
 * (sorted position -> emission index), "inst_gid" u32[R] (emission index -> Gaussian id; the
 * reference's point_list is inst_gid[src]), "flags" u8[R], "rowbase" u32[R+1], "row_sync" u32[2] (ticket and done-counter of the
 * row compaction, zero between kernels); image — "final_T" f32[H*W], "n_contrib" u32[H*W], "ranges" u32[tiles,2]. */
const void *olsr_geometry_field(const void *geometry_buffer, int32_t P, int32_t F, const char *name);
const void *olsr_binning_field(const void *binning_buffer, int64_t num_rendered, int32_t F,
                               const char *name);
const void *olsr_image_field(const void *image_buffer, int32_t width, int32_t height, int32_t tile,
                             const char *name);

/* Per-stage HIP-event timing (events recorded on the stream the kernels run on).
 * olsr_set_profiling(1) clears the log and starts recording one event per stage of every
 * forward/backward issued by this thread (no synchronisation is added);
 * olsr_get_stage_times waits for the last event and returns, in issue order, one
 * (stage name, milliseconds) entry per stage executed since then (up to `max`). */
void olsr_set_profiling(int enable);
int olsr_get_stage_times(const char **names, float *ms, int max);

/* Debug aid (kernel tuning): while a device buffer of max_launches * max_blocks * 8 uint64 is set, every block of the
 * next radix-sort passes issued by this thread records the shader clock at its phase boundaries ({ticket, keys
 * counted, counts published, ranked, predecessors summed, written}; index (launch * max_blocks + block) * 8 + phase).
 * NULL switches it off. */
void olsr_debug_sort_timing(unsigned long long *device_buffer, int max_blocks, int max_launches);

/* Host logic of the radix passes, exposed for tests: the keys-per-thread and the number of 1024-thread blocks a sort of
 * n keys is launched with (n_is_capacity != 0: n bounds a count only known on the device, see olsr_forward_async), and
 * whether n is sorted by the one-kernel passes at all (return value: 1) or by the multi-kernel fallback (0). */
int olsr_debug_sort_plan(int64_t n, int n_is_capacity, int32_t *keys_per_thread, int32_t *blocks);

/* Test hook for the synchronisation-error path (OLSR_STATUS_SYNC_ERROR), process-wide.  fault_bits: bit 0 / bit 1 = in every
 * later forward the block holding ticket 0 of the first depth-sort / tile-sort pass never publishes its digit counts, which is
 * what its successors see when a status word is lost; spin_limit: polls a look-back makes before it gives up (0 restores the
 * default, 2^22 — seconds; tests use a few thousand).  A negative argument leaves that knob as it is. */
void olsr_debug_sync_fault(int fault_bits, int spin_limit);

/* The drop-in olsr_backward's guess (scratch_alloc != NULL), process-wide: sets the ratio of rows per instance it guesses
 * from when ratio >= 0 (packed_survivor_waves != 0: the reference mode of 15x15 tiles), stores in *redone_out (may be NULL)
 * how many guessed backwards had to be redone exactly so far, and returns the ratio in force. */
float olsr_debug_rows_ratio(int32_t packed_survivor_waves, float ratio, int32_t *redone_out);

/* Tuning / test knobs of the radix passes, process-wide.  keys_per_thread in {2, 4, 8, 12, 16} pins the instantiation (0:
 * chosen from the input size); resident_blocks > 0 replaces the 256 blocks a round is planned for; legacy != 0 forces the
 * multi-kernel passes at any size.  A negative argument leaves that knob as it is.  The library reads the environment
 * (OLSR_SORT_KPT, OLSR_SORT_RESIDENT, OLSR_SORT_LEGACY) ONCE, when it is loaded, to seed them; nothing on a call path
 * touches getenv.  Not for use while frames are in flight (a forward and its backward must see the same plan). */
void olsr_debug_sort_knobs(int keys_per_thread, int resident_blocks, int legacy);

/* The depth sort of at most 8 192 Gaussians is ONE launch of one workgroup (histogram, the frame's bookkeeping and the four
 * 8-bit passes inside the block; round 5) instead of a histogram launch and four radix passes with a ~10 us floor each; same
 * order bit for bit.  enable = 0 sends small frames through the pass kernels as well (tests compare the two), 1 restores the
 * default, negative leaves it.  Process-wide; seeded once from OLSR_SORT_SMALL.  A keys_per_thread pinned through
 * olsr_debug_sort_knobs also selects the pass kernels. */
void olsr_debug_sort_small(int enable);

/* Visible-set compaction of the depth sort (round 6): the sort orders only the Gaussians that emit instances — the histogram
 * kernel, which reads every key anyway, writes their (key, index) densely in index order and counts digits of those only; the
 * passes sort that many keys.  Same lists bit for bit.  enable = 0 sorts every Gaussian as rounds 1-5 did (tests compare the
 * two), 1 restores the default, negative leaves it.  Process-wide; seeded once from OLSR_SORT_COMPACT.  Not used with a carried
 * depth order (whose domain is every Gaussian), by the one-launch sort of <= 8 192 Gaussians, nor beyond 2 M Gaussians. */
void olsr_debug_sort_compact(int enable);

/* Diagnostic: while a device buffer of 2 x capacity uint64 is set, every forward / backward composite launch of this process
 * is bracketed by two one-thread kernels on its stream that write {device wall clock (100 MHz), stream << 8 | kind} — kind 0 / 1:
 * in front of / behind the forward composite (+ its tile-order kernel), 2 / 3: the backward composite — into consecutive
 * entries.  Reads the overlap of several frames in flight without a profiler (scripts/probe/composite_overlap.py).  The stamps
 * cost four tiny launches per frame.  NULL switches it off. */
void olsr_debug_composite_stamps(unsigned long long *device_buffer, int capacity);

/* Test instrument (round 6; never on a product path): the composite backward — CR/backward.cu:932-1201 (language_render_cuda),
 * 706-930 (renderCUDA), 684-702 (render_cuda_reduce_sum) — restated on the GPU in the reference's OWN association: its per-lane
 * state and expressions in source order, the 225-lane integer-halving tree through shared memory in the tree's own pairing
 * (OLSR_BWD_REFERENCE; lane order in double for OLSR_BWD_EXACT, like the oracle), one row per instance the tile does not skip,
 * a Gaussian's rows added one after the other in sorted-list order.  It runs on the state buffers a forward left (either
 * entry; num_rendered as for olsr_backward) and writes the composite-level gradients only: dL_dmeans2D [P,3], dL_dconic [P,4],
 * dL_dopacity [P], dL_dcolors [P,3], dL_dlanguage [P,F], dL_ddepths [P].  These EQUAL the CPU oracle's bit for bit
 * (tests/test_gpu_bwd_ordered.py); the product's fast kernel, which re-associates the same sums, is compared with this one on the
 * GPU at sizes the oracle needs minutes for.  scene->bwd_mode and tile select the variant; a NULL language / depth cotangent
 * counts as zeros.  scratch: olsr_debug_backward_ordered_scratch_bytes(num_rendered, F) bytes.  Tens of milliseconds per frame.
 * condition != 0: the outputs are not the gradients but their CONDITION A — the same sums with every product replaced by the
 * product of magnitudes and every difference by the sum of magnitudes.  To first order any re-association of the sums and
 * any few-ulp variation of the value path moves an element by at most K x 2^-24 x A, K of the order of the operations a term
 * went through; the tests hold the fast kernel to that, element by element ("it differs by rounding only"). */
size_t olsr_debug_backward_ordered_scratch_bytes(int64_t num_rendered, int32_t F);
int olsr_debug_backward_ordered(const olsr_scene *scene, const void *geometry_buffer, int32_t num_rendered,
                                const void *binning_buffer, const void *image_buffer,
                                const float *dL_dout_color, const float *dL_dout_language, const float *dL_dout_depth,
                                void *scratch,
                                float *dL_dmeans2D, float *dL_dconic, float *dL_dopacity, float *dL_dcolors,
                                float *dL_dlanguage, float *dL_ddepths, int32_t condition, void *hip_stream);

/* Test / experiment knob: threads per workgroup of the radix passes and their histogram kernels.  0 (default): the call
 * decides — 1024, or 256 for a scene that carries OLSR_FLAG_FRAMES_IN_FLIGHT; 256 / 1024: forced for every later forward.
 * Any other argument only reads the value back.  Same lists bit for bit.  Process-wide; seeded once from OLSR_SORT_THREADS.
 * Returns the value in force. */
int olsr_debug_sort_threads(int threads);

/* Test hook: the carve log.  While it is on for the calling thread, every sub-array that a sizing function or an entry
 * carves out of a state or scratch buffer is recorded as (base rounded up to 256 bytes, or 0 for a sizing carve; offset
 * from that base; bytes).  olsr_debug_carve_log(enable) clears the log and switches it on (!= 0) or off (0);
 * olsr_debug_carve_log_read copies up to `max` records to `out` (may be NULL) and returns how many the log holds.  Off
 * (the default) it costs one branch per sub-array and allocates nothing. */
void olsr_debug_carve_log(int enable);
int olsr_debug_carve_log_read(uint64_t *out /* [3 * max] */, int max);

/* Test hook, host only: the 32-bit words the carve of the geometry state (binning == 0, n Gaussians) or of the binning state
 * (binning != 0, n instances) leaves for the status rows of the one-kernel radix passes, behind the tickets, the digit totals
 * and the look-back words of its synchronisation area.  0 for n < 0. */
int64_t olsr_debug_sort_status_room(int64_t n, int binning);

/* Test instrument: the composites' exp (csrc/olsr_device.h, pinned_expf and its packed form) against the sequence it replaced
 * (pinned_expf_ref), bit for bit, on the GPU.  For each of the `count` float32 bit patterns from first_bits on (first_bits +
 * count <= 2^32) it evaluates both forms scalar, packed with the pattern in lane x and ANOTHER pattern of the range in lane y,
 * and packed with the lanes swapped; both lanes of a packed result are compared.  out (host memory): [0] / [1] / [2] the number
 * of patterns whose scalar / packed / swapped results differ, [3] the lowest differing pattern, or ~0 if there is none.
 * Synchronous, on the null stream. */
int olsr_debug_exp_sweep(uint32_t first_bits, uint64_t count, uint64_t out[4]);

/* Test instrument (never on a product path): the activations the preprocess kernels apply to raw parameters (OLSR_ACT_*),
 * evaluated by the device functions those kernels call (csrc/olsr_device.h: act_sigmoid, expf, act_normalize4), one thread per
 * Gaussian.  For each (raw, out) pair — opacities [P], scales [P,3], rotations [P,4], device memory — an array whose bit is set
 * in `activations` gets sigmoid / exp / normalize, an array whose bit is clear is copied; a pair with a NULL end is skipped.
 * With these values as an activations = 0 scene, every other step of the raw-parameter path can be held to an equality
 * (tests/test_gpu_activations.py).  OLSR_ERR_ARG: P < 0, bits outside OLSR_ACT_*.  Asynchronous on hip_stream. */
int olsr_debug_activate(int32_t P, int32_t activations, const float *opacities_raw, const float *scales_raw,
                        const float *rotations_raw, float *opacities_out, float *scales_out, float *rotations_out,
                        void *hip_stream);

const char *olsr_last_error(void);
const char *olsr_version(void);

#ifdef __cplusplus
}
#endif
#endif /* OLSR_H_INCLUDED */

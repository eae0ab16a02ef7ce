/* olsr_clip_trunk.h — the CLIP ConvNeXt image tower: an RGB frame in, the three maps olsr_hr_net_forward reads out.
 *
 * Restates, forward only, eval(), float32, what the reference reaches through sed_model.py:154-197 and
 * open_clip/timm_model.py:125-146 (forward(x, dense=True)), with d = dims, R = resolution:
 *   x      = ((image * 255) - mean[c]) / std[c]                                  utils/slam_backend.py:538-541, sed_model.py:158
 *   x      = F.interpolate(x, size=(R, R), mode="bilinear", align_corners=False)   normalised first, resized second
 *   stem   : Conv2d(3, d0, 4, stride 4, bias), LayerNorm over channels per pixel
 *   stage i: (i > 0) LayerNorm over channels, Conv2d(d[i-1], d[i], 2, stride 2, bias); then depths[i] blocks
 *   block  : y = x + gamma * fc2(GELU(fc1(LN(dwconv7x7(x)))))                     modeling/transformer/convnext.py:52-88
 *            depthwise 7x7 with padding 3 and a bias, LN over channels, fc1 C -> 4C, fc2 4C -> C, gamma [C]
 *   head   : per pixel of stage 3, LayerNorm over d3, Linear(d3, E, bias=False)   (norm_pre and the pool are identities here)
 *   res2 = stage 0's output [d0,R/4,R/4], res3 = stage 1's output [d1,R/8,R/8], clip_vis_dense [E,R/32,R/32], channel-major.
 *
 * ARITHMETIC.  Everything is float32 but LayerNorm's statistics.  A dense layer's output is a running sum that starts from the
 * bias (the head: from 0); to it the partial sum of each 64 k in turn is added, and a partial sum is one fmaf chain from 0
 * that takes its k in blocks of 16, inside a block in the order k0 + 4 q + j for j = 0..3, q = 0..3
 * (v_mfma_f32_16x16x4_f32, csrc/olsr_dense.h); k of a 2x2 downsample is (2 ky + kx) Cin + c, k of the stem is
 * 16 c + 4 ky + kx.  The depthwise convolution is one fmaf chain from the bias over the taps ky, kx ascending; a padded tap
 * adds nothing.  LayerNorm: mean = sum(v) / C and var = sum((v - mean)^2) / C in double, each sum as 64 partial sums over the
 * channels c = lane (mod 64) ascending, combined by a fixed butterfly; then fmaf((float)((v - mean) / sqrt(var + eps)), w, b).
 * GELU is 0.5 x (1 + erf(x * 0.70710678118654752440f)) with the device library's erff.  The residual is x + (gamma * branch),
 * two roundings.  The bilinear sample is the restatement of k_hr_net.hip:
 * hy (hx p00 + lx p01) + ly (hx p10 + lx p11) on the normalised pixels.  No atomics, no split k: a pixel's result does not
 * depend on how a launch was tiled, the two block paths below give the same bits, and a call is bit-reproducible.
 *
 * LAUNCHES.  A block of C <= OLSR_CLIP_TRUNK_FUSED_MAX_C channels is two launches: depthwise + LayerNorm, then fc1 -> GELU ->
 * fc2 -> residual per 64-pixel tile with the hidden row passing through LDS 64 neurons at a time (the hidden map is never
 * stored).  A wider block is three: depthwise + LayerNorm, fc1 + GELU, fc2 + residual, each dense launch tiled over 64 pixels
 * x 64 neurons.  The call's launches, in order: stem convolution, stem LayerNorm, then per stage the downsample (i > 0) and
 * its blocks' launches, then the head.  Bit k of `launches` (bit k & 63 of word k >> 6) switches launch k on; all zero: every
 * launch.  olsr_clip_trunk_launches gives their number, at most OLSR_CLIP_TRUNK_MAX_LAUNCHES.
 *
 * PACKED PARAMETERS (float32, 16-byte aligned; every weight as the A operand reads it, [out][k] row-major):
 *   block(C), 8 C^2 + 58 C floats:
 *     dw_w [49][C] (conv_dw.weight [C,1,7,7] as [ky kx][c]) | dw_b [C] | ln_w [C] | ln_b [C] | fc1_w [4C][C] | fc1_b [4C] |
 *     fc2_w [C][4C] | fc2_b [C] | gamma [C]
 *   trunk:
 *     stem_w [d0][48] (stem.0.weight [d0,3,4,4] as it lies) | stem_b [d0] | stem_ln_w [d0] | stem_ln_b [d0] |
 *     per stage i: (i > 0: ds_ln_w [d(i-1)] | ds_ln_b [d(i-1)] | ds_w [d_i][4][d(i-1)] (downsample.1.weight [d_i,d(i-1),2,2] as
 *     [out][ky kx][in]) | ds_b [d_i]) | depths[i] x block(d_i) |
 *     head_ln_w [d3] | head_ln_b [d3] | proj [E][d3]
 *
 * WORKSPACE.  16-byte aligned.  Two maps of the largest stage (pixel-major) and the hidden map of the largest three-launch
 * stage: for the real model 4 x 192*192*192*4 bytes.  Stage 0's hidden map (4 of those alone) does not exist.
 *
 * Same library and conventions as olsr.h: device pointers, OLSR_OK or a negative code with olsr_last_error(), every argument
 * error is OLSR_ERR_ARG before anything touches the device, the calls enqueue on hip_stream, read nothing back and do not
 * synchronise.  OLSR_ERR_ARG: a NULL pointer; a dim that is no positive multiple of 64 or above 4096; embed_dim no positive
 * multiple of 16; R no positive multiple of 32 or above 4096; a depth < 1 or more launches than the mask holds; H, W, h or w
 * < 1 or a product above 2^31 - 1; a std that is 0 or not finite, a mean that is not finite; ln_eps not positive; a launch
 * bit beyond the last launch; packed parameters or workspace not 16-byte aligned, any map not 4-byte aligned; a workspace
 * smaller than its _workspace_bytes.
 *
 * OUT OF SCOPE: the text tower, SED's head, half precision, any backward, reading image files. */
#ifndef OLSR_CLIP_TRUNK_H_INCLUDED
#define OLSR_CLIP_TRUNK_H_INCLUDED

#include "olsr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OLSR_CLIP_TRUNK_FUSED_MAX_C 256
#define OLSR_CLIP_TRUNK_MAX_LAUNCHES 128
#define OLSR_CLIP_TRUNK_MAX_DIM 4096

typedef struct olsr_convnext_block_params {
  int32_t C, h, w;           /* channels (a multiple of 64), map size */
  int32_t _pad0;
  double ln_eps;             /* 1e-6 in the reference */
  uint64_t workspace_bytes;  /* what `workspace` holds */
} olsr_convnext_block_params;

/* 0 for sizes olsr_convnext_block refuses */
size_t olsr_convnext_block_workspace_bytes(int32_t C, int32_t h, int32_t w);
/* one block, out of place: x, y [C,h,w] channel-major and contiguous; block_params: block(C) above */
int olsr_convnext_block(const olsr_convnext_block_params *p, const float *x, const float *block_params, float *y,
                        void *workspace, void *hip_stream);

typedef struct olsr_clip_trunk_params {
  int32_t depths[4], dims[4];
  int32_t embed_dim;         /* E */
  int32_t H, W;              /* the image's size */
  int32_t R;                 /* the tower's resolution: the image is resized to R x R */
  float mean[3], std[3];     /* clip_pixel_mean, clip_pixel_std (on the 0 ... 255 scale) */
  int32_t _pad0, _pad1;
  double ln_eps;
  uint64_t launches[2];      /* see LAUNCHES */
  uint64_t workspace_bytes;  /* what `workspace` holds */
} olsr_clip_trunk_params;

/* 0 for a configuration olsr_clip_trunk_forward refuses (launches, ln_eps and workspace_bytes are not looked at) */
size_t olsr_clip_trunk_workspace_bytes(const olsr_clip_trunk_params *p);
size_t olsr_clip_trunk_packed_floats(const olsr_clip_trunk_params *p);
int32_t olsr_clip_trunk_launches(const olsr_clip_trunk_params *p);
/* image [3,H,W] in [0, 1], contiguous; res2 [d0,R/4,R/4], res3 [d1,R/8,R/8], clip_vis_dense [E,R/32,R/32], contiguous */
int olsr_clip_trunk_forward(const olsr_clip_trunk_params *p, const float *image, const float *packed_params, float *res2,
                            float *res3, float *clip_vis_dense, void *workspace, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* OLSR_CLIP_TRUNK_H_INCLUDED */

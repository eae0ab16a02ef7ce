/* olsr_single_stage.h — the single-stage language chain 768 -> 15 -> 768 (language.single_stage_ae: True).
 *
 * Seven of the reference's eight Replica configurations run without an online autoencoder: one general AutoencoderMLP
 * (language/autoencoder/model.py:15-62) goes straight to the 15-channel code and back,
 *   encoder  768 -> 384 -> 192 -> 96 -> 48 -> 24 -> 15      decoder  15 -> 24 -> 48 -> 96 -> 192 -> 384 -> 384 -> 768
 * (utils/slam_backend.py:117-119, eval/evaluate_langslam.py:358-367).  A keyframe's language target is
 * auto_model.encode(rows).T.view(15,192,192) with nothing trained online (utils/slam_backend.py:556-576 with :562 false), and
 * the 2-D evaluation decodes a rendered code map with model.decode(codes) alone (eval/evaluate_langslam.py:266-273).  The two
 * entries below are that chain's encode and stage A of its text query, one launch each; stage B of the query is
 * olsr_lang_query_relevancy (olsr.h), which reads similarities only.  olsr_lang_encoder_encode and olsr_lang_query_sims
 * (olsr.h) stay the two-stage chain's and keep rejecting these width lists.  Same library, same conventions as olsr.h: device
 * pointers, OLSR_OK or a negative code with olsr_last_error(), every argument error is OLSR_ERR_ARG before anything touches the
 * device, a call enqueues on hip_stream, reads nothing back and does not synchronise.  No atomics: both are bit-reproducible. */
#ifndef OLSR_SINGLE_STAGE_H_INCLUDED
#define OLSR_SINGLE_STAGE_H_INCLUDED

#include "olsr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the encoder 768 -> 15 (AutoencoderMLP.encode in eval(), model.py:52-56) -----------------------------------------------
 *   h1 = W0 x + b0;   h(k+1) = W(k) relu(bn(k)(h(k))) + b(k), k = 1..5;   codes = h6 / |h6|
 *   bn(h) = alpha h + beta per channel, alpha = weight / sqrt(running_var + bn_eps), beta = bias - running_mean alpha, both
 *   computed in double and rounded once, applied as one fmaf in the producing layer's epilogue (never folded into weights)
 * Arithmetic is float32.  768 -> 384 -> 192 -> 96 -> 48 run on v_mfma_f32_16x16x4_f32 (a fixed fmaf chain per output, the k
 * order of olsr_lang_encoder_encode's layers).  The tail scheme: 48 -> 24 and 24 -> 15, whose widths are no multiples of the
 * 16-wide matrix tile, run per pixel on the vector unit as fmaf chains that start from the bias and take k in ascending
 * order; that order is part of the result's bits.  ReLU is fmaxf(., 0) with a NaN kept (torch's ReLU: a NaN input row gives a
 * NaN code row and touches no other row), |h6|^2 is accumulated in double in channel order, codes = h6 / (float)sqrt of it,
 * and the norm has no epsilon: a row whose h6 is exactly zero gives NaN, as in the reference.  A pixel's result does not
 * depend on the other pixels of the call, and both input layouts give the same bits.
 *   widths          the layer widths, input first: {768, 384, 192, 96, 48, 24, 15}, n_widths = 7; any other list (the
 *                   two-stage {768, 512, 256, 128, 64, 32} included) is OLSR_ERR_ARG
 *   features768     device float, N >= 1 pixels.  OLSR_LANG_ENCODER_IN_CHANNELS: [768] planes of N pixels, plane_stride >= N
 *                   elements apart — a [1,768,h,w] tensor, or one item of a batch, read in place; no alignment is assumed and
 *                   nothing beyond pixel N - 1 of a plane is read.  OLSR_LANG_ENCODER_IN_ROWS: [N,768] (plane_stride unused)
 *   encoder_params  device float[396927], 16-byte aligned: AutoencoderMLP.encoder in state_dict order without
 *                   num_batches_tracked: encoder.0.weight [384,768], encoder.0.bias [384], encoder.1.{weight, bias,
 *                   running_mean, running_var} [384], encoder.3.weight [192,384], encoder.3.bias, encoder.4.*, encoder.6.*,
 *                   encoder.7.*, encoder.9.*, encoder.10.*, encoder.12.*, encoder.13.*, encoder.15.weight [15,24],
 *                   encoder.15.bias [15]
 *   codes           device float[15,N] (OLSR_LANG_AE_CODES_CHANNELS: low_dim.T.view(15,h,w), the language target
 *                   olsr_mapping_loss reads, without a transpose pass) or [N,15] (OLSR_LANG_AE_CODES_ROWS) */
#define OLSR_SS_ENCODER_PARAMS 396927 /* 393951 Linear + 2976 BatchNorm */
#define OLSR_SS_DECODER_PARAMS 542544
typedef struct olsr_ss_encoder_params {
  int32_t n_widths;
  int32_t widths[8];
  int32_t in_layout;     /* OLSR_LANG_ENCODER_IN_* */
  int32_t code_layout;   /* OLSR_LANG_AE_CODES_* */
  int64_t plane_stride;  /* elements between two channel planes (channel layout) */
  double bn_eps;         /* BatchNorm1d's eps: 1e-5 */
} olsr_ss_encoder_params;
int olsr_ss_encoder_encode(const olsr_ss_encoder_params *params, int32_t N, const float *features768,
                           const float *encoder_params, float *codes, void *hip_stream);

/* ---- stage A of the text query (eval/evaluate_langslam.py:266-273, AutoencoderMLP.decode, model.py:58-62) ------------------
 * The contract of olsr_lang_query_sims without online_params: codes -> model.decode (15 -> 24 -> 48 -> 96 -> 192 -> 384 ->
 * 384 -> 768, ReLU between layers, x / |x|) -> the products with the K phrase rows, in one launch that stores nothing wider
 * than K per pixel.  15 -> 24 -> 48 run per pixel on the vector unit as bias-first, k-ascending fmaf chains (decoder.0.weight
 * [24,15] has rows that are not 16-byte aligned), every later layer on v_mfma_f32_16x16x4_f32; |y|^2 is accumulated in double.
 * The NaN rule: ReLU keeps a NaN here, as torch's does, so a NaN code pixel gives NaN similarities for that pixel and for no
 * other.  (olsr_lang_query_sims' plain fmaxf turns a NaN activation into 0; it stays as it is.)
 *   params          olsr_lang_query_params with widths {15, 24, 48, 96, 192, 384, 384, 768}, n_widths = 8; every other list,
 *                   the two-stage {32, 192, 256, 384, 512, 768} included, is OLSR_ERR_ARG.  K, n_pos, n_labels, the sizes and
 *                   flags are checked as olsr_lang_query_sims checks them
 *   codes           device float[15,in_height,in_width], channel-major.  When (dec_width, dec_height) differs they are
 *                   resampled first, as F.interpolate(mode="bilinear", align_corners=False) (evaluate_langslam.py:270)
 *   decoder_params  device float[542544], 16-byte aligned: AutoencoderMLP.decoder in state_dict order (decoder.0.weight
 *                   [24,15], decoder.0.bias [24], decoder.2.weight [48,24], ... decoder.12.weight [768,384], decoder.12.bias)
 *   phrases         device float[K,768], unit rows, 16-byte aligned, 1 <= K <= 64
 *   sims            device float[K,dec_height,dec_width]: <decode(codes), phrase>
 * olsr_lang_query_relevancy takes these similarities as they are; it validates its width list against the two-stage chain,
 * so hand it a struct that carries that list. */
int olsr_ss_query_sims(const olsr_lang_query_params *params, const float *codes, const float *decoder_params,
                       const float *phrases, float *sims, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* OLSR_SINGLE_STAGE_H_INCLUDED */

/* olsr_frame_ingest.h — a frame's ingest: the RGB-D frame as the sensor (or the decoder) leaves it -> the float32 image and
 * depth every other entry consumes.
 *
 * Restates, on the device and in one launch, what the reference does per frame on the host before anything reaches the GPU
 * (ReplicaDataset.__getitem__ / TUMDataset.__getitem__, utils/dataset.py:316-350, and the depth conversion of
 * get_loss_tracking / add_new_keyframe):
 *   image = torch.from_numpy(image / 255.0).clamp(0.0, 1.0).permute(2, 0, 1).to(torch.float32)
 *   depth = torch.from_numpy(np.array(depth) / depth_scale).to(torch.float32)
 * i.e. with N = W H pixels, i = v W + u:
 *   image[c][i] = (float) min(max((double) rgb[3 i + c] / 255.0, 0.0), 1.0)          c = 0, 1, 2
 *   depth_out[i] = (float) ((double) depth[i] / depth_scale)
 * Both quotients are IEEE double divisions, narrowed to float32 once.  The 256 possible colour values are evaluated once per
 * workgroup by exactly that expression and looked up; the depth quotient is evaluated per pixel.  A float32 depth that is NaN
 * or infinite stays so.  For a float32 depth and a depth_scale that float32 holds exactly, the result equals numpy's float32
 * quotient (a double quotient narrowed to 24 bits rounds once: 53 >= 2 * 24 + 2).
 *
 * One launch, no atomics, no scratch, no host read: the same bits every run.  Every output element is written by an ordinary
 * vector store; four pixels per lane, as one 16-byte store per plane where the destination address is 16-byte aligned
 * (a contiguous torch tensor with plane_stride % 4 == 0 always is), four 4-byte stores otherwise.  Nothing outside
 * rgb[0, 3 N), depth[0, N), image[c plane_stride + [0, N)) and depth_out[0, N) is read or written, whatever the alignment of
 * the pointers: the 3-byte pixel stream may start at any byte address, depth at any multiple of its element size, the outputs
 * at any multiple of 4.
 *
 * OUT OF SCOPE: the undistortion branch of the datasets (cv2.remap of a distorted image ahead of these statements), image
 * decoding, and the monocular datasets' missing depth.
 *
 * Same library and conventions as olsr.h: device pointers, OLSR_OK or a negative code with olsr_last_error(), every argument
 * error is OLSR_ERR_ARG before anything touches the device, the call enqueues on hip_stream and does not synchronise.
 * OLSR_ERR_ARG: a NULL pointer; W or H <= 0; W H above 2^31 - 1; plane_stride < W H; an unknown depth_type; depth_scale not
 * finite or <= 0; depth not aligned to its element size; image or depth_out not aligned to 4 bytes. */
#ifndef OLSR_FRAME_INGEST_H_INCLUDED
#define OLSR_FRAME_INGEST_H_INCLUDED

#include "olsr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OLSR_INGEST_DEPTH_U16 0
#define OLSR_INGEST_DEPTH_F32 1
typedef struct olsr_frame_ingest_params {
  int32_t W, H;          /* image size */
  int32_t depth_type;    /* OLSR_INGEST_DEPTH_*: the element type of `depth` */
  int32_t _pad0;
  int64_t plane_stride;  /* floats between the three planes of `image`, >= W H */
  double depth_scale;    /* Dataset.Calibration.depth_scale, > 0 */
} olsr_frame_ingest_params;
int olsr_frame_ingest(const olsr_frame_ingest_params *p, const uint8_t *rgb /* [H,W,3] interleaved */,
                      const void *depth /* [H,W] uint16 or float */, float *image /* [3] planes of [H,W] */,
                      float *depth_out /* [H,W] */, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* OLSR_FRAME_INGEST_H_INCLUDED */

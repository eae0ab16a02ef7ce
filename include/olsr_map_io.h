/* olsr_map_io.h — the Gaussian map as the reference's point_cloud.ply record, packed and unpacked on the device.
 *
 * GaussianModel.save_ply (gaussian_splatting/scene/gaussian_model.py:478-563) makes seven device-to-host copies, one
 * np.concatenate and one Python tuple per row.  Here the record array [P, width] is packed on the device in the file's column
 * order and leaves it in one copy; load_ply's column lookup (:585-689) runs the other way in one launch.  Per row, float32:
 *   x y z | nx ny nz (zeros) | f_dc_0..2 | f_rest_0..3(M-1)-1 | f_language_0..F-1 | opacity | scale_0..2 | rot_0..3
 *   width = 14 + 3 M + F                                                  (M = 1, F = 15: 32 floats = 128 bytes)
 *   f_dc_c = shs[p, 0, c]      f_rest_{c (M - 1) + k} = shs[p, 1 + k, c]    (the reference's transpose(1, 2).flatten)
 * The parameters are the raw ones the map holds (opacity logit, log scale, unnormalised quaternion), as in the reference.
 * Both kernels only move 32-bit words: NaN payloads, -0, infinities and denormals survive.
 *
 * A workgroup takes OLSR_MAP_PLY_BLOCK_ROWS consecutive rows: each array's slice for the block and the block's span of `rows`
 * are contiguous, are read and written with 16-byte accesses where the address allows (a scalar head and tail where it does
 * not) and meet in LDS, where the f_rest transposition is an index.  64-bit element offsets throughout.  One launch, no
 * atomics, no scratch.
 *
 * Deviations from the reference, stated: (1) olsr_map_ply_unpack reads the language channels, which load_ply never does;
 * (2) the header text the Python layer writes (map_io.ply_header) is restated from the PLY format and plyfile's known output,
 * not recorded from a run of plyfile; (3) only all-float32 little-endian binary files are read.
 *
 * Same library and conventions as olsr.h: device pointers (except `col`), OLSR_OK or a negative code with olsr_last_error(),
 * every argument error is OLSR_ERR_ARG before anything touches the device, the call enqueues on hip_stream and does not
 * synchronise.  OLSR_ERR_ARG: a NULL pointer that is needed (src / dst / rows / col; means3D, shs, opacities, scales,
 * rotations and, F > 0, language of the map), or one not aligned to 4 bytes; P < 0; M outside 1 ... 16 or not a perfect
 * square; F outside 0 ... 32; n_cols < 1 or above OLSR_MAP_PLY_MAX_COLS; a col[j] >= n_cols or < -1; a col[j] = -1 on a
 * column that is neither a normal nor a language channel.  P = 0 succeeds and launches nothing. */
#ifndef OLSR_MAP_IO_H_INCLUDED
#define OLSR_MAP_IO_H_INCLUDED

#include "olsr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OLSR_MAP_PLY_MAX_M 16
#define OLSR_MAP_PLY_MAX_F 32
#define OLSR_MAP_PLY_MAX_WIDTH 94    /* 14 + 3 * 16 + 32 */
#define OLSR_MAP_PLY_BLOCK_ROWS 64   /* rows per workgroup: 64 * 94 floats = 23.5 KiB of LDS at the widest record */
#define OLSR_MAP_PLY_MAX_COLS 6016   /* float properties per vertex of a file: one row of it must fit the LDS image */

/* 14 + 3 M + F, or OLSR_ERR_ARG */
int olsr_map_ply_width(int32_t M, int32_t F);

/* rows[p, :] = the record of row p of src, p in [0, P).  Reads rows [0, P) of means3D, shs, opacities, scales, rotations and
 * (F > 0) language; writes exactly P * width floats. */
int olsr_map_ply_pack(int32_t P, int32_t M, int32_t F, const olsr_map_buffers *src, float *rows /* [P, width] */,
                      void *hip_stream);

/* The other way, from a file's body as it lies: rows [P, n_cols], col[j] = the file column that feeds record column j, -1 =
 * absent (allowed on the three normals, which are never stored and whose entries are ignored, and on a language channel, which
 * then is 0.0f).  `col` is HOST memory, [width]; it travels in the kernel's arguments.  Writes rows [0, P) of means3D, shs,
 * opacities, scales, rotations and (F > 0) language, and nothing else of dst. */
int olsr_map_ply_unpack(int32_t P, int32_t M, int32_t F, int32_t n_cols, const int32_t *col /* host, [width] */,
                        const float *rows /* device, [P, n_cols] */, const olsr_map_buffers *dst, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* OLSR_MAP_IO_H_INCLUDED */

// olsr_host.h — what the host sources of the C-ABI (olsr_api.hip, olsr_dropin.hip, olsr_entries.hip, olsr_diag.hip) share:
// the error channel, the checks around a launch, and the few functions one of them defines for another.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <string>

#include "../../include/olsr.h"
#include "olsr_kernels.h"
#include "olsr_state.h"

namespace olsr {

// sets olsr_last_error() of this thread and returns `code` (olsr_api.hip)
int fail(int code, const std::string& msg);

#define HIP_TRY(expr)                                                                          \
  do {                                                                                         \
    hipError_t _e = (expr);                                                                    \
    if (_e != hipSuccess)                                                                      \
      return fail(OLSR_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(_e));         \
  } while (0)

// (an int-returning step of the library: pass its error on)
#define OLSR_TRY(expr)                \
  do {                                \
    const int _rc = (expr);           \
    if (_rc != OLSR_OK) return _rc;   \
  } while (0)

// after a kernel launch: did the runtime accept it?
inline int launch_check(const char* what) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? OLSR_OK : fail(OLSR_ERR_DEVICE, std::string(what) + " launch: " + hipGetErrorString(e));
}

// a launch_* that makes a runtime call of its own ahead of its kernels (a memset, a function attribute) returns that
// call's error: the entry `who` reports it, or goes on to launch_check
inline int launch_failed(const char* who, hipError_t e) {
  return fail(OLSR_ERR_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
}
inline int launch_check(const char* who, hipError_t own) {
  return own == hipSuccess ? launch_check(who) : launch_failed(who, own);
}

// profiling marks and composite stamps (olsr_diag.hip); both do nothing unless a diagnostic entry switched them on
void mark(const char* name, hipStream_t st);
void stamp(hipStream_t st, int kind);

// CHECK_CUDA(A, debug), CR/auxiliary.h:166-173
inline int stage_check(const olsr_scene& s, const char* stage, hipStream_t st) {
  const int rc = launch_check(stage);
  if (rc != OLSR_OK || !s.debug) return rc;
  const hipError_t e = hipStreamSynchronize(st);
  return e == hipSuccess ? OLSR_OK : fail(OLSR_ERR_DEVICE, std::string(stage) + ": " + hipGetErrorString(e));
}
// the end of one stage of a forward / backward of `scene` on `stream`
#define STAGE(scene, name, stream)               \
  do {                                           \
    OLSR_TRY(stage_check(scene, name, stream));  \
    mark(name, stream);                          \
  } while (0)

inline bool supported_F(int F) { return F == 0 || F == 3 || F == 15 || F == 16 || F == 32; }

// tiles along one extent of the image, and of a w x h image (tile <= 0: the default, 15)
inline int tiles_along(int extent, int tile) { return (extent + tile - 1) / tile; }
inline size_t tile_count(int w, int h, int tile) {
  if (tile <= 0) tile = 15;
  return (size_t)tiles_along(w, tile) * (size_t)tiles_along(h, tile);
}

// ---- scratch layouts that two of the host sources share (each file's own are beside its kernels)
// the losses' partial sums, five floats for each of n blocks (stand-alone: loss_blocks) or tiles (fused into the forward)
inline float* loss_partials_carve(void* buf, size_t n, size_t& bytes) {
  Carver c(buf);
  float* partials = c.take<float>(5 * n);
  bytes = c.total();
  return partials;
}
// the ordered debug backward: one gradient row and one flag byte per instance
struct OrderedBwdScratch {
  float* rows;    // [R][grad_row(F)]
  uint8_t* used;  // [R]
  static OrderedBwdScratch carve(void* buf, size_t R, int grad_row_floats, size_t& bytes) {
    Carver c(buf);
    OrderedBwdScratch s;
    s.rows = c.take<float>(R * (size_t)grad_row_floats);
    s.used = c.take<uint8_t>(R);
    bytes = c.total();
    return s;
  }
};

// ---- host state of the synchronising (drop-in) entry, olsr_dropin.hip
// the instance count on the host: arm() before the depth sort's histogram kernel is launched, wait() after the sort
int pinned_count_arm(FusedHouse& house);
int pinned_count_wait(hipStream_t st, int32_t* count);
// a token for this forward and the mapped words its last kernel posts the gradient-row counts and a synchronisation error to
int rows_ring_post(hipStream_t st, ForwardTail& tail);
// a synchronisation error of an earlier frame on this device and stream: OLSR_ERR_DEVICE (and the flag cleared) if one is
// pending; the device view of that flag, for the backward's last kernel (nullptr before the first olsr_forward)
int sticky_sync_error_check(hipStream_t st);
int32_t* sticky_sync_error_dev(hipStream_t st);
// the hint buffer of (current device, st, ntiles); nullptr: run without a hint
uint32_t* order_hint_of(int ntiles, hipStream_t st);
// what the drop-in backward learns about a frame's gradient rows per instance ([1]: packed survivor waves)
extern std::atomic<float> g_rows_ratio[2];
extern std::atomic<int32_t> g_rows_redos;
// The drop-in backward (olsr_backward with scratch_alloc) waits for a posted count, or guesses, only when the bound would
// cost more scratch than this.
constexpr size_t ROWS_WAIT_BYTES = (size_t)64 << 20;

}  // namespace olsr

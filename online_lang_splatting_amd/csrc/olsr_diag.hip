// olsr_diag.hip — diagnostics and test hooks of the C-ABI: profiling marks, composite stamps, the radix passes' knobs and
// their seeding from the environment, the state buffers' fields by name, the olsr_debug_* setters and the activation hook.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <vector>

#include "olsr_device.h"
#include "olsr_host.h"

using namespace olsr;

namespace {

thread_local bool g_profiling = false;
struct StageMark {
  const char* name;
  hipEvent_t ev;
};
thread_local std::vector<StageMark> g_marks;

void marks_reset() {
  for (auto& m : g_marks) (void)hipEventDestroy(m.ev);
  g_marks.clear();
}

// Diagnostic (olsr_debug_composite_stamps): one-thread kernels in front of and behind every composite launch write the
// device's wall clock (100 MHz, common to all XCDs) into a caller's buffer — when did each composite become eligible, when had
// it finished, on which stream — so that the overlap of several frames in flight can be read without a profiler in the way.
struct StampState {
  unsigned long long* buf = nullptr;
  int capacity = 0;
  std::atomic<int> next{0};
} g_stamps;
__global__ void stamp_kernel(unsigned long long* slot, unsigned long long tag) {
  slot[0] = wall_clock64();
  slot[1] = tag;
}

// olsr_debug_exp_sweep: the composites' exp (pinned_expf / pinned_expf2) against the sequence it replaced, bit for bit, over
// a range of argument bit patterns.  acc = {scalar mismatches, packed mismatches with the pattern in lane x, packed mismatches
// with the pattern in lane y, first (lowest) mismatching pattern or ~0}.  The other lane holds ANOTHER pattern of the range
// (half the range further on, wrapping), so a scale that leaks from one lane to the other shows.
__global__ __launch_bounds__(256) void exp_sweep_kernel(u32 first, unsigned long long count, unsigned long long* acc) {
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
  const unsigned long long shift = (count + 1) / 2;
  unsigned long long bad_s = 0, bad_x = 0, bad_y = 0, first_bad = ~0ull;
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) {
    const u32 pat = first + (u32)i;
    unsigned long long j = i + shift;
    if (j >= count) j -= count;
    const u32 other = count > 1 ? first + (u32)j : (pat == 0xC1200000u ? 0xC1A00000u : 0xC1200000u);  // (one pattern: -10 / -20)
    const float a = bits2f(pat), b = bits2f(other);
    const u32 ra = f2bits(pinned_expf_ref(a)), rb = f2bits(pinned_expf_ref(b));
    const bool ms = f2bits(pinned_expf(a)) != ra;
    const v2f_ nx = pinned_expf2(v2f_{a, b}), ox = pinned_expf2_ref(v2f_{a, b});
    const bool mx = f2bits(nx.x) != f2bits(ox.x) || f2bits(nx.y) != f2bits(ox.y) || f2bits(nx.x) != ra || f2bits(nx.y) != rb;
    const v2f_ ny = pinned_expf2(v2f_{b, a}), oy = pinned_expf2_ref(v2f_{b, a});
    const bool my = f2bits(ny.x) != f2bits(oy.x) || f2bits(ny.y) != f2bits(oy.y) || f2bits(ny.x) != rb || f2bits(ny.y) != ra;
    bad_s += ms;
    bad_x += mx;
    bad_y += my;
    if ((ms || mx || my) && (unsigned long long)pat < first_bad) first_bad = pat;
  }
  if (bad_s) atomicAdd(acc + 0, bad_s);
  if (bad_x) atomicAdd(acc + 1, bad_x);
  if (bad_y) atomicAdd(acc + 2, bad_y);
  if (first_bad != ~0ull) atomicMin(acc + 3, first_bad);
}

// olsr_debug_activate: the activations the preprocess kernels fold in (OLSR_ACT_*), through the very device functions they
// call — act_sigmoid / expf / act_normalize4 of olsr_device.h —, a Gaussian per thread.  An array whose flag is off is copied.
__global__ __launch_bounds__(256) void debug_activate_kernel(int P, int act, const float* __restrict__ opacities_raw,
                                                             const float* __restrict__ scales_raw,
                                                             const float* __restrict__ rotations_raw,
                                                             float* __restrict__ opacities_out, float* __restrict__ scales_out,
                                                             float* __restrict__ rotations_out) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= P) return;
  const size_t idx = (size_t)r;
  if (opacities_raw) {
    const float x = opacities_raw[idx];
    opacities_out[idx] = (act & OLSR_ACT_OPACITY_SIGMOID) ? act_sigmoid(x) : x;
  }
  if (scales_raw) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float v = scales_raw[3 * idx + k];
      scales_out[3 * idx + k] = (act & OLSR_ACT_SCALE_EXP) ? expf(v) : v;
    }
  }
  if (rotations_raw) {
    float q4[4];
    if (act & OLSR_ACT_ROTATION_NORMALIZE) {
      act_normalize4(rotations_raw + 4 * idx, q4);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) q4[k] = rotations_raw[4 * idx + k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) rotations_out[4 * idx + k] = q4[k];
  }
}

}  // namespace

namespace olsr {

void mark(const char* name, hipStream_t st) {
  if (!g_profiling || g_marks.size() >= (1u << 16)) return;
  StageMark m{name, nullptr};
  if (hipEventCreate(&m.ev) != hipSuccess) return;
  (void)hipEventRecord(m.ev, st);
  g_marks.push_back(m);
}

void stamp(hipStream_t st, int kind) {
  if (!g_stamps.buf) return;
  const int i = g_stamps.next.fetch_add(1);
  if (i >= g_stamps.capacity) return;
  stamp_kernel<<<1, 1, 0, st>>>(g_stamps.buf + 2 * (size_t)i, ((unsigned long long)(uintptr_t)st << 8) | (unsigned)kind);
}

// The carve log (olsr_state.h): per thread, three words per Carver::take
thread_local bool g_carve_log_on = false;
namespace {
thread_local std::vector<uint64_t> g_carve_log;
constexpr size_t CARVE_LOG_MAX_WORDS = 3u << 16;
}  // namespace
void carve_log_append(const void* base, size_t offset, size_t bytes) {
  if (g_carve_log.size() >= CARVE_LOG_MAX_WORDS) return;
  g_carve_log.push_back((uint64_t)(uintptr_t)base);
  g_carve_log.push_back((uint64_t)offset);
  g_carve_log.push_back((uint64_t)bytes);
}

// The radix passes' knobs (olsr_state.h): seeded from the environment once, when the library is loaded
SortKnobs& sort_knobs() {
  static SortKnobs k;
  return k;
}

}  // namespace olsr

namespace {
struct SortKnobsFromEnv {
  SortKnobsFromEnv() {
    auto num = [](const char* name) {
      const char* e = std::getenv(name);
      return e ? std::atoi(e) : 0;
    };
    sort_knobs().kpt = num("OLSR_SORT_KPT");
    sort_knobs().resident = num("OLSR_SORT_RESIDENT");
    sort_knobs().legacy = num("OLSR_SORT_LEGACY") == 1 ? 1 : 0;
    if (std::getenv("OLSR_SORT_SMALL")) sort_knobs().small_sort = num("OLSR_SORT_SMALL") != 0 ? 1 : 0;
    if (std::getenv("OLSR_SORT_COMPACT")) sort_knobs().compact = num("OLSR_SORT_COMPACT") != 0 ? 1 : 0;
    if (num("OLSR_SORT_THREADS") == 1024 || num("OLSR_SORT_THREADS") == 256) sort_knobs().threads = num("OLSR_SORT_THREADS");
  }
} g_sort_knobs_from_env;
}  // namespace

extern "C" {

const void* olsr_geometry_field(const void* geometry_buffer, int32_t P, int32_t F, const char* name) {
  const GeometryState g = GeometryState::carve(const_cast<void*>(geometry_buffer), (size_t)P, grad_row(supported_F(F) ? F : 0));
  if (!std::strcmp(name, "depths")) return g.depths;
  if (!std::strcmp(name, "means2D")) return g.means2D;
  if (!std::strcmp(name, "cov3D")) return g.cov3D;
  if (!std::strcmp(name, "conic_opacity")) return g.conic_opacity;
  if (!std::strcmp(name, "rgb")) return g.rgb;
  if (!std::strcmp(name, "clamped")) return g.clamped;
  if (!std::strcmp(name, "tiles_touched")) return g.tiles_touched;
  if (!std::strcmp(name, "depth_order")) return g.depth_order;  // (the sort's own buffer: every Gaussian, compaction off)
  if (!std::strcmp(name, "depth_order_compacted")) return g.gacc;  // u32[counters[CNT_SORTED]]: the emitting Gaussians in depth order
  if (!std::strcmp(name, "counters")) return g.counters;
  if (!std::strcmp(name, "emit_totals")) return g.emit_status;
  if (!std::strcmp(name, "inst_start")) return g.inst_start;
  if (!std::strcmp(name, "blended")) return g.blended;  // u8[P]: some pixel blended the Gaussian in this frame's forward
  if (!std::strcmp(name, "carry_miss")) return g.carry_miss;  // u32: != 0 = this frame's carried depth order was not repairable
  if (!std::strcmp(name, "carry_totals")) return g.carry_totals;
  if (!std::strcmp(name, "sort_keys")) return g.key_a;  // u32[P] (valid after a forward whose carried order was repaired)
  return nullptr;
}

const void* olsr_binning_field(const void* binning_buffer, int64_t num_rendered, int32_t F, const char* name) {
  (void)F;
  const BinningState b = BinningState::carve(const_cast<void*>(binning_buffer), (size_t)num_rendered);
  if (!std::strcmp(name, "inst_gid")) return b.inst_gid;
  if (!std::strcmp(name, "flags")) return b.flags;
  if (!std::strcmp(name, "rowbase")) return b.rowbase;
  if (!std::strcmp(name, "row_sync")) return b.tickets + BT_ROWS;  // {ticket, finished blocks} of the row compaction
  if (!std::strcmp(name, "key_a")) return b.key_a;
  if (!std::strcmp(name, "key_b")) return b.key_b;
  if (!std::strcmp(name, "src")) return b.src;
  if (!std::strcmp(name, "val_b")) return b.val_b;
  return nullptr;
}

const void* olsr_image_field(const void* image_buffer, int32_t width, int32_t height, int32_t tile, const char* name) {
  const ImageState im =
      ImageState::carve(const_cast<void*>(image_buffer), (size_t)width * height, tile_count(width, height, tile));
  if (!std::strcmp(name, "final_T")) return im.final_T;
  if (!std::strcmp(name, "n_contrib")) return im.n_contrib;
  if (!std::strcmp(name, "ranges")) return im.ranges;
  if (!std::strcmp(name, "tile_work")) return im.tile_work;    // [2][tiles]
  if (!std::strcmp(name, "tile_order")) return im.tile_order;  // [tiles]
  return nullptr;
}

void olsr_set_profiling(int enable) {
  g_profiling = enable != 0;
  marks_reset();
}

int olsr_get_stage_times(const char** names, float* ms, int max) {
  if (g_marks.size() < 2) return 0;
  (void)hipEventSynchronize(g_marks.back().ev);
  int n = 0;
  for (size_t i = 1; i < g_marks.size() && n < max; ++i) {
    if (!std::strcmp(g_marks[i].name, "begin")) continue;  // interval between two calls
    float t = 0.f;
    if (hipEventElapsedTime(&t, g_marks[i - 1].ev, g_marks[i].ev) != hipSuccess) t = -1.f;
    names[n] = g_marks[i].name;
    ms[n] = t;
    ++n;
  }
  return n;
}

void olsr_debug_carve_log(int enable) {
  g_carve_log_on = enable != 0;
  g_carve_log.clear();
  if (!g_carve_log_on) g_carve_log.shrink_to_fit();
}

int olsr_debug_carve_log_read(uint64_t* out, int max) {
  const int n = (int)(g_carve_log.size() / 3);
  for (int i = 0; out && i < n && i < max; ++i)
    for (int k = 0; k < 3; ++k) out[3 * i + k] = g_carve_log[3 * (size_t)i + k];
  return n;
}

int64_t olsr_debug_sort_status_room(int64_t n, int binning) {
  if (n < 0) return 0;
  // (a base that is never dereferenced: the carve only adds offsets to it)
  void* base = reinterpret_cast<void*>((uintptr_t)ALIGN);
  if (binning) {
    const BinningState b = BinningState::carve(base, (size_t)n);
    return (int64_t)((b.sync_words + b.sync_count) - b.tile_status);
  }
  const GeometryState g = GeometryState::carve(base, (size_t)n, grad_row(0));
  return (int64_t)((g.sync_words + g.sync_count) - g.sort_status);
}

void olsr_debug_sort_timing(unsigned long long* device_buffer, int max_blocks, int max_launches) {
  debug_set_sort_timing(device_buffer, max_blocks, max_launches);
}

void olsr_debug_sync_fault(int fault_bits, int spin_limit) {
  if (fault_bits >= 0) sort_knobs().fault = fault_bits & 3;
  if (spin_limit >= 0) sort_knobs().spin_limit = spin_limit > 0 ? spin_limit : (1 << 22);
}

void olsr_debug_sort_knobs(int keys_per_thread, int resident_blocks, int legacy) {
  if (keys_per_thread >= 0) sort_knobs().kpt = keys_per_thread;
  if (resident_blocks >= 0) sort_knobs().resident = resident_blocks;
  if (legacy >= 0) sort_knobs().legacy = legacy ? 1 : 0;
}

void olsr_debug_composite_stamps(unsigned long long* device_buffer, int capacity) {
  g_stamps.buf = device_buffer;
  g_stamps.capacity = device_buffer ? capacity : 0;
  g_stamps.next = 0;
}

int olsr_debug_sort_threads(int threads) {
  if (threads == 0 || threads == 256 || threads == 1024) sort_knobs().threads = threads;
  return sort_knobs().threads.load();
}

void olsr_debug_sort_compact(int enable) {
  if (enable >= 0) sort_knobs().compact.store(enable ? 1 : 0, std::memory_order_relaxed);
}

void olsr_debug_sort_small(int enable) {
  if (enable >= 0) sort_knobs().small_sort = enable ? 1 : 0;
}

int olsr_debug_sort_plan(int64_t n, int n_is_capacity, int32_t* keys_per_thread, int32_t* blocks) {
  const SortPlan p = sort_plan((long long)n, n_is_capacity != 0);
  if (keys_per_thread) *keys_per_thread = p.kpt;
  if (blocks) *blocks = p.nblk;
  return fused_sort_applicable(n, 32) ? 1 : 0;
}

int olsr_debug_exp_sweep(uint32_t first_bits, uint64_t count, uint64_t* out) {
  if (out == nullptr || count > (1ull << 32) || (unsigned long long)first_bits + count > (1ull << 32)) return OLSR_ERR_ARG;
  unsigned long long host[4] = {0ull, 0ull, 0ull, ~0ull};
  unsigned long long* dev = nullptr;
  if (hipMalloc(&dev, sizeof(host)) != hipSuccess) return OLSR_ERR_ALLOC;
  bool ok = hipMemcpy(dev, host, sizeof(host), hipMemcpyHostToDevice) == hipSuccess;
  if (ok && count > 0) {
    const unsigned long long want = (count + 255) / 256;
    exp_sweep_kernel<<<(unsigned)(want < 16384 ? want : 16384), 256>>>(first_bits, count, dev);
    ok = hipGetLastError() == hipSuccess;
  }
  ok = ok && hipMemcpy(host, dev, sizeof(host), hipMemcpyDeviceToHost) == hipSuccess;
  (void)hipFree(dev);
  if (!ok) return OLSR_ERR_DEVICE;
  for (int i = 0; i < 4; ++i) out[i] = host[i];
  return OLSR_OK;
}

int olsr_debug_activate(int32_t P, int32_t activations, const float* opacities_raw, const float* scales_raw,
                        const float* rotations_raw, float* opacities_out, float* scales_out, float* rotations_out,
                        void* hip_stream) {
  if (P < 0) return fail(OLSR_ERR_ARG, "debug_activate: P must be >= 0");
  if (activations & ~(OLSR_ACT_OPACITY_SIGMOID | OLSR_ACT_SCALE_EXP | OLSR_ACT_ROTATION_NORMALIZE))
    return fail(OLSR_ERR_ARG, "debug_activate: activations holds unknown OLSR_ACT_* bits");
  // a pair of which either end is NULL is skipped
  const bool op = opacities_raw && opacities_out, sc = scales_raw && scales_out, rot = rotations_raw && rotations_out;
  if (P == 0 || !(op || sc || rot)) return OLSR_OK;
  debug_activate_kernel<<<(unsigned)(((int64_t)P + 255) / 256), 256, 0, (hipStream_t)hip_stream>>>(
      P, activations, op ? opacities_raw : nullptr, sc ? scales_raw : nullptr, rot ? rotations_raw : nullptr, opacities_out,
      scales_out, rotations_out);
  return launch_check("debug_activate");
}

size_t olsr_debug_backward_ordered_scratch_bytes(int64_t num_rendered, int32_t F) {
  if (num_rendered < 0 || !supported_F(F)) return 0;
  size_t bytes = 0;
  OrderedBwdScratch::carve(nullptr, (size_t)num_rendered, grad_row(F), bytes);
  return bytes;
}

}  // extern "C"

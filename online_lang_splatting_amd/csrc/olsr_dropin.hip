// olsr_dropin.hip — host-side state of the synchronising, reference-shaped entry (olsr_forward, and the olsr_backward that
// allocates its scratch through a callback): the instance count and the gradient-row counts the GPU posts into mapped host
// memory, the sticky synchronisation-error flags, the per-view tile-order hints and the rows-per-instance estimate.
// The sync-free entries use none of it.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "olsr_host.h"

using namespace olsr;

namespace {

// The drop-in (synchronising) entry needs the instance count on the host (the reference's blocking D2H,
// CR/rasterizer_impl.cu:454-455).  No copy, no event: block 0 of the histogram kernel stores the count and then a
// sequence number into two words of mapped, coherent host memory with system-scope stores ("the data is the flag"),
// and the host polls the second word — while the GPU goes straight on to the depth sort.  (A hipMemcpyAsync in the
// stream cost a 4 us copy kernel and a 6 us bubble in front of the first radix pass.)
// (the two words live until the process ends: a thread_local destructor could run after the HIP runtime's teardown)
struct PinnedCount {
  int32_t* p = nullptr;   // host view: {count, sequence}
  int32_t* dp = nullptr;  // device view of the same two words
  int32_t seq = 0;
};
thread_local PinnedCount g_pinned;

// The drop-in backward sizes its row scratch from the frame's exact gradient-row count without a synchronisation: the
// forward's last kernel posts {rows (4 slots), rows (packed survivor waves), sequence} into one slot of a ring of mapped
// host words; the matching backward — which runs after the caller's loss, long after the forward finished — looks its
// token up (olsr_live_rows) and falls back to the bound when the slot is not there (yet, or any more).
constexpr int ROWS_RING = 256;
// A synchronisation error (olsr_state.h, CNT_SYNC_ERROR) is detected on the device after the call that caused it has returned.
// The sync-free entries report it through their status words; for the reference-shaped, synchronising API the last kernel of
// a forward / backward also raises a flag in mapped host memory, and the FIRST library call after the GPU got there fails
// with OLSR_ERR_DEVICE — the way an asynchronous HIP error surfaces.
// Round 6: the flag is keyed by (device, stream) — one of STICKY_SLOTS mapped host
// words behind the rows ring, handed out in first-come order under a mutex; a call looks at the word of ITS device and stream
// only, so the error of a frame issued on one stream no longer fails an unrelated call on another.  When more (device,
// stream) pairs than slots have been seen, the last slot is shared by the rest (attribution degrades to "one of those").
constexpr int STICKY_SLOTS = 64;
// the mapped host words of the drop-in entry: one allocation, made by the first olsr_forward of the process
struct DropInWords {
  int32_t rows[ROWS_RING][4];    // slot token % ROWS_RING: {rows (4 slots), rows (packed survivor waves), token, -}
  int32_t sticky[STICKY_SLOTS];  // sticky_slot_of(stream): != 0 = a frame on that (device, stream) had a synchronisation error
};
// (process-wide: PyTorch runs a backward on its autograd thread, not on the thread that called the forward)
struct RowsRing {
  std::atomic<DropInWords*> p{nullptr};  // host view
  DropInWords* dp = nullptr;             // device view
  std::atomic<int32_t> seq{0};
  std::mutex init;
};
RowsRing g_rows;
thread_local int32_t g_last_token = 0;  // token of the last olsr_forward of this thread (0: none)

struct StickyKeys {
  std::mutex m;
  int n = 0;
  int dev[STICKY_SLOTS];
  hipStream_t st[STICKY_SLOTS];
} g_sticky_keys;
int sticky_slot_of(hipStream_t st) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::lock_guard<std::mutex> lk(g_sticky_keys.m);
  for (int i = 0; i < g_sticky_keys.n; ++i)
    if (g_sticky_keys.dev[i] == dev && g_sticky_keys.st[i] == st) return i;
  if (g_sticky_keys.n < STICKY_SLOTS - 1) {
    g_sticky_keys.dev[g_sticky_keys.n] = dev;
    g_sticky_keys.st[g_sticky_keys.n] = st;
    return g_sticky_keys.n++;
  }
  return STICKY_SLOTS - 1;
}

// (per-view tile orders of the synchronising entry: described at order_hint_of below)
__global__ void hint_init_kernel(uint32_t* base, int ntiles) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t total = (size_t)HINT_HDR + (size_t)HINT_SLOTS * (size_t)ntiles;
  if (i >= total) return;
  if (i < 4 + HINT_SLOTS) base[i] = 0u;
  else if (i < HINT_HDR) base[i] = 0x7FC00000u;  // NaN: matches no view
  else base[i] = (uint32_t)((i - HINT_HDR) % (size_t)ntiles);
}
// (the slot is picked by block 0 of the depth sort's histogram kernel — hint_pick_wave, k_sort.hip: a launch of its own, one
//  wave, cost the synchronising entry 5 us per frame on its dependent chain)

// ---- launch-order hint of the synchronising entry ---------------------------------------------------------------
// olsr_forward keeps no caller-owned state between calls, but the forward composite finishes ~10 % sooner when a frame's
// heavy tiles are started first (tile_order_inout of olsr_forward_async).  The library therefore keeps, per (device,
// stream, tile count), the order measured on the previous frame issued on that stream.  Forwards on one stream execute in
// order, so the array is a complete permutation whenever a kernel reads it; no result depends on its content (a hint from
// another view of another scene is merely a worse guess).  A few KB each, at most 64 of them (least recently used evicted),
// allocated stream-ordered; the survivors live until the process ends.
// Several orders per (device, stream, tile count), one per VIEW the stream has rendered (round 4): the reference's mapping
// loop renders its window of keyframes one after the other on one stream (utils/slam_backend.py:510-670), so "the previous
// frame's order" belongs to another view — and a stale order costs the forward composite 25-35 % with one frame in flight
// (0.17 -> 0.23 ms at config 3, scripts/probe/arc_views.py).  A one-wave kernel in front of the composite compares the frame's
// view matrix with the HINT_SLOTS stored ones and names the nearest slot (within HINT_VIEW_TOL per entry), else recycles the
// least recently used one; the composite reads that slot's order, the tile-order kernel writes this frame's order back into
// it.  Buffer (32-bit words): [0] chosen slot, [1] use counter, [4, 4 + S) last use of every slot, then S x 16 floats (view
// matrices, NaN = empty), then S x ntiles orders (each a permutation at all times: iota initially).
struct OrderHints {
  struct Entry {
    int dev;
    hipStream_t st;
    int ntiles;
    uint32_t* buf;
  };
  std::mutex m;
  std::vector<Entry> v;
  // evicted buffers, never freed while anything may still use them: a thread that fetched the pointer a
  // moment before the eviction still launches kernels on it, and the evicted stream may have a forward in flight.  They are
  // handed to the next new key of the same (device, tile count) — any content is a legal hint (the header's slot index is
  // always 0..15, whoever wrote it last; orders that are no permutations are ignored entry by entry) — and only when more
  // than 64 of them wait is the oldest freed, after a synchronisation of its device.
  std::vector<Entry> spare;
} g_order_hints;

}  // namespace

namespace olsr {

// Gradient rows per instance of the frame whose count the drop-in backward verified last ([1]: packed survivor waves), and
// how often a guessed scratch size had to be followed by an exact second backward (olsr_debug_rows_ratio).
std::atomic<float> g_rows_ratio[2] = {{0.f}, {0.f}};
std::atomic<int32_t> g_rows_redos{0};

int pinned_count_arm(FusedHouse& house) {
  if (!g_pinned.p) {
    HIP_TRY(hipHostMalloc((void**)&g_pinned.p, 2 * sizeof(int32_t), hipHostMallocMapped | hipHostMallocCoherent));
    HIP_TRY(hipHostGetDevicePointer((void**)&g_pinned.dp, g_pinned.p, 0));
    g_pinned.p[0] = 0;
    g_pinned.p[1] = 0;
  }
  g_pinned.seq = (g_pinned.seq == 0x7FFFFFFF) ? 1 : g_pinned.seq + 1;
  house.host_mailbox = g_pinned.dp;
  house.host_seq = g_pinned.seq;
  return OLSR_OK;
}

// the reference's blocking D2H (CR/rasterizer_impl.cu:454-455) — but the count was ready before the depth sort,
// which keeps running while the host waits here and allocates
int pinned_count_wait(hipStream_t st, int32_t* count) {
  volatile int32_t* box = g_pinned.p;
  const auto t0 = std::chrono::steady_clock::now();
  for (uint32_t spin = 0; __atomic_load_n(&box[1], __ATOMIC_ACQUIRE) != g_pinned.seq; ++spin) {
    __builtin_ia32_pause();
    if ((spin & 0xFFFFu) == 0xFFFFu) {  // every ~65 k polls: did the stream die, or is this taking seconds?
      const hipError_t q = hipStreamQuery(st);
      if (q != hipSuccess && q != hipErrorNotReady) return fail(OLSR_ERR_DEVICE, hipGetErrorString(q));
      if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(20)) {
        // the frame's kernels are still enqueued and write into buffers the caller frees on error: drain first
        (void)hipStreamSynchronize(st);
        if (__atomic_load_n(&box[1], __ATOMIC_ACQUIRE) == g_pinned.seq) break;  // (it was only slow)
        return fail(OLSR_ERR_DEVICE, "the instance count never arrived from the device");
      }
    }
  }
  *count = box[0];
  if (*count < 0) return fail(OLSR_ERR_CAPACITY, "instance count exceeds 2^31-1");
  return OLSR_OK;
}

int rows_ring_post(hipStream_t st, ForwardTail& tail) {
  if (!g_rows.p.load(std::memory_order_acquire)) {
    std::lock_guard<std::mutex> lk(g_rows.init);
    if (!g_rows.p.load(std::memory_order_relaxed)) {
      DropInWords* hp = nullptr;
      HIP_TRY(hipHostMalloc((void**)&hp, sizeof(DropInWords), hipHostMallocMapped | hipHostMallocCoherent));
      HIP_TRY(hipHostGetDevicePointer((void**)&g_rows.dp, hp, 0));
      std::memset(hp, 0, sizeof(DropInWords));
      g_rows.p.store(hp, std::memory_order_release);
    }
  }
  int32_t tok = g_rows.seq.fetch_add(1) + 1;
  if (tok <= 0 || tok >= 0x7FFFFF00) {  // (wrap: tokens stay positive)
    g_rows.seq.store(1);
    tok = 1;
  }
  g_last_token = tok;
  tail.rows_dev = g_rows.dp->rows[tok % ROWS_RING];
  tail.rows_seq = tok;
  tail.sticky = &g_rows.dp->sticky[sticky_slot_of(st)];
  return OLSR_OK;
}

int sticky_sync_error_check(hipStream_t st) {
  DropInWords* w = g_rows.p.load(std::memory_order_acquire);
  if (!w || __atomic_exchange_n(&w->sticky[sticky_slot_of(st)], 0, __ATOMIC_ACQ_REL) == 0) return OLSR_OK;
  return fail(OLSR_ERR_DEVICE,
              "device-side synchronisation error in an earlier frame issued on this device and stream: a look-back of its radix "
              "sort / row compaction never received a predecessor's counts (state buffer corrupted mid-frame?); that frame's "
              "images are invalid and its gradients are zeros.  (Reported like an asynchronous HIP error, by the first "
              "reference-shaped call on the same device and stream after the GPU got there; callers that need the error "
              "attributed to a frame use the sync-free entries, whose status words are per frame.)");
}
int32_t* sticky_sync_error_dev(hipStream_t st) {
  return g_rows.p.load(std::memory_order_acquire) ? &g_rows.dp->sticky[sticky_slot_of(st)] : nullptr;
}

// the hint buffer of (current device, st, ntiles): header + HINT_SLOTS orders (layout above); nullptr: run without a hint
uint32_t* order_hint_of(int ntiles, hipStream_t st) {
  int dev = 0;
  if (ntiles <= 0 || hipGetDevice(&dev) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> lk(g_order_hints.m);
  auto& v = g_order_hints.v;
  for (size_t i = 0; i < v.size(); ++i)
    if (v[i].dev == dev && v[i].st == st && v[i].ntiles == ntiles) {
      const OrderHints::Entry e = v[i];  // most recently used last (LRU order)
      v.erase(v.begin() + (long)i);
      v.push_back(e);
      return e.buf;
    }
  auto& spare = g_order_hints.spare;
  if (v.size() >= 64) {
    // a caller that keeps creating streams / resolutions: the least recently used hint is retired to the spare list (see
    // above), not freed — its pointer may be in another thread's hands, its stream may still be writing it
    spare.push_back(v.front());
    v.erase(v.begin());
    if (spare.size() > 64) {
      const OrderHints::Entry old = spare.front();
      spare.erase(spare.begin());
      int cur = dev;
      (void)hipSetDevice(old.dev);
      (void)hipDeviceSynchronize();  // nothing that could still touch it is in flight after this (rare by construction)
      (void)hipFree(old.buf);
      (void)hipSetDevice(cur);
    }
  }
  const size_t words = (size_t)HINT_HDR + (size_t)HINT_SLOTS * (size_t)ntiles;
  uint32_t* buf = nullptr;
  for (size_t i = 0; i < spare.size() && !buf; ++i)
    if (spare[i].dev == dev && spare[i].ntiles == ntiles) {
      buf = spare[i].buf;
      spare.erase(spare.begin() + (long)i);
    }
  // stream-ordered allocation: no device synchronisation on the hot olsr_forward path the first time a key is seen
  if (!buf && hipMallocAsync((void**)&buf, sizeof(uint32_t) * words, st) != hipSuccess) {
    (void)hipGetLastError();
    if (hipMalloc((void**)&buf, sizeof(uint32_t) * words) != hipSuccess) {
      (void)hipGetLastError();
      return nullptr;
    }
  }
  hint_init_kernel<<<(unsigned)((words + 255) / 256), 256, 0, st>>>(buf, ntiles);
  v.push_back({dev, st, ntiles, buf});
  return buf;
}

}  // namespace olsr

extern "C" {

int32_t olsr_last_forward_token(void) { return g_last_token; }

int64_t olsr_live_rows(int32_t token, int32_t packed_survivor_waves) {
  DropInWords* w = g_rows.p.load(std::memory_order_acquire);
  if (token <= 0 || !w) return -1;
  const volatile int32_t* slot = w->rows[token % ROWS_RING];
  if (__atomic_load_n(&slot[2], __ATOMIC_ACQUIRE) != token) return -1;
  const int64_t v = (int64_t)(uint32_t)slot[packed_survivor_waves ? 1 : 0];
  return (__atomic_load_n(&slot[2], __ATOMIC_ACQUIRE) == token) ? v : -1;  // (not overwritten meanwhile)
}

int32_t olsr_live_rows_overwritten(int32_t token) {
  DropInWords* w = g_rows.p.load(std::memory_order_acquire);
  if (token <= 0 || !w) return 0;
  const int32_t seen = __atomic_load_n(&w->rows[token % ROWS_RING][2], __ATOMIC_ACQUIRE);
  return (seen > token && seen - token < (1 << 30)) ? 1 : 0;
}

int64_t olsr_live_rows_wait(int32_t token, int32_t packed_survivor_waves, int32_t timeout_us) {
  int64_t v = olsr_live_rows(token, packed_survivor_waves);
  DropInWords* w = g_rows.p.load(std::memory_order_acquire);
  if (v >= 0 || timeout_us <= 0 || token <= 0 || !w) return v;
  const volatile int32_t* slot = w->rows[token % ROWS_RING];
  const auto t0 = std::chrono::steady_clock::now();
  for (uint32_t spin = 0;; ++spin) {
    const int32_t seen = __atomic_load_n(&slot[2], __ATOMIC_ACQUIRE);
    if (seen == token) return olsr_live_rows(token, packed_survivor_waves);
    // tokens grow by one per forward (wrapping to 1 at INT32_MAX): a larger one in the slot means ours was overwritten
    if (seen > token && seen - token < (1 << 30)) return -1;
    __builtin_ia32_pause();
    if ((spin & 0xFFu) == 0xFFu &&
        std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(timeout_us))
      return -1;
  }
}

int64_t olsr_backward_rows(int32_t token, int32_t packed_survivor_waves, int64_t num_rendered, int32_t F) {
  static const int32_t wait_us = [] {
    const char* e = std::getenv("OLSR_ROWS_WAIT_US");
    return e ? std::atoi(e) : 5000;
  }();
  const int64_t bound = (num_rendered > 0 ? num_rendered : 0) * (packed_survivor_waves ? 2 : 4);
  int64_t v = olsr_live_rows(token, packed_survivor_waves);
  if (v < 0 && olsr_backward_scratch_bytes(bound, F) > ROWS_WAIT_BYTES)
    v = olsr_live_rows_wait(token, packed_survivor_waves, wait_us);
  return (v >= 0 && v <= bound) ? v : bound;
}

float olsr_debug_rows_ratio(int32_t packed_survivor_waves, float ratio, int32_t* redone_out) {
  std::atomic<float>& r = g_rows_ratio[packed_survivor_waves ? 1 : 0];
  if (ratio >= 0.f) r.store(ratio);
  if (redone_out) *redone_out = g_rows_redos.load();
  return r.load();
}

}  // extern "C"

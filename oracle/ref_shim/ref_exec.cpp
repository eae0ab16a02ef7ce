// ref_exec.cpp — the scheduler of the execution model declared in cuda_runtime.h.  TEST INFRASTRUCTURE ONLY.
//
// One OS thread.  The threads of a block are ucontext fibers; a fiber runs until it reaches a barrier or returns, then
// hands the processor to the next live fiber in ascending thread rank, cyclically.  Every live fiber has therefore
// reached barrier k before the first one leaves it, which is all a barrier promises; the interleaving between barriers
// (rank 0 first, each rank to its next barrier) is one of the schedules a GPU may choose, and it is always the same one.
// Blocks run one at a time in ascending linear index, so a launch's float atomics happen in one fixed order.
#include "cuda_runtime.h"

#include <sys/mman.h>
#include <ucontext.h>

#include <vector>

#if defined(__SANITIZE_ADDRESS__)
#include <sanitizer/common_interface_defs.h>
#define REF_ASAN 1
#else
#define REF_ASAN 0
#endif

namespace ref_exec {

uint3 thread_idx = {0, 0, 0}, block_idx = {0, 0, 0};
dim3 block_dim(1, 1, 1), grid_dim(1, 1, 1);

namespace {

constexpr size_t kStackBytes = 256 * 1024;

struct Fiber {
  ucontext_t ctx;
  char* stack = nullptr;
  bool live = false;
  unsigned count_calls = 0;  // how many block_sync_count calls this fiber has made in this block
};

std::vector<Fiber> fibers;
ucontext_t main_ctx;
int n_threads = 0, cur = -1;
const std::function<void()>* body = nullptr;
// block_sync_count: the running total of the call in progress and which call (per-fiber ordinal) it belongs to
int count_acc = 0;
unsigned count_gen = ~0u;

void set_thread(int t) {
  cur = t;
  thread_idx.x = (unsigned)t % block_dim.x;
  thread_idx.y = ((unsigned)t / block_dim.x) % block_dim.y;
  thread_idx.z = (unsigned)t / (block_dim.x * block_dim.y);
}

int next_live(int t) {
  for (int i = 1; i <= n_threads; ++i) {
    const int u = (t + i) % n_threads;
    if (fibers[u].live) return u;
  }
  return -1;
}

#if REF_ASAN
const void* main_stack_bottom = nullptr;
size_t main_stack_size = 0;
#endif

// Leave the running context for fiber `to` (to < 0: the launching context).  `from` < 0: called from the launcher;
// dying: the running fiber has returned from the kernel and is never resumed.
void switch_to(int from, int to, bool dying) {
  ucontext_t* src = from < 0 ? &main_ctx : &fibers[from].ctx;
  ucontext_t* dst = to < 0 ? &main_ctx : &fibers[to].ctx;
  if (to >= 0) set_thread(to);
#if REF_ASAN
  void* fake = nullptr;
  if (to < 0)
    __sanitizer_start_switch_fiber(dying ? nullptr : &fake, main_stack_bottom, main_stack_size);
  else
    __sanitizer_start_switch_fiber(dying ? nullptr : &fake, fibers[to].stack, kStackBytes);
#endif
  if (dying)
    setcontext(dst);
  else
    swapcontext(src, dst);
#if REF_ASAN
  // resumed: tell ASan we are back on this stack (when the launcher is left for the first time it learns its own bounds)
  const void* old_bottom = nullptr;
  size_t old_size = 0;
  __sanitizer_finish_switch_fiber(fake, &old_bottom, &old_size);
#endif
}

void fiber_entry() {
#if REF_ASAN
  {
    const void* old_bottom = nullptr;
    size_t old_size = 0;
    __sanitizer_finish_switch_fiber(nullptr, &old_bottom, &old_size);
    if (main_stack_bottom == nullptr) {  // the first fiber ever entered was entered from the launcher
      main_stack_bottom = old_bottom;
      main_stack_size = old_size;
    }
  }
#endif
  (*body)();
  const int me = cur;
  fibers[me].live = false;
  switch_to(me, next_live(me), true);
  std::abort();  // not reached
}

void run_block() {
  if ((int)fibers.size() < n_threads) fibers.resize(n_threads);
  for (int t = 0; t < n_threads; ++t) {
    Fiber& f = fibers[t];
    if (!f.stack) {
      void* p = mmap(nullptr, kStackBytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
      if (p == MAP_FAILED) std::abort();
      f.stack = (char*)p;
    }
    getcontext(&f.ctx);
    f.ctx.uc_stack.ss_sp = f.stack;
    f.ctx.uc_stack.ss_size = kStackBytes;
    f.ctx.uc_link = nullptr;
    makecontext(&f.ctx, fiber_entry, 0);
    f.live = true;
    f.count_calls = 0;
  }
  count_acc = 0;
  count_gen = ~0u;
  switch_to(-1, 0, false);  // comes back when the last live fiber has returned
  cur = -1;
}

}  // namespace

void block_sync() {
  const int me = cur;
  const int nx = next_live(me);
  if (nx == me) return;  // the only live thread of the block
  switch_to(me, nx, false);
}

int block_sync_count(int pred) {
  Fiber& f = fibers[cur];
  const unsigned call = f.count_calls++;
  if (count_gen != call) {  // the first thread to arrive at this call opens its total; every thread has read the last
    count_gen = call;       // call's total before the barrier that closed that call released this one
    count_acc = 0;
  }
  count_acc += pred != 0;
  block_sync();
  const int total = count_acc;
  block_sync();
  return total;
}

void run_grid(dim3 grid, dim3 block, const std::function<void()>& fn) {
  if (cur >= 0) std::abort();  // no launches from inside a kernel
  grid_dim = grid;
  block_dim = block;
  n_threads = (int)(block.x * block.y * block.z);
  body = &fn;
  if (n_threads <= 0) return;
  for (unsigned z = 0; z < grid.z; ++z)
    for (unsigned y = 0; y < grid.y; ++y)
      for (unsigned x = 0; x < grid.x; ++x) {
        block_idx = {x, y, z};
        run_block();
      }
  body = nullptr;
}

}  // namespace ref_exec

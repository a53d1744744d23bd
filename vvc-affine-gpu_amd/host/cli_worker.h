// cli_worker.h -- the `vame` CLI's GPU side: the owning handles, what main and
// the workers share, and the worker itself (cli_worker.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <condition_variable>
#include <cstdint>
#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/vame.h"
#include "cli_options.h"
#include "cli_plan.h"

namespace vame_cli {

// A HIP object that is released when its owner goes out of scope, on whichever
// path; move-only, filled through put() by the HIP call that creates it.
template <class T, hipError_t (*Release)(T)>
class Handle {
  T h_{};

 public:
  Handle() = default;
  Handle(Handle&& o) noexcept : h_(std::exchange(o.h_, T{})) {}
  Handle& operator=(Handle&& o) noexcept {
    std::swap(h_, o.h_);
    return *this;
  }
  ~Handle() {
    if (h_) (void)Release(h_);
  }
  operator T() const { return h_; }
  T* put() { return &h_; }
};
using Stream = Handle<hipStream_t, hipStreamDestroy>;
using Event = Handle<hipEvent_t, hipEventDestroy>;
using DeviceBlock = Handle<void*, hipFree>;
using PinnedBlock = Handle<void*, hipHostFree>;

struct Context {  // a vame_ctx, destroyed with its owner
  vame_ctx* ctx = nullptr;
  Context() = default;
  Context(const Context&) = delete;
  Context& operator=(const Context&) = delete;
  ~Context() {
    if (ctx) vame_destroy(ctx);
  }
};

struct Slab {
  PinnedBlock block;  // one POC's results (Layout)
  char* host() const { return (char*)(void*)block; }
  int owner = 0;  // the worker whose pool it returns to
  int poc = 0, nrefs = 0;
  float pred_ns[4] = {0, 0, 0, 0};  // per-launch mode kernel times
  float fused_ns = 0;
};

struct Shared {
  std::mutex mu;
  std::condition_variable cv;
  // one pool per worker: a worker running ahead of the in-order writer can only
  // exhaust its own slabs, never the ones the writer is waiting for
  std::vector<std::vector<Slab*>> pools;
  std::map<int, Slab*> done;
  std::string error;
  bool failed = false;
};

struct Job {
  int worker, device;
  std::vector<int> pocs;
  const Settings* set;
  const uint16_t* orig;   // host, POC p at frame p-1
  const uint16_t* recon;  // host, POC p at frame p
  const Layout* L;
  Shared* S;
};

double now_s();
bool trace_enabled();  // VAME_CLI_TRACE=1: the timeline on stderr (host and GPU)

// One device: runs its POCs in order on one stream, uploading each batch's
// frames on a second stream while the previous batch computes, and hands each
// POC's results (pinned host slab) to the writer.  On an error it records the
// first message in S (Shared::error), wakes everyone and returns; whichever
// way it returns, it has released everything it created.
void gpu_worker(Job J);

}  // namespace vame_cli

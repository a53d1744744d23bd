// cli_worker.cpp -- one worker of the `vame` CLI: a context, three streams and
// an uploader thread on one device (cli_worker.h).
//
// What the success path keeps fixed, because HIP maps a process's streams onto
// GPU_MAX_HW_QUEUES = 4 hardware queues in the order they are created and the
// measured fix of the gap between batches (profiles/r03_copy_prio_ab.txt)
// rests on that mapping: vame_create first (it creates the engine's side
// stream), then the compute, upload and download streams and nothing else up
// front; the copy streams with an explicit priority; per batch the calls of
// Worker::run in their order; two result slots.
#include "cli_worker.h"

#include <sys/time.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <thread>

namespace vame_cli {

double now_s() {
  struct timeval tv;
  gettimeofday(&tv, nullptr);
  return (double)tv.tv_sec + (double)tv.tv_usec / 1e6;
}

bool trace_enabled() { return getenv("VAME_CLI_TRACE") && atoi(getenv("VAME_CLI_TRACE")) != 0; }

namespace {

void fail(Shared* S, const std::string& msg) {
  std::lock_guard<std::mutex> g(S->mu);
  if (!S->failed) S->error = msg;
  S->failed = true;
  S->cv.notify_all();
}

// Both report through a Shared* S in scope and leave the calling step with
// false; the caller's owners release what exists so far.
#define GPU_CHECK(x, what)                                        \
  do {                                                            \
    hipError_t e_ = (x);                                          \
    if (e_ != hipSuccess) {                                       \
      fail(S, std::string(what) + ": " + hipGetErrorString(e_)); \
      return false;                                               \
    }                                                             \
  } while (0)
#define VAME_CHECK(x, what)                                                                 \
  do {                                                                                      \
    int rc_ = (x);                                                                          \
    if (rc_ != 0) {                                                                         \
      fail(S, std::string(what) + ": " + vame_strerror(rc_) + " " + vame_last_hip_error()); \
      return false;                                                                         \
    }                                                                                       \
  } while (0)

// Frames go up on their own stream from a thread of their own, batch by batch
// ahead of the kernels (copies from pageable host memory block the calling
// thread, so the launching thread never waits for them); batch b's kernels
// wait for issued[b] on the device.
struct Uploader {
  // inputs, set before start()
  int device = 0;
  hipStream_t stream = nullptr;
  size_t frame_samples = 0;
  const uint16_t* orig = nullptr;                    // host, POC p at frame p-1
  const uint16_t* recon = nullptr;                   // host, label l at frame l
  const std::map<int, uint16_t*>* dorig = nullptr;   // device, by POC
  const std::map<int, uint16_t*>* drecon = nullptr;  // device, by label
  const std::vector<std::vector<int>>* batches = nullptr;
  const std::vector<Event>* issued = nullptr;  // recorded once batch b's copies are enqueued
  Shared* S = nullptr;
  // progress
  std::mutex mu;
  std::condition_variable cv;
  size_t done = 0;  // batches whose uploads are issued and whose event is recorded
  bool failed = false;
  std::thread t;

  void start() {
    t = std::thread([this] { run(); });
  }
  void join() {
    if (t.joinable()) t.join();
  }
  // true once batch k's uploads are issued, false if they never will be
  bool wait(size_t k) {
    std::unique_lock<std::mutex> g(mu);
    cv.wait(g, [&] { return done > k || failed; });
    return done > k;
  }
  void run() {
    hipError_t e = hipSetDevice(device);
    std::set<const uint16_t*> uploaded;
    auto put = [&](uint16_t* dst, const uint16_t* src) {
      if (e == hipSuccess && uploaded.insert(dst).second)
        e = hipMemcpyAsync(dst, src, frame_samples * 2, hipMemcpyHostToDevice, stream);
    };
    for (size_t b = 0; b < batches->size() && e == hipSuccess; b++) {
      {
        std::lock_guard<std::mutex> g(S->mu);
        if (S->failed) break;
      }
      for (int p : (*batches)[b]) {
        put(dorig->at(p), orig + (size_t)(p - 1) * frame_samples);
        int refs[4];
        const int n = vame_ref_list(p, refs);
        for (int r = 0; r < n; r++) put(drecon->at(refs[r]), recon + (size_t)refs[r] * frame_samples);
      }
      if (e == hipSuccess) e = hipEventRecord((*issued)[b], stream);
      std::lock_guard<std::mutex> g(mu);
      if (e == hipSuccess) done = b + 1;
      cv.notify_all();
    }
    std::lock_guard<std::mutex> g(mu);
    failed = e != hipSuccess || done < batches->size();
    cv.notify_all();
  }
};

// The worker's timeline (printed under VAME_CLI_TRACE=1): host wall times and
// the events that bound the stream's start, its first and last kernel and,
// when tracing, every batch.
struct Trace {
  bool on = false;
  double w0 = 0, w1 = 0, w2 = 0, wFirst = 0;  // start; context made; allocations done; first launch issued
  double kernelSum = 0;                       // ms, fused batches
  int late = 0;                               // batches issued after the previous one had finished on the GPU
  Event tStart, tFirst, tLast;
  std::vector<Event> gs, ge;  // per-batch GPU boundaries, created only when tracing

  bool start(Shared* S, hipStream_t st, size_t nbatches) {
    GPU_CHECK(hipEventCreate(tStart.put()), "hipEventCreate");
    GPU_CHECK(hipEventCreate(tFirst.put()), "hipEventCreate");
    GPU_CHECK(hipEventCreate(tLast.put()), "hipEventCreate");
    GPU_CHECK(hipEventRecord(tStart, st), "hipEventRecord");
    gs.resize(nbatches);
    ge.resize(nbatches);
    w2 = now_s();
    return true;
  }
  // before batch k's calls; prev_computed: the previous batch's last event
  bool batch_begin(Shared* S, hipStream_t st, size_t k, hipEvent_t prev_computed) {
    if (on && k > 0 && hipEventQuery(prev_computed) == hipSuccess) late++;  // the GPU waited for this thread
    if (on) {
      GPU_CHECK(hipEventCreate(gs[k].put()), "hipEventCreate");
      GPU_CHECK(hipEventCreate(ge[k].put()), "hipEventCreate");
      GPU_CHECK(hipEventRecord(gs[k], st), "hipEventRecord");
    }
    if (k == 0) {
      GPU_CHECK(hipEventRecord(tFirst, st), "hipEventRecord");
      wFirst = now_s();
    }
    return true;
  }
  bool batch_end(Shared* S, hipStream_t st, size_t k) {
    if (on) GPU_CHECK(hipEventRecord(ge[k], st), "hipEventRecord");
    return true;
  }
  void report(int worker) const {
    float toFirst = 0, span = 0;
    (void)hipEventElapsedTime(&toFirst, tStart, tFirst);
    (void)hipEventElapsedTime(&span, tFirst, tLast);
    fprintf(stderr,
            "[trace] worker %d: host create %.1f ms, allocations %.1f ms, first launch issued at %.1f ms, "
            "results in at %.1f ms; GPU: stream start -> first launch %.1f ms, first launch -> last "
            "kernel %.1f ms, kernels %.1f ms (gaps %.1f ms)\n",
            worker, (w1 - w0) * 1e3, (w2 - w1) * 1e3, (wFirst - w0) * 1e3, (now_s() - w0) * 1e3, toFirst, span,
            kernelSum, span - kernelSum);
    fprintf(stderr, "[trace] worker %d: %d of %zu batches issued after the previous one had finished; gaps (ms):",
            worker, late, gs.size());
    for (size_t b = 1; b < gs.size(); b++) {
      float g = 0, len = 0;
      (void)hipEventElapsedTime(&g, ge[b - 1], gs[b]);
      (void)hipEventElapsedTime(&len, gs[b], ge[b]);
      fprintf(stderr, " %.2f/%.1f", g, len);
    }
    fprintf(stderr, "\n");
  }
};

// A worker's state.  Members are released in reverse order of declaration,
// after ~Worker has joined the uploader and drained the streams: events,
// device blocks, streams, then the context -- on every way out of run().
struct Worker {
  const Job& J;
  Shared* S;
  const Settings& set;
  const Layout& L;
  const size_t fsz;  // samples per frame
  const int B;       // POCs per batch slot
  const int predMask;

  Context ctx;
  Stream st, up, dn;  // compute; frame uploads; result downloads
  // frames: orig of each POC, recon of every label its rings hold, in two
  // blocks, uploaded per batch (Uploader); results: two batch slots of B POC
  // layouts each
  DeviceBlock origBlk, reconBlk, dres;
  std::map<int, uint16_t*> dorig, drecon;
  std::vector<std::vector<int>> batches;
  std::vector<Event> upEv;
  // two slots: batch k+1 is enqueued before the host waits for batch k's
  // copies, which run on their own stream while batch k+1 computes (batch
  // k+2 reuses the slot only after the host saw those copies complete)
  Event e0[2], e1[2], computed[2], copied[2];
  std::vector<std::pair<Event, Event>> evs[2];  // per-launch timing events, [r * 4 + m]
  Trace tr;
  Uploader uploader;

  explicit Worker(const Job& j)
      : J(j), S(j.S), set(*j.set), L(*j.L), fsz((size_t)j.set->W * j.set->H),
        B(j.set->per_launch ? 1 : kBatchPocs), predMask(vame_pred_mask(j.set->mode_mask)) {
    tr.on = trace_enabled();
    tr.w0 = now_s();
  }
  ~Worker() {
    uploader.join();
    for (hipStream_t s : {(hipStream_t)st, (hipStream_t)up, (hipStream_t)dn})
      if (s) (void)hipStreamSynchronize(s);
  }

  char* result(int slot, int j) const { return (char*)(void*)dres + ((size_t)slot * B + j) * L.bytes; }
  bool coded(int m) const { return (predMask >> m) & 1; }

  bool setup_context();
  bool setup_frames();
  bool setup_results();
  bool take_slabs(const std::vector<int>& pocs, std::vector<Slab*>& batch);
  bool issue_fused(const std::vector<Slab*>& batch, int slot);
  bool issue_per_launch(const std::vector<Slab*>& batch, int slot);
  bool download(const std::vector<Slab*>& batch, int slot);
  bool finish(const std::vector<Slab*>& batch, int slot);
  bool run();
};

bool Worker::setup_context() {
  GPU_CHECK(hipSetDevice(J.device), "hipSetDevice");
  VAME_CHECK(vame_create(&ctx.ctx, J.device, set.W, set.H), "vame_create");
  VAME_CHECK(vame_set_max_pairs(ctx.ctx, kMaxBatchPairs), "vame_set_max_pairs");
  tr.w1 = now_s();
  VAME_CHECK(vame_set_prof(ctx.ctx, set.prof ? 1 : 0), "vame_set_prof");
  GPU_CHECK(hipStreamCreateWithFlags(st.put(), hipStreamNonBlocking), "hipStreamCreate");
  // The copy streams are created with an explicit priority: created like the
  // compute stream, one of them shared its hardware queue with it (HIP maps
  // streams onto GPU_MAX_HW_QUEUES = 4 queues, and this process has five
  // streams), so each batch's 285 MB result download at C5 (5.1 ms at PCIe
  // rate) sat in front of the next batch's kernels: 0.30 s of idle GPU per
  // 240 4K frames (VAME_CLI_TRACE).  VAME_CLI_COPY_PRIO=0 restores that.
  const int copyPrio = getenv("VAME_CLI_COPY_PRIO") ? atoi(getenv("VAME_CLI_COPY_PRIO")) : 1;
  if (copyPrio) {
    int lo = 0, hi = 0;
    GPU_CHECK(hipDeviceGetStreamPriorityRange(&lo, &hi), "hipDeviceGetStreamPriorityRange");
    const int pr = copyPrio > 0 ? lo : hi;
    GPU_CHECK(hipStreamCreateWithPriority(up.put(), hipStreamNonBlocking, pr), "hipStreamCreate");
    GPU_CHECK(hipStreamCreateWithPriority(dn.put(), hipStreamNonBlocking, pr), "hipStreamCreate");
  } else {
    GPU_CHECK(hipStreamCreateWithFlags(up.put(), hipStreamNonBlocking), "hipStreamCreate");
    GPU_CHECK(hipStreamCreateWithFlags(dn.put(), hipStreamNonBlocking), "hipStreamCreate");
  }
  return true;
}

bool Worker::setup_frames() {
  const std::vector<int> labels = recon_labels(J.pocs);
  GPU_CHECK(hipMalloc(origBlk.put(), J.pocs.size() * fsz * 2), "hipMalloc frames");
  GPU_CHECK(hipMalloc(reconBlk.put(), labels.size() * fsz * 2), "hipMalloc frames");
  for (size_t i = 0; i < J.pocs.size(); i++) dorig[J.pocs[i]] = (uint16_t*)(void*)origBlk + i * fsz;
  for (size_t i = 0; i < labels.size(); i++) drecon[labels[i]] = (uint16_t*)(void*)reconBlk + i * fsz;
  batches = plan_batches(J.pocs, set.per_launch);
  upEv.resize(batches.size());
  for (auto& e : upEv) GPU_CHECK(hipEventCreateWithFlags(e.put(), hipEventDisableTiming), "hipEventCreate");
  uploader.device = J.device;
  uploader.stream = up;
  uploader.frame_samples = fsz;
  uploader.orig = J.orig;
  uploader.recon = J.recon;
  uploader.dorig = &dorig;
  uploader.drecon = &drecon;
  uploader.batches = &batches;
  uploader.issued = &upEv;
  uploader.S = S;
  uploader.start();
  return true;
}

bool Worker::setup_results() {
  GPU_CHECK(hipMalloc(dres.put(), 2 * (size_t)B * L.bytes), "hipMalloc results");
  for (int i = 0; i < 2; i++) {
    GPU_CHECK(hipEventCreate(e0[i].put()), "hipEventCreate");
    GPU_CHECK(hipEventCreate(e1[i].put()), "hipEventCreate");
    GPU_CHECK(hipEventCreateWithFlags(computed[i].put(), hipEventDisableTiming), "hipEventCreate");
    GPU_CHECK(hipEventCreateWithFlags(copied[i].put(), hipEventDisableTiming), "hipEventCreate");
  }
  return tr.start(S, st, batches.size());
}

// a free slab of this worker's pool for each POC; false once the run has failed
bool Worker::take_slabs(const std::vector<int>& pocs, std::vector<Slab*>& batch) {
  for (int p : pocs) {
    std::unique_lock<std::mutex> g(S->mu);
    auto& pool = S->pools[J.worker];
    S->cv.wait(g, [&] { return S->failed || !pool.empty(); });
    if (S->failed) return false;
    Slab* slab = pool.back();
    pool.pop_back();
    slab->poc = p;
    slab->nrefs = std::min(4, p);
    batch.push_back(slab);
  }
  return true;
}

bool Worker::issue_fused(const std::vector<Slab*>& batch, int slot) {
  vame_poc_result out[kBatchPocs];
  const uint16_t* rp[kBatchPocs][4];
  vame_poc_job jobs[kBatchPocs];
  for (size_t j = 0; j < batch.size(); j++) {
    const int p = batch[j]->poc;
    int refs[4];
    const int nrefs = vame_ref_list(p, refs);
    memset(&out[j], 0, sizeof out[j]);
    for (int r = 0; r < nrefs; r++) {
      rp[j][r] = drecon[refs[r]];
      for (int m = 0; m < 4; m++) {
        if (!coded(m)) continue;
        out[j].cost[r][m] = (int64_t*)(result(slot, (int)j) + L.off_cost[r][m]);
        out[j].cpmvs[r][m] = (vame_cpmvs*)(result(slot, (int)j) + L.off_cp[r][m]);
      }
    }
    jobs[j] = vame_poc_job{dorig[p], rp[j], nrefs, vame_lambda(set.qp, p), &out[j]};
  }
  GPU_CHECK(hipEventRecord(e0[slot], st), "hipEventRecord");
  VAME_CHECK(vame_affine_me_batch(ctx.ctx, jobs, (int)batch.size(), set.mode_mask, set.extra, st),
             "vame_affine_me_batch");
  GPU_CHECK(hipEventRecord(e1[slot], st), "hipEventRecord");
  return true;
}

// main.cpp:754-966: per refIdx, FULL_2CP, FULL_3CP, HALF_2CP, HALF_3CP
bool Worker::issue_per_launch(const std::vector<Slab*>& batch, int slot) {
  const int p = batch[0]->poc;
  int refs[4];
  const int nrefs = vame_ref_list(p, refs);
  const float lambda = vame_lambda(set.qp, p);
  auto dcost = [&](int r, int m) { return (int64_t*)(result(slot, 0) + L.off_cost[r][m]); };
  auto dcp = [&](int r, int m) { return (vame_cpmvs*)(result(slot, 0) + L.off_cp[r][m]); };
  while (evs[slot].size() < (size_t)nrefs * 4) {  // created when a POC first needs them
    std::pair<Event, Event> e;
    GPU_CHECK(hipEventCreate(e.first.put()), "hipEventCreate");
    GPU_CHECK(hipEventCreate(e.second.put()), "hipEventCreate");
    evs[slot].push_back(std::move(e));
  }
  for (int r = 0; r < nrefs; r++)
    for (int m = 0; m < 4; m++) {
      if (!coded(m)) continue;
      auto& e = evs[slot][r * 4 + m];
      GPU_CHECK(hipEventRecord(e.first, st), "hipEventRecord");
      VAME_CHECK(vame_affine_me(ctx.ctx, drecon[refs[r]], dorig[p], lambda, m >> 1, (m & 1) ? 3 : 2, set.extra,
                                (m & 1) ? dcp(r, m - 1) : nullptr, dcost(r, m), dcp(r, m), st),
                 "vame_affine_me");
      GPU_CHECK(hipEventRecord(e.second, st), "hipEventRecord");
    }
  return true;
}

// the slot's results into the batch's slabs, on the download stream, once computed
bool Worker::download(const std::vector<Slab*>& batch, int slot) {
  GPU_CHECK(hipStreamWaitEvent(dn, computed[slot], 0), "hipStreamWaitEvent");
  for (size_t j = 0; j < batch.size(); j++)
    GPU_CHECK(hipMemcpyAsync(batch[j]->host(), result(slot, (int)j), L.bytes, hipMemcpyDeviceToHost, dn), "D2H");
  GPU_CHECK(hipEventRecord(copied[slot], dn), "hipEventRecord");
  return true;
}

// waits for a slot's copies, collects its kernel times, hands the slabs to the writer
bool Worker::finish(const std::vector<Slab*>& batch, int slot) {
  auto collect = [&] {
    if (hipEventSynchronize(copied[slot]) != hipSuccess) return false;
    float ms = 0;
    if (!set.per_launch) {
      if (hipEventElapsedTime(&ms, e0[slot], e1[slot]) != hipSuccess) return false;
      batch[0]->fused_ns = ms * 1e6f;  // the batch's kernel time, reported once
      tr.kernelSum += ms;
      return true;
    }
    Slab* s = batch[0];
    for (int r = 0; r < s->nrefs; r++)
      for (int m = 0; m < 4; m++) {
        if (!coded(m)) continue;
        if (hipEventElapsedTime(&ms, evs[slot][r * 4 + m].first, evs[slot][r * 4 + m].second)) return false;
        s->pred_ns[m] += ms * 1e6f;
      }
    return true;
  };
  if (!collect()) {
    fail(S, "waiting for results failed");
    return false;
  }
  std::lock_guard<std::mutex> g(S->mu);
  for (Slab* s : batch) S->done[s->poc] = s;
  S->cv.notify_all();
  return true;
}

bool Worker::run() {
  if (!setup_context() || !setup_frames() || !setup_results()) return false;
  std::vector<Slab*> pending;  // the batch enqueued last: finished only after the next one is enqueued
  int pslot = 0;
  for (size_t k = 0; k < batches.size(); k++) {
    const int slot = (int)(k & 1);
    std::vector<Slab*> batch;
    if (!take_slabs(batches[k], batch)) return false;
    if (!uploader.wait(k)) {  // this batch's frames: issued by the uploader, then waited for on the device
      fail(S, "upload frames failed");
      return false;
    }
    GPU_CHECK(hipStreamWaitEvent(st, upEv[k], 0), "hipStreamWaitEvent");
    if (!tr.batch_begin(S, st, k, computed[slot ^ 1])) return false;
    if (!(set.per_launch ? issue_per_launch(batch, slot) : issue_fused(batch, slot))) return false;
    if (!tr.batch_end(S, st, k)) return false;
    GPU_CHECK(hipEventRecord(computed[slot], st), "hipEventRecord");
    if (k + 1 == batches.size()) GPU_CHECK(hipEventRecord(tr.tLast, st), "hipEventRecord");
    if (!download(batch, slot)) return false;
    if (!pending.empty() && !finish(pending, pslot)) return false;
    pending = batch;
    pslot = slot;
  }
  if (!pending.empty() && !finish(pending, pslot)) return false;
  if (tr.on) tr.report(J.worker);
  return true;
}

}  // namespace

void gpu_worker(Job J) {
  Worker w(J);
  (void)w.run();
}

}  // namespace vame_cli

// vame_engine.hip -- the fused search of the MI355X affine-ME engine
// (include/vame.h): its kernels' instances, the context and the launcher.
//
// Replaces the reference's OpenCL host launch boundary (main.cpp:473-552 buffer
// management, :754-966 clSetKernelArg/clEnqueueNDRangeKernel for the four
// kernel objects).  vame_create uploads what vame_templates.cpp builds; a call
// packs one kernel-argument struct and enqueues on the caller's stream.  The
// entry points of the later stages are in vame_stages.hip.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/vame.h"
#include "vame_kernel.h"
#include "vame_mc_core.h"
#include "vame_partition.h"
#include "vame_bipred.h"
#include "vame_ctx.h"
#include "vame_templates.h"

#if VAME_SPLIT_TU
namespace vame {
VAME_2CP_KERNELS(extern)  // defined in vame_kernels_2cp.hip
}
#endif

using namespace vame;

static_assert(sizeof(vame_cpmvs) == 28, "Cpmvs layout (typedef.h)");
static_assert(sizeof(vame_cpmvs_dev) == 28, "Cpmvs layout (typedef.h)");

namespace {

int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e && *e ? atoi(e) : dflt;
}

// The seed-reuse regions of the two-sub-block kernels for `pairs` pairs per
// launch: [ctu2 | half2w | half2h | quad2], each [pairs * nCtus * items][5][NSB]
// int32 (vame_kernel.h: p.bestS + ((pair * nCtus + ctu) * nItems + item) * 5 *
// NSB; quad2: sized for its largest item set).
size_t best_layout(const vame_ctx* c, int pairs, size_t off[4]) {
  const size_t per = (size_t)pairs * c->nCtus * 5;
  int nq2 = 0;  // the SBL2 items index the region by their item index
  for (int a = 0; a < 3; a++) nq2 = std::max({nq2, c->quadN[1][a], c->quadN[3][a]});
  off[0] = 0;
  off[1] = off[0] + per * c->nBig1 * Cfg<kKindCtu2>::NSB;
  off[2] = off[1] + per * c->nHalfW * Cfg<kKindHalf2W>::NSB;
  off[3] = off[2] + per * c->nHalfH * Cfg<kKindHalf2H>::NSB;
  return off[3] + per * nq2 * Cfg<kKindQuad2>::NSB;
}

int alloc_best(vame_ctx* c, int pairs) {
  if (c->bestS) {
    VAME_HIP(hipDeviceSynchronize());  // no launch may still use the old buffer
    VAME_HIP(hipFree(c->bestS));
    c->bestS = nullptr;
  }
  c->bestPending = false;
  const size_t words = best_layout(c, pairs, c->bestOff);
  if (hipMalloc(&c->bestS, words * sizeof(int32_t)) != hipSuccess) {
    (void)hipGetLastError();
    c->bestS = nullptr;
    return VAME_E_NOMEM;
  }
  c->maxPairs = pairs;
  return VAME_OK;
}

void fill_common(KParams& kp, const vame_ctx* c, int extra) {
  kp.W = c->W;
  kp.H = c->H;
  kp.nCtus = c->nCtus;
  kp.ctusPerRow = c->ctusPerRow;
  kp.extra = extra;
}

// Per-kernel timing (vame_set_timing(ctx, 1)): the kernel's own dispatch
// packet carries the start / stop events (hipExtLaunchKernel), so timing adds
// no marker packets to the streams and the interval is the dispatch's own
// execution, as rocprofv3 reports it (timed dispatches still cost ~0.8 % of a
// c2 step, with or without the events' system-scope fence, as did the event
// records around each launch used before).  Returns the (start, stop) pair for the
// next launch of kernel class `cls`, or nulls with timing off.
int time_events(vame_ctx* c, int cls, hipEvent_t& start, hipEvent_t& stop) {
  start = stop = nullptr;
  if (!((c->timing >> cls) & 1)) return VAME_OK;
  auto& v = c->ev[cls];
  if (c->evUsed[cls] == v.size()) {
    std::pair<hipEvent_t, hipEvent_t> e;
    VAME_HIP(hipEventCreate(&e.first));
    VAME_HIP(hipEventCreate(&e.second));
    v.push_back(e);
  }
  start = v[c->evUsed[cls]].first;
  stop = v[c->evUsed[cls]].second;
  c->evUsed[cls]++;
  return VAME_OK;
}

// Block order (affine_me_body): groups of about c->groupCombos (ctu, pair)
// combinations, whose tiles and original samples the XCDs' L2s hold while
// every item of a CTU passes -- the 3 pairs of a 1080p 2-frame step, or one
// chunk of CTU rows of one 2160p pair -- and within a group, the (ctu, pair)
// combinations of each template item in slots padded to a multiple of 8 per
// (pair, chunk), so every item of a CTU lands on the same XCD (padding blocks
// exit at once).  Returns the grid size.
unsigned block_grid(const vame_ctx* c, int cls, KParams& k) {
  k.order = c->dOrder[cls];
  k.nChunks = c->nChunks[cls];
  k.cpp = c->cpp[cls];
  k.groupPairs = k.nChunks > 1 ? 1 : std::max(1, std::min(k.nPairs, c->groupCombos[cls] / k.cpp));
  k.groupPer = k.groupPairs * k.cpp;
  const int groups = (k.nPairs + k.groupPairs - 1) / k.groupPairs * k.nChunks;
  return (unsigned)(groups * k.nItems * k.groupPer);
}

// The kernel instances by launch mode (vame_kernel.h MODE: 1 = 2-CP only,
// 2 = 3-CP only, 3 = 2-CP then 3-CP), at [MODE - 1]; nullptr: the launch plan
// never runs the kernel in that mode, so no instance of it is built.  A
// 2-CP-only launch runs the SBL1 and SBL2 quadrant items in one affine_me_quad
// kernel (the short c2 step needs the two kinds of items side by side: 0.889
// vs 0.953 ms as two kernels) and the 128x64 and 64x128 CUs in one
// affine_me_half2 launch (c2 0.883 vs 0.888 ms); the other modes run
// affine_me_quad2 beside affine_me_quad (c4 291.3 vs 298.8 ms in one kernel,
// whose two bodies spill 104 vs 28 B per lane) and affine_me_half2w then
// affine_me_half2h (c4 290.9 vs 292.5 ms merged: 88 vs 20 B per lane),
// profiles/r06_quad2_ab.txt.
using KernelFn = void (*)(KParams);
constexpr KernelFn kQuadProf[3] = {affine_me_quad_prof<1>, affine_me_quad_prof<2>, affine_me_quad_prof<3>};
constexpr KernelFn kQuad[3] = {affine_me_quad<1>, affine_me_quad<2>, affine_me_quad<3>};
constexpr KernelFn kCtuProf[3] = {affine_me_ctu_prof<1>, affine_me_ctu_prof<2>, affine_me_ctu_prof<3>};
constexpr KernelFn kCtu2[3] = {affine_me_ctu2<1>, affine_me_ctu2<2>, affine_me_ctu2<3>};
constexpr KernelFn kHalfProf[3] = {affine_me_half_prof<1>, affine_me_half_prof<2>, affine_me_half_prof<3>};
constexpr KernelFn kHalf2H[3] = {nullptr, affine_me_half2h<2>, affine_me_half2h<3>};
constexpr KernelFn kHalf2W[3] = {nullptr, affine_me_half2w<2>, affine_me_half2w<3>};
constexpr KernelFn kQuad2[3] = {nullptr, affine_me_quad2<2>, affine_me_quad2<3>};
constexpr KernelFn kHalf2[3] = {affine_me_half2<1>, nullptr, nullptr};

// Launch one kernel: with the dispatch-carried timing events and AQL flags, or
// (the caller's stream under capture) as a plain launch, which the graph records.
hipError_t launch_kernel(KernelFn kernel, unsigned grid, unsigned threads, hipStream_t s, hipEvent_t t0, hipEvent_t t1,
                         int flags, const KParams& kp, bool capture) {
  if (grid == 0) return hipSuccess;  // no work items (a kernel class without CUs)
  if (capture)
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(threads), 0, s, kp);
  else
    hipExtLaunchKernelGGL(kernel, dim3(grid), dim3(threads), 0, s, t0, t1, flags, kp);
  return hipGetLastError();
}

// One dispatch of a launch: the kernel, its work items and where it runs.
struct Dispatch {
  KernelFn kernel;
  unsigned threads;
  const Item* items;
  int nItems;
  int32_t* bestS;  // the kernel's region of the seed-reuse sums, or nullptr
  int order;       // block-order class (block_grid)
  int timing;      // timing class (vame_ctx::timing)
  bool side;       // on the quadrant stream: the side stream of a forked call
};

// The dispatches of one launch in issue order, at most six; returns their
// number.  The quadrant kernels: affine_me_quad_prof over item set 2 under
// PROF, affine_me_quad over set 3 in a 2-CP-only launch, else affine_me_quad2
// (set 1) on the quadrant stream and affine_me_quad (set 0) on the caller's.
// The 128-class kernels (bigItems), all on the caller's stream: the 128x128
// CUs, then the 128x64 and 64x128 CUs.  A forked call issues the 128-class
// kernels first, a call on one stream the quadrant kernels.
int launch_plan(const vame_ctx* c, int mode, bool quadFull, bool quadHalf, bool bigItems, bool fork,
                Dispatch (&plan)[6]) {
  const int m = mode - 1, aset = quadFull && quadHalf ? 2 : quadFull ? 0 : 1;
  const auto quad = [&](KernelFn k, int set, int timing, bool side) {
    return Dispatch{k, Cfg<kKindQuad>::THREADS, c->dQuad + c->quadOff[set][aset], c->quadN[set][aset],
                    c->bestS + c->bestOff[3], 0, timing, side};
  };
  const auto big = [&](KernelFn k, unsigned threads, const Item* items, int nItems, int region, int timing) {
    return Dispatch{k, threads, items, nItems, region < 0 ? nullptr : c->bestS + c->bestOff[region], 1, timing, false};
  };
  Dispatch q[2], b[3];
  int nq = 0, nb = 0;
  if (quadFull || quadHalf) {
    if (c->prof) {
      q[nq++] = quad(kQuadProf[m], 2, 0, true);
    } else if (mode == 1) {
      q[nq++] = quad(kQuad[m], 3, 0, true);
    } else {
      q[nq++] = quad(kQuad2[m], 1, 6, true);
      q[nq++] = quad(kQuad[m], 0, 0, false);
    }
  }
  if (bigItems) {
    if (c->prof) {
      b[nb++] = big(kCtuProf[m], Cfg<kKindCtu>::THREADS, c->dBig1, c->nBig1, 0, 1);
      b[nb++] = big(kHalfProf[m], Cfg<kKindHalf>::THREADS, c->dHalf, c->nHalf, -1, 2);
    } else {
      b[nb++] = big(kCtu2[m], Cfg<kKindCtu2>::THREADS, c->dBig1, c->nBig1, 0, 3);
      if (mode == 1) {  // both orientations, dHalfW then dHalfH: the two regions' span
        b[nb++] = big(kHalf2[m], Cfg<kKindHalf2W>::THREADS, c->dHalfW, c->nHalfW + c->nHalfH, 1, 4);
      } else {
        b[nb++] = big(kHalf2W[m], Cfg<kKindHalf2W>::THREADS, c->dHalfW, c->nHalfW, 1, 4);
        b[nb++] = big(kHalf2H[m], Cfg<kKindHalf2H>::THREADS, c->dHalfH, c->nHalfH, 2, 5);
      }
    }
  }
  Dispatch* end = plan;
  if (fork) end = std::copy(b, b + nb, end);
  end = std::copy(q, q + nq, end);
  if (!fork) end = std::copy(b, b + nb, end);
  return (int)(end - plan);
}

// The join of a forked call: the caller's stream waits for the side stream.
int join_side(vame_ctx* c, hipStream_t stream, bool capture) {
  if (c->valueSync != 0 && c->syncWord && !capture) {
    const uint32_t v = ++c->joinSeq;
    VAME_HIP(hipStreamWriteValue32(c->side, c->syncWord, v, 0));
    VAME_HIP(hipStreamWaitValue32(stream, c->syncWord, v, hipStreamWaitValueGte, 0xFFFFFFFFu));
  } else {
    VAME_HIP(hipEventRecord(c->evJoin, c->side));
    VAME_HIP(hipStreamWaitEvent(stream, c->evJoin, 0));
  }
  return VAME_OK;
}

// One dispatch for the pairs of kp on stream s.
int dispatch(vame_ctx* c, const Dispatch& d, const KParams& kp, hipStream_t s, int flags, bool capture) {
  KParams k = kp;
  k.items = d.items;
  k.nItems = d.nItems;
  k.bestS = d.bestS;
  const unsigned grid = block_grid(c, d.order, k);
  hipEvent_t t0 = nullptr, t1 = nullptr;
  if (!capture) VAME_TRY(time_events(c, d.timing, t0, t1));
  VAME_HIP(launch_kernel(d.kernel, grid, d.threads, s, t0, t1, flags, k, capture));
  return VAME_OK;
}

// The launches of one call.  By default (VAME_STREAMS=2) the 128-class
// kernels run on the caller's stream and the quadrant kernel on a side stream
// forked from it: the 128-class workgroups, issued first and ahead of the
// fork's cross-stream hop, take their CUs before the quadrant workgroups fill
// the GPU, and the quadrant workgroups then fill the room beside them (a
// 512-thread affine_me_ctu2 workgroup leaves a CU room for two quadrant
// workgroups, a 256-thread half2 one for three).  Kernels of one stream run
// one after the other, so only separate streams overlap them.  The launches
// of one batch (maxPairs pairs each) fork once and join once: launch k + 1's
// kernels follow launch k's on their own streams.  Under capture (the
// caller's stream is being captured into a graph) the fork and join are
// events, the graph's edges.
int launch_direct(vame_ctx* c, const std::vector<KParams>& kps, bool quadFull, bool quadHalf, bool bigItems,
                  hipStream_t stream, bool capture) {
  if (VAME_ABLATE & 16) bigItems = false;  // timing-only builds
  if (VAME_ABLATE & 32) quadFull = quadHalf = false;
  if (kps.empty()) return VAME_OK;
  const int mode = (kps[0].run2 ? 1 : 0) | (kps[0].run3 ? 2 : 0);  // the kernel instance (MODE)
  if (mode == 0) return VAME_OK;
  const bool fork = c->streams == 2 && bigItems && (quadFull || quadHalf);
  if (fork && !c->side) return VAME_E_INVALID;
  Dispatch plan[6];
  const int n = launch_plan(c, mode, quadFull, quadHalf, bigItems, fork, plan);
  if (fork) {
    VAME_HIP(hipEventRecord(c->evFork, stream));
    VAME_HIP(hipStreamWaitEvent(c->side, c->evFork, 0));
  }
  int rc = VAME_OK;
  int issued = 0;  // VAME_STREAMS=1: kernels after a call's first may start before it ends
  for (size_t k = 0; k < kps.size() && rc == VAME_OK; k++)
    for (int i = 0; i < n && rc == VAME_OK; i++) {
      const int flags = c->streams == 1 && issued++ > 0 ? hipExtAnyOrderLaunch : 0;
      rc = dispatch(c, plan[i], kps[k], fork && plan[i].side ? c->side : stream, flags, capture);
    }
  // after a failed launch too: earlier kernels went to the side stream, so
  // order them before the caller's stream anyway -- the caller never frees or
  // reuses result buffers they still write (best effort, the first error is
  // the one reported)
  if (fork) {
    const int jrc = join_side(c, stream, capture);
    if (rc == VAME_OK) rc = jrc;
  }
  return rc;
}

int launch(vame_ctx* c, const std::vector<KParams>& kps, bool quadFull, bool quadHalf, bool bigItems,
           hipStream_t stream) {
  if (kps.empty()) return VAME_OK;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  VAME_HIP(hipStreamIsCapturing(stream, &cs));
  if (cs == hipStreamCaptureStatusInvalidated) return VAME_E_INVALID;
  const bool capture = cs == hipStreamCaptureStatusActive;
  // the seed-reuse sums (allocated with the context): one buffer per context,
  // so a call on another stream than the last user's waits for it first
  const bool useBest = !c->prof && kps[0].run2 && kps[0].run3;  // quad2 and the 128-class kernels
  if (useBest && !c->bestS) return VAME_E_NOMEM;
  if (useBest && !capture && c->bestPending && c->bestStream != stream)
    VAME_HIP(hipStreamWaitEvent(stream, c->bestEv, 0));
  const int rc = launch_direct(c, kps, quadFull, quadHalf, bigItems, stream, capture);
  if (useBest && !capture) {
    VAME_HIP(hipEventRecord(c->bestEv, stream));  // after the join: every kernel of the call
    c->bestStream = stream;
    c->bestPending = true;
  }
  return rc;
}

}  // namespace

extern "C" {

int vame_create(vame_ctx** out, int device, int width, int height) {
  if (!out) return VAME_E_INVALID;
  *out = nullptr;
  const int nCtus = num_ctus(width, height);
  if (!nCtus) return VAME_E_INVALID;
  int ndev = 0;
  VAME_HIP(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return VAME_E_INVALID;
  DeviceGuard guard(device);
  VAME_HIP(guard.err);
  Templates t;
  if (!build_templates(t)) return VAME_E_INVALID;
  vame_ctx* c = new vame_ctx();
  c->device = device;
  c->W = width;
  c->H = height;
  c->nCtus = nCtus;
  c->ctusPerRow = (width + kCtu - 1) / kCtu;  // T8: integer ceil
  c->nBig1 = (int)t.big1.size();
  c->nHalf = (int)t.half.size();
  c->nHalfW = t.nHalfW;
  c->nHalfH = t.nHalfH;
  memcpy(c->quadOff, t.quadOff, sizeof(c->quadOff));
  memcpy(c->quadN, t.quadN, sizeof(c->quadN));
  // the runtime knobs (include/vame.h; results are bit-identical under every
  // setting, the defaults are the measured best)
  c->streams = env_int("VAME_STREAMS", 2) == 1 ? 1 : 2;
  c->valueSync = env_int("VAME_SYNC", 1) != 0 ? 1 : 0;
  c->groupCombos[0] = c->groupCombos[1] = std::max(8, env_int("VAME_GROUP_COMBOS", 408));
  hipError_t e = hipSuccess;
  auto upload = [&](Item*& d, const std::vector<Item>& v) {
    if (e == hipSuccess && !v.empty()) e = hipMalloc(&d, v.size() * sizeof(Item));
    if (e == hipSuccess && !v.empty()) e = hipMemcpy(d, v.data(), v.size() * sizeof(Item), hipMemcpyHostToDevice);
  };
  upload(c->dQuad, t.quad);
  upload(c->dBig1, t.big1);
  upload(c->dHalf, t.half);
  upload(c->dHalfW, t.halfWH);
  if (c->dHalfW) c->dHalfH = c->dHalfW + t.nHalfW;
  for (int k = 0; k < 2 && e == hipSuccess; k++) {
    const std::vector<int32_t> order = build_order(nCtus, c->ctusPerRow, c->groupCombos[k], c->nChunks[k], c->cpp[k]);
    e = hipMalloc(&c->dOrder[k], order.size() * sizeof(int32_t));
    if (e == hipSuccess)
      e = hipMemcpy(c->dOrder[k], order.data(), order.size() * sizeof(int32_t), hipMemcpyHostToDevice);
  }
  // the side stream the default launch structure uses, created here, not
  // during a launch (a launch may be under stream capture): a process has
  // GPU_MAX_HW_QUEUES = 4 hardware queues and HIP shares them between its
  // streams beyond that, so an idle stream created here could put the
  // caller's own copy streams on the quadrant kernel's queue (the CLI's
  // compute, upload and download streams + the side stream are four)
  if (e == hipSuccess && c->streams == 2) e = hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->evJoin, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->evFork, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->bestEv, hipEventDisableTiming);
  if (e == hipSuccess && c->valueSync) {
    if (hipExtMallocWithFlags(reinterpret_cast<void**>(&c->syncWord), 8, hipMallocSignalMemory) != hipSuccess ||
        hipMemset(c->syncWord, 0, 8) != hipSuccess) {
      (void)hipGetLastError();
      if (c->syncWord) (void)hipFree(c->syncWord);
      c->syncWord = nullptr;
      c->valueSync = 0;  // events instead
    }
  }
  if (e == hipSuccess) e = hipMalloc(&c->mcScratch, kMcScratchWords * sizeof(int32_t));
  if (e == hipSuccess) e = hipMalloc(&c->partScratch, (size_t)nCtus * kPartScratchWords * sizeof(int32_t));
  if (e == hipSuccess) {  // vame_bipred's candidate tables
    const BiTable bt = build_bi_table(width, height);
    for (int a = 0; a < 2; a++) {
      c->biNCand[a] = bt.nCand[a];
      c->biNGroup[a] = bt.nGroup[a];
    }
    const size_t candBytes = bt.cands.size() * sizeof(BiCand), groupBytes = bt.groupCand.size() * sizeof(int32_t);
    e = hipMalloc(&c->biCands, candBytes);
    if (e == hipSuccess) e = hipMemcpy(c->biCands, bt.cands.data(), candBytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc(&c->biGroupCand, groupBytes);
    if (e == hipSuccess) e = hipMemcpy(c->biGroupCand, bt.groupCand.data(), groupBytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc(&c->biPairSatd, bt.cands.size() * kBiPairs * sizeof(int64_t));
  }
  if (e != hipSuccess) {
    snprintf(g_hip_err, sizeof(g_hip_err), "%s", hipGetErrorString(e));
    vame_destroy(c);
    return VAME_E_DEVICE;
  }
  // the seed-reuse sums for kMaxPairs pairs per launch (vame_set_max_pairs
  // resizes them): ~1 GB at 3840x2160, 260 MB at 1920x1080
  const int rc = alloc_best(c, kMaxPairs);
  if (rc != VAME_OK) {
    vame_destroy(c);
    return rc;
  }
  *out = c;
  return VAME_OK;
}

int vame_set_max_pairs(vame_ctx* c, int max_pairs) {
  if (!c || max_pairs < 1 || max_pairs > kMaxPairs) return VAME_E_INVALID;
  if (max_pairs == c->maxPairs && c->bestS) return VAME_OK;
  DeviceGuard guard(c->device);
  VAME_HIP(guard.err);
  return alloc_best(c, max_pairs);
}

int vame_get_max_pairs(vame_ctx* c) { return c ? c->maxPairs : VAME_E_INVALID; }

void vame_destroy(vame_ctx* c) {
  if (!c) return;
  DeviceGuard guard(c->device);
  for (Item* d : {c->dQuad, c->dBig1, c->dHalf, c->dHalfW})  // dHalfH lies inside dHalfW's block
    if (d) (void)hipFree(d);
  if (c->bestS) (void)hipFree(c->bestS);
  for (int k = 0; k < 2; k++)
    if (c->dOrder[k]) (void)hipFree(c->dOrder[k]);
  if (c->side) (void)hipStreamDestroy(c->side);
  for (hipEvent_t e : {c->evJoin, c->evFork, c->bestEv, c->packEv})
    if (e) (void)hipEventDestroy(e);
  if (c->syncWord) (void)hipFree(c->syncWord);
  if (c->dPackSegs) (void)hipFree(c->dPackSegs);
  if (c->mcScratch) (void)hipFree(c->mcScratch);
  if (c->partScratch) (void)hipFree(c->partScratch);
  if (c->biCands) (void)hipFree(c->biCands);
  if (c->biGroupCand) (void)hipFree(c->biGroupCand);
  if (c->biPairSatd) (void)hipFree(c->biPairSatd);
  for (int k = 0; k < kTimingClasses; k++)
    for (auto& e : c->ev[k]) {
      (void)hipEventDestroy(e.first);
      (void)hipEventDestroy(e.second);
    }
  delete c;
}

int vame_affine_me(vame_ctx* c, const uint16_t* ref, const uint16_t* cur, float lambda, int align,
                   int nCP, int extra, const vame_cpmvs* prev, int64_t* cost, vame_cpmvs* cpmvs,
                   void* stream) {
  if (!c || !ref || !cur || !cost || !cpmvs) return VAME_E_INVALID;
  if ((align != 0 && align != 1) || (nCP != 2 && nCP != 3) || extra < 0 || extra > 64)
    return VAME_E_INVALID;
  if (nCP == 3 && !prev) return VAME_E_INVALID;
  DeviceGuard guard(c->device);
  VAME_HIP(guard.err);
  KParams kp;
  memset(&kp, 0, sizeof(kp));
  fill_common(kp, c, extra);
  kp.pair[0].cur = cur;
  kp.pair[0].ref = ref;
  kp.pair[0].lambda = lambda;
  kp.nPairs = 1;
  kp.run2 = nCP == 2;
  kp.run3 = nCP == 3;
  const int mode = align * 2 + (nCP - 2);
  kp.pair[0].cost[mode] = cost;
  kp.pair[0].cpmv[mode] = reinterpret_cast<vame_cpmvs_dev*>(cpmvs);
  kp.prev[align] = reinterpret_cast<const vame_cpmvs_dev*>(prev);
  return launch(c, std::vector<KParams>{kp}, align == 0, align == 1, align == 0, (hipStream_t)stream);
}

int vame_affine_me_batch(vame_ctx* c, const vame_poc_job* jobs, int njobs, int mode_mask,
                         int extra, void* stream) {
  if (!c || !jobs || njobs < 1) return VAME_E_INVALID;
  if (!(mode_mask & VAME_MODE_2CP) || (mode_mask & ~15) || extra < 0 || extra > 64)
    return VAME_E_INVALID;
  const bool run3 = (mode_mask & VAME_MODE_3CP) != 0;
  const int preds = vame_pred_mask(mode_mask);  // alignment selection: only those items launch
  const bool doFull = (preds & 1) != 0, doHalf = (preds & 4) != 0;
  for (int j = 0; j < njobs; j++) {
    const vame_poc_job& jb = jobs[j];
    if (!jb.cur || !jb.refs || !jb.out || jb.nrefs < 1) return VAME_E_INVALID;
    if (jb.nrefs > 4) return VAME_E_UNSUPPORTED;
    for (int r = 0; r < jb.nrefs; r++) {
      if (!jb.refs[r]) return VAME_E_INVALID;
      for (int m = 0; m < 4; m++) {
        const bool need = ((preds >> m) & 1) != 0;
        if (need && (!jb.out->cost[r][m] || !jb.out->cpmvs[r][m])) return VAME_E_INVALID;
      }
    }
  }
  DeviceGuard guard(c->device);
  VAME_HIP(guard.err);
  // every (POC, refIdx) pair of the batch, maxPairs per launch
  std::vector<KParams> kps;
  KParams kp;
  memset(&kp, 0, sizeof(kp));
  fill_common(kp, c, extra);
  kp.run2 = 1;
  kp.run3 = run3;
  for (int j = 0; j < njobs; j++) {
    const vame_poc_job& jb = jobs[j];
    for (int r = 0; r < jb.nrefs; r++) {
      PairArgs& pa = kp.pair[kp.nPairs++];
      pa.cur = jb.cur;
      pa.ref = jb.refs[r];
      pa.lambda = jb.lambda;
      for (int m = 0; m < 4; m++) {
        pa.cost[m] = jb.out->cost[r][m];
        pa.cpmv[m] = reinterpret_cast<vame_cpmvs_dev*>(jb.out->cpmvs[r][m]);
      }
      const bool last = j == njobs - 1 && r == jb.nrefs - 1;
      if (kp.nPairs == c->maxPairs || last) {
        kps.push_back(kp);
        kp.nPairs = 0;
      }
    }
  }
  return launch(c, kps, doFull, doHalf, doFull, (hipStream_t)stream);
}

int vame_affine_me_poc(vame_ctx* c, const uint16_t* cur, const uint16_t* const* refs, int nrefs,
                       float lambda, int mode_mask, int extra, const vame_poc_result* out,
                       void* stream) {
  if (!out) return VAME_E_INVALID;
  const vame_poc_job job{cur, refs, nrefs, lambda, out};
  return vame_affine_me_batch(c, &job, 1, mode_mask, extra, stream);
}

int vame_set_prof(vame_ctx* c, int enable) {
  if (!c) return VAME_E_INVALID;
  c->prof = enable != 0;
  return VAME_OK;
}

int vame_set_timing(vame_ctx* c, int enable) {
  if (!c) return VAME_E_INVALID;
  // kernel classes timed (bit k: class k, see vame_ctx::timing): 2 = the
  // quadrant kernels (classes 0 and 6), any other non-zero value every class;
  // VAME_TIMING_KEEP (16) keeps the launches recorded so far (a caller timing
  // a sample of its steps toggles timing between them)
  const bool keep = (enable & VAME_TIMING_KEEP) != 0;
  enable &= ~VAME_TIMING_KEEP;
  c->timing = enable == 2 ? (1 | 64) : enable != 0 ? (1 << kTimingClasses) - 1 : 0;
  if (!keep)
    for (size_t& u : c->evUsed) u = 0;
  return VAME_OK;
}

int vame_get_timing(vame_ctx* c, int cls, double* total_ms, int* launches, int reset) {
  if (!c || cls < 0 || cls >= kTimingClasses || !total_ms || !launches) return VAME_E_INVALID;
  DeviceGuard guard(c->device);
  VAME_HIP(guard.err);
  double t = 0;
  for (size_t i = 0; i < c->evUsed[cls]; i++) {
    float ms = 0;
    VAME_HIP(hipEventSynchronize(c->ev[cls][i].second));
    VAME_HIP(hipEventElapsedTime(&ms, c->ev[cls][i].first, c->ev[cls][i].second));
    t += ms;
  }
  *total_ms = t;
  *launches = (int)c->evUsed[cls];
  if (reset) c->evUsed[cls] = 0;
  return VAME_OK;
}

const char* vame_strerror(int code) {
  switch (code) {
    case VAME_OK: return "ok";
    case VAME_E_INVALID: return "invalid argument";
    case VAME_E_DEVICE: return "HIP runtime error";
    case VAME_E_NOMEM: return "out of memory";
    case VAME_E_UNSUPPORTED: return "unsupported";
    default: return "unknown error";
  }
}

const char* vame_last_hip_error(void) { return g_hip_err; }

#if VAME_PHASE_TIMING
// profiling-only builds: per-phase shader-clock sums [kernel: quad, ctu, half,
// ctu2, half2w, half2h][kPhSlots] (see vame_instr.h)
int vame_debug_phase_cycles(unsigned long long* out, int reset) {
  if (!out) return VAME_E_INVALID;
  VAME_HIP(hipDeviceSynchronize());
  VAME_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_phase_cycles), sizeof(g_phase_cycles)));
  if (reset) {
    unsigned long long z[7 * kPhSlots] = {};
    VAME_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_phase_cycles), z, sizeof(z)));
  }
  return VAME_OK;
}
#endif
#if VAME_COUNT_PRED
// instrumentation builds: sub-block predictions run, [quad, ctu], and those of
// them whose window left the staged tile, [2 + quad 2-CP, quad 3-CP, ctu 2-CP,
// ctu 3-CP], and of those the ones a 4 / 8 / 16 px wider margin would hold,
// [6 + quad x3, ctu x3], then the wave lane slots [12 + kernel], [14 + kernel],
// [16 + kernel], and [18 ..] the two-sub-block quadrant waves (see vame_instr.h)
int vame_debug_pred_count(unsigned long long* out24, int reset) {
  if (!out24) return VAME_E_INVALID;
  VAME_HIP(hipDeviceSynchronize());
  VAME_HIP(hipMemcpyFromSymbol(out24, HIP_SYMBOL(g_pred_count), sizeof(unsigned long long) * 24));
  if (reset) {
    unsigned long long z[24] = {};
    VAME_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_pred_count), z, sizeof(z)));
  }
  return VAME_OK;
}
#endif
const char* vame_version(void) { return "vame 0.1 (gfx950)"; }

}  // extern "C"

// vame_ctx.h -- the engine's context and what every unit with C entry points
// (vame_engine.hip, vame_stages.hip, vame_pack.hip) shares: the error
// plumbing, the device guard and the checks of reference and result arrays.
// Private to the library.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

#include "../../include/vame.h"
#include "vame_items.h"

// text of the calling thread's last HIP error (vame_last_hip_error)
inline thread_local char g_hip_err[256] = "";

#define VAME_HIP(x)                                                               \
  do {                                                                            \
    hipError_t e_ = (x);                                                          \
    if (e_ != hipSuccess) {                                                       \
      snprintf(g_hip_err, sizeof(g_hip_err), "%s (%s:%d)", hipGetErrorString(e_), \
               __FILE__, __LINE__);                                               \
      return VAME_E_DEVICE;                                                       \
    }                                                                             \
  } while (0)

#define VAME_TRY(x)        \
  do {                     \
    int rc_ = (x);         \
    if (rc_) return rc_;   \
  } while (0)

constexpr int kTimingClasses = 7;

// One segment of a record pack: the n records of one (POC, refIdx, PRED),
// costs to slab[off .. off + n), CPMV components after them.
struct PackSeg {
  const int64_t* cost;
  const int32_t* cpmv;  // vame_cpmvs, 7 int32 per record
  long long off;
  int n, ncp;
};

struct vame_ctx {
  int device, W, H, nCtus, ctusPerRow;
  // device copies of the work-item templates (vame_templates.h, Templates):
  // the quadrant items of four sets [s][FULL | HALF | both alignments] at
  // dQuad + quadOff[s][a]; the 128x128 item (dBig1: affine_me_ctu2;
  // affine_me_ctu_prof under PROF) and every 128x64 / 64x128 item (dHalfW /
  // dHalfH, adjacent: affine_me_half2w / _half2h, or both in one
  // affine_me_half2 launch; both in dHalf for affine_me_half_prof under PROF)
  vame::Item* dQuad = nullptr;
  int quadOff[4][3] = {}, quadN[4][3] = {};
  vame::Item* dBig1 = nullptr;
  vame::Item* dHalf = nullptr;
  vame::Item* dHalfW = nullptr;
  vame::Item* dHalfH = nullptr;
  int nBig1 = 0, nHalf = 0, nHalfW = 0, nHalfH = 0;
  // The 3-CP seed-reuse sums of the kernels with two sub-blocks per lane
  // (affine_me_ctu2, _half2w, _half2h, affine_me_quad2: 5 int32 per sub-block
  // of every (pair, CTU, item) of a launch; vame_kernel.h KParams::bestS), sized
  // for maxPairs pairs per launch and allocated by vame_create /
  // vame_set_max_pairs -- never inside a launch, so a captured call holds no
  // allocation.  bestOff[k]: the region of kernel k (ctu2, half2w, half2h,
  // quad2).  It is one
  // buffer per context: a call that uses it on another stream than the last
  // one waits for bestEv, recorded after that call.
  int32_t* bestS = nullptr;
  size_t bestOff[4] = {0, 0, 0, 0};
  int maxPairs = 0;
  hipEvent_t bestEv = nullptr;
  hipStream_t bestStream = nullptr;
  bool bestPending = false;
  // block order (block_grid), per kernel class (0 quadrant, 1 128-class):
  // slot -> CTU table, group size, CTU chunks, slots per (pair, chunk)
  int32_t* dOrder[2] = {nullptr, nullptr};
  int groupCombos[2] = {408, 408}, nChunks[2] = {1, 1}, cpp[2] = {0, 0};
  // Streams of a call (VAME_STREAMS).  Kernels of one stream run one after
  // the other on MI355X even without the AQL barrier bit
  // (hipExtAnyOrderLaunch: profiles/ubench/anyorder_overlap.hip, three 50-us
  // kernels take 155 us on one stream, ~90 on three), so by default (2) the
  // quadrant kernel runs on a side stream forked from the caller's and the
  // 128-class kernels on the caller's stream, issued first;
  // 1: every kernel on the caller's stream, the quadrant kernel first with
  // the barrier bit, the others after it in any order.
  int streams = 2;
  hipStream_t side = nullptr;
  hipEvent_t evFork = nullptr, evJoin = nullptr;
  // VAME_SYNC (default 1): the join as a stream memory operation -- the side
  // stream writes a sequence number to a signal-memory word
  // (hipStreamWriteValue32, ordered after its earlier work), the caller's
  // stream waits for it (hipStreamWaitValue32) -- ~6 us per cross-stream hop
  // on MI355X against ~12 with an event record + hipStreamWaitEvent
  // (profiles/ubench/stream_hop.hip).  The fork stays an event: its slower
  // hop is the head start that lets the 128-class workgroups, issued on the
  // caller's stream, take their CUs before the quadrant kernel fills the GPU.
  // 0, a word that cannot be allocated, or a caller's stream under capture:
  // events.
  int valueSync = 1;
  uint32_t* syncWord = nullptr;
  uint32_t joinSeq = 0;
  // optional per-kernel timing: (start, end) event pairs per kernel class
  // (0 affine_me_quad, 1 128x128 CUs in affine_me_ctu_prof, 2 128x64 / 64x128
  // CUs in affine_me_half_prof, 3 128x128 CUs in affine_me_ctu2, 4 / 5 128x64 /
  // 64x128 CUs in affine_me_half2w / _half2h -- 4 both, in affine_me_half2, in
  // 2-CP-only launches --, 6 affine_me_quad2)
  int timing = 0;
  // PROF on (vame_set_prof): the *_prof kernels
  bool prof = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev[kTimingClasses];
  size_t evUsed[kTimingClasses] = {};
  // vame_pack_records: the segment table of the last pack (host copy kept
  // until the next call) and its device copy
  std::vector<PackSeg> packSegs;
  PackSeg* dPackSegs = nullptr;
  size_t dPackCap = 0;
  hipEvent_t packEv = nullptr;  // after the last pack kernel (it read the device table)
  // vame_affine_mc: the sub-block offsets of up to VAME_MC_MAX_CUS descriptors
  // and the scan's block sums (kMcScratchWords int32, ~4 MB), allocated by
  // vame_create so that a call allocates nothing
  int32_t* mcScratch = nullptr;
  // vame_partition: per CTU the leaf count, the leaves by top-left block and
  // the blocks' owners, handed from the decision kernel to the emitting one
  int32_t* partScratch = nullptr;
  // vame_bipred: the in-frame candidate CUs of the resolution and the map
  // group of 16 sub-blocks -> candidate (vame_templates.h, BiTable), and the
  // pair SATD sums, 6 int64 per candidate
  vame::BiCand* biCands = nullptr;
  int32_t* biGroupCand = nullptr;
  int64_t* biPairSatd = nullptr;
  int biNCand[2] = {0, 0}, biNGroup[2] = {0, 0};
};

// Makes c->device current for one C-ABI call and restores the caller's device
// on every return path: the entry points must not change the calling thread's
// current device (a torch thread holding engines on two GPUs would otherwise
// see torch.cuda.current_device() move under it).
struct DeviceGuard {
  int prev = -1;
  hipError_t err;
  explicit DeviceGuard(int dev) {
    err = hipGetDevice(&prev);
    if (err == hipSuccess && prev != dev) err = hipSetDevice(dev);
  }
  ~DeviceGuard() {
    int now = -1;
    if (prev >= 0 && hipGetDevice(&now) == hipSuccess && now != prev) (void)hipSetDevice(prev);
  }
};

// The reference frames of a call into its parameter block: each non-null and
// 4-byte aligned (the kernels read window rows as dwords).
inline bool set_refs(const uint16_t* (&dst)[4], const uint16_t* const* refs, int nrefs) {
  for (int r = 0; r < nrefs; r++) {
    if (!refs[r] || (reinterpret_cast<uintptr_t>(refs[r]) & 3)) return false;
    dst[r] = refs[r];
  }
  return true;
}

// The search's result arrays of refIdx 0 .. nrefs-1 for the PREDs in
// `pred_mask` into a parameter block: each non-null.
template <typename C, typename V>
inline bool set_result(C* (&cost)[4][4], V* (&cpmv)[4][4], const vame_poc_result* res, int nrefs, int pred_mask) {
  for (int r = 0; r < nrefs; r++)
    for (int m = 0; m < 4; m++) {
      if (!((pred_mask >> m) & 1)) continue;
      if (!res->cost[r][m] || !res->cpmvs[r][m]) return false;
      cost[r][m] = res->cost[r][m];
      cpmv[r][m] = reinterpret_cast<V*>(res->cpmvs[r][m]);
    }
  return true;
}

// vame_instr.h -- the instrumentation switches of the device code.  The product
// build sets none of them; `make ablate | variant | count | phase` and
// profiles/dup_split.py, phase_profile.py and count_preds.py do.  The device
// counters are defined here, so every unit that includes this has its own.
#pragma once
#include <hip/hip_runtime.h>

namespace vame {

// Instrumentation builds only (the product build sets neither):
// VAME_ABLATE (timing-only builds, results are wrong): bit 0 skip the solve,
// bit 1 skip the gradient math, bit 2 skip the reductions of the equations,
// bit 3 skip the prediction math, bit 4 skip the 128-class launch, bit 5 skip
// the quadrant launch, bit 8 (host) 128-class templates without the 128x64 /
// 64x128 items, bit 9 every 9x9 window read from the tile (no clamped-global path),
// bit 10 the same in the 3-CP pass only, bit 11 no seed-reuse sums stored by
// the two-sub-block kernels' 2-CP pass.
#ifndef VAME_ABLATE
#define VAME_ABLATE 0
#endif
// VAME_DUP (timing-only builds, results stay correct): run a phase twice to
// price it in throughput terms: bit 0 prediction, bit 1 gradient, bit 2
// equation reduction, bit 6 the tile staging round trip, bit 4 the solve (on the system itself, before the real
// one rebuilds it: no extra LDS); with bit 5 set, only in the 3-CP pass.  The
// rest of an iteration: bit 7 the CU's MV field (mv_field), bit 8 the extended
// prediction rows (DPP neighbour columns, edge-row publication and reads),
// bit 9 the SATD segment sum, bit 10 the cost / best step, bit 11 the CPMV
// update (scaleDeltaMvs, clamp, clip, rate bits, flag sums).
#ifndef VAME_DUP
#define VAME_DUP 0
#endif

// VAME_COUNT_PRED (instrumentation builds, libvame_count.so): every lane counts
// the sub-block predictions it runs (the exact early exit skips the rest of
// the algorithmic n_pred per sub-block); g_pred_count[kernel: quad, ctu], and
// [2 + 2 kernel + (3-CP pass)]: those whose 9x9 window left the staged tile
// (the clamped-global path); [12 + kernel]: 64 lane slots per wave that runs a
// prediction step, [14 + kernel] / [16 + kernel]: the same slots and the
// predictions run, of waves holding several CUs (autonomous, < 64 sub-blocks
// per CU) -- the lanes an iteration spends on settled CUs.  [18 ..]: the
// quadrant kernel's autonomous two-sub-block wave tasks of CUs of 32 or 64
// sub-blocks: [18] the wave-iterations that ran a prediction step, [19] those
// of them after iteration 0 whose live CUs held <= 64 sub-blocks (what the
// hand-over to one sub-block per lane can take), [20] the same at iteration 0
// (tasks with CUs outside the frame or fewer CUs than a wave holds), [21] the
// lane slots of their prediction passes (64 per pass), [22] the predictions
// run in them, [23] the wave-iterations run after a hand-over.
#ifndef VAME_COUNT_PRED
#define VAME_COUNT_PRED 0
#endif
#if VAME_COUNT_PRED
__device__ unsigned long long g_pred_count[24];
#define PC_DECL unsigned pc_n = 0, pc_w = 0, pc_mw = 0, pc_me = 0, pc2[6] = {};
#define PC_ADD                                                           \
  {                                                                      \
    pc_n++;                                                              \
    const unsigned long long m_ = __builtin_amdgcn_ballot_w64(true);     \
    if (__lane_id() == __builtin_ctzll(m_)) {                            \
      pc_w += 64;                                                        \
      if (!coop && pcLogS < 6) {                                         \
        pc_mw += 64;                                                     \
        pc_me += __popcll(m_);                                           \
      }                                                                  \
    }                                                                    \
  }
// one call per iteration of an autonomous two-sub-block quadrant wave of CUs of
// 32 or 64 sub-blocks: m_ the lanes that predict, per_ the sub-blocks each runs
#define PC2_ITER(m_, per_, iter_)                                                        \
  {                                                                                      \
    const unsigned long long l_ = (m_);                                                  \
    if (l_ && __lane_id() == __builtin_ctzll(l_)) {                                      \
      const unsigned sb_ = (unsigned)__popcll(l_) * (per_); /* live sub-blocks */        \
      pc2[0]++;                                                                          \
      if (sb_ <= 64u) pc2[(iter_) == 0 ? 2 : 1]++;                                       \
      pc2[3] += 64u * (per_);                                                            \
      pc2[4] += sb_;                                                                     \
      if ((per_) == 1) pc2[5]++;                                                         \
    }                                                                                    \
  }
#define PC_FLUSH                                                                                \
  {                                                                                             \
    if (pc_n) atomicAdd(&g_pred_count[REGION == 128], (unsigned long long)pc_n);               \
    if (pc_w) atomicAdd(&g_pred_count[12 + (REGION == 128)], (unsigned long long)pc_w);        \
    if (pc_mw) atomicAdd(&g_pred_count[14 + (REGION == 128)], (unsigned long long)pc_mw);      \
    if (pc_me) atomicAdd(&g_pred_count[16 + (REGION == 128)], (unsigned long long)pc_me);      \
    for (int i_ = 0; i_ < 6; i_++)                                                              \
      if (pc2[i_]) atomicAdd(&g_pred_count[18 + i_], (unsigned long long)pc2[i_]);              \
  }
#else
#define PC_DECL
#define PC_ADD
#define PC2_ITER(m_, per_, iter_)
#define PC_FLUSH
#endif

// VAME_PHASE_TIMING (profiling-only builds, libvame_phase.so): every wave sums
// the shader clock spent per phase and adds it to g_phase_cycles at exit.
#ifndef VAME_PHASE_TIMING
#define VAME_PHASE_TIMING 0
#endif
enum { kPhStage, kPhPredict, kPhCost, kPhGradient, kPhSolve, kPhTail, kPhReduce, kNumPhases };
#if VAME_PHASE_TIMING
// [kernel: quad, ctu, half, ctu2, half2w, half2h, quad2][phase + kNumPhases for the
// 3-CP pass; then SIMD-slot use (2), workgroups, workgroup lifetimes]
// (kPhGradient: the gradient sums; kPhReduce: the equations' reduction and
// the barrier after it)
constexpr int kPhSlots = 2 * kNumPhases + 4;
__device__ unsigned long long g_phase_cycles[7][kPhSlots];
#define PH_DECL unsigned long long ph_acc[2 * kNumPhases] = {}; unsigned long long ph_t = __builtin_amdgcn_s_memtime(); const unsigned long long ph_t0 = ph_t;
#define PH_MARK(i) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); ph_acc[(i) + ph_off] += t_ - ph_t; ph_t = t_; }
// plus SIMD-slot use: [12] = waves x block lifetime, [13] = sum of wave lifetimes
__shared__ unsigned long long s_ph_blk[3];  // min start, max end, sum of lifetimes
__shared__ int s_ph_done;
#define PH_FLUSH { \
  if (lane == 0) { \
    for (int i_ = 0; i_ < 2 * kNumPhases; i_++) atomicAdd(&g_phase_cycles[KIND][i_], ph_acc[i_]); \
    const unsigned long long t1_ = __builtin_amdgcn_s_memtime(); \
    atomicMax(&s_ph_blk[1], t1_); \
    atomicAdd(&s_ph_blk[2], t1_ - ph_t0); \
    const int nw_ = (int)(blockDim.x >> 6); \
    if (atomicAdd(&s_ph_done, 1) == nw_ - 1) { \
      atomicAdd(&g_phase_cycles[KIND][2 * kNumPhases], (unsigned long long)nw_ * (s_ph_blk[1] - s_ph_blk[0])); \
      atomicAdd(&g_phase_cycles[KIND][2 * kNumPhases + 1], s_ph_blk[2]); \
      atomicAdd(&g_phase_cycles[KIND][2 * kNumPhases + 2], 1ull); \
      atomicAdd(&g_phase_cycles[KIND][2 * kNumPhases + 3], s_ph_blk[1] - s_ph_blk[0]); \
    } \
  } }
#define PH_INIT { if (tid == 0) { s_ph_blk[0] = ~0ull; s_ph_blk[1] = 0; s_ph_blk[2] = 0; s_ph_done = 0; } }
#define PH_START { if (lane == 0) atomicMin(&s_ph_blk[0], ph_t0); }
#elif defined(VAME_ISA_MARKS)  // analysis builds: phase ends as comments in the ISA
#define PH_DECL
#define PH_MARK(i) asm volatile("; PHASE_END " #i);
#define PH_FLUSH
#define PH_INIT
#define PH_START
#else
#define PH_DECL
#define PH_MARK(i)
#define PH_FLUSH
#define PH_INIT
#define PH_START
#endif

}  // namespace vame

// vame_kernel.h -- the search kernel of the affine-ME hot path (HIP, CDNA4):
// its launch parameters, its LDS layout, the
// reduction of the normal equations, the kernel body and the kernels.  The
// device functions it is built from are in vame_dev.h, the instrumentation
// switches in vame_instr.h.  Only vame_engine.hip and vame_kernels_2cp.hip
// include this header.
//
// One workgroup = one work item, for one (POC, refIdx) pair, holding the
// candidate CUs of one or more CU-size groups over one staged reference tile:
//   affine_me_quad     a 64x64 quadrant of a CTU, 256 threads, one sub-block
//                      per lane: up to 16 wave tasks or a chain of cooperative
//                      groups;
//   affine_me_quad2    the quadrant's CUs of 32-128 sub-blocks, two vertically
//                      stacked sub-blocks per lane (in 2-CP-only launches these
//                      items run inside affine_me_quad);
//   affine_me_ctu2     one 128x128 CU per 512-thread workgroup, two sub-blocks
//                      per lane;
//   affine_me_half2 / _half2w / _half2h
//                      one 128x64 / 64x128 CU per 256-thread workgroup, two
//                      sub-blocks per lane;
//   affine_me_quad_prof / _ctu_prof / _half_prof
//                      the same search with PROF (vame_set_prof), one sub-block
//                      per lane.
// The workgroup runs the complete gradient-based CPMV refinement of
// affine.cl:195-917 for all of its CUs -- 2 control points, then 3 control
// points seeded from the 2-CP winner of the same CU (affine.cl:81-105) --
// without leaving the CU:
//   * the reference region (+16 px margin, clamp-to-edge padded) is staged
//     once into LDS; every 9x9 filter window of every iteration is read from
//     there (windows leaving the tile fall back to clamped global loads);
//   * predictions live in a CU-compact LDS buffer; gradients are computed on
//     the fly from it (no global gradient / equation scratch);
//   * each CU's normal equations are reduced as exact integer sums (14 values
//     for 2 CP, 24 moments for 3 CP) with DPP segment reductions and solved by
//     the CU's lanes with the reference's double-precision elimination,
//     operation for operation.
// Two scheduling modes per work item (chosen on the host, vame_templates.cpp):
//   autonomous  every CU has <= 64 lanes and is owned by ONE wave; each wave
//               iterates its CUs on its own (wave-local LDS ordering only, no
//               workgroup barrier inside the iteration loop);
//   cooperative larger CUs span several waves; one workgroup barrier per phase
//               and the partial sums meet in LDS int64 atomics.
// Per iteration and CU (run_pass's loop in affine_me_body; the work-item
// setup, the solve + update and the result write are functions, the other
// phases' statements are in the loop, see the comment above affine_me_body):
// predict (one lane per 4x4 sub-block: MV field, window, 6-tap H/V filter on
// v_dot2_i32_i16, SATD) -> cost (one lane per CU) -> gradient (Sobel on packed
// int16 sample pairs, CU-border replication, residual, five dot2 sums per
// sub-block) -> reduce -> solve + update (the CU's segment).
// Bit-exactness notes (SURVEY.md §8a traps): integer math is exact and
// order-free; the only float work is floor(lambda*bits) (single precision)
// and the FP64 solve (compiled with -ffp-contract=off, explicit fma where the
// reference's FP_CONTRACT=ON fuses, affine.cl:851); (int)double follows
// v_cvt_i32_f64 (NaN -> 0, saturate) explicitly.
#pragma once
#include <hip/hip_runtime.h>

#include "vame_dev.h"
#include "vame_items.h"

// VAME_RELAYOUT (compile-time, default on): the 2-CP-only launches' two-sub-block
// quadrant waves hand their last live CUs over to one sub-block per lane
// (affine_me_body, kRelay).  `make variant NAME=norelayout DEFS=-DVAME_RELAYOUT=0`
// builds the A/B partner without it.
#ifndef VAME_RELAYOUT
#define VAME_RELAYOUT 1
#endif

namespace vame {

// One (POC, refIdx) pair of a launch: the reference's kernel arguments for it
// (affine.cl:11 / :960: frames, lambda, result arrays per PRED).
struct PairArgs {
  const uint16_t* cur;
  const uint16_t* ref;
  int64_t* cost[4];           // [FULL_2CP, FULL_3CP, HALF_2CP, HALF_3CP]
  vame_cpmvs_dev* cpmv[4];
  float lambda;
  int32_t pad;
};
constexpr int kMaxPairs = 32;  // pairs per launch (kernel-argument table, 2.9 KB)

struct KParams {
  PairArgs pair[kMaxPairs];
  const vame_cpmvs_dev* prev[2];  // [align]: 3-CP seeds when the 2-CP pass is not run
  // kernels with two sub-blocks per lane (affine_me_ctu2 / _half2w / _half2h):
  // the five gradient sums of every sub-block at its CU's best 2-CP iteration
  // (3-CP seed reuse), per (pair, CTU, item): [nPairs * nCtus * nItems][5][NSB]
  // -- global, not LDS, so that two / four workgroups fit a CU
  int32_t* bestS;
  const Item* items;
  const int32_t* order;      // [nChunks][cpp]: CTU of each padded combination slot, -1 = padding
  int nItems, nCtus, nPairs;
  int groupPairs, groupPer;  // groups of the block order (see affine_me_body)
  int nChunks, cpp;          // CTU chunks per pair, padded combination slots per (pair, chunk)
  int W, H, ctusPerRow;
  int extra;
  int run2, run3;
};

// Wave priority (s_setprio) during the latency-bound solve: its dependent
// FP64 / LDS chain issues ahead of other waves' prediction work (~0.5 %;
// priority 1 / 3 and priority over the whole post-prediction part measured
// the same).
constexpr int kSolvePrio = 3;

// Per-CU refinement state.  `live` drops to 0 when the CU is out of frame or
// when an update leaves its CPMVs unchanged -- or returns them to the previous
// iteration's: the next CPMVs are a function of the current ones alone (the
// prediction, gradients and solve depend on nothing else), so the iterations
// after a fixed point or a period-2 cycle only repeat predictions and costs
// already seen (never strictly better) -- skipping them leaves the result
// bit-identical.
struct CuState {
  int32_t cur[6];
  int32_t prev[6];  // the CPMVs of the previous iteration (period-2 cycle test)
  int32_t best[6];
  int64_t bestCost;
  int64_t bestCostSnap;  // bestCost as of the iteration's start (read by every lane of the CU)
  int32_t satd;
  int32_t inframe;
  int32_t live;
  int32_t rate;      // calc_affine_bits of cur (set at init and by the update)
  int32_t bestSatd;  // 2-CP pass: SATD of the best CPMVs
  int32_t bestHasS;  // 2-CP pass: the best CPMVs' gradient sums are in s_bestS
  int32_t seedSkip;  // 3-CP pass: iteration 0 reuses the 2-CP winner's prediction
  int32_t pad;
};

// Segment sums over aligned segments of 2^LOGS lanes (LOGS <= 6; the host packs
// every wave with CUs of one size, so the segment size is wave-uniform): the
// LAST lane of every segment ends with the segment total.  row_shr steps inside
// a 16-lane DPP row, then row_bcast:15 / row_bcast:31 across rows (GFX9 DPP);
// a segment's last lane only ever adds lanes of its own segment, so no masking
// is needed.  One v_add_u32_dpp per step.
template <int LOGS>
__device__ __forceinline__ int seg_sum_c(int v) {
  if (LOGS > 0) v += dpp32<0x111, 0xF>(v);
  if (LOGS > 1) v += dpp32<0x112, 0xF>(v);
  if (LOGS > 2) v += dpp32<0x114, 0xF>(v);
  if (LOGS > 3) v += dpp32<0x118, 0xF>(v);
  if (LOGS > 4) v += dpp32<0x142, 0xA>(v);
  if (LOGS > 5) v += dpp32<0x143, 0xC>(v);
  return v;
}

// Reduction of a CU's equations over its sub-blocks (one per lane), as a
// transposing butterfly on whole int64 values (sums of |x| < 2^44 over <= 256
// lanes: exact).  The NV values of every lane are summed over the segment
// (the CU's lanes in this wave) by halving exchanges: at a step over lane bit
// b, the lanes with bit b clear keep the first half of their values and send
// the second half to the partner lane (lane ^ 2^b), which keeps the second
// half -- so each step halves the values a lane holds and doubles the lanes
// they are summed over.  Steps run cheapest first, while the counts are
// largest: bits 3 and 2 (two bank-masked DPP add pairs), bit 5
// (v_permlane32_swap), bit 4 (v_permlane16_swap), bits 1 and 0 (selects and a
// DPP quad_perm add; in practice plain row sums, the counts being 1 by then).  After the last step every value is held, fully summed, by exactly one
// lane of the segment, which stores it (autonomous items: int64 slots) or adds
// it (cooperative items: int64 LDS atomics across waves).  Integer sums: the
// order is free.

// Lane-bit selects: lane l gets (l >> B) & 1 ? if1 : if0.  Issued as the VOP3
// v_cndmask_b32 with the constant lane mask in an SGPR pair: the VOP2 form the
// compiler picks (condition in VCC) runs ~3x slower when two follow each other
// (profiles/ubench/valu_rate.hip: 7.7 vs 2.5 SIMD cycles per instruction in
// the reductions' select-select-DPP pattern).
constexpr unsigned long long kLaneBitMask[2] = {0xAAAAAAAAAAAAAAAAull, 0xCCCCCCCCCCCCCCCCull};
template <int B>
__device__ __forceinline__ int sel_bit(int if0, int if1) {
  int r;
  asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(if0), "v"(if1), "s"(kLaneBitMask[B]));
  return r;
}
template <int B>
__device__ __forceinline__ long long sel_bit64(long long if0, long long if1) {
  const int lo = sel_bit<B>((int)(unsigned long long)if0, (int)(unsigned long long)if1);
  const int hi = sel_bit<B>((int)((unsigned long long)if0 >> 32), (int)((unsigned long long)if1 >> 32));
  return (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}
// value of lane ^ 2^B for the quad bits (B < 2): DPP quad_perm
template <int B>
__device__ __forceinline__ long long partner64(long long v) {
  static_assert(B == 0 || B == 1, "quad bits only");
  constexpr int ctrl = B == 1 ? 0x4E : 0xB1;  // quad_perm [2,3,0,1] / [1,0,3,2]
  const int lo = (int)(unsigned long long)v, hi = (int)((unsigned long long)v >> 32);
  const int rl = dpp32<ctrl, 0xF>(lo), rh = dpp32<ctrl, 0xF>(hi);
  return (long long)(((unsigned long long)(unsigned)rh << 32) | (unsigned)rl);
}
// Bits 3 / 2 of the lane are bank bits of the DPP row (banks 2-3 / 1-3), so
// one exchange is two bank-masked DPP adds into the same register: the lanes
// with the bit clear get a + partner(a), the others b + partner(b) (a lane's
// DPP source reads happen before any lane writes).  Each 64-bit add is
// v_add_co / v_addc_co with DPP; the carry in VCC stays within the lanes one
// masked pair enables.  Hazard waits are explicit (the backend does not look
// inside inline asm): one s_nop 1 ahead of the block covers a DPP read of a
// register the preceding VALU instruction wrote; inside the block every DPP
// source (a's and b's halves) was written before it, so no further waits
// (round 1 waited before each of the four: c3 -1 % without them).
template <int B>
__device__ __forceinline__ long long xchg_masked64(long long a, long long b) {
  unsigned al = (unsigned)(unsigned long long)a, ah = (unsigned)((unsigned long long)a >> 32);
  const unsigned bl = (unsigned)(unsigned long long)b, bh = (unsigned)((unsigned long long)b >> 32);
  if constexpr (B == 3) {
    asm("s_nop 1\n\tv_add_co_u32_dpp %0, vcc, %0, %0 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
        "v_addc_co_u32_dpp %1, vcc, %1, %1, vcc row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
        "v_add_co_u32_dpp %0, vcc, %2, %2 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
        "v_addc_co_u32_dpp %1, vcc, %3, %3, vcc row_ror:8 row_mask:0xf bank_mask:0xc"
        : "+v"(al), "+v"(ah)
        : "v"(bl), "v"(bh)
        : "vcc");
  } else {
    static_assert(B == 2, "bank bits only");
    asm("s_nop 1\n\tv_add_co_u32_dpp %0, vcc, %0, %0 row_shl:4 row_mask:0xf bank_mask:0x5\n\t"
        "v_addc_co_u32_dpp %1, vcc, %1, %1, vcc row_shl:4 row_mask:0xf bank_mask:0x5\n\t"
        "v_add_co_u32_dpp %0, vcc, %2, %2 row_shr:4 row_mask:0xf bank_mask:0xa\n\t"
        "v_addc_co_u32_dpp %1, vcc, %3, %3, vcc row_shr:4 row_mask:0xf bank_mask:0xa"
        : "+v"(al), "+v"(ah)
        : "v"(bl), "v"(bh)
        : "vcc");
  }
  return (long long)(((unsigned long long)ah << 32) | al);
}

constexpr int ceil_half(int m) { return (m + 1) / 2; }

// Step order for a segment of 2^LOGS lanes: bits 3 2 5 4 1 0, restricted to
// bits < LOGS -- cheapest per pair-step first, while the counts are largest:
// a bank-masked DPP step (bits 3, 2) is ~11 SIMD cycles per int64 pair, a
// permlane swap step (bits 5, 4) ~14 (v_permlane32_swap issues at ~5.3
// cycles, profiles/r01_valu_rate.txt), a quad step (bits 1, 0) ~16.  The
// counts reach 1 before bits 1 / 0, which then become plain DPP row sums.
// (Round 1 ran 5 4 3 2 1 0; this order: c2 -0.6 %, c3 -0.3 %.)
template <int LOGS>
struct Schedule {
  static constexpr int bit(int i) {
    constexpr int all[6] = {3, 2, 5, 4, 1, 0};
    int n = 0;
    for (int k = 0; k < 6; k++)
      if (all[k] < LOGS) {
        if (n == i) return all[k];
        n++;
      }
    return -1;
  }
};

// One exchange of a halving step over lane bit B: a is the value the lanes
// with bit B clear keep, b the one the others keep; returns this lane's kept
// value summed with its partner's.
template <int B>
__device__ __forceinline__ long long pair_step(long long a, long long b) {
  if constexpr (B >= 4) {
    const unsigned al = (unsigned)(unsigned long long)a, ah = (unsigned)((unsigned long long)a >> 32);
    const unsigned bl = (unsigned)(unsigned long long)b, bh = (unsigned)((unsigned long long)b >> 32);
    // bit 5: lanes 0-31 end with a summed over (l, l^32), lanes 32-63 with b
    const auto rl = B == 5 ? __builtin_amdgcn_permlane32_swap(al, bl, false, false)
                           : __builtin_amdgcn_permlane16_swap(al, bl, false, false);
    const auto rh = B == 5 ? __builtin_amdgcn_permlane32_swap(ah, bh, false, false)
                           : __builtin_amdgcn_permlane16_swap(ah, bh, false, false);
    return (long long)(((unsigned long long)rh[0] << 32) | rl[0]) +
           (long long)(((unsigned long long)rh[1] << 32) | rl[1]);
  } else if constexpr (B == 3 || B == 2) {
    return xchg_masked64<B>(a, b);
  } else {
    return sel_bit64<B>(a, b) + partner64<B>(sel_bit64<B>(b, a));
  }
}
// Halving step over lane bit B on the first M values of x (the rest unused):
// afterwards x[0 .. ceil(M/2)) holds this lane's kept half.
template <int B, int M>
__device__ __forceinline__ void halve64(long long* x) {
  constexpr int H = (M + 1) / 2;
#pragma unroll
  for (int j = 0; j < H; j++) x[j] = pair_step<B>(x[j], j + H < M ? x[j + H] : 0);
}
// Runs the halving steps while the count is > 1.  A remaining segment bit
// after the count reached 1 becomes a plain sum (row_shr:2^B), valid in the
// lanes whose bit is set.
template <int LOGS, int STEP, int M>
__device__ __forceinline__ void butterfly64(long long* x) {
  if constexpr (STEP < LOGS) {
    constexpr int B = Schedule<LOGS>::bit(STEP);
    if constexpr (M > 1) {
      halve64<B, M>(x);
      butterfly64<LOGS, STEP + 1, ceil_half(M)>(x);
    } else {
      static_assert(B <= 2, "plain steps only on DPP row bits");
      const int lo = (int)(unsigned long long)x[0], hi = (int)((unsigned long long)x[0] >> 32);
      const int rl = dpp32<0x110 + (1 << B), 0xF>(lo), rh = dpp32<0x110 + (1 << B), 0xF>(hi);
      x[0] += (long long)(((unsigned long long)(unsigned)rh << 32) | (unsigned)rl);
      butterfly64<LOGS, STEP + 1, M>(x);
    }
  }
}

// Count left per lane after the schedule.
template <int LOGS, int M>
constexpr int final_count() {
  int m = M;
  for (int i = 0; i < LOGS; i++)
    if (m > 1) m = ceil_half(m);
  return m;
}

// Window of value indices a lane holds after the schedule: [off, off + count),
// valid below `limit` (the upper half of an odd count carries a zero pad).
template <int LOGS, int K>
__device__ __forceinline__ void held_window(int lidx, int& off, int& limit) {
  off = 0;
  limit = K;
  int m = K;
#pragma unroll
  for (int i = 0; i < LOGS; i++) {
    if (m <= 1) break;
    const int b = Schedule<LOGS>::bit(i);
    const int h = ceil_half(m);
    if ((lidx >> b) & 1) {
      off += h;
    } else {
      limit = off + h;
    }
    m = h;
  }
}

// Value i of a lane's contribution: its sub-block's, or with SBL = 2 the sum
// of its two (vertically stacked: same u, rows v[0], v[1]) -- integer sums, so
// adding before the reduction is exact.
template <int NCP, int SBL>
__device__ __forceinline__ long long lane_value(int i, const int (&S)[SBL][5], int u, const int (&v)[SBL]) {
  long long r = eq_value<NCP>(i, S[0], u, v[0]);
#pragma unroll
  for (int j = 1; j < SBL; j++) r += eq_value<NCP>(i, S[j], u, v[j]);
  return r;
}

template <int NCP, int LOGS, bool COOP, int SBL>
__device__ __forceinline__ void reduce_equations_64(const int (&S)[SBL][5], int u, const int (&v)[SBL], bool owner,
                                                    long long* dst) {
  constexpr int NV = NCP == 2 ? kNumVal2 : kNumMom;
  long long x[NV];
  {
    // the first halving step is fused with the values' generation: values
    // j and j + NV/2 are formed and exchanged at once, so at most half of them
    // are live (for the 24 3-CP moments this removed the 3-CP passes' spills;
    // for the 14 2-CP values it is neutral to -0.2 % since the bank-masked
    // steps run first)
    constexpr int H = ceil_half(NV);
    constexpr int B0 = Schedule<LOGS>::bit(0);
#pragma unroll
    for (int j = 0; j < H; j++)
      x[j] = pair_step<B0>(lane_value<NCP, SBL>(j, S, u, v), j + H < NV ? lane_value<NCP, SBL>(j + H, S, u, v) : 0);
    butterfly64<LOGS, 1, H>(x);
  }
  constexpr int CNT = final_count<LOGS, NV>();
  const int lidx = __lane_id() & ((1 << LOGS) - 1);
  int off, limit;
  held_window<LOGS, NV>(lidx, off, limit);
  // the plain steps' bits (after the count reached 1) must be set
  constexpr int kPlain = [] {
    int m = NV, mask = 0;
    for (int i = 0; i < LOGS; i++) {
      if (m > 1)
        m = ceil_half(m);
      else
        mask |= 1 << Schedule<LOGS>::bit(i);
    }
    return mask;
  }();
  const bool ok = owner && (lidx & kPlain) == kPlain;
  if (ok) {
#pragma unroll
    for (int j = 0; j < CNT; j++) {
      const int idx = off + j;
      if (idx < limit) {
        if constexpr (COOP)
          atomicAdd(reinterpret_cast<unsigned long long*>(&dst[idx]), (unsigned long long)x[j]);
        else
          dst[idx] = x[j];  // int64 slots
      }
    }
  }
}

template <int NCP, int SBL>
__device__ __forceinline__ void reduce_equations(const int (&S)[SBL][5], int u, const int (&v)[SBL], int logS,
                                                 bool owner, bool coop, long long* dst) {
  if (coop) {  // cooperative items: whole-wave segments, partial sums meet in LDS atomics
    reduce_equations_64<NCP, 6, true, SBL>(S, u, v, owner, dst);
    return;
  }
  switch (logS) {  // wave-uniform; autonomous waves hold CUs of 16, 32 or 64 sub-blocks
    case 4: reduce_equations_64<NCP, 4, false, SBL>(S, u, v, owner, dst); break;
    case 5: reduce_equations_64<NCP, 5, false, SBL>(S, u, v, owner, dst); break;
    default: reduce_equations_64<NCP, 6, false, SBL>(S, u, v, owner, dst); break;
  }
}


// The LDS of one work item (a kernel's workgroup), laid out for kernel class
// KIND (BEST: a 2-CP pass feeds a 3-CP pass, MODE 3).  A kernel entry declares
// it; the quadrant kernel's bodies for one and for two sub-blocks per lane
// share one (affine_me_quad).  Members ordered by alignment (no padding: four
// quadrant workgroups need <= 40,960 B each).
template <int KIND, bool BEST>
struct Lds {
  using C = Cfg<KIND>;
  static constexpr int SBL = C::SBL;
  static constexpr bool STASH = SBL == 2 && C::STASH;
  alignas(16) uint16_t tile[C::TILE_ELEMS];
  uint4 coef[48];
  long long val[C::MAXCU][kNumMom];
  double mat[C::MAXCU][42];  // per CU: N x (N + 1) system, N <= 6
  CuState st[C::MAXCU];
  // row 0 / row 3 of every lane's prediction (packed pairs): of its sub-block,
  // or with two stacked sub-blocks per lane (SBL = 2) the upper one's top and
  // the lower one's bottom row (their inner rows stay in the lane)
  uint2 top[C::THREADS];
  uint2 bot[C::THREADS];
  // SBL = 2: the upper sub-block's prediction, parked in LDS from its SATD to
  // the gradient step (row r of lane t at [r][t]), so the lower one's
  // prediction runs with no extra live registers
  uint2 pred[STASH ? 4 : 1][STASH ? C::THREADS : 1];
  CuSlot cu[C::ITEMCU];
  // the five gradient sums of every sub-block at its CU's best 2-CP iteration
  // (3-CP seed reuse, see the 3-CP init); SBL = 2 keeps them in p.bestS
  int bestS[5][SBL == 1 && BEST ? C::NSB : 1];
  int hdr[2];  // item header, next wave task to claim
  uint8_t eqmap[76];  // EqMap entries 0..73
};

// ------------------------------------------------------------ work-item setup
// What the phases of a work item share, all wave-uniform: its (POC, refIdx)
// pair, its CTU and the tile staged for it.
struct ItemCtx {
  const Item* it;
  const uint16_t* ref;
  const uint16_t* cur;
  int W, H;
  int pairIdx, itemIdx, ctu, ctuX, ctuY;
  int tx0, ty0;      // tile origin (frame)
  int tileW, tileH;  // the staged extent
  bool regionOut;    // the region lies wholly outside the frame: nothing staged, nothing predicted
};

// XCD-aware block -> (group, item, ctu, pair).  A group is groupPairs
// pairs x one chunk of CTU rows (a working set of a few hundred (ctu, pair)
// combinations that the XCDs' L2s hold: at 1080p three whole pairs, at 2160p
// part of one); within a group the order is item-major: all (ctu, pair)
// blocks of template item 0 first, then item 1, ...; the host lists the
// costlier items first, so the tail is made of short workgroups.  Each
// (pair, chunk) has cpp combination slots, a multiple of 8, so slot j runs
// on XCD j % 8 (blocks are dealt round-robin over the 8 XCDs) for every item
// and pair: the items of one CTU re-read its reference tile and original
// samples from the same L2, and the host's slot -> CTU table (`order`) gives
// each XCD a compact strip of CTUs, so neighbouring tiles' margins come from
// that L2 too.  False for a padding slot (uniform: the workgroup exits at
// once, before any barrier).
template <int KIND>
__device__ __forceinline__ bool locate_item(const KParams& p, ItemCtx& w) {
  using C = Cfg<KIND>;
  const int b = blockIdx.x;
  const int gsz = p.nItems * p.groupPer;
  const int grp = b / gsz, gr = b % gsz;
  w.itemIdx = gr / p.groupPer;
  const int rest = gr % p.groupPer;
  w.pairIdx = (grp / p.nChunks) * p.groupPairs + rest / p.cpp;  // (POC, refIdx) pair of this launch
  if (w.pairIdx >= p.nPairs) return false;
  w.ctu = p.order[(grp % p.nChunks) * p.cpp + rest % p.cpp];
  if (w.ctu < 0) return false;
  w.it = p.items + w.itemIdx;
  w.ref = p.pair[w.pairIdx].ref;
  w.cur = p.pair[w.pairIdx].cur;
  w.W = p.W;
  w.H = p.H;
  w.ctuX = (w.ctu % p.ctusPerRow) * kCtu;
  w.ctuY = (w.ctu / p.ctusPerRow) * kCtu;
  // the region origin is read with scalar loads, so the reference tile's loads
  // are in flight together with the item's descriptor loads (one latency
  // round), and one barrier publishes both
  w.tx0 = w.ctuX + (int)w.it->rx - C::MARGIN;
  w.ty0 = w.ctuY + (int)w.it->ry - C::MARGIN;
  w.regionOut = w.tx0 + C::MARGIN >= w.W || w.ty0 + C::MARGIN >= w.H;
  // the staged extent: the whole square tile, or (affine_me_half) the CU's
  // region + margin, a 160 x 96 or 96 x 160 part of the square storage
  w.tileW = KIND == kKindHalf ? (int)w.it->rw + 2 * C::MARGIN : C::TILE_W;
  w.tileH = KIND == kKindHalf ? (int)w.it->rh + 2 * C::MARGIN : C::TILE_H;
  return true;
}

// The reference region (+margin) on its way into LDS, clamp-to-edge padded,
// in 16-byte chunks, kStagePer of them per thread: stage_load reads them from
// the frame into registers, stage_store writes them to the tile.  A region
// wholly outside the frame (the bottom CTU row at 1080p) has no in-frame CU:
// nothing is predicted, its tile is never read.
template <int KIND>
constexpr int kStagePer =
    (Cfg<KIND>::TILE_H * (Cfg<KIND>::TILE_W / 8) + Cfg<KIND>::THREADS - 1) / Cfg<KIND>::THREADS;
template <int KIND>
__device__ __forceinline__ void stage_load(const ItemCtx& w, int tid, uint4 (&tv)[kStagePer<KIND>]) {
  using C = Cfg<KIND>;
  const int CPR = w.tileW / 8;  // chunks per tile row
  const int NCH = w.tileH * CPR;
  if (w.regionOut) return;
#pragma unroll
  for (int j = 0; j < kStagePer<KIND>; j++) {
    const int ch = tid + j * C::THREADS;
    if (ch < NCH) {
      const int ty = ch / CPR, cx = (ch % CPR) * 8;
      const int fy = clampi(w.ty0 + ty, 0, w.H - 1), fx = w.tx0 + cx;
      const uint16_t* row = w.ref + (size_t)fy * w.W;
      if (fx >= 0 && fx + 7 < w.W) {
        tv[j] = *reinterpret_cast<const uint4*>(row + fx);
      } else {
        unsigned a[8];
#pragma unroll
        for (int m = 0; m < 8; m++) a[m] = row[clampi(fx + m, 0, w.W - 1)];
        tv[j] = make_uint4(a[0] | (a[1] << 16), a[2] | (a[3] << 16), a[4] | (a[5] << 16),
                           a[6] | (a[7] << 16));
      }
    }
  }
}
template <int KIND>
__device__ __forceinline__ void stage_store(const ItemCtx& w, int tid, const uint4 (&tv)[kStagePer<KIND>],
                                            uint16_t* s_tile) {
  using C = Cfg<KIND>;
  const int CPR = w.tileW / 8;
  const int NCH = w.tileH * CPR;
  if (w.regionOut) return;
#pragma unroll
  for (int j = 0; j < kStagePer<KIND>; j++) {
    const int ch = tid + j * C::THREADS;
    if (ch < NCH) *reinterpret_cast<uint4*>(&s_tile[(ch / CPR) * C::TP + (ch % CPR) * 8]) = tv[j];
  }
}

// The item's descriptors and the tables every phase reads from LDS: writes
// s_cu, s_coef, s_eqmap and s_hdr, zeroes s_val.
template <int KIND>
__device__ __forceinline__ void publish_item(const Item* it, int tid, CuSlot* s_cu, uint4* s_coef,
                                             uint8_t* s_eqmap, int* s_hdr, long long* s_val) {
  using C = Cfg<KIND>;
  if (tid < C::ITEMCU) s_cu[tid] = it->cu[tid];
  if (tid < 48) s_coef[tid] = reinterpret_cast<const uint4*>(&kCoefTab)[tid];
  if (tid < 76) s_eqmap[tid] = kEqMap.v[tid];
  if (tid == 0) {
    s_hdr[0] = it->coop | (it->nTasks << 16);
    s_hdr[1] = 4;  // tasks 0 .. 3: waves 0 .. 3
  }
  for (int i = tid; i < C::MAXCU * kNumMom; i += C::THREADS) s_val[i] = 0;
}

// A task's lanes: the task's wave-uniform values and the lane's place in it
// (fixed for the task).
struct TaskCtx {
  int tid, lane, wv;
  int cuB, cuE;  // the CU slots [cuB, cuE) of this wave's task (uniform)
  int logL;      // log2 lanes per CU
  int logS;      // log2 of the segment: the lanes of one CU in one wave
  int nCuW;      // lanes of this wave doing per-CU work
  int myCu;      // the lane's CU slot, or -1
  int local;     // the lane's sub-block (raster order in its CU)
  int sbIdx;     // its prediction rows in s_top / s_bot / s_pred / s_bestS
  int sx, sy;    // its sub-block's position in the CU (SBL = 2: the upper one's)
  int sbCols;    // sub-block columns of the CU
  bool active;   // the CU lies inside the frame (affine.cl:192-193)
  bool leader;   // last lane of its segment: holds the segment sums
  Geo g;
};
// Reads the task's slots in s_cu (slots 0 .. of a cooperative item, the
// wave's own slots wv * kTaskCu .. of an autonomous one).
template <int KIND>
__device__ __forceinline__ TaskCtx task_lanes(const ItemCtx& w, int tid, bool coop, const CuSlot* s_cu) {
  constexpr int SBL = Cfg<KIND>::SBL;
  TaskCtx t;
  t.tid = tid;
  t.lane = tid & 63;
  t.wv = tid >> 6;
  const int lidx = coop ? tid : t.lane;
  const CuSlot t0 = s_cu[coop ? 0 : t.wv * kTaskCu];
  int cuB = coop ? 0 : t.wv * kTaskCu;
  int cuE = cuB + t0.taskCus;
  int logL = t0.taskLogL;
  t.cuB = __builtin_amdgcn_readfirstlane(cuB);
  t.cuE = __builtin_amdgcn_readfirstlane(cuE);
  t.logL = __builtin_amdgcn_readfirstlane(logL);
  t.logS = min(t.logL, 6);
  t.nCuW = coop ? (t.wv == 0 ? t.cuE : 0) : t.cuE - t.cuB;
  const int kLane = t.cuB + (lidx >> t.logL);
  t.myCu = kLane < t.cuE ? kLane : -1;
  t.g.x = t.g.y = t.g.lw = t.g.lh = t.g.w = t.g.h = 0;
  t.local = lidx & ((1 << t.logL) - 1);
  t.sbIdx = 0;
  t.sx = 0;
  t.sy = 0;
  t.sbCols = 1;
  t.active = false;
  if (t.myCu >= 0) {
    const CuSlot cs = s_cu[t.myCu];
    t.g.lw = cs.lw;
    t.g.lh = cs.lh;
    t.g.w = 1 << t.g.lw;
    t.g.h = 1 << t.g.lh;
    t.g.x = w.ctuX + cs.x;
    t.g.y = w.ctuY + cs.y;
    // the lane's own prediction rows: a task's CUs take consecutive lanes
    // (of the workgroup, or of the running wave), in raster order within
    // each (SBL = 2: a lane per column and pair of sub-block rows, its two
    // sub-blocks at sy and sy + 4)
    t.sbIdx = tid;
    t.sbCols = 1 << (t.g.lw - 2);
    t.sx = (t.local & (t.sbCols - 1)) << 2;
    t.sy = (t.local >> (t.g.lw - 2)) << (SBL == 2 ? 3 : 2);
    t.active = (t.g.x + t.g.w <= w.W) && (t.g.y + t.g.h <= w.H);  // affine.cl:192-193
  }
  t.leader = t.myCu >= 0 && (t.lane & ((1 << t.logS) - 1)) == (1 << t.logS) - 1;
  return t;
}

// The hand-over of an autonomous two-sub-block task whose live CUs (liveCus:
// bit k for slot cuB + k) together hold <= 64 sub-blocks: the wave's lanes
// take them one sub-block per lane (relayout_lane, vame_items.h), each live CU
// an aligned segment of its 32 or 64 sub-blocks in raster order; the CUs keep
// their slots, so their state, moments and systems stay where they are.  The
// lane's prediction rows (sbIdx) are the wave's own as before, the rows above
// and below now sbCols lanes away in both s_top and s_bot.
__device__ __forceinline__ void relayout_task(const ItemCtx& w, unsigned liveCus, const CuSlot* s_cu, TaskCtx& t) {
  const int logNsb = t.logL + 1;
  const RelayoutLane rl = relayout_lane((int)__lane_id(), liveCus, logNsb);
  t.logL = t.logS = logNsb;
  t.myCu = rl.cu < 0 ? -1 : t.cuB + rl.cu;
  t.local = rl.sb;
  t.sbIdx = t.myCu >= 0 ? t.tid : 0;  // (a lane without a CU so far had none)
  t.g.x = t.g.y = t.g.lw = t.g.lh = t.g.w = t.g.h = 0;
  t.sx = 0;
  t.sy = 0;
  t.sbCols = 1;
  t.active = t.myCu >= 0;  // a live CU lies inside the frame
  if (t.myCu >= 0) {
    const CuSlot cs = s_cu[t.myCu];
    t.g.lw = cs.lw;
    t.g.lh = cs.lh;
    t.g.w = 1 << t.g.lw;
    t.g.h = 1 << t.g.lh;
    t.g.x = w.ctuX + cs.x;
    t.g.y = w.ctuY + cs.y;
    t.sbCols = 1 << (t.g.lw - 2);
    t.sx = (t.local & (t.sbCols - 1)) << 2;
    t.sy = (t.local >> (t.g.lw - 2)) << 2;
  }
  t.leader = t.myCu >= 0 && (t.lane & ((1 << logNsb) - 1)) == (1 << logNsb) - 1;
}

// The next task's CU slots into this task's (lane li < kTaskCu of the
// workgroup or of the wave copies slot li to dstBase + li): reads and writes
// s_cu.  Cooperative: after every wave's last read of them; autonomous: the
// wave's own, read by this wave only.
template <int KIND>
__device__ __forceinline__ void take_task_slots(int next, int li, int dstBase, CuSlot* s_cu) {
  if (li < kTaskCu) s_cu[dstBase + li] = s_cu[min(next, Cfg<KIND>::ITEMCU / kTaskCu - 1) * kTaskCu + li];
}

// ------------------------------------------------------------------- phases
// Small pieces the phases' statements (and their timing-only second runs) share.
__device__ __forceinline__ int seg_sum(int logS, int v) {  // logS is wave-uniform: 4, 5 or 6
  return logS == 4 ? seg_sum_c<4>(v) : logS == 5 ? seg_sum_c<5>(v) : seg_sum_c<6>(v);
}
// ext_row with the neighbour columns fetched by DPP (wave_shr:1 / wave_shl:1)
__device__ __forceinline__ uint4 ext_row_dpp(const uint2& p) {
  return ext_row(p, dpp32<0x138, 0xF>((int)p.y), dpp32<0x130, 0xF>((int)p.x));
}
// row_newbcast:7 -- the value of lane 7 of each DPP row, in every lane of the row
__device__ __forceinline__ int bcast_lane7(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x157, 0xF, 0xF, false); }

// The lane's extended rows (SBL = 1: neighbour columns by DPP into X[1..4];
// SBL = 2: the gradient phase forms the extended rows of both sub-blocks) and
// its edge rows, published for the sub-blocks above and below: writes
// s_top[idx] and s_bot[idx].
template <int SBL>
__device__ __forceinline__ void publish_rows(const uint2 (&Pr)[SBL][4], int idx, uint2* s_top, uint2* s_bot,
                                             uint4 (&X)[6]) {
  if constexpr (SBL == 1) {
#pragma unroll
    for (int r = 0; r < 4; r++) X[r + 1] = ext_row_dpp(Pr[0][r]);
  }
  s_top[idx] = Pr[0][0];
  s_bot[idx] = Pr[SBL - 1][3];
}

// The edge rows of the sub-blocks above and below lane idx's: reads s_bot / s_top.
template <int THREADS>
__device__ __forceinline__ void edge_rows(int idx, int sbCols, const uint2* s_top, const uint2* s_bot, uint2& tb,
                                          uint2& bt) {
  tb = s_bot[max(idx - sbCols, 0)];
  bt = s_top[min(idx + sbCols, THREADS - 1)];
}

// affine.cl:860-893 on the first eight lanes of a CU's segment, one CPMV
// component per lane: lane loc < 2 ncp applies the update to its component
// (deltas in M: LT = (d0, d2), RT = (d1, d3), LB = (d4, d5); 2 CP: LB stays
// (0, 0)) -- cj its value so far, v the new one -- and lane 7 ends with the
// lane sum f: bits 0-3 the components that moved, bits 4-7 those that differ
// from the previous iteration's, bits 8.. the rate of the new CPMVs
// (calc_affine_bits, aux_functions.cl:2140-2189), which rides on the same
// sum: component j codes q_j - q_(j & 1) for j >= 2 (RT - LT from lane j - 2,
// LB - LT from lane j - 4).  Reads M and st; stores nothing.
template <int ncp, bool STORE>
__device__ __forceinline__ int update_lanes(int loc, const double* M, CuState& st, int cx, int cy, int W, int H) {
  int f = 0, q = 0;
  if (loc < 2 * ncp) {
    const int j = loc;
    const double d = M[j == 1 ? 2 : j == 2 ? 1 : j];
    const int cj = st.cur[j], pj = st.prev[j];
    const int v = update_cpmv(cj, d, (j & 1) ? cy : cx, (j & 1) ? H : W);
    f = (v != cj ? 1 : 0) | (v != pj ? 16 : 0);
    if constexpr (STORE) {
      st.prev[j] = cj;
      st.cur[j] = v;
    }
    q = to_quarter(v);
  }
  const int q2 = dpp32<0x112, 0xF>(q), q4 = dpp32<0x114, 0xF>(q);
  if (loc < 2 * ncp) f += eg_bits(q - (loc >= 4 ? q4 : loc >= 2 ? q2 : 0)) << 8;
  f += dpp32<0x111, 0xF>(f);  // row_shr:1, 2, 4: lane 7 sums lanes 0..7
  f += dpp32<0x112, 0xF>(f);
  f += dpp32<0x114, 0xF>(f);
  return f;
}

// Solve + CPMV update (affine.cl:782-893), per CU segment: the CU's lanes in
// its first wave solve its system together (reads s_val[cu], s_eqmap; s_mat[cu]
// is scratch and ends holding the deltas), then its first eight lanes update
// the CPMVs: writes s_st[cu] cur, prev, live, rate (keepS, cooperative: also
// the next cost phase's bestCostSnap and a fresh satd).  Returns, in the CU's
// lane 7, whether the CU stays live.
template <int ncp, bool coop, bool keepS, int kDup>
__device__ __forceinline__ bool solve_update_phase(const ItemCtx& w, const TaskCtx& t, const CuSlot* s_cu,
                                                   CuState* s_st, long long (*s_val)[kNumMom], double (*s_mat)[42],
                                                   const uint8_t* s_eqmap) {
  int cuS = t.myCu, loc = t.local;
  opaque(cuS);  // recomputed, not loop-carried (VGPRs)
  opaque(loc);
  const bool solver = cuS >= 0 && loc < 64;
  const bool act = solver && s_st[cuS].live;
  const int Ls = 1 << t.logS;
  double dd[6] = {0, 0, 0, 0, 0, 0};
  long long* V = s_val[cuS < 0 ? 0 : cuS];
  double* M = s_mat[cuS < 0 ? 0 : cuS];
  const CuSlot cs = s_cu[cuS < 0 ? 0 : cuS];
  if constexpr ((kDup & 16) != 0) {  // timing-only: a throw-away solve first
    // on M itself, keeping V: the real solve below rebuilds M from V (no
    // extra LDS, so the occupancy is the product build's)
    double dd2[6] = {0, 0, 0, 0, 0, 0};
    double* M2 = M;
    seg_solve<ncp, true>(V, M2, s_eqmap, loc, Ls, act, coop, cs.lw, cs.lh, dd2);
    asm volatile("" ::"v"(dd2[0]), "v"(dd2[1]), "v"(dd2[3]));
    wave_sync();
  }
  seg_solve<ncp>(V, M, s_eqmap, loc, Ls, act, coop, cs.lw, cs.lh, dd);
  if (keepS && coop && solver && loc == 7) {  // the next cost phase's view; fresh SATD sums
    CuState& st = s_st[cuS];
    st.bestCostSnap = st.bestCost;
    st.satd = 0;
  }
  const int cx = w.ctuX + cs.x, cy = w.ctuY + cs.y;
  if constexpr ((kDup & 2048) != 0) {  // timing-only: the update again, without its stores
    if (act && loc < 8) {
      int l2 = loc;
      opaque(l2);
      const int f2 = update_lanes<ncp, false>(l2, M, s_st[cuS], cx, cy, w.W, w.H);
      asm volatile("" ::"v"(f2));
    }
  }
  bool liveNew = false;
  if (act && loc < 8) {
    CuState& st = s_st[cuS];
    const int f = update_lanes<ncp, true>(loc, M, st, cx, cy, w.W, w.H);
    if (loc == 7) {
      // moved, and not back to the previous (flag fields: bits 0-3 and 4-7)
      liveNew = (f & 15) != 0 && ((f >> 4) & 15) != 0;
      st.live = liveNew;
      st.rate = f >> 8;
    }
  }
  return liveNew;
}

// Whether a CU of the task is still live: reads s_st (after the sync that
// follows the update).
__device__ __forceinline__ bool any_cu_live(const TaskCtx& t, const CuState* s_st) {
  bool anyLive = false;
  for (int k = t.cuB; k < t.cuE; k++) anyLive |= s_st[k].live != 0;
  return anyLive;
}

// Results (affine.cl:928-957), one lane per CU of the task: reads s_st and
// s_cu, writes the pair's cost and CPMV arrays.
template <int ncp>
__device__ __forceinline__ void write_results(const PairArgs& pa, const ItemCtx& w, const TaskCtx& t,
                                              const CuSlot* s_cu, const CuState* s_st) {
  if (t.lane >= t.nCuW) return;
  int k = __lane_id();  // == lane, recomputed: not a spilled loop-carried copy
  opaque(k);
  k += t.cuB;
  const CuState& st = s_st[k];
  const CuSlot cs = s_cu[k];
  const int mode = cs.align * 2 + (ncp - 2);
  const size_t idx = (size_t)w.ctu * (cs.align ? kHalfCusPerCtu : kFullCusPerCtu) + cs.outOff;
  pa.cost[mode][idx] = st.bestCost;
  vame_cpmvs_dev o;
  o.ncps = ncp;
  o.ltx = st.best[0]; o.lty = st.best[1]; o.rtx = st.best[2];
  o.rty = st.best[3]; o.lbx = st.best[4]; o.lby = st.best[5];
  pa.cpmv[mode][idx] = o;
}

// MODE (one kernel per launch mode, so each holds only the pass copies it
// runs): 1 = 2-CP only, 2 = 3-CP only (seeds from p.prev), 3 = 2-CP then 3-CP.
// L: the work item's LDS (Lds<KIND>, or a layout that holds it).
// Functions of their own: the work-item setup (locate_item, stage_load /
// stage_store, publish_item, task_lanes), solve + update (solve_update_phase),
// the result write (write_results), the task hand-over's copy
// (take_task_slots) and the small pieces above.  The init of the CPMVs, the
// prediction, the cost / best step, the gradient sums and the equations'
// reduction are statements of run_pass's loop: as functions they change some
// kernels' scratch bytes (profiles/search_body_refactor_ab.txt).  Every barrier, phase
// mark, priority change and loop exit is in the loop itself.
template <int KIND, bool PROF, int MODE, typename L>
__device__ __forceinline__ void affine_me_body(const KParams& p, L& lds) {
  constexpr bool run2 = (MODE & 1) != 0, run3 = (MODE & 2) != 0;
  using C = Cfg<KIND>;
  constexpr int REGION = C::REGION;  // instrumentation slots: 128 = the 128-class kernels
  (void)REGION;
  static_assert((C::TP * 2) % 16 == 0 && C::TILE_W % 8 == 0, "16-byte tile rows");
  constexpr int SBL = C::SBL;
  constexpr bool STASH = SBL == 2 && C::STASH;
  using Own = Lds<KIND, run2 && run3>;  // the layout this body needs: L's arrays are at least as large
  static_assert(sizeof(L::tile) >= sizeof(Own::tile) && sizeof(L::top) >= sizeof(Own::top) &&
                    sizeof(L::bestS) >= sizeof(Own::bestS) && sizeof(L::pred) >= sizeof(Own::pred) &&
                    sizeof(L::val) >= sizeof(Own::val) && sizeof(L::mat) >= sizeof(Own::mat) &&
                    sizeof(L::st) >= sizeof(Own::st) && sizeof(L::cu) >= sizeof(Own::cu),
                "LDS layout too small for this kernel class");
  uint16_t* s_tile = lds.tile;
  uint2* s_top = lds.top;
  uint2* s_bot = lds.bot;
  auto& s_bestS = lds.bestS;
  auto& s_pred = lds.pred;
  auto& s_val = lds.val;
  auto& s_mat = lds.mat;
  uint4* s_coef = lds.coef;
  uint8_t* s_eqmap = lds.eqmap;
  CuState* s_st = lds.st;
  CuSlot* s_cu = lds.cu;
  int* s_hdr = lds.hdr;
  __shared__ long long s_dup[(VAME_DUP & 4) ? kNumMom : 1];  // timing-only builds

  const int tid = threadIdx.x;
  [[maybe_unused]] const int lane = tid & 63;  // (the phase-timing macros)
  const int wv = tid >> 6;
  constexpr int ph_off = 0;  // phase-timing slots (3-CP pass: +kNumPhases)
  (void)ph_off;
  PH_DECL
  PC_DECL

  ItemCtx w;
  if (!locate_item<KIND>(p, w)) return;
  const PairArgs& pa = p.pair[w.pairIdx];
  // the item's values under the names the loop's statements use (every one is
  // used there; reading w.* / t.* directly in the loop instead moves
  // affine_me_half_prof<3>'s scratch from 24 to 28 B)
  const uint16_t* __restrict__ ref = w.ref;
  const uint16_t* __restrict__ cur = w.cur;
  const int W = w.W, H = w.H, ctu = w.ctu, ctuX = w.ctuX, ctuY = w.ctuY, pairIdx = w.pairIdx, itemIdx = w.itemIdx;
  const int tx0 = w.tx0, ty0 = w.ty0, tileW = w.tileW, tileH = w.tileH;
  // ---- stage the tile and publish the item: one barrier for both
  uint4 tv[kStagePer<KIND>];
  if constexpr ((VAME_DUP & 64) != 0) {  // timing-only: one extra staging round trip
    int tid2 = tid;
    opaque(tid2);
    stage_load<KIND>(w, tid2, tv);
    stage_store<KIND>(w, tid2, tv, s_tile);
    __syncthreads();
  }
  stage_load<KIND>(w, tid, tv);
  publish_item<KIND>(w.it, tid, s_cu, s_coef, s_eqmap, s_hdr, &s_val[0][0]);
  PH_INIT
  stage_store<KIND>(w, tid, tv, s_tile);
  __syncthreads();
  PH_START
  const int hdr = __builtin_amdgcn_readfirstlane(s_hdr[0]);
  const int nTasks = (hdr >> 16) & 0xFF;
  const bool coop = C::COOP && (!C::AUTO || (hdr & 1) != 0);
  const bool claim = C::AUTO && (hdr & 2) != 0;  // autonomous: waves claim tasks as they finish
  PH_MARK(kPhStage)
  if (!coop && wv >= nTasks) {  // wave-uniform: an autonomous wave without CUs
    PH_FLUSH
    return;
  }

  // Tasks over the one staged tile: a cooperative item's tasks one after
  // another, an autonomous wave's tasks wv, wv + 4, ... (or, claiming, wv
  // and then the next unclaimed task when it finishes).  Each task's CU slots
  // are first moved into slots 0 .. (cooperative) or the wave's own slots
  // wv * kTaskCu .. (autonomous: its CU state, moments and systems; its
  // sub-blocks use the wave's own prediction rows, so its tasks need no
  // workgroup barrier).
  const int tidItem = tid;
  for (int task = coop ? 0 : __builtin_amdgcn_readfirstlane(wv);;) {
    // the thread's ids re-derived per task (opaque): as values carried
    // around the task loop, everything computed from them was hoisted out of
    // it and held in spill slots, whose writes reached HBM
    int tidTask = tidItem;
    opaque(tidTask);
    TaskCtx t = task_lanes<KIND>(w, tidTask, coop, s_cu);
    // the task's values under the names the loop's statements use (the lane's
    // place in the task changes only at a hand-over, see relayout_task)
    const int tid = t.tid, lane = t.lane, wv = t.wv, cuB = t.cuB, nCuW = t.nCuW;
    int sbIdx = t.sbIdx, logS = t.logS, myCu = t.myCu, local = t.local, sx = t.sx, sy = t.sy, sbCols = t.sbCols;
    bool active = t.active, leader = t.leader;
    Geo g = t.g;
    [[maybe_unused]] const int pcLogS = t.logS;  // (the prediction counters)
    // one copy of the pass per CP count and item class: ncp and coop are
    // compile-time constants in each, so the 2-CP pass carries none of the 3-CP
    // selects and branches, and each copy keeps its spills outside its loops
    auto run_pass = [&](auto ncpTag, auto coopTag, auto keepTag) {
      constexpr int ncp = decltype(ncpTag)::value;
      constexpr bool coop = decltype(coopTag)::value;
      constexpr bool keepS = decltype(keepTag)::value;  // 2-CP pass that feeds a 3-CP pass
      constexpr int ph_off = ncp == 3 ? kNumPhases : 0;
      (void)ph_off;
      constexpr int kDup = (VAME_DUP & 32) && ncp != 3 ? 0 : VAME_DUP;  // timing-only builds
      const int niter = (ncp == 3 ? 4 : 5) + p.extra;
      // The hand-over (2-CP-only launches' two-sub-block quadrant tasks): once
      // the task's live CUs hold <= 64 sub-blocks the wave finishes the task
      // one sub-block per lane (relayout_task) -- one prediction, rows and
      // gradient pass per iteration instead of two half-empty ones.  Nothing
      // per lane outlives an iteration but its place in the task: the CU state,
      // the moments and the system are in LDS, the predictions are formed anew
      // from the tile and the equation sums are exact integers, so the
      // results do not depend on the layout.
      constexpr bool kRelay = VAME_RELAYOUT && KIND == kKindQuad2 && MODE == 1 && ncp == 2 && !coop;
      [[maybe_unused]] bool relaid = false;  // wave-uniform: this task runs one sub-block per lane

      // ---- per-CU initial CPMVs (2 CP: zero; 3 CP: derived from the 2-CP winner)
      if (lane < nCuW) {
        int k = __lane_id();  // == lane, recomputed: not a spilled loop-carried copy
        opaque(k);
        k += cuB;
        const CuSlot cs = s_cu[k];
        CuState& st = s_st[k];
        const int cx = ctuX + cs.x, cy = ctuY + cs.y;
        int c[6] = {0, 0, 0, 0, 0, 0};
        if (ncp == 3) {
          int prev[4];
          if (run2) {
            for (int i = 0; i < 4; i++) prev[i] = st.best[i];
          } else {
            const vame_cpmvs_dev& pv =
                p.prev[cs.align][(size_t)ctu * (cs.align ? kHalfCusPerCtu : kFullCusPerCtu) + cs.outOff];
            prev[0] = pv.ltx; prev[1] = pv.lty; prev[2] = pv.rtx; prev[3] = pv.rty;
          }
          // affine.cl:81-105
          int lbx, lby;
          derive_lb(prev[0], prev[1], prev[2], prev[3], cs.lw, cs.lh, cx, cy, W, H, lbx, lby);
          c[0] = prev[0]; c[1] = prev[1]; c[2] = prev[2]; c[3] = prev[3]; c[4] = lbx; c[5] = lby;
          // Seed reuse (exact): when the derived LB reproduces the 2-CP motion
          // field -- (LB - LT) << (7 - log2 h) == (-(RT - LT).y, (RT - LT).x)
          // << (7 - log2 w), i.e. no rounding or clipping in the derivation
          // (always so for square CUs) -- iteration 0's MV field, spread test,
          // prediction and gradients are those of the 2-CP winner, whose SATD
          // and per-sub-block gradient sums the 2-CP pass kept.  Iteration 0
          // then only re-prices the rate and rebuilds the 6-parameter equations.
          int skip = 0, satd0 = 0;
          if (run2 && st.bestHasS) {
            const int hx = shl(prev[2] - prev[0], 7 - cs.lw), hy = shl(prev[3] - prev[1], 7 - cs.lw);
            const int vx = shl(lbx - prev[0], 7 - cs.lh), vy = shl(lby - prev[1], 7 - cs.lh);
            if (vx == -hy && vy == hx) {
              skip = 1;
              satd0 = st.bestSatd;
            }
          }
          st.seedSkip = skip;
          st.satd = satd0;
        } else {
          st.satd = 0;
          st.bestHasS = 0;
        }
        // fresh constants (opaque): as loop-carried values the compiler kept
        // them in spill slots, whose scratch traffic reached HBM
        int never = (int)0x80000000;  // outside the clamped CPMV range: never matches
        int costInit = (int)kCostInit;
        opaque(never);
        opaque(costInit);
        for (int i = 0; i < 6; i++) {
          st.cur[i] = c[i];
          st.prev[i] = never;
          st.best[i] = c[i];
        }
        st.bestCost = (long long)costInit;
        st.bestCostSnap = (long long)costInit;
        st.rate = affine_bits(c, ncp);
        st.inframe = (cx + (1 << cs.lw) <= W) && (cy + (1 << cs.lh) <= H);
        st.live = st.inframe;
      }
      phase_sync(coop);

      for (int iter = 0; iter <= niter; iter++) {
        // =============== prediction + SATD (affine.cl:208-393) ===============
        // Everything a lane produces here is only read while its CU is live
        // (the CU's lanes are uniformly live or not), so the whole step runs
        // under `live`: the DPP neighbour reads at the CU's edges may see lanes
        // of other CUs, whose columns the border replication discards.
        // this lane's prediction and original rows (packed pairs), per sub-block
        // (SBL = 2: the originals are read again in the gradient step)
        uint2 Pr[SBL][4], Og[SBL][4];
        uint4 X[6];          // extended rows 0..3 (X[1..4]) and the neighbours' edges
        const bool live = active && s_st[myCu < 0 ? 0 : myCu].live;
        // 3-CP iteration 0 of a seed-reuse CU: SATD (set at init) and gradient
        // sums come from the 2-CP pass
        const bool reuse = ncp == 3 && iter == 0 && s_st[myCu < 0 ? 0 : myCu].seedSkip;
#if VAME_COUNT_PRED
        if constexpr (KIND == kKindQuad2 && ncp == 2) {
          if (!coop && pcLogS < 6) PC2_ITER(__builtin_amdgcn_ballot_w64(live), relaid ? 1u : 2u, iter)
        }
#endif
        if (live && !reuse && !(VAME_ABLATE & 8)) {
          PC_ADD
          Geo gp = g;
          int sxp = sx, syp = sy;
          opaque_geo(gp, sxp, syp);  // recomputed per phase (not hoisted: VGPRs)
          int cp[6];
          for (int i = 0; i < 6; i++) cp[i] = s_st[myCu].cur[i];
          const MvField f = mv_field(cp, ncp, gp.lw, gp.lh);
          if constexpr ((kDup & 128) != 0) {  // timing-only: the MV field again
            int cp2[6];
            for (int i = 0; i < 6; i++) cp2[i] = cp[i];
            int lw2 = gp.lw;
            opaque(cp2[0]);
            opaque(lw2);
            const MvField f2 = mv_field(cp2, ncp, lw2, gp.lh);
            if (ncp == 3)
              asm volatile("" ::"v"(f2.bx), "v"(f2.by), "v"(f2.hx), "v"(f2.hy), "v"(f2.vx), "v"(f2.vy),
                           "v"((int)f2.spread));
            else
              asm volatile("" ::"v"(f2.bx), "v"(f2.by), "v"(f2.hx), "v"(f2.hy), "v"((int)f2.spread));
          }
          int satdLane = 0;
#pragma unroll
          for (int j = 0; j < SBL; j++) {
            if (kRelay && j > 0 && relaid) break;  // uniform: one sub-block per lane
            bool outside;
            satdLane += predict_sb<C::TILE, C::TP, PROF, (VAME_ABLATE & 1024) != 0 && ncp == 3, ncp>(
                f, sxp, syp + 4 * j, gp, s_tile, tx0, ty0, tileW - 9, tileH - 9, ref, cur, W, H, s_coef, Pr[j],
                Og[j], outside);
            if (SBL == 2 && j == 0) {
#pragma unroll
              for (int r = 0; r < 4; r++)
                if constexpr (STASH) s_pred[r][sbIdx] = Pr[0][r];
            }
#if VAME_COUNT_PRED
            {  // instrumentation: windows outside the tile, per kernel and pass, one atomic per wave
              const unsigned long long out = __builtin_amdgcn_ballot_w64(outside);
              if (out && __lane_id() == __builtin_ctzll(__builtin_amdgcn_ballot_w64(true)))
                atomicAdd(&g_pred_count[2 + 2 * (REGION == 128) + (ncp == 3)], (unsigned long long)__popcll(out));
            }
            if (j > 0) PC_ADD
#endif
          }
          if (kDup & 1) {
            MvField f2 = f;
            opaque(f2.bx);
            uint2 P2[4], O2[4];
            bool out2;
            int s2 = predict_sb<C::TILE, C::TP, PROF>(f2, sxp, syp, gp, s_tile, tx0, ty0, tileW - 9, tileH - 9,
                                                      ref, cur, W, H, s_coef, P2, O2, out2);
            s2 += (int)(P2[0].x ^ P2[3].y ^ O2[1].x);
            asm volatile("" ::"v"(s2));
          }
          // extended rows (neighbour columns by DPP), edge rows published for
          // the sub-blocks above and below (SBL = 2: the gradient step forms
          // the extended rows of both sub-blocks)
          if (kRelay && relaid) {  // the one sub-block's own top and bottom row
            s_top[sbIdx] = Pr[0][0];
            s_bot[sbIdx] = Pr[0][3];
          } else {
            publish_rows<SBL>(Pr, sbIdx, s_top, s_bot, X);
          }
          if constexpr ((kDup & 256) != 0) {  // timing-only: the extended rows and edge stores again
            int i2 = sbIdx;
            opaque(i2);
            uint2 Q[SBL][4];
#pragma unroll
            for (int j = 0; j < SBL; j++)
#pragma unroll
              for (int r = 0; r < 4; r++) {
                Q[j][r] = Pr[j][r];
                opaque(reinterpret_cast<int&>(Q[j][r].x));
              }
            uint4 X2[6];
            publish_rows<SBL>(Q, i2, s_top, s_bot, X2);
            if constexpr (SBL == 1) {
#pragma unroll
              for (int r = 0; r < 4; r++) asm volatile("" ::"v"(X2[r + 1].x), "v"(X2[r + 1].w));
            }
          }
          if constexpr ((kDup & 512) != 0) {  // timing-only: the SATD segment sum again
            int s2 = satdLane;
            opaque(s2);
            const int v2 = seg_sum(logS, s2);
            asm volatile("" ::"v"(v2));
          }
          const int v = seg_sum(logS, satdLane);
          if (leader) {
            if (coop)
              atomicAdd(&s_st[myCu].satd, v);
            else
              s_st[myCu].satd = v;
          }
        }
        phase_sync(coop);
        PH_MARK(kPhPredict)

        // =============== cost, best update (affine.cl:416-457) ===============
        // The cost is the SATD sum plus floor(lambda * (bits + 2)), the rate
        // bits of the current CPMVs (calc_affine_bits, aux_functions.cl:2140-
        // 2189) kept in CuState by the update step; the strict best is kept.
        const bool lastIter = iter == niter;
        bool better = false;  // keepS: this lane's CU improved
        if constexpr ((kDup & 1024) != 0) {  // timing-only: the pricing again (before the real one)
          int bet2 = 0;
          if (myCu >= 0 && (keepS || local == 7)) {
            const CuState& st = s_st[myCu];
            int r2 = st.rate;
            opaque(r2);
            if (iter == 0 || st.live) bet2 = price(st.satd, pa.lambda, r2) < st.bestCost;
          }
          if (!keepS) bet2 = bcast_lane7(bet2);
          asm volatile("" ::"v"(bet2));
        }
        if constexpr (!keepS) {
          // the CU's lane 7 prices and keeps the best; lanes 0-5 copy the CPMVs
          int bet = 0;
          if (myCu >= 0 && local == 7) {
            CuState& st = s_st[myCu];
            if (iter == 0 || st.live) {
              const long long cost = price(st.satd, pa.lambda, st.rate);
              if (cost < st.bestCost) {
                st.bestCost = cost;
                bet = 1;
              }
            }
            st.satd = 0;
          }
          bet = bcast_lane7(bet);
          if (myCu >= 0 && local < 6 && bet) s_st[myCu].best[local] = s_st[myCu].cur[local];
        } else {
          // 2-CP pass followed by a 3-CP pass: every lane of the CU prices it, so
          // each knows whether its CU improved and keeps its gradient sums for
          // the 3-CP seed reuse.  The comparison is against the best cost as of
          // the iteration's start: autonomous items read bestCost (the CU's
          // lanes are one wave, whose LDS reads precede lane 7's write);
          // cooperative items read bestCostSnap, refreshed in the solve phase.
          if (myCu >= 0) {
            CuState& st = s_st[myCu];
            if (iter == 0 || st.live) {
              const long long cost = price(st.satd, pa.lambda, st.rate);
              better = cost < (coop ? st.bestCostSnap : st.bestCost);
              if (better && local == 7) {
                st.bestCost = cost;
                st.bestSatd = st.satd;
                st.bestHasS = !lastIter && st.live;  // its gradient sums follow in this iteration
              }
            }
            if (local < 6 && better) st.best[local] = st.cur[local];
          }
        }
        PH_MARK(kPhCost)
        if (lastIter) {  // uniform; the results below are written by other lanes
          phase_sync(coop);
          break;
        }

        // =============== gradients + normal equations (affine.cl:477-752) ===============
        {
          int S[SBL][5];
#pragma unroll
          for (int j = 0; j < SBL; j++)
#pragma unroll
            for (int k = 0; k < 5; k++) S[j][k] = 0;
          // SBL = 2: the seed-reuse sums in global memory, per (pair, CTU): a
          // uniform base and 32-bit lane offsets (recomputed, not hoisted)
          char* gBest = SBL == 2 ? reinterpret_cast<char*>(p.bestS + ((size_t)(pairIdx * p.nCtus + ctu) * p.nItems +
                                                                      itemIdx) * 5 * C::NSB)
                                 : nullptr;
          auto gbest = [&](int k, int j) -> int32_t& {
            int i = sbIdx;
            opaque(i);
            return *reinterpret_cast<int32_t*>(gBest + (unsigned)(k * C::NSB + j * C::THREADS + i) * 4u);
          };
          if (reuse && live) {
#pragma unroll
            for (int j = 0; j < SBL; j++)
#pragma unroll
              for (int k = 0; k < 5; k++) S[j][k] = SBL == 1 ? s_bestS[k][sbIdx] : gbest(k, j);
          } else if (live && !(VAME_ABLATE & 2)) {
            // the neighbours' edge rows, extended by the left / right lanes' copies
            // the sub-blocks above / below, computed here (kept live across the
            // passes, the index was spilled)
            int nbIdx = sbIdx;
            if constexpr (SBL == 2) opaque(nbIdx);  // recomputed, not hoisted (VGPRs)
            uint2 tb, bt;
            edge_rows<C::THREADS>(nbIdx, sbCols, s_top, s_bot, tb, bt);
            X[0] = ext_row_dpp(tb);
            if constexpr ((kDup & 256) != 0) {  // timing-only: the neighbours' edge rows again
              int n2 = nbIdx;
              opaque(n2);
              uint2 tb2, bt2;
              edge_rows<C::THREADS>(n2, sbCols, s_top, s_bot, tb2, bt2);
              const uint4 a2 = ext_row_dpp(tb2), b2 = ext_row_dpp(bt2);
              asm volatile("" ::"v"(a2.x), "v"(a2.w), "v"(b2.x), "v"(b2.w));
            }
            Geo gg = g;
            int sxg = sx, syg = sy;
            if constexpr (SBL == 2) opaque_geo(gg, sxg, syg);
            if constexpr (SBL == 1) {
              X[5] = ext_row_dpp(bt);
              grad_sb(sxg, syg, gg, X, Og[0], S[0]);
            } else {
              // upper sub-block: rows X[1..4] its own, X[5] the lower one's top row;
              // lower sub-block: X[0] the upper one's bottom row, X[5] the lane
              // below's; the original rows read again (the frame base + 32-bit offsets)
#pragma unroll
              for (int j = 0; j < SBL; j++) {
                if (STASH && j == 0) {
#pragma unroll
                  for (int r = 0; r < 4; r++) Pr[0][r] = s_pred[r][sbIdx];
                }
#pragma unroll
                for (int r = 0; r < 4; r++)
                  X[r + 1] = ext_row_dpp(Pr[j][r]);
                const bool below = j + 1 < SBL && !(kRelay && relaid);  // the row below is the lane's own
                X[5] = ext_row_dpp(below ? Pr[j + 1 < SBL ? j + 1 : j][0] : bt);
                {
                  const unsigned b0 = (unsigned)((gg.y + syg + 4 * j) * W + gg.x + sxg) * 2u, bw = (unsigned)W * 2u;
                  const char* base = reinterpret_cast<const char*>(cur);
#pragma unroll
                  for (int r = 0; r < 4; r++) Og[j][r] = *reinterpret_cast<const uint2*>(base + (b0 + (unsigned)r * bw));
                }
                grad_sb(sxg, syg + 4 * j, gg, X, Og[j], S[j]);
                if (kRelay && relaid) break;  // uniform: one sub-block per lane
                if (j + 1 < SBL) X[0] = X[4];  // the lower sub-block's row above = the upper one's row 3
              }
            }
            if (kDup & 2) {
              int S2[5];
              int sxd = sxg;
              opaque(sxd);
              grad_sb(sxd, syg, gg, X, Og[0], S2);
              asm volatile("" ::"v"(S2[0] ^ S2[1] ^ S2[2] ^ S2[3] ^ S2[4]));
            }
            if (keepS && better && !(SBL == 2 && (VAME_ABLATE & 2048))) {  // the best iteration's sums, for the 3-CP seed reuse
#pragma unroll
              for (int j = 0; j < SBL; j++)
#pragma unroll
                for (int k = 0; k < 5; k++) {
                  if constexpr (SBL == 1)
                    s_bestS[k][sbIdx] = S[j][k];
                  else
                    gbest(k, j) = S[j][k];
                }
            }
          }
          PH_MARK(kPhGradient)
          if (!(VAME_ABLATE & 4)) {
            long long* dst = s_val[myCu < 0 ? 0 : myCu];
            int va[SBL];
#pragma unroll
            for (int j = 0; j < SBL; j++) va[j] = sy + 2 + 4 * j;
            if (kRelay && relaid) {  // the one sub-block's values alone
              int S1[1][5], v1[1] = {va[0]};
#pragma unroll
              for (int k = 0; k < 5; k++) S1[0][k] = S[0][k];
              reduce_equations<2, 1>(S1, sx + 2, v1, logS, myCu >= 0, coop, dst);
            } else if (ncp == 2)
              reduce_equations<2, SBL>(S, sx + 2, va, logS, myCu >= 0, coop, dst);
            else
              reduce_equations<3, SBL>(S, sx + 2, va, logS, myCu >= 0, coop, dst);
            if constexpr ((kDup & 4) != 0) {
              int ud = sx + 2;
              opaque(ud);
              if (ncp == 2)
                reduce_equations<2, SBL>(S, ud, va, logS, myCu >= 0, coop, s_dup);
              else
                reduce_equations<3, SBL>(S, ud, va, logS, myCu >= 0, coop, s_dup);
            }
          }
        }
        phase_sync(coop);
        PH_MARK(kPhReduce)

        // =============== solve + CPMV update (affine.cl:782-893), per CU segment ===============
        __builtin_amdgcn_s_setprio(kSolvePrio);
        if (!(VAME_ABLATE & 1)) {
          const bool liveNew = solve_update_phase<ncp, coop, keepS, kDup>(w, t, s_cu, s_st, s_val, s_mat, s_eqmap);
          if (!coop) {
            const unsigned long long liveBal = __ballot(liveNew);  // lane 7 of every CU that stays live
            if (liveBal == 0) {
              __builtin_amdgcn_s_setprio(0);
              break;
            }
            if constexpr (kRelay) {
              // the hand-over: CUs of 32 or 64 sub-blocks (16 or 32 lanes each so
              // far), not handed over yet, the live ones fitting the wave's lanes
              if (!relaid && t.logL < 6 && (__popcll(liveBal) << (t.logL + 1)) <= 64) {
                unsigned liveCus = 0;
                for (int k = 0; k < (64 >> t.logL); k++)
                  liveCus |= (unsigned)((liveBal >> ((k << t.logL) + 7)) & 1) << k;
                relayout_task(w, liveCus, s_cu, t);
                sbIdx = t.sbIdx; logS = t.logS; myCu = t.myCu; local = t.local; sx = t.sx; sy = t.sy; sbCols = t.sbCols;
                active = t.active; leader = t.leader; g = t.g;
                relaid = true;
              }
            }
          }
        }
        __builtin_amdgcn_s_setprio(0);
        phase_sync(coop);
        PH_MARK(kPhSolve)
        if (coop && !any_cu_live(t, s_st)) break;
      }
      // =============== results (affine.cl:928-957) ===============
      write_results<ncp>(pa, w, t, s_cu, s_st);
      phase_sync(coop);
      PH_MARK(kPhTail)
    };
    using I2 = std::integral_constant<int, 2>;
    using I3 = std::integral_constant<int, 3>;
    using T = std::true_type;
    using F = std::false_type;
    // keepS: the 2-CP pass feeds a 3-CP pass (seed reuse)
    using KeepS = std::integral_constant<bool, run3>;
    if (C::COOP && coop) {
      if constexpr (C::COOP) {
        if constexpr (run2) run_pass(I2{}, T{}, KeepS{});
        if constexpr (run3) run_pass(I3{}, T{}, F{});
      }
    } else {
      if constexpr (run2) run_pass(I2{}, F{}, KeepS{});
      if constexpr (run3) run_pass(I3{}, F{}, F{});
    }
    if (!C::QUAD) break;  // 128-class items: one task
    // the next task's CU slots into this task's (cooperative: after every wave's
    // last read of them, autonomous: the wave's own, read by this wave only)
    int next = task + (coop ? 1 : 4);
    if (claim) {
      int v = 0;
      if (lane == 0) v = atomicAdd(&s_hdr[1], 1);
      next = __builtin_amdgcn_readfirstlane(v);
    }
    if (next >= nTasks) break;
    if (coop) {
      take_task_slots<KIND>(next, tid, 0, s_cu);
      __syncthreads();
    } else if constexpr (VAME_RELAYOUT && KIND == kKindQuad2 && MODE == 1) {
      // the wave's slot base re-derived (opaque): carried from the task's
      // start past the hand-over's code it took a spill slot
      int tidEnd = tidItem;
      opaque(tidEnd);
      take_task_slots<KIND>(next, tidEnd & 63, (tidEnd >> 6) * kTaskCu, s_cu);
      wave_sync();
    } else {
      take_task_slots<KIND>(next, lane, wv * kTaskCu, s_cu);
      wave_sync();
    }
    task = next;
  }
  PH_FLUSH
  PC_FLUSH
}

// Distinct entry points so profiles tell the work-item classes apart.
// Quadrant items: 4 workgroups per CU fit the LDS (~36-41 KB each), so cap the
// VGPRs at 128 to let all 16 waves be resident.  An item flagged SBL2 (Item
// coop bit 2: the CUs of 32-128 sub-blocks) runs the body with two stacked
// sub-blocks per lane, the others (16-sub-block and 64x64 CUs) with one; both
// bodies share the workgroup's LDS (one Lds<kKindQuad, ...>).
__device__ __forceinline__ bool quad_item_sbl2(const KParams& p) {
  const int b = blockIdx.x;
  const int gr = b % (p.nItems * p.groupPer);
  return (p.items[gr / p.groupPer].coop & 4) != 0;
}
//
// Which launch modes hand affine_me_quad SBL2 items (the engine's launch
// plan): only the 2-CP-only launches; in the others the SBL2 items go to
// affine_me_quad2 and affine_me_quad is built without the two-sub-block body,
// whose registers would otherwise spill into the one-sub-block body too
// (104 vs 0 B per lane in MODE 3).
template <int MODE>
constexpr bool kQuadMerged = MODE == 1;
template <int MODE>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(4))) void affine_me_quad(
    KParams p) {
  __shared__ Lds<kKindQuad, MODE == 3> lds;
  if constexpr (kQuadMerged<MODE>) {
    if (quad_item_sbl2(p)) {
      affine_me_body<kKindQuad2, false, MODE>(p, lds);
      return;
    }
  }
  affine_me_body<kKindQuad, false, MODE>(p, lds);
}
// The SBL2 items as a kernel of their own (MODE 2 and 3).
template <int MODE>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(4))) void affine_me_quad2(
    KParams p) {
  __shared__ Lds<kKindQuad2, MODE == 3> lds;
  affine_me_body<kKindQuad2, false, MODE>(p, lds);
}
// ONE 128x128 CU per 512-thread workgroup, two stacked sub-blocks per lane,
// two workgroups per CU (~72 KB of LDS each; the 3-CP seed-reuse sums in
// global memory): 128 VGPRs so both fit.
template <int MODE>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4))) void affine_me_ctu2(KParams p) {
  __shared__ Lds<kKindCtu2, MODE == 3> lds;
  affine_me_body<kKindCtu2, false, MODE>(p, lds);
}
// ONE 128x64 (w) / 64x128 (h) CU per 256-thread workgroup, two stacked
// sub-blocks per lane, four workgroups per CU (~40 KB of LDS each).
template <int MODE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void affine_me_half2w(KParams p) {
  __shared__ Lds<kKindHalf2W, MODE == 3> lds;
  affine_me_body<kKindHalf2W, false, MODE>(p, lds);
}
template <int MODE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void affine_me_half2h(KParams p) {
  __shared__ Lds<kKindHalf2H, MODE == 3> lds;
  affine_me_body<kKindHalf2H, false, MODE>(p, lds);
}
// Both orientations in one launch (an item's region width tells which), so
// the 128x64 and 64x128 CUs run side by side instead of one kernel after the
// other on the stream; the 64x128 layout's LDS holds the 128x64 one's.  MODE
// 1 only: with 3-CP the two bodies in one kernel spill (88 vs 20 B per lane).
template <int MODE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void affine_me_half2(KParams p) {
  __shared__ Lds<kKindHalf2H, MODE == 3> lds;
  const int gr = blockIdx.x % (p.nItems * p.groupPer);
  const Item& it = p.items[gr / p.groupPer];
  if (it.rw > it.rh)
    affine_me_body<kKindHalf2W, false, MODE>(p, lds);
  else
    affine_me_body<kKindHalf2H, false, MODE>(p, lds);
}
// The same with PROF (vame_set_prof): the quadrant items (one sub-block per
// lane, every quadrant CU); the 128x128 CU in one 1024-thread workgroup per
// CU (~100 KB of LDS), one lane per sub-block; each 128x64 / 64x128 CU in a
// 512-thread workgroup, two per CU (~74 KB of LDS each).
template <int MODE>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(4))) void affine_me_quad_prof(
    KParams p) {
  __shared__ Lds<kKindQuad, MODE == 3> lds;
  affine_me_body<kKindQuad, true, MODE>(p, lds);
}
template <int MODE>
__global__ __launch_bounds__(1024) void affine_me_ctu_prof(KParams p) {
  __shared__ Lds<kKindCtu, MODE == 3> lds;
  affine_me_body<kKindCtu, true, MODE>(p, lds);
}
template <int MODE>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4))) void affine_me_half_prof(KParams p) {
  __shared__ Lds<kKindHalf, MODE == 3> lds;
  affine_me_body<kKindHalf, true, MODE>(p, lds);
}

// The 2-CP-only (MODE 1) product kernels are compiled in a translation unit of
// their own, vame_kernels_2cp.hip, whose optimisation flags suit them (the
// Makefile); the engine's unit declares them instead of
// instantiating them.  They are the MODE 1 kernels the engine launches: the
// split kernels (affine_me_quad2, affine_me_half2w / _half2h) have no MODE 1
// instance.  Instrumentation builds keep every kernel in one unit: their
// device counters are per unit.
#if VAME_COUNT_PRED || VAME_PHASE_TIMING
#define VAME_SPLIT_TU 0
#else
#define VAME_SPLIT_TU 1
#endif
#define VAME_2CP_KERNELS(X)                 \
  X template __global__ void affine_me_quad<1>(KParams);   \
  X template __global__ void affine_me_ctu2<1>(KParams);   \
  X template __global__ void affine_me_half2<1>(KParams);

}  // namespace vame

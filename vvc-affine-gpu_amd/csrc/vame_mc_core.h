// vame_mc_core.h -- what the prediction-side units share (vame_mc.hip,
// vame_bipred.hip, vame_birefine.hip; vame_partition.hip for the descriptors):
// the CU descriptors and their validity rule, the concatenation of the valid
// descriptors' sub-blocks (scan, count, offsets, launch), and one hypothesis:
// the search's prediction of a 4x4 sub-block from CPMVs up to its second-stage
// accumulators, bit-exact with predict_sb (vame_dev.h) (DESIGN.md §11, §13,
// §14).
//
// What is here is what could move without changing the code the compiler
// emits for the predict and refine kernels (their device assembly equals that
// of the open-coded form, so their speed is settled by comparison).  Left in
// the kernels for that reason, each a few lines whose extraction re-schedules
// the kernel around it: the descriptor lookup, the reference select, the block
// load / store, the coefficient staging, birefine_kernel's composition of the
// validity predicates, and mc_predict_kernel's own copy of the hypothesis
// (a hypothesis function there costs the PROF instance a wave of occupancy).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "vame_dev.h"

namespace vame {

// ---------------------------------------------------------------- descriptors
// device view of vame_mc_cu (include/vame.h): 12 int32
struct McCu {
  int32_t x, y, w, h, ref;
  int32_t ncps, ltx, lty, rtx, rty, lbx, lby;
};
// device view of vame_mc_bicu (include/vame.h): 20 int32; the first 12 are a McCu
struct McBiCu {
  int32_t x, y, w, h, ref0;
  int32_t ncps0, c0[6];  // LTx, LTy, RTx, RTy, LBx, LBy
  int32_t ref1;          // -1: uni-predicted from (ref0, c0)
  int32_t ncps1, c1[6];
};
static_assert(sizeof(McCu) == 48, "vame_mc_cu layout");
static_assert(sizeof(McBiCu) == 80, "vame_mc_bicu layout");

constexpr int kMcMaxCus = 1 << 20;  // VAME_MC_MAX_CUS
// int32 words of a context's scratch table: the offsets of kMcMaxCus
// descriptors and the total, then the sums of the 1024 scan blocks
constexpr size_t kMcScratchWords = (size_t)kMcMaxCus + 1 + 1024;
constexpr int kMcScanBlock = 1024;  // descriptors per scan block (one per thread)
constexpr int kMcThreads = 256;     // prediction workgroups
constexpr int kMcMaxBlocks = 2048;  // prediction grid (grid-strided beyond it)
static_assert(kMcMaxCus <= kMcScanBlock * kMcScanBlock, "two scan levels");

// The parameter block of vame_affine_mc (Cu = McCu) and vame_affine_mc_bi
// (Cu = McBiCu); MVP: of vame_affine_mc_bi_p, the same block and the predictors
// (DESIGN.md §17).  The kernels of the calls without predictors are the MVP =
// false instances: they take the block they always took and hold no predictor
// code.
template <class Cu, bool MVP = false>
struct McParamsT {
  const uint16_t* cur;      // NULL when cost is
  const uint16_t* refs[4];
  const Cu* cus;
  uint16_t* pred;           // or NULL
  int64_t* cost;            // or NULL
  int32_t* bad;
  int32_t* offs;            // [ncus + 1]: first sub-block of each descriptor; the total
  int32_t* blockSum;        // [1024]: sub-blocks per scan block
  int ncus, nrefs, W, H;
  float lambda;
  // vame_affine_mc_dev, vame_affine_mc_bi: the count lives on the device,
  // clamped to [0, ncus] (ncus sizes the grids); NULL: the count is ncus
  const int32_t* ncusDev;
};
template <class Cu>
struct McParamsT<Cu, true> : McParamsT<Cu, false> {
  const int32_t* preds;  // vame_cpmvs (7 int32), two per bi descriptor: hypothesis h of descriptor i at 2i + h
};
using McParams = McParamsT<McCu>;
using McBiParams = McParamsT<McBiCu>;
using McBiParamsP = McParamsT<McBiCu, true>;
// The three launches of one vame_affine_mc / vame_affine_mc_bi call on
// `stream` (ncus >= 1).
hipError_t mc_launch(const McParams& p, bool prof, hipStream_t stream);
hipError_t mc_bi_launch(const McBiParams& p, hipStream_t stream);
hipError_t mc_bi_p_launch(const McBiParamsP& p, hipStream_t stream);

// ------------------------------------------------------------------- validity
__device__ __forceinline__ bool mc_size_ok(int v) { return v == 16 || v == 32 || v == 64 || v == 128; }
__device__ __forceinline__ bool mc_mv_ok(int v) { return v >= kMvMin && v <= kMvMax; }
__device__ __forceinline__ bool mc_cp_ok(int ncps, const int32_t (&c)[6]) {
  bool ok = (ncps == 2 || ncps == 3) && mc_mv_ok(c[0]) && mc_mv_ok(c[1]) && mc_mv_ok(c[2]) && mc_mv_ok(c[3]);
  if (ncps == 3) ok = ok && mc_mv_ok(c[4]) && mc_mv_ok(c[5]);
  return ok;
}
// What both kinds share: the CU's rectangle in the frame and the first
// hypothesis (a reference the call holds, 2 or 3 CPMVs in range).
__device__ __forceinline__ bool mc_hyp0_ok(int x, int y, int w, int h, int ref, int ncps, const int32_t (&c)[6],
                                           int W, int H, int nrefs) {
  bool ok = mc_size_ok(w) && mc_size_ok(h) && x >= 0 && y >= 0 && ((x | y) & 3) == 0;
  ok = ok && x <= W - w && y <= H - h;  // after the size test: no overflow
  return ok && ref >= 0 && ref < nrefs && mc_cp_ok(ncps, c);
}
__device__ __forceinline__ bool mc_cu_ok(const McCu& cu, int W, int H, int nrefs) {
  const int32_t c[6] = {cu.ltx, cu.lty, cu.rtx, cu.rty, cu.lbx, cu.lby};
  return mc_hyp0_ok(cu.x, cu.y, cu.w, cu.h, cu.ref, cu.ncps, c, W, H, nrefs);
}
__device__ __forceinline__ bool mc_cu_ok(const McBiCu& cu, int W, int H, int nrefs) {
  bool ok = mc_hyp0_ok(cu.x, cu.y, cu.w, cu.h, cu.ref0, cu.ncps0, cu.c0, W, H, nrefs);
  ok = ok && cu.ref1 >= -1 && cu.ref1 < nrefs;
  if (cu.ref1 >= 0) ok = ok && mc_cp_ok(cu.ncps1, cu.c1);
  return ok;
}

// --------------------------------------------------------------- predictors
// A predictor (vame_cpmvs: nCPs, which is ignored, then LT, RT, LB) is valid
// when all six components lie within [kMvMin, kMvMax], whatever the model of
// the hypothesis it prices; an invalid one makes its descriptor invalid.
constexpr int kMvpWords = 7;
__device__ __forceinline__ bool mvp_ok(const int32_t* P) {
  bool ok = true;
#pragma unroll
  for (int k = 1; k < kMvpWords; k++) ok = ok && mc_mv_ok(P[k]);
  return ok;
}
// The predictors of descriptor i: one for a uni descriptor (McCu), two for a
// bi descriptor, the second not read when ref1 < 0.
__device__ __forceinline__ bool mvp_cu_ok(const McCu&, const int32_t* preds, int i) {
  return mvp_ok(preds + (size_t)i * kMvpWords);
}
__device__ __forceinline__ bool mvp_cu_ok(const McBiCu& cu, const int32_t* preds, int i) {
  const int32_t* P = preds + (size_t)i * 2 * kMvpWords;
  return mvp_ok(P) && (cu.ref1 < 0 || mvp_ok(P + kMvpWords));
}

// ------------------------------------------------- sub-block concatenation
// The descriptors of a call: `cap`, or the device-side count clamped to [0, cap].
__device__ __forceinline__ int mc_ncus(const int32_t* ncusDev, int cap) {
  return ncusDev ? min(max(*ncusDev, 0), cap) : cap;
}

// Sum over the workgroup's 1024 threads: the exclusive prefix of `v` in thread
// order (return value) and the total (every thread).
__device__ __forceinline__ int block_scan_1024(int v, int* s_wave, int& total) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int up = __shfl_up(incl, d, 64);
    if (lane >= d) incl += up;
  }
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < kMcScanBlock / 64; w++) {
    const int s = s_wave[w];
    if (w < wave) before += s;
    all += s;
  }
  total = all;
  return before + incl - v;
}

// Validate each descriptor, count its sub-blocks (0 for an invalid one), zero
// its cost, flag `bad`; exclusive scan of the counts inside the scan block.
template <class Cu, bool MVP = false>
__global__ __launch_bounds__(kMcScanBlock) void mc_count_kernel(McParamsT<Cu, MVP> p) {
  __shared__ int s_wave[kMcScanBlock / 64];
  const int i = blockIdx.x * kMcScanBlock + threadIdx.x;
  const int ncus = mc_ncus(p.ncusDev, p.ncus);
  int n = 0;
  bool flag = false;
  if (i < ncus) {
    const Cu cu = p.cus[i];
    bool ok = mc_cu_ok(cu, p.W, p.H, p.nrefs);
    if constexpr (MVP) ok = ok && mvp_cu_ok(cu, p.preds, i);
    n = ok ? (cu.w * cu.h) >> 4 : 0;
    flag = !ok;
    if (p.cost) p.cost[i] = 0;
  }
  const unsigned long long m = __builtin_amdgcn_ballot_w64(flag);
  if (m && (int)__lane_id() == __builtin_ctzll(m)) atomicOr(p.bad, 1);
  int total;
  const int excl = block_scan_1024(n, s_wave, total);
  if (i < ncus) p.offs[i] = excl;
  if (threadIdx.x == 0) p.blockSum[blockIdx.x] = total;
}

// offs[i] += the counts of the scan blocks before i's (at most 1024 of them:
// one per thread, summed by the workgroup); the last block writes the total.
// It reads no descriptor: Cu only names the call's parameter block, so that the
// kernel keeps the arguments it had (two identical instantiations, one per unit).
template <class Cu, bool MVP = false>
__global__ __launch_bounds__(kMcScanBlock) void mc_offsets_kernel(McParamsT<Cu, MVP> p) {
  __shared__ int s_wave[kMcScanBlock / 64];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int ncus = mc_ncus(p.ncusDev, p.ncus);
  int base;
  block_scan_1024(tid < b ? p.blockSum[tid] : 0, s_wave, base);
  const int i = b * kMcScanBlock + tid;
  if (i < ncus) p.offs[i] += base;
  // scan blocks past a device-side count hold no sub-blocks
  if (b == (int)gridDim.x - 1 && tid == 0) p.offs[ncus] = base + p.blockSum[b];
}

// Count, offsets and `predict` (the unit's kernel, grid-strided over the
// concatenation) on `stream`.
template <class Cu, bool MVP>
hipError_t mc_launch_concat(const McParamsT<Cu, MVP>& p, void (*predict)(McParamsT<Cu, MVP>), hipStream_t stream) {
  const int nb = (p.ncus + kMcScanBlock - 1) / kMcScanBlock;
  hipLaunchKernelGGL((mc_count_kernel<Cu, MVP>), dim3(nb), dim3(kMcScanBlock), 0, stream, p);
  hipLaunchKernelGGL((mc_offsets_kernel<Cu, MVP>), dim3(nb), dim3(kMcScanBlock), 0, stream, p);
  // at most 1024 sub-blocks per descriptor: 4 workgroups
  const int grid = (int)std::min<long long>(4ll * p.ncus, kMcMaxBlocks);
  hipLaunchKernelGGL(predict, dim3(grid), dim3(kMcThreads), 0, stream, p);
  return hipGetLastError();
}

// ------------------------------------------------------------- small pieces
// Sum over the 16 lanes of a DPP row, in every lane of the row.
__device__ __forceinline__ int row_sum16(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true);   // quad_perm:[1,0,3,2]
  v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, true);   // quad_perm:[2,3,0,1]
  v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, true);  // row_half_mirror
  v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, true);  // row_mirror
  return v;
}

// ----------------------------------------------------------------- hypothesis
// One prediction of the search for the sub-block at (sx, sy) of the CU
// (x, y, 2^lw, 2^lh), up to the rounding shift: sub-block MV and spread test
// (affine.cl:215-252), roundAndClipMv against the CU position, clamp-to-edge
// window (affine.cl:254-326), the 6-tap two-stage filter (aux_functions.cl:
// 1096-1239) into acc = sum + 512 + (8192 << 6), whose uni sample is
// clampi(acc >> 10, 0, 1023).  Every load is clamped to the frame, whatever the
// CPMVs hold.
__device__ __forceinline__ void mc_hyp_acc(const uint16_t* __restrict__ ref, int x, int y, int lw, int lh,
                                           const int (&cp)[6], int ncps, int sx, int sy, int W, int H,
                                           const uint4* s_coef, int (&acc)[4][4]) {
  const MvField f = mv_field(cp, ncps, lw, lh);
  const int px = f.spread ? (1 << (lw - 1)) : sx + 2, py = f.spread ? (1 << (lh - 1)) : sy + 2;
  // |h|, |v| <= 2^21 (components within [-2^17, 2^17), << (7 - log2 size)),
  // px, py <= 128: the 24-bit products are exact
  int mx = f.bx + __mul24(f.hx, px) + __mul24(f.vx, py);
  int my = f.by + __mul24(f.hy, px) + __mul24(f.vy, py);
  mx = (mx + 64 - (mx >= 0)) >> 7;  // roundMv (aux_functions.cl:38-47)
  my = (my + 64 - (my >= 0)) >> 7;
  // clipMv (aux_functions.cl:51-67) on the frame position of the MV's target, as predict_sb
  const int ax = clampi(mx + shl(x, 4), -135 * 16, (W + 7) * 16);
  const int ay = clampi(my + shl(y, 4), -135 * 16, (H + 7) * 16);
  const int fx = ax & 15, fy = ay & 15;
  const int wx = (ax >> 4) + sx - 2, wy = (ay >> 4) + sy - 2;  // window origin (frame)
  const uint4 KA = s_coef[fx * 3], KB = s_coef[fx * 3 + 1];  // even window start: parity-0 taps
#pragma unroll
  for (int r = 0; r < 4; r++)
#pragma unroll
    for (int c = 0; c < 4; c++) acc[r][c] = 524800;  // (1 << 9) + (8192 << 6)
  filter_rows_global(ref, wx, wy, W, H, KA, KB, reinterpret_cast<const unsigned*>(s_coef), fy, acc);
}

// The bi sample of two hypotheses, clampi((a + b) >> 11, 0, 1023): the sum of
// the unrounded second-stage values, rounded once; packed rows.  With a == b
// it is the uni sample: (2 * acc) >> 11 == acc >> 10.
__device__ __forceinline__ void mc_bi_pack(const int (&a)[4][4], const int (&b)[4][4], uint2 (&P)[4]) {
#pragma unroll
  for (int r = 0; r < 4; r++) {
    int s[4];
#pragma unroll
    for (int c = 0; c < 4; c++) s[c] = clampi((a[r][c] + b[r][c]) >> 11, 0, 1023);
    P[r] = make_uint2(pack16(s[0], s[1]), pack16(s[2], s[3]));
  }
}

}  // namespace vame

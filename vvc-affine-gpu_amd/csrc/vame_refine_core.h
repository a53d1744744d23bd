// vame_refine_core.h -- what the list forms of the search's iteration share
// (vame_birefine.hip: vame_bipred_refine; vame_search.hip: vame_affine_search;
// DESIGN.md §14, §15): one workgroup per descriptor, one lane per 4x4
// sub-block (SB of them in the largest class), the prediction samples P_m of
// the moving CPMVs in LDS.  Here are the workgroup sums and one gradient step
// -- Sobel gradients on P_m, the moments, solveEqual, scaleDeltaMvs, the
// wrapping add, the clamp to +-2^17 and clipMv (update_cpmv) -- built from the
// search's device functions (vame_dev.h).  The error term is e = E - P_m: E is
// 2 cur - P_fixed for a bi descriptor and cur for a uni one.
#pragma once
#include "vame_mc_core.h"

namespace vame {

static_assert(kNumVal2 <= kNumMom, "one moment table for both models");

__device__ __forceinline__ int br_wave_sum(int v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}
__device__ __forceinline__ long long br_wave_sum64(long long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// Sum of `v` over the workgroup, in every lane (called by all of them).
template <int NT>
__device__ __forceinline__ long long br_block_sum(int v, unsigned long long* s_sum) {
  v = br_wave_sum(v);
  if constexpr (NT == 64) return v;
  __syncthreads();  // the readers of the previous sum are done
  if (threadIdx.x == 0) *s_sum = 0;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) atomicAdd(s_sum, (unsigned long long)(long long)v);
  __syncthreads();
  return (long long)*s_sum;
}

// The lane's share of the CU's moments (eq_value's order) into s_V: the sum
// over its sub-blocks, a wave sum, then one 64-bit LDS add per wave and value
// (integer: any order).
template <int NCP, int SB>
__device__ __forceinline__ void br_accumulate(const int (&S)[SB][5], int u, const int (&v)[SB], long long* s_V) {
  constexpr int NV = NCP == 3 ? kNumMom : kNumVal2;
#pragma unroll
  for (int k = 0; k < NV; k++) {
    long long t = 0;
#pragma unroll
    for (int q = 0; q < SB; q++) t += eq_value<NCP>(k, S[q], u, v[q]);
    t = br_wave_sum64(t);
    if ((threadIdx.x & 63) == 0) atomicAdd(reinterpret_cast<unsigned long long*>(s_V + k), (unsigned long long)t);
    __builtin_amdgcn_sched_barrier(0);  // one value at a time, not 24 of them in flight
  }
}

// One step of the search's update on the samples in s_pm (int16 [h][w]) with
// e = E - P_m, for the CU (x, y, 2^lw, 2^lh) of the frame W x H and the model
// of ncp CPMVs: cc becomes the next CPMVs (a 2-CP model never changes LB);
// returns whether they moved.  Called by every lane of the workgroup; s_V
// (kNumMom) and s_M (42) are scratch, free again on return, and so is s_pm.
template <int NT, int SB>
__device__ __forceinline__ bool br_step(const uint2* s_pm, const uint2 (&E)[SB][4], long long* s_V, double* s_M,
                                        const Geo& g, int ncp, bool active, int nq, int sx, int sy, int syStep, int W,
                                        int H, int (&cc)[6]) {
  const int tid = threadIdx.x;
  if (tid < kNumMom) s_V[tid] = 0;
  __syncthreads();
  int S[SB][5] = {};
  int vq[SB];
#pragma unroll
  for (int q = 0; q < SB; q++) vq[q] = sy + q * syStep + 2;
  if (active) {
    const uint16_t* pm16 = reinterpret_cast<const uint16_t*>(s_pm);
    const int xl = max(sx - 1, 0), xr = min(sx + 4, g.w - 1);
#pragma unroll
    for (int q = 0; q < SB; q++) {
      if (q >= nq) break;
      const int syq = sy + q * syStep;
      uint4 X[6];
#pragma unroll
      for (int k = 0; k < 6; k++) {
        const int row = clampi(syq - 1 + k, 0, g.h - 1) * g.w;
        const uint2 pq = s_pm[(row + sx) >> 2];
        X[k] = ext_row(pq, (unsigned)pm16[row + xl] << 16, (unsigned)pm16[row + xr]);
      }
      grad_sb(sx, syq, g, X, E[q], S[q]);
    }
  }
  if (ncp == 3)
    br_accumulate<3, SB>(S, sx + 2, vq, s_V);
  else
    br_accumulate<2, SB>(S, sx + 2, vq, s_V);
  __syncthreads();
  if (tid < 64) {  // the first wave solves; the deltas come back in s_M[0 .. 2 ncp)
    double dd[6];
    if (ncp == 3)
      seg_solve<3, true>(s_V, s_M, kEqMap.v, tid, 64, true, false, g.lw, g.lh, dd);
    else
      seg_solve<2, true>(s_V, s_M, kEqMap.v, tid, 64, true, false, g.lw, g.lh, dd);
  }
  __syncthreads();
  bool moved = false;
#pragma unroll
  for (int j = 0; j < 6; j++) {
    if (j < 2 * ncp) {
      const double d = s_M[j == 1 ? 2 : j == 2 ? 1 : j];  // LT = (d0, d2), RT = (d1, d3), LB = (d4, d5)
      const int v = update_cpmv(cc[j], d, (j & 1) ? g.y : g.x, (j & 1) ? H : W);
      moved = moved || v != cc[j];
      cc[j] = v;
    }
  }
  __syncthreads();  // s_M, s_V and s_pm are free again
  return moved;
}

}  // namespace vame

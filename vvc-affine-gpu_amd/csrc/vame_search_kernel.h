// vame_search_kernel.h -- search_kernel, the kernel of vame_affine_search
// (PT = SearchParams; instantiated in vame_search.hip) and of
// vame_affine_search_p (PT = SearchParamsP; instantiated in vame_search_p.hip,
// a unit of its own, so that the unit of the calls without predictors holds the
// kernels it always held and compiles to the code it always compiled to;
// DESIGN.md §17).  The description of the kernel is vame_search.hip's.
#pragma once
#include <hip/hip_runtime.h>

#include "vame_refine_core.h"
#include "vame_search.h"

namespace vame {

__device__ __forceinline__ bool search_cu_ok(const McCu& cu, const SearchParams& p, int) {
  return mc_cu_ok(cu, p.W, p.H, p.nrefs);
}
__device__ __forceinline__ bool search_cu_ok(const McCu& cu, const SearchParamsP& p, int i) {
  return mc_cu_ok(cu, p.W, p.H, p.nrefs) && mvp_cu_ok(cu, p.preds, i);
}
// An iteration's cost: the workgroup's SATD sum and the rate of the CPMVs c.
// Against descriptor i's predictor the rate is formed by the first lane alone
// (six predictor loads and the bits inside its branch, nothing held across the
// iteration) and enters the workgroup sum -- with that lane's SATD in a one-wave
// workgroup, as the start value of the LDS sum otherwise: the same integer.
template <int NT>
__device__ __forceinline__ long long search_cost(const SearchParams& p, int, int, const int* c, int ncp, int s,
                                                 unsigned long long* s_sum) {
  return br_block_sum<NT>(s, s_sum) + mc_rate(p.lambda, affine_bits(c, ncp) + kRuiBits);
}
__device__ __forceinline__ int search_rate_p(const SearchParamsP& p, int i, const int* c, int ncp) {
  MvPred<true> pp;
  pp.load(p.preds + (size_t)i * kMvpWords);
  return (int)mc_rate(p.lambda, pp.bits(c, ncp) + kRuiBits);
}
template <int NT>
__device__ __forceinline__ long long search_cost(const SearchParamsP& p, int i, int tid, const int* c, int ncp, int s,
                                                 unsigned long long* s_sum) {
  if constexpr (NT == 64) {
    if (tid == 0) s += search_rate_p(p, i, c, ncp);
    return br_wave_sum(s);
  }
  // br_block_sum (vame_refine_core.h) with the rate as the sum's start value
  const int v = br_wave_sum(s);
  __syncthreads();  // the readers of the previous sum are done
  if (tid == 0) *s_sum = (unsigned long long)(long long)search_rate_p(p, i, c, ncp);
  __syncthreads();
  if ((tid & 63) == 0) atomicAdd(s_sum, (unsigned long long)(long long)v);
  __syncthreads();
  return (long long)*s_sum;
}

// PT = SearchParamsP: vame_affine_search_p, every iteration's rate against the
// descriptor's predictor (affine_bits_p), which so takes part in which
// iteration wins; an invalid predictor makes the descriptor invalid.
template <int NT, int SB, class PT>
__global__ __launch_bounds__(NT) void search_kernel(PT p) {
  __shared__ uint4 s_coef[48];
  __shared__ uint2 s_pm[NT * SB * 4];  // P, int16 [h][w]: 16 samples per sub-block
  __shared__ long long s_V[kNumMom];
  __shared__ double s_M[42];
  __shared__ unsigned long long s_sum;
  const int tid = threadIdx.x, i = blockIdx.x;
  if (i >= mc_ncus(p.ncusDev, p.maxCus)) return;
  const McCu cu = p.cus[i];
  const bool ok = search_cu_ok(cu, p, i);  // vame_affine_mc's validity rules
  const int nsb = ok ? (cu.w * cu.h) >> 4 : 0;      // an invalid descriptor goes with the smallest class
  if ((nsb <= 64 ? 64 : nsb <= 256 ? 256 : 1024) != NT * SB) return;
  if (!ok) {
    if (tid == 0) {
      p.out[i] = cu;
      p.cost[i] = 0;
      atomicOr(p.bad, 1);
    }
    return;
  }
  if (tid < 48) s_coef[tid] = reinterpret_cast<const uint4*>(&kCoefTab)[tid];
  __syncthreads();

  const int W = p.W, H = p.H;
  const int lw = 31 - __clz(cu.w), lh = 31 - __clz(cu.h);
  const bool active = tid < nsb;          // the lane holds a sub-block
  const int nq = SB == 1 ? 1 : nsb / NT;  // and, in a CU that fills the workgroup, nq of them (uniform)
  const int sx0 = (tid & ((cu.w >> 2) - 1)) << 2, sy0 = (tid >> (lw - 2)) << 2;
  const int syStep = (NT >> (lw - 2)) << 2;  // rows between a lane's sub-blocks
  Geo g;
  g.x = cu.x; g.y = cu.y; g.lw = lw; g.lh = lh; g.w = cu.w; g.h = cu.h;
  const int ncp = cu.ncps;
  int cc[6] = {cu.ltx, cu.lty, cu.rtx, cu.rty, cu.lbx, cu.lby};  // a 2-CP descriptor keeps its LB as given
  int best[6];
#pragma unroll
  for (int k = 0; k < 6; k++) best[k] = cc[k];
  const uint16_t* __restrict__ ref =
      cu.ref == 0 ? p.refs[0] : cu.ref == 1 ? p.refs[1] : cu.ref == 2 ? p.refs[2] : p.refs[3];

  uint2 O[SB][4] = {};
  if (active) {
    // x, sx are multiples of 4 and so is W: every row of a block is 8-byte aligned
    const char* base = reinterpret_cast<const char*>(p.cur);
    const size_t bw = (size_t)W * 2u;
#pragma unroll
    for (int q = 0; q < SB; q++) {
      if (q >= nq) break;
      const size_t b0 = ((size_t)(cu.y + sy0 + q * syStep) * W + cu.x + sx0) * 2u;
#pragma unroll
      for (int r = 0; r < 4; r++) O[q][r] = *reinterpret_cast<const uint2*>(base + (b0 + r * bw));
    }
  }

  const int niter = (ncp == 3 ? 4 : 5) + p.extra;
  long long bestCost = 0x7fffffffffffffffll;  // iteration 0's cost always replaces it
#pragma unroll 1
  for (int it = 0;; it++) {
    // the lane's geometry is loop-invariant: hidden from the optimizer, or every
    // address and monomial derived from it is hoisted and held across the loop
    int sx = sx0, sy = sy0;
    opaque(sx);
    opaque(sy);
    int s = 0;
    if (active) {
#pragma unroll
      for (int q = 0; q < SB; q++) {
        if (q >= nq) break;
        const int syq = sy + q * syStep;
        int acc[4][4];
        mc_hyp_acc(ref, cu.x, cu.y, lw, lh, cc, ncp, sx, syq, W, H, s_coef, acc);
        uint2 P[4];
#pragma unroll
        for (int r = 0; r < 4; r++)
          P[r] = make_uint2(pack16(clampi(acc[r][0] >> 10, 0, 1023), clampi(acc[r][1] >> 10, 0, 1023)),
                            pack16(clampi(acc[r][2] >> 10, 0, 1023), clampi(acc[r][3] >> 10, 0, 1023)));
        s += satd_4x4(O[q], P);
        // P for the gradient step (unused after the last cost)
#pragma unroll
        for (int r = 0; r < 4; r++) s_pm[((syq + r) * cu.w + sx) >> 2] = P[r];
      }
    }
    const long long cost = search_cost<NT>(p, i, tid, cc, ncp, s, &s_sum);
    if (cost < bestCost) {
      bestCost = cost;
#pragma unroll
      for (int k = 0; k < 6; k++) best[k] = cc[k];
    }
    if (it == niter) break;
    // unchanged CPMVs repeat this iteration's prediction and cost: never strictly better
    if (!br_step<NT, SB>(s_pm, O, s_V, s_M, g, ncp, active, nq, sx, sy, syStep, W, H, cc)) break;
  }
  if (tid == 0) {
    McCu o = cu;
    o.ltx = best[0]; o.lty = best[1]; o.rtx = best[2]; o.rty = best[3];
    if (ncp == 3) {
      o.lbx = best[4];
      o.lby = best[5];
    }
    p.out[i] = o;
    p.cost[i] = bestCost;
  }
}

template <class PT>
inline hipError_t search_launch_t(const PT& p, hipStream_t stream) {
  hipLaunchKernelGGL((search_kernel<64, 1, PT>), dim3(p.maxCus), dim3(64), 0, stream, p);
  hipLaunchKernelGGL((search_kernel<256, 1, PT>), dim3(p.maxCus), dim3(256), 0, stream, p);
  hipLaunchKernelGGL((search_kernel<512, 2, PT>), dim3(p.maxCus), dim3(512), 0, stream, p);
  return hipGetLastError();
}
}  // namespace vame

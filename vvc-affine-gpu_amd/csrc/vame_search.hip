// vame_search.hip -- the search's iteration from caller-given CPMVs on a CU
// list (vame_affine_search) and the glue of vame_affine_me_seeded
// (include/vame.h).
//
// search_kernel is the uni form of birefine_kernel (vame_birefine.hip): one
// workgroup per descriptor, one lane per 4x4 sub-block, the same three size
// classes -- 64, 256 and 1024 sub-blocks on 64, 256 and 512 lanes -- launched
// over the whole capacity, a workgroup whose descriptor is past the device-side
// count or of another class leaving at once.  Per lane, in registers: the
// original block; in LDS: the prediction's samples P as int16 [h][w] for the
// Sobel neighbourhood, the 24 int64 moments and the 6x7 FP64 system.  The
// iteration is oracle/vame_oracle.c:run_cu's with init = the descriptor's
// CPMVs: predict (mc_hyp_acc, the search's prediction), cost = SATD +
// floor(lambda * (bits + 2)), take it under strict < (iteration 0 always),
// then one gradient step with e = cur - P (br_step, vame_refine_core.h).
//
// vame_affine_me_seeded, on the context's table of in-frame candidates:
//   seeded_build_kernel   one lane per (refIdx, candidate): a non-zero seed in
//                         range appends a 2-CP descriptor LT = RT = seed and
//                         where its result goes (an atomic slot: the order of
//                         the list varies, what is scattered back does not)
//   search_kernel         on the list, in place
//   seeded_lb_kernel      3-CP in the mask: the 3-CP descriptor from the 2-CP
//                         winner, LB as the fused search derives it
//                         (affine.cl:81-105)
//   search_kernel         on those
//   seeded_merge_kernel   a row takes cost and CPMVs where the new cost is
//                         strictly lower
#include <hip/hip_runtime.h>

#include "vame_refine_core.h"
#include "vame_search.h"

namespace vame {

template <int NT, int SB>
__global__ __launch_bounds__(NT) void search_kernel(SearchParams p) {
  __shared__ uint4 s_coef[48];
  __shared__ uint2 s_pm[NT * SB * 4];  // P, int16 [h][w]: 16 samples per sub-block
  __shared__ long long s_V[kNumMom];
  __shared__ double s_M[42];
  __shared__ unsigned long long s_sum;
  const int tid = threadIdx.x, i = blockIdx.x;
  if (i >= mc_ncus(p.ncusDev, p.maxCus)) return;
  const McCu cu = p.cus[i];
  const bool ok = mc_cu_ok(cu, p.W, p.H, p.nrefs);  // vame_affine_mc's validity rules
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
    const long long cost = br_block_sum<NT>(s, &s_sum) + mc_rate(p.lambda, affine_bits(cc, ncp) + kRuiBits);
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

hipError_t search_launch(const SearchParams& p, hipStream_t stream) {
  hipLaunchKernelGGL((search_kernel<64, 1>), dim3(p.maxCus), dim3(64), 0, stream, p);
  hipLaunchKernelGGL((search_kernel<256, 1>), dim3(p.maxCus), dim3(256), 0, stream, p);
  hipLaunchKernelGGL((search_kernel<512, 2>), dim3(p.maxCus), dim3(512), 0, stream, p);
  return hipGetLastError();
}

// ------------------------------------------------------- vame_affine_me_seeded
constexpr int kSeededThreads = 256;

__global__ __launch_bounds__(kSeededThreads) void seeded_zero_kernel(SeededParams p) {
  if (threadIdx.x == 0) *p.work.count = 0;
}

__global__ __launch_bounds__(kSeededThreads) void seeded_build_kernel(SeededParams p) {
  const int nc = p.candEnd - p.candBegin;
  const int t = blockIdx.x * kSeededThreads + threadIdx.x;
  if (t >= nc * p.search.nrefs) return;
  const int r = t / nc;
  const BiCand cd = p.cands[p.candBegin + t - r * nc];
  const int align = (cd.shape >> 8) & 1;
  const int32_t* seed = nullptr;
#pragma unroll
  for (int rr = 0; rr < 4; rr++)
#pragma unroll
    for (int aa = 0; aa < 2; aa++)
      if (rr == r && aa == align) seed = p.seed[rr][aa];
  const int mx = seed[2 * (size_t)cd.row], my = seed[2 * (size_t)cd.row + 1];
  if (mx == 0 && my == 0) return;
  if (!mc_mv_ok(mx) || !mc_mv_ok(my)) {
    atomicOr(p.search.bad, 1);
    return;
  }
  const int k = atomicAdd(p.work.count, 1);  // < cap: one slot per (refIdx, candidate)
  McCu cu;
  cu.x = cd.xy & 0xFFFF;
  cu.y = cd.xy >> 16;
  cu.w = 1 << (cd.shape & 15);
  cu.h = 1 << ((cd.shape >> 4) & 15);
  cu.ref = r;
  cu.ncps = 2;
  cu.ltx = cu.rtx = mx;
  cu.lty = cu.rty = my;
  cu.lbx = cu.lby = 0;
  p.work.cus2[k] = cu;
  p.work.slot[2 * k] = r | (align << 2);
  p.work.slot[2 * k + 1] = cd.row;
}

__global__ __launch_bounds__(kSeededThreads) void seeded_lb_kernel(SeededParams p) {
  const int k = blockIdx.x * kSeededThreads + threadIdx.x;
  if (k >= min(*p.work.count, p.cap)) return;
  McCu cu = p.work.cus2[k];
  const int lw = 31 - __clz(cu.w), lh = 31 - __clz(cu.h);
  // affine.cl:81-105, as the fused search derives its 3-CP start
  int lbx, lby;
  derive_lb(cu.ltx, cu.lty, cu.rtx, cu.rty, lw, lh, cu.x, cu.y, p.search.W, p.search.H, lbx, lby);
  cu.ncps = 3;
  cu.lbx = lbx;
  cu.lby = lby;
  p.work.cus3[k] = cu;
}

__device__ __forceinline__ void seeded_take(const SeededParams& p, int r, int m, int row, const McCu& cu,
                                            long long cost, int ncps) {
  int64_t* c = nullptr;
  int32_t* v = nullptr;
#pragma unroll
  for (int rr = 0; rr < 4; rr++)
#pragma unroll
    for (int mm = 0; mm < 4; mm++)
      if (rr == r && mm == m) {
        c = p.cost[rr][mm];
        v = p.cpmv[rr][mm];
      }
  if (!(cost < c[row])) return;
  c[row] = cost;
  v += (size_t)row * 7;
  v[0] = ncps;
  v[1] = cu.ltx; v[2] = cu.lty; v[3] = cu.rtx; v[4] = cu.rty;
  v[5] = ncps == 3 ? cu.lbx : 0;
  v[6] = ncps == 3 ? cu.lby : 0;
}

__global__ __launch_bounds__(kSeededThreads) void seeded_merge_kernel(SeededParams p) {
  const int k = blockIdx.x * kSeededThreads + threadIdx.x;
  if (k >= min(*p.work.count, p.cap)) return;
  const int ra = p.work.slot[2 * k], row = p.work.slot[2 * k + 1];
  const int r = ra & 3, align = ra >> 2;
  seeded_take(p, r, 2 * align, row, p.work.cus2[k], p.work.cost2[k], 2);
  if (p.with3) seeded_take(p, r, 2 * align + 1, row, p.work.cus3[k], p.work.cost3[k], 3);
}

hipError_t seeded_launch(const SeededParams& p, hipStream_t stream) {
  const int n = p.cap;
  hipLaunchKernelGGL(seeded_zero_kernel, dim3(1), dim3(kSeededThreads), 0, stream, p);
  if (n == 0) return hipGetLastError();
  const dim3 grid((n + kSeededThreads - 1) / kSeededThreads), block(kSeededThreads);
  hipLaunchKernelGGL(seeded_build_kernel, grid, block, 0, stream, p);
  SearchParams s = p.search;
  s.maxCus = n;
  s.ncusDev = p.work.count;
  s.cus = s.out = p.work.cus2;
  s.cost = p.work.cost2;
  hipError_t e = search_launch(s, stream);
  if (e != hipSuccess) return e;
  if (p.with3) {
    hipLaunchKernelGGL(seeded_lb_kernel, grid, block, 0, stream, p);
    s.cus = s.out = p.work.cus3;
    s.cost = p.work.cost3;
    e = search_launch(s, stream);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(seeded_merge_kernel, grid, block, 0, stream, p);
  return hipGetLastError();
}

}  // namespace vame

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

#include <type_traits>

#include "vame_search_kernel.h"

namespace vame {

hipError_t search_launch(const SearchParams& p, hipStream_t stream) { return search_launch_t(p, stream); }
// the searches of the seeded calls: vame_affine_me_seeded_p's are vame_search_p.hip's
static hipError_t seeded_search(const SearchParams& p, hipStream_t stream) { return search_launch(p, stream); }
static hipError_t seeded_search(const SearchParamsP& p, hipStream_t stream) { return search_p_launch(p, stream); }

// ------------------------------------------------------- vame_affine_me_seeded
constexpr int kSeededThreads = 256;

__global__ __launch_bounds__(kSeededThreads) void seeded_zero_kernel(SeededParams p) {
  if (threadIdx.x == 0) *p.work.count = 0;
}

// PT = SeededParamsP: the row's predictor (its mvp entry, LT = RT = LB) goes
// with the descriptor; a row whose predictor is out of range is skipped.
template <class PT>
__global__ __launch_bounds__(kSeededThreads) void seeded_build_kernel(PT p) {
  constexpr bool MVP = std::is_same<PT, SeededParamsP>::value;
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
  int qx = 0, qy = 0;
  if constexpr (MVP) {
    const int32_t* mvp = nullptr;
#pragma unroll
    for (int rr = 0; rr < 4; rr++)
#pragma unroll
      for (int aa = 0; aa < 2; aa++)
        if (rr == r && aa == align) mvp = p.mvp[rr][aa];
    qx = mvp[2 * (size_t)cd.row];
    qy = mvp[2 * (size_t)cd.row + 1];
    if (!mc_mv_ok(qx) || !mc_mv_ok(qy)) {
      atomicOr(p.search.bad, 1);
      return;
    }
  }
  const int k = atomicAdd(p.work.count, 1);  // < cap: one slot per (refIdx, candidate)
  if constexpr (MVP) {
    int32_t* P = p.preds + (size_t)k * kMvpWords;
    P[0] = 3;
    P[1] = P[3] = P[5] = qx;
    P[2] = P[4] = P[6] = qy;
  }
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

// The launches of vame_affine_me_seeded (PT = SeededParams, ST = SearchParams)
// and of vame_affine_me_seeded_p (SeededParamsP, SearchParamsP): the zero, lb
// and merge kernels take the base block in both.
template <class PT, class ST>
static hipError_t seeded_launch_t(const PT& p, ST s, hipStream_t stream) {
  const SeededParams& base = p;
  const int n = p.cap;
  hipLaunchKernelGGL(seeded_zero_kernel, dim3(1), dim3(kSeededThreads), 0, stream, base);
  if (n == 0) return hipGetLastError();
  const dim3 grid((n + kSeededThreads - 1) / kSeededThreads), block(kSeededThreads);
  hipLaunchKernelGGL(seeded_build_kernel<PT>, grid, block, 0, stream, p);
  s.maxCus = n;
  s.ncusDev = p.work.count;
  s.cus = s.out = p.work.cus2;
  s.cost = p.work.cost2;
  hipError_t e = seeded_search(s, stream);
  if (e != hipSuccess) return e;
  if (p.with3) {
    hipLaunchKernelGGL(seeded_lb_kernel, grid, block, 0, stream, base);
    s.cus = s.out = p.work.cus3;
    s.cost = p.work.cost3;
    e = seeded_search(s, stream);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(seeded_merge_kernel, grid, block, 0, stream, base);
  return hipGetLastError();
}
hipError_t seeded_launch(const SeededParams& p, hipStream_t stream) { return seeded_launch_t(p, p.search, stream); }
hipError_t seeded_p_launch(const SeededParamsP& p, hipStream_t stream) {
  SearchParamsP s;
  static_cast<SearchParams&>(s) = p.search;
  s.preds = p.preds;
  return seeded_launch_t(p, s, stream);
}

// ---------------------------------------------------------------- vame_reprice
// One lane per (refIdx, in-frame candidate): for each PRED of the candidate's
// alignment in the mask, cost -= floor(lambda * (affine_bits + 2)), cost +=
// floor(lambda * (affine_bits_p + 2)) with the row's predictor LT = RT = LB.
// Pure arithmetic; a row whose predictor is out of range is skipped.
__global__ __launch_bounds__(kSeededThreads) void reprice_kernel(RepriceParams p) {
  const int nc = p.candEnd - p.candBegin;
  const int t = blockIdx.x * kSeededThreads + threadIdx.x;
  if (t >= nc * p.nrefs) return;
  const int r = t / nc;
  const BiCand cd = p.cands[p.candBegin + t - r * nc];
  const int align = (cd.shape >> 8) & 1;
  const int32_t* mvp = nullptr;
  int64_t* c[2] = {nullptr, nullptr};
  const int32_t* v[2] = {nullptr, nullptr};
#pragma unroll
  for (int rr = 0; rr < 4; rr++)
#pragma unroll
    for (int aa = 0; aa < 2; aa++)
      if (rr == r && aa == align) {
        mvp = p.mvp[rr][aa];
        c[0] = p.cost[rr][2 * aa];
        c[1] = p.cost[rr][2 * aa + 1];
        v[0] = p.cpmv[rr][2 * aa];
        v[1] = p.cpmv[rr][2 * aa + 1];
      }
  if (!c[0] && !c[1]) return;  // no PRED of this alignment in the mask
  const int qx = mvp[2 * (size_t)cd.row], qy = mvp[2 * (size_t)cd.row + 1];
  if (!mc_mv_ok(qx) || !mc_mv_ok(qy)) {
    atomicOr(p.bad, 1);
    return;
  }
  const int P[6] = {qx, qy, qx, qy, qx, qy};
#pragma unroll
  for (int m = 0; m < 2; m++) {
    if (!c[m]) continue;
    const int32_t* a = v[m] + (size_t)cd.row * 7;
    int cp[6];
#pragma unroll
    for (int k = 0; k < 6; k++) cp[k] = a[1 + k];
    c[m][cd.row] += mc_rate(p.lambda, affine_bits_p(cp, P, 2 + m) + kRuiBits) -
                    mc_rate(p.lambda, affine_bits(cp, 2 + m) + kRuiBits);
  }
}

hipError_t reprice_launch(const RepriceParams& p, hipStream_t stream) {
  const int n = (p.candEnd - p.candBegin) * p.nrefs;
  if (n > 0)
    hipLaunchKernelGGL(reprice_kernel, dim3((n + kSeededThreads - 1) / kSeededThreads), dim3(kSeededThreads), 0, stream,
                       p);
  return hipGetLastError();
}

}  // namespace vame

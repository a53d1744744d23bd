// vame_bipred.hip -- affine bi-prediction (include/vame.h).
//
// A hypothesis is one prediction of vame_affine_mc up to its second-stage
// accumulator (mc_hyp_acc, vame_mc_core.h); the bi sample of two hypotheses is
// the sum of their accumulators, rounded once (mc_bi_pack).
//
//   vame_affine_mc_bi   mc_count_kernel / mc_offsets_kernel (vame_mc_core.h)
//                       on 20-word descriptors, then mc_bi_predict_kernel:
//                       vame_affine_mc's three launches, one lane per 4x4
//                       sub-block, two filter passes into two accumulator sets
//   vame_bipred         the best reference pair of every in-frame candidate CU.
//                       The candidates are fixed geometry: vame_create builds
//                       their table and the map group of 16 sub-blocks ->
//                       candidate, so a lane finds its CU with one load.
//     bipred_init_kernel    INT64_MAX / -1 into every row of the alignments in
//                           the mask, zero into the pair sums
//     bipred_rows_kernel    one lane per 4x4 sub-block: each reference's
//                           hypothesis (its cheaper model) predicted once, the
//                           up to four accumulator sets held in registers (64
//                           VGPRs); the up to six pair SATDs from them, a DPP
//                           row sum and one 64-bit atomic add per row and pair
//                           (integer sums: deterministic)
//     bipred_close_kernel   one lane per candidate: the pairs' rates, the first
//                           minimum, bi_cost and bi_sel
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "vame_bipred.h"

namespace vame {

constexpr int kBiThreads = 256;  // vame_bipred's workgroups
constexpr long long kBiInf = 0x7fffffffffffffffll;
static_assert(sizeof(BiCand) == 16, "one 16-byte load");

// MVP: vame_affine_mc_bi_p, the rate against the descriptor's predictors
// (affine_bits_p); the samples do not depend on them.
template <bool MVP>
__global__ __launch_bounds__(kMcThreads) void mc_bi_predict_kernel(McParamsT<McBiCu, MVP> p) {
  __shared__ uint4 s_coef[48];
  const int tid = threadIdx.x;
  if (tid < 48) s_coef[tid] = reinterpret_cast<const uint4*>(&kCoefTab)[tid];
  __syncthreads();
  const int W = p.W, H = p.H;
  const int ncus = mc_ncus(p.ncusDev, p.ncus);
  const int total = p.offs[ncus];
  for (int g = blockIdx.x * kMcThreads + tid; g < total; g += (int)gridDim.x * kMcThreads) {
    // the last descriptor whose offset is <= g (descriptors without
    // sub-blocks share their successor's offset and are never found)
    int lo = 0, hi = ncus;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (p.offs[mid] <= g)
        lo = mid;
      else
        hi = mid;
    }
    const McBiCu cu = p.cus[lo];
    const int local = g - p.offs[lo];
    const int lw = 31 - __clz(cu.w), lh = 31 - __clz(cu.h);
    const int sx = (local & ((cu.w >> 2) - 1)) << 2, sy = (local >> (lw - 2)) << 2;
    const int cp0[6] = {cu.c0[0], cu.c0[1], cu.c0[2], cu.c0[3], cu.c0[4], cu.c0[5]};
    const int cp1[6] = {cu.c1[0], cu.c1[1], cu.c1[2], cu.c1[3], cu.c1[4], cu.c1[5]};
    const uint16_t* __restrict__ ref0 =
        cu.ref0 == 0 ? p.refs[0] : cu.ref0 == 1 ? p.refs[1] : cu.ref0 == 2 ? p.refs[2] : p.refs[3];
    int acc[4][4];
    mc_hyp_acc(ref0, cu.x, cu.y, lw, lh, cp0, cu.ncps0, sx, sy, W, H, s_coef, acc);
    uint2 P[4];
    int bits = MVP ? 0 : affine_bits(cp0, cu.ncps0) + kRuiBits;  // MVP: by the CU's first lane, below
    if (cu.ref1 >= 0) {
      const uint16_t* __restrict__ ref1 =
          cu.ref1 == 0 ? p.refs[0] : cu.ref1 == 1 ? p.refs[1] : cu.ref1 == 2 ? p.refs[2] : p.refs[3];
      int acc1[4][4];
      mc_hyp_acc(ref1, cu.x, cu.y, lw, lh, cp1, cu.ncps1, sx, sy, W, H, s_coef, acc1);
      mc_bi_pack(acc, acc1, P);
      if constexpr (!MVP) bits += affine_bits(cp1, cu.ncps1) + kRuiBits;
    } else {
      mc_bi_pack(acc, acc, P);  // (2 * acc) >> 11 == acc >> 10
    }

    // x, sx are multiples of 4 and so is W: every row of the block is 8-byte aligned
    const size_t b0 = ((size_t)(cu.y + sy) * W + cu.x + sx) * 2u, bw = (size_t)W * 2u;
    if (p.pred) {
      char* base = reinterpret_cast<char*>(p.pred);
#pragma unroll
      for (int r = 0; r < 4; r++) *reinterpret_cast<uint2*>(base + (b0 + r * bw)) = P[r];
    }
    if (p.cost) {
      const char* base = reinterpret_cast<const char*>(p.cur);
      uint2 O[4];
#pragma unroll
      for (int r = 0; r < 4; r++) O[r] = *reinterpret_cast<const uint2*>(base + (b0 + r * bw));
      long long v = row_sum16(satd_4x4(O, P));
      // the CU's first lane adds the rate: each hypothesis with its own ruiBits
      if constexpr (MVP) {
        if (local == 0) {  // against the hypotheses' predictors, read by this lane alone
          MvPred<true> pp;
          pp.load(p.preds + (size_t)lo * 2 * kMvpWords);
          bits = pp.bits(cp0, cu.ncps0) + kRuiBits;
          if (cu.ref1 >= 0) {
            pp.load(p.preds + ((size_t)lo * 2 + 1) * kMvpWords);
            bits += pp.bits(cp1, cu.ncps1) + kRuiBits;
          }
        }
      }
      if (local == 0) v += mc_rate(p.lambda, bits);
      if ((local & 15) == 0) atomicAdd(reinterpret_cast<unsigned long long*>(p.cost + lo), (unsigned long long)v);
    }
  }
}

hipError_t mc_bi_launch(const McBiParams& p, hipStream_t stream) {
  return mc_launch_concat(p, mc_bi_predict_kernel<false>, stream);
}
hipError_t mc_bi_p_launch(const McBiParamsP& p, hipStream_t stream) {
  return mc_launch_concat(p, mc_bi_predict_kernel<true>, stream);
}

// ------------------------------------------------------------------ vame_bipred

// The model of refIdx r's hypothesis for a row of alignment `align`: the first
// minimum under strict < over 2-CP, 3-CP among the PREDs in the mask.
template <int R>
__device__ __forceinline__ int bi_model(const BiRowsParams& p, int align, int row) {
  const int m2 = (p.predMask >> (2 * align)) & 1, m3 = (p.predMask >> (2 * align + 1)) & 1;
  if (!m3) return 0;
  if (!m2) return 1;
  const int64_t* c2 = align ? p.cost[R][2] : p.cost[R][0];
  const int64_t* c3 = align ? p.cost[R][3] : p.cost[R][1];
  return c3[row] < c2[row] ? 1 : 0;
}
template <int R>
__device__ __forceinline__ void bi_load_cp(const BiRowsParams& p, int align, int m, int row, int (&cp)[6]) {
  const int32_t* a = align ? (m ? p.cpmv[R][3] : p.cpmv[R][2]) : (m ? p.cpmv[R][1] : p.cpmv[R][0]);
  a += (size_t)row * 7;
#pragma unroll
  for (int k = 0; k < 6; k++) cp[k] = a[1 + k];
}

__global__ __launch_bounds__(kBiThreads) void bipred_init_kernel(BiRowsParams p) {
  const int i = blockIdx.x * kBiThreads + threadIdx.x;
#pragma unroll
  for (int a = 0; a < 2; a++)
    if (p.biCost[a] && i < p.rowsOf[a]) {
      p.biCost[a][i] = kBiInf;
      p.biSel[a][i] = -1;
    }
  if (i < (p.candEnd - p.candBegin) * kBiPairs) p.pairSatd[(size_t)p.candBegin * kBiPairs + i] = 0;
}

template <int R>
__device__ __forceinline__ void bi_hyp(const BiRowsParams& p, const BiCand& cd, int sx, int sy,
                                       const uint4* s_coef, int (&acc)[4][4]) {
  const int align = (cd.shape >> 8) & 1;
  const int m = bi_model<R>(p, align, cd.row);
  int cp[6];
  bi_load_cp<R>(p, align, m, cd.row, cp);
  mc_hyp_acc(p.refs[R], cd.xy & 0xFFFF, cd.xy >> 16, cd.shape & 15, (cd.shape >> 4) & 15, cp, 2 + m, sx, sy, p.W,
             p.H, s_coef, acc);
}

__device__ __forceinline__ void bi_pair(const BiRowsParams& p, const int (&a)[4][4], const int (&b)[4][4],
                                        const uint2 (&O)[4], bool first, int cand, int pair) {
  uint2 P[4];
  mc_bi_pack(a, b, P);
  const int v = row_sum16(satd_4x4(O, P));
  if (first)
    atomicAdd(reinterpret_cast<unsigned long long*>(p.pairSatd + (size_t)cand * kBiPairs + pair),
              (unsigned long long)(long long)v);
}

__global__ __launch_bounds__(kBiThreads) void bipred_rows_kernel(BiRowsParams p) {
  __shared__ uint4 s_coef[48];
  const int tid = threadIdx.x;
  if (tid < 48) s_coef[tid] = reinterpret_cast<const uint4*>(&kCoefTab)[tid];
  __syncthreads();
  // a group of 16 lanes (one DPP row) is 16 sub-blocks of one candidate
  const int group = p.groupBegin + blockIdx.x * (kBiThreads / 16) + (tid >> 4);
  if (group >= p.groupEnd) return;
  const int cand = p.groupCand[group];
  const BiCand cd = p.cands[cand];
  const int local = ((group - cd.first) << 4) | (tid & 15);
  const int lw = cd.shape & 15;
  const int sx = (local & ((1 << (lw - 2)) - 1)) << 2, sy = (local >> (lw - 2)) << 2;
  const int x = cd.xy & 0xFFFF, y = cd.xy >> 16;

  uint2 O[4];
  {
    const char* base = reinterpret_cast<const char*>(p.cur);
    const size_t b0 = ((size_t)(y + sy) * p.W + x + sx) * 2u, bw = (size_t)p.W * 2u;
#pragma unroll
    for (int r = 0; r < 4; r++) O[r] = *reinterpret_cast<const uint2*>(base + (b0 + r * bw));
  }
  const bool first = (tid & 15) == 0;
  const int nrefs = p.nrefs;  // >= 2
  int a0[4][4], a1[4][4];
  bi_hyp<0>(p, cd, sx, sy, s_coef, a0);
  bi_hyp<1>(p, cd, sx, sy, s_coef, a1);
  bi_pair(p, a0, a1, O, first, cand, 0);
  if (nrefs > 2) {
    int a2[4][4];
    bi_hyp<2>(p, cd, sx, sy, s_coef, a2);
    bi_pair(p, a0, a2, O, first, cand, 1);
    bi_pair(p, a1, a2, O, first, cand, 3);
    if (nrefs > 3) {
      int a3[4][4];
      bi_hyp<3>(p, cd, sx, sy, s_coef, a3);
      bi_pair(p, a0, a3, O, first, cand, 2);
      bi_pair(p, a1, a3, O, first, cand, 4);
      bi_pair(p, a2, a3, O, first, cand, 5);
    }
  }
}

// PT = BiRowsParamsP: the rate against the row's predictor of refIdx R (its mvp
// entry, LT = RT = LB); false when that predictor is out of range.
template <int R, class PT>
__device__ __forceinline__ bool bi_rate(const PT& p, int align, int row, int& m, int& bits) {
  m = bi_model<R>(p, align, row);
  int cp[6];
  bi_load_cp<R>(p, align, m, row, cp);
  if constexpr (std::is_same<PT, BiRowsParamsP>::value) {
    const int32_t* mvp = align ? p.mvp[R][1] : p.mvp[R][0];
    const int qx = mvp[2 * (size_t)row], qy = mvp[2 * (size_t)row + 1];
    if (!mc_mv_ok(qx) || !mc_mv_ok(qy)) return false;
    const int P[6] = {qx, qy, qx, qy, qx, qy};
    bits = affine_bits_p(cp, P, 2 + m) + kRuiBits;
  } else {
    bits = affine_bits(cp, 2 + m) + kRuiBits;
  }
  return true;
}

template <class PT>
__global__ __launch_bounds__(kBiThreads) void bipred_close_kernel(PT p) {
  const int cand = p.candBegin + blockIdx.x * kBiThreads + threadIdx.x;
  if (cand >= p.candEnd) return;
  const BiCand cd = p.cands[cand];
  const int align = (cd.shape >> 8) & 1, row = cd.row;
  int m[4] = {0, 0, 0, 0}, bits[4] = {0, 0, 0, 0};
  bool ok = bi_rate<0>(p, align, row, m[0], bits[0]);
  ok = bi_rate<1>(p, align, row, m[1], bits[1]) && ok;
  if (p.nrefs > 2) ok = bi_rate<2>(p, align, row, m[2], bits[2]) && ok;
  if (p.nrefs > 3) ok = bi_rate<3>(p, align, row, m[3], bits[3]) && ok;
  if (!ok) return;  // vame_bipred_p: a row with a predictor out of range keeps INT64_MAX / -1
  long long best = kBiInf;
  int sel = -1;
  int pair = 0;
#pragma unroll
  for (int r0 = 0; r0 < 3; r0++)
#pragma unroll
    for (int r1 = r0 + 1; r1 < 4; r1++, pair++) {
      if (r1 >= p.nrefs) continue;
      const long long v = p.pairSatd[(size_t)cand * kBiPairs + pair] + mc_rate(p.lambda, bits[r0] + bits[r1]);
      if (v < best) {
        best = v;
        sel = r0 + 4 * m[r0] + 8 * r1 + 32 * m[r1];
      }
    }
  p.biCost[align][row] = best;
  p.biSel[align][row] = sel;
}

template <class PT>
static hipError_t bipred_launch_t(const PT& p, hipStream_t stream) {
  const int nCand = p.candEnd - p.candBegin, nGroups = p.groupEnd - p.groupBegin;
  const int nInit = std::max(std::max(p.biCost[0] ? p.rowsOf[0] : 0, p.biCost[1] ? p.rowsOf[1] : 0), nCand * kBiPairs);
  if (nInit > 0)
    hipLaunchKernelGGL(bipred_init_kernel, dim3((nInit + kBiThreads - 1) / kBiThreads), dim3(kBiThreads), 0, stream,
                       static_cast<const BiRowsParams&>(p));
  if (p.nrefs >= 2 && nCand > 0) {
    hipLaunchKernelGGL(bipred_rows_kernel, dim3((nGroups + kBiThreads / 16 - 1) / (kBiThreads / 16)), dim3(kBiThreads),
                       0, stream, static_cast<const BiRowsParams&>(p));
    hipLaunchKernelGGL(bipred_close_kernel<PT>, dim3((nCand + kBiThreads - 1) / kBiThreads), dim3(kBiThreads), 0, stream,
                       p);
  }
  return hipGetLastError();
}
hipError_t bipred_launch(const BiRowsParams& p, hipStream_t stream) { return bipred_launch_t(p, stream); }
hipError_t bipred_p_launch(const BiRowsParamsP& p, hipStream_t stream) { return bipred_launch_t(p, stream); }

}  // namespace vame

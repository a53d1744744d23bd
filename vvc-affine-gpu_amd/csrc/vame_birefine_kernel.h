// vame_birefine_kernel.h -- birefine_kernel, the kernel of vame_bipred_refine
// (PT = BiRefineParams; instantiated in vame_birefine.hip) and of
// vame_bipred_refine_p (PT = BiRefineParamsP; instantiated in
// vame_birefine_p.hip, a unit of its own, so that the unit of the call without
// predictors compiles to the code it always compiled to).  The
// description of the kernel is vame_birefine.hip's.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "vame_birefine.h"
#include "vame_refine_core.h"

namespace vame {

// NT lanes, SB sub-blocks per lane: sub-block tid + q * NT, q < SB, so a lane's
// sub-blocks share their column (NT is a multiple of the CU's sub-block row).
// PT = BiRefineParamsP: vame_bipred_refine_p, hypothesis h's rate against its
// predictor preds[2i + h] (affine_bits_p) in the start cost and in every
// comparison; an invalid predictor makes the descriptor invalid.
template <int NT, int SB, class PT>
__global__ __launch_bounds__(NT) void birefine_kernel(PT p) {
  constexpr bool MVP = std::is_same<PT, BiRefineParamsP>::value;
  __shared__ uint4 s_coef[48];
  __shared__ uint2 s_pm[NT * SB * 4];  // P_m, int16 [h][w]: 16 samples per sub-block
  __shared__ long long s_V[kNumMom];
  __shared__ double s_M[42];
  __shared__ unsigned long long s_sum;
  const int tid = threadIdx.x, i = blockIdx.x;
  if (i >= mc_ncus(p.ncusDev, p.maxCus)) return;
  const McBiCu cu = p.cus[i];
  // vame_affine_mc_bi's validity rules
  bool ok = mc_size_ok(cu.w) && mc_size_ok(cu.h) && cu.x >= 0 && cu.y >= 0 && ((cu.x | cu.y) & 3) == 0;
  ok = ok && cu.x <= p.W - cu.w && cu.y <= p.H - cu.h;  // after the size test: no overflow
  ok = ok && cu.ref0 >= 0 && cu.ref0 < p.nrefs && mc_cp_ok(cu.ncps0, cu.c0);
  ok = ok && cu.ref1 >= -1 && cu.ref1 < p.nrefs;
  if (cu.ref1 >= 0) ok = ok && mc_cp_ok(cu.ncps1, cu.c1);
  if constexpr (MVP) ok = ok && mvp_cu_ok(cu, p.preds, i);
  const int nsb = ok ? (cu.w * cu.h) >> 4 : 0;  // an invalid descriptor goes with the smallest class
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
  int bA[6], bB[6];  // best CPMVs of hypothesis 0 / 1
#pragma unroll
  for (int k = 0; k < 6; k++) {
    bA[k] = cu.c0[k];
    bB[k] = cu.c1[k];
  }
  MvPred<MVP> pA, pB;  // the predictors of hypothesis 0 / 1
  if constexpr (MVP) {
    pA.load(p.preds + (size_t)i * 2 * kMvpWords);
    pB.load(p.preds + ((size_t)i * 2 + (cu.ref1 >= 0)) * kMvpWords);  // uni: the second is not read
  }
  const uint16_t* __restrict__ ref0 =
      cu.ref0 == 0 ? p.refs[0] : cu.ref0 == 1 ? p.refs[1] : cu.ref0 == 2 ? p.refs[2] : p.refs[3];
  const uint16_t* __restrict__ ref1 =
      cu.ref1 == 0 ? p.refs[0] : cu.ref1 == 1 ? p.refs[1] : cu.ref1 == 2 ? p.refs[2] : p.refs[3];

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

  // A uni descriptor (copied through with vame_affine_mc's cost) and rounds = 0
  // are round 0 cut after its first cost: hypothesis 0 held, and for a bi
  // descriptor hypothesis 1 predicted as given.  There is one prediction site:
  // step -1 of a round predicts the fixed hypothesis, steps 0 .. niter the
  // moving one.
  const bool uni = cu.ref1 < 0;
  const int nrounds = (uni || p.rounds == 0) ? 1 : p.rounds;
  long long bestCost = 0x7fffffffffffffffll;  // round 0's first cost, the descriptor's own, always replaces it

#pragma unroll 1
  for (int t = 0; t < nrounds; t++) {
    const bool m1 = (t & 1) == 0;  // round 0 moves hypothesis 1
    int cf[6], cc[6];              // the fixed hypothesis, the moving one's current CPMVs
#pragma unroll
    for (int k = 0; k < 6; k++) {
      cf[k] = m1 ? bA[k] : bB[k];
      cc[k] = m1 ? bB[k] : bA[k];
    }
    const int nF = m1 ? cu.ncps0 : cu.ncps1, nM = m1 ? cu.ncps1 : cu.ncps0;
    const uint16_t* __restrict__ refF = m1 ? ref0 : ref1;
    const uint16_t* __restrict__ refM = m1 ? ref1 : ref0;
    const int bitsF = (m1 ? pA : pB).bits(cf, nF) + kRuiBits;
    const int niter = (uni || p.rounds == 0) ? 0 : nM == 3 ? 4 : 5;
    int accF[SB][4][4] = {};
    uint2 Of[SB][4] = {};  // 2 cur - P_fixed, packed int16
#pragma unroll 1
    for (int it = -1;; it++) {
      const bool fix = it < 0;
      // the lane's geometry is loop-invariant: hidden from the optimizer, or every
      // address and monomial derived from it is hoisted and held across the loop
      int sx = sx0, sy = sy0;
      opaque(sx);
      opaque(sy);
      int s = 0;
      if (active) {
        int cx[6];
#pragma unroll
        for (int k = 0; k < 6; k++) cx[k] = fix ? cf[k] : cc[k];
#pragma unroll
        for (int q = 0; q < SB; q++) {
          if (q >= nq) break;
          const int syq = sy + q * syStep;
          int acc[4][4];
          mc_hyp_acc(fix ? refF : refM, cu.x, cu.y, lw, lh, cx, fix ? nF : nM, sx, syq, W, H, s_coef, acc);
          if (fix) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
              int d[4];
#pragma unroll
              for (int c = 0; c < 4; c++) {
                accF[q][r][c] = acc[r][c];
                const unsigned o = c < 2 ? O[q][r].x : O[q][r].y;
                d[c] = 2 * (int)((c & 1) ? o >> 16 : o & 0xFFFFu) - clampi(acc[r][c] >> 10, 0, 1023);
              }
              Of[q][r] = make_uint2(pack16(d[0], d[1]), pack16(d[2], d[3]));
            }
          }
          if (!fix || uni) {  // uni: (2 * acc) >> 11 == acc >> 10, the cost below is vame_affine_mc's
            uint2 P[4];
            mc_bi_pack(acc, accF[q], P);
            s += satd_4x4(O[q], P);
            // P_m for the gradient step (unused after the last cost)
#pragma unroll
            for (int r = 0; r < 4; r++)
              s_pm[((syq + r) * cu.w + sx) >> 2] =
                  make_uint2(pack16(clampi(acc[r][0] >> 10, 0, 1023), clampi(acc[r][1] >> 10, 0, 1023)),
                             pack16(clampi(acc[r][2] >> 10, 0, 1023), clampi(acc[r][3] >> 10, 0, 1023)));
          }
        }
      }
      if (fix) {
        if (!uni) continue;
        it = 0;
      }
      const int bitsM = uni ? 0 : (m1 ? pB : pA).bits(cc, nM) + kRuiBits;
      const long long cost = br_block_sum<NT>(s, &s_sum) + mc_rate(p.lambda, bitsM + bitsF);
      if (cost < bestCost) {
        bestCost = cost;
        if (!uni) {
#pragma unroll
          for (int k = 0; k < 6; k++) {
            if (m1)
              bB[k] = cc[k];
            else
              bA[k] = cc[k];
          }
        }
      }
      if (it == niter) break;

      // one step of the search's update on P_m with e = 2 cur - P_f - P_m
      const bool moved = br_step<NT, SB>(s_pm, Of, s_V, s_M, g, nM, active, nq, sx, sy, syStep, W, H, cc);
      // unchanged CPMVs repeat this iteration's prediction and cost: never strictly better
      if (!moved) break;
    }
  }
  if (tid == 0) {
    McBiCu o = cu;
#pragma unroll
    for (int k = 0; k < 6; k++) {
      o.c0[k] = bA[k];
      o.c1[k] = bB[k];
    }
    p.out[i] = o;
    p.cost[i] = bestCost;
  }
}

template <class PT>
inline hipError_t birefine_launch_t(const PT& p, hipStream_t stream) {
  hipLaunchKernelGGL((birefine_kernel<64, 1, PT>), dim3(p.maxCus), dim3(64), 0, stream, p);
  hipLaunchKernelGGL((birefine_kernel<256, 1, PT>), dim3(p.maxCus), dim3(256), 0, stream, p);
  hipLaunchKernelGGL((birefine_kernel<512, 2, PT>), dim3(p.maxCus), dim3(512), 0, stream, p);
  return hipGetLastError();
}
}  // namespace vame

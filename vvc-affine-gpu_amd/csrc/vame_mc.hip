// vame_mc.hip -- affine motion compensation of caller-given CPMVs
// (vame_affine_mc, include/vame.h): the prediction and the cost of one
// prediction step of the search (vame_dev.h: mv_field, filter_rows_global,
// prof_refine, satd_4x4, affine_bits), for any list of CUs.
//
// Work mapping: one lane per 4x4 sub-block over the
// concatenation of every valid descriptor's sub-blocks.  A CU holds 16 .. 1024
// sub-blocks, always a multiple of 16, so with the exclusive prefix sum of the
// per-descriptor counts every aligned group of 16 lanes -- one DPP row --
// belongs to exactly one CU: the CU's SATD is a DPP row sum and one 64-bit
// atomic add per row (integer sums: the order is free, costs are
// deterministic).  Three launches on the caller's stream, none of which reads
// anything on the host; the first two and the launch sequence are
// vame_mc_core.h's, shared with vame_affine_mc_bi:
//   mc_count_kernel    validate each descriptor, count its sub-blocks (0 for
//                      an invalid one), zero its cost, flag `bad`; exclusive
//                      scan of the counts inside blocks of 1024 descriptors
//   mc_offsets_kernel  add the sum of the blocks before; the total goes to
//                      offs[ncus]
// (vame_affine_mc_dev: ncus is read from device memory by each kernel and
// clamped to the capacity that sized the grids)
//   mc_predict_kernel  grid-strided over the total (read from device memory);
//                      a lane finds its CU by binary search in the offsets
// Windows are read straight from the frame (filter_rows_global: aligned
// dwords, per-sample clamped loads at the left / right edge); there is no
// staged tile: a CU is predicted once, not once per iteration.
#include <hip/hip_runtime.h>

#include "vame_mc_core.h"

namespace vame {

// One prediction of the search for sub-block g of the concatenation: the
// hypothesis (mc_hyp_acc), then the reference's rounding and clipPel
// (aux_functions.cl:1096-1239) or PROF where the search applies it; then the
// prediction's store and / or its SATD against the original and the rate of
// the CPMVs (affine.cl:416-446).
template <bool PROF>
__global__ __launch_bounds__(kMcThreads) void mc_predict_kernel(McParams p) {
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
    const McCu cu = p.cus[lo];
    const int local = g - p.offs[lo];
    const int lw = 31 - __clz(cu.w), lh = 31 - __clz(cu.h);
    const int sx = (local & ((cu.w >> 2) - 1)) << 2, sy = (local >> (lw - 2)) << 2;
    const int cp[6] = {cu.ltx, cu.lty, cu.rtx, cu.rty, cu.lbx, cu.lby};
    // the hypothesis, open-coded: it is mc_hyp_acc (vame_mc_core.h) statement for
    // statement and has to stay so (test_uni_descriptors_equal_affine_mc,
    // tests/test_gpu_bipred.py, compares the two bit for bit); PROF below needs
    // f, fx, fy, wx, wy, and the function form costs this kernel's PROF instance
    // a wave of occupancy
    const MvField f = mv_field(cp, cu.ncps, lw, lh);
    const uint16_t* __restrict__ ref =
        cu.ref == 0 ? p.refs[0] : cu.ref == 1 ? p.refs[1] : cu.ref == 2 ? p.refs[2] : p.refs[3];

    const int px = f.spread ? (cu.w >> 1) : sx + 2, py = f.spread ? (cu.h >> 1) : sy + 2;
    // |h|, |v| <= 2^21 (components within [-2^17, 2^17), << (7 - log2 size)),
    // px, py <= 128: the 24-bit products are exact
    int mx = f.bx + __mul24(f.hx, px) + __mul24(f.vx, py);
    int my = f.by + __mul24(f.hy, px) + __mul24(f.vy, py);
    mx = (mx + 64 - (mx >= 0)) >> 7;  // roundMv (aux_functions.cl:38-47)
    my = (my + 64 - (my >= 0)) >> 7;
    // clipMv (aux_functions.cl:51-67) on the frame position of the MV's target, as predict_sb
    const int ax = clampi(mx + shl(cu.x, 4), -135 * 16, (W + 7) * 16);
    const int ay = clampi(my + shl(cu.y, 4), -135 * 16, (H + 7) * 16);
    const int fx = ax & 15, fy = ay & 15;
    const int wx = (ax >> 4) + sx - 2, wy = (ay >> 4) + sy - 2;  // window origin (frame)

    const uint4 KA = s_coef[fx * 3], KB = s_coef[fx * 3 + 1];  // even window start: parity-0 taps
    int acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
      for (int c = 0; c < 4; c++) acc[r][c] = 524800;  // (1 << 9) + (8192 << 6)
    filter_rows_global(ref, wx, wy, W, H, KA, KB, reinterpret_cast<const unsigned*>(s_coef), fy, acc);
    int pr[4][4];
    if (PROF && !f.spread) {  // applyPROF = enablePROF && !isSpread (aux_functions.cl:1101)
      prof_refine(acc, f, fx, fy,
                  [&](int r, int c) {
                    return (int)ref[(size_t)clampi(wy + r, 0, H - 1) * W + clampi(wx + c, 0, W - 1)];
                  },
                  pr);
    } else {
#pragma unroll
      for (int r = 0; r < 4; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) pr[r][c] = clampi(acc[r][c] >> 10, 0, 1023);  // clipPel
    }
    uint2 P[4];
#pragma unroll
    for (int r = 0; r < 4; r++) P[r] = make_uint2(pack16(pr[r][0], pr[r][1]), pack16(pr[r][2], pr[r][3]));

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
      // the CU's first lane adds floor(lambda * (bits + 2)) (affine.cl:442-446)
      if (local == 0) v += mc_rate(p.lambda, affine_bits(cp, cu.ncps) + kRuiBits);
      if ((local & 15) == 0) atomicAdd(reinterpret_cast<unsigned long long*>(p.cost + lo), (unsigned long long)v);
    }
  }
}

hipError_t mc_launch(const McParams& p, bool prof, hipStream_t stream) {
  return mc_launch_concat(p, prof ? mc_predict_kernel<true> : mc_predict_kernel<false>, stream);
}

}  // namespace vame

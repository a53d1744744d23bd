// vame_mc.hip -- affine motion compensation of caller-given CPMVs
// (vame_affine_mc, include/vame.h): the prediction and the cost of one
// prediction step of the search (vame_kernel.h: mv_field, filter_rows_global,
// prof_refine, satd_4x4, affine_bits), for any list of CUs.
//
// Work mapping: one lane per 4x4 sub-block over the
// concatenation of every valid descriptor's sub-blocks.  A CU holds 16 .. 1024
// sub-blocks, always a multiple of 16, so with the exclusive prefix sum of the
// per-descriptor counts every aligned group of 16 lanes -- one DPP row --
// belongs to exactly one CU: the CU's SATD is a DPP row sum and one 64-bit
// atomic add per row (integer sums: the order is free, costs are
// deterministic).  Three launches on the caller's stream, none of which reads
// anything on the host:
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

#include <algorithm>

#include "vame_kernel.h"

namespace vame {

constexpr int kMcScanBlock = 1024;  // descriptors per scan block (one per thread)
constexpr int kMcThreads = 256;     // prediction workgroups
constexpr int kMcMaxBlocks = 2048;  // prediction grid (grid-strided beyond it)
static_assert(kMcMaxCus <= kMcScanBlock * kMcScanBlock, "two scan levels");
static_assert(sizeof(McCu) == 48, "vame_mc_cu layout");

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

__device__ __forceinline__ bool mc_size_ok(int v) { return v == 16 || v == 32 || v == 64 || v == 128; }
__device__ __forceinline__ bool mc_mv_ok(int v) { return v >= kMvMin && v <= kMvMax; }

// The descriptors of a call: p.ncus, or the device-side count of
// vame_affine_mc_dev clamped to [0, p.ncus].
__device__ __forceinline__ int mc_ncus(const McParams& p) {
  return p.ncusDev ? min(max(*p.ncusDev, 0), p.ncus) : p.ncus;
}

__global__ __launch_bounds__(kMcScanBlock) void mc_count_kernel(McParams p) {
  __shared__ int s_wave[kMcScanBlock / 64];
  const int i = blockIdx.x * kMcScanBlock + threadIdx.x;
  const int ncus = mc_ncus(p);
  int n = 0;
  bool flag = false;
  if (i < ncus) {
    const McCu cu = p.cus[i];
    bool ok = mc_size_ok(cu.w) && mc_size_ok(cu.h) && cu.x >= 0 && cu.y >= 0 && ((cu.x | cu.y) & 3) == 0;
    ok = ok && cu.x <= p.W - cu.w && cu.y <= p.H - cu.h;  // after the size test: no overflow
    ok = ok && cu.ref >= 0 && cu.ref < p.nrefs && (cu.ncps == 2 || cu.ncps == 3);
    ok = ok && mc_mv_ok(cu.ltx) && mc_mv_ok(cu.lty) && mc_mv_ok(cu.rtx) && mc_mv_ok(cu.rty);
    if (cu.ncps == 3) ok = ok && mc_mv_ok(cu.lbx) && mc_mv_ok(cu.lby);
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
__global__ __launch_bounds__(kMcScanBlock) void mc_offsets_kernel(McParams p) {
  __shared__ int s_wave[kMcScanBlock / 64];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int ncus = mc_ncus(p);
  int base;
  block_scan_1024(tid < b ? p.blockSum[tid] : 0, s_wave, base);
  const int i = b * kMcScanBlock + tid;
  if (i < ncus) p.offs[i] += base;
  // scan blocks past a device-side count hold no sub-blocks
  if (b == (int)gridDim.x - 1 && tid == 0) p.offs[ncus] = base + p.blockSum[b];
}

// Sum over the 16 lanes of a DPP row, in every lane of the row.
__device__ __forceinline__ int row_sum16(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true);   // quad_perm:[1,0,3,2]
  v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, true);   // quad_perm:[2,3,0,1]
  v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, true);  // row_half_mirror
  v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, true);  // row_mirror
  return v;
}

// One prediction of the search for sub-block g of the concatenation: sub-block
// MV and spread test (affine.cl:215-252), roundAndClipMv against the CU
// position, clamp-to-edge window (affine.cl:254-326), 6-tap filter with the
// reference's rounding and clipPel (aux_functions.cl:1096-1239), PROF where
// the search applies it; then the prediction's store and / or its SATD
// against the original and the rate of the CPMVs (affine.cl:416-446).
template <bool PROF>
__global__ __launch_bounds__(kMcThreads) void mc_predict_kernel(McParams p) {
  __shared__ uint4 s_coef[48];
  const int tid = threadIdx.x;
  if (tid < 48) s_coef[tid] = reinterpret_cast<const uint4*>(&kCoefTab)[tid];
  __syncthreads();
  const int W = p.W, H = p.H;
  const int ncus = mc_ncus(p);
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
      if (local == 0) v += (long long)(int)floorf(__fmul_rn(p.lambda, (float)(affine_bits(cp, cu.ncps) + kRuiBits)));
      if ((local & 15) == 0) atomicAdd(reinterpret_cast<unsigned long long*>(p.cost + lo), (unsigned long long)v);
    }
  }
}

hipError_t mc_launch(const McParams& p, bool prof, hipStream_t stream) {
  const int nb = (p.ncus + kMcScanBlock - 1) / kMcScanBlock;
  hipLaunchKernelGGL(mc_count_kernel, dim3(nb), dim3(kMcScanBlock), 0, stream, p);
  hipLaunchKernelGGL(mc_offsets_kernel, dim3(nb), dim3(kMcScanBlock), 0, stream, p);
  // at most 1024 sub-blocks per descriptor: 4 workgroups
  const int grid = (int)std::min<long long>(4ll * p.ncus, kMcMaxBlocks);
  if (prof)
    hipLaunchKernelGGL(mc_predict_kernel<true>, dim3(grid), dim3(kMcThreads), 0, stream, p);
  else
    hipLaunchKernelGGL(mc_predict_kernel<false>, dim3(grid), dim3(kMcThreads), 0, stream, p);
  return hipGetLastError();
}

}  // namespace vame

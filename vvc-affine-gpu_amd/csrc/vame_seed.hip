// vame_seed.hip -- integer-pel seed search (vame_seed_search; include/vame.h,
// DESIGN.md §15): for every candidate CU of a CTU the integer displacement of
// the smallest SAD + rate inside +-radius.
//
// Every candidate CU, aligned or half-aligned, is a union of 8x8 blocks on the
// CTU's 8-sample grid, so one displacement costs the CTU's 256 block SADs once
// and every CU is four reads of their 16x16 summed-area table.
//
//   seed_init_kernel   INT64_MAX / (0, 0) into every row of the (refIdx,
//                      alignment) pairs in the mask
//   seed_sad_kernel    one workgroup per (CTU, refIdx, dy), one lane per 8x8
//                      block.  The lane holds its 64 cur samples in registers
//                      (32 packed dwords); the reference strip of the CTU's
//                      128 rows at dy, 128 + 2 radius samples wide, clamped to
//                      the frame edges while staged, lies in LDS (50 KB).  The
//                      dx run in batches of eight: per row two 16-byte LDS
//                      reads give the 16 samples that serve all eight (the odd
//                      ones through v_alignbit), 32 v_sad_u16 per row.  Per
//                      batch: row prefix in a DPP row (a block row is one),
//                      column prefix by 128 lanes, then every lane prices its
//                      two candidates (485 per CTU) for the eight dx and keeps
//                      the minimum of cost << 13 | order index in registers.
//                      At the end one 64-bit atomic minimum per candidate into
//                      its cost entry: the minimum over the dy workgroups in
//                      any order is the first minimum of the rule's order.
//   seed_close_kernel  one lane per row: key -> cost and mv
//
// Bounds: a strip row holds 200 samples (128 + 64 + 8: the last batch's reads
// run up to 7 samples past the widest window); a lane's reads end at sample
// (15 + 8) * 8 + 15 = 199.  Costs stay below 2^25 + |rate| < 2^32, keys below
// 2^45; the order index is at most 65^2 = 4225 < 2^13.
#include "vame_seed.h"

#include "vame_mc_core.h"

namespace vame {

constexpr int kSeedThreads = 256;
constexpr int kSeedPitch = 200;  // samples per strip row
constexpr int kSeedBatch = 8;    // dx per batch
constexpr int kSeedCands = kFullCusPerCtu + kHalfCusPerCtu;
constexpr long long kSeedInf = 0x7fffffffffffffffll;

// The CTU's candidates: bx | by << 4 | bw << 8 | bh << 13 (8-sample units) |
// output offset << 18 | align << 27.
struct SeedTab {
  uint32_t v[kSeedCands];
};
constexpr SeedTab make_seed_tab() {
  SeedTab t{};
  int n = 0;
  for (int g = 0; g < kFullGroups; g++) {
    const int w = kFullW[g], h = kFullH[g], per = kCtu / w;
    for (int k = 0; k < (kCtu * kCtu) / (w * h); k++)
      t.v[n++] = (uint32_t)((k % per) * w / 8) | (uint32_t)((k / per) * h / 8) << 4 | (uint32_t)(w / 8) << 8 |
                 (uint32_t)(h / 8) << 13 | (uint32_t)(kFullStride[g] + k) << 18;
  }
  for (int g = 0; g < kHalfGroups; g++)
    for (int k = 0; k < kHalfN[g]; k++)
      t.v[n++] = (uint32_t)kHalfX8[g][k] | (uint32_t)kHalfY8[g][k] << 4 | (uint32_t)(kHalfW[g] / 8) << 8 |
                 (uint32_t)(kHalfH[g] / 8) << 13 | (uint32_t)(kHalfStride[g] + k) << 18 | 1u << 27;
  return t;
}
static __constant__ SeedTab kSeedTab = make_seed_tab();

template <class T>
__device__ __forceinline__ T seed_sel(T const (&a)[4][2], int r, int align) {
  T v = a[0][0];
#pragma unroll
  for (int rr = 0; rr < 4; rr++)
#pragma unroll
    for (int aa = 0; aa < 2; aa++)
      if (rr == r && aa == align) v = a[rr][aa];
  return v;
}

__global__ __launch_bounds__(kSeedThreads) void seed_init_kernel(SeedParams p) {
  const int i = blockIdx.x * kSeedThreads + threadIdx.x;
#pragma unroll
  for (int r = 0; r < 4; r++)
#pragma unroll
    for (int a = 0; a < 2; a++)
      if (p.cost[r][a] && i < p.nCtus * (a ? kHalfCusPerCtu : kFullCusPerCtu)) {
        p.cost[r][a][i] = kSeedInf;
        p.mv[r][a][2 * i] = 0;
        p.mv[r][a][2 * i + 1] = 0;
      }
}

// inclusive prefix of v over the 16 lanes of a DPP row
__device__ __forceinline__ int seed_row_prefix(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, true);  // row_shr:1
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, true);  // row_shr:2
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, true);  // row_shr:4
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, true);  // row_shr:8
  return v;
}

__global__ __launch_bounds__(kSeedThreads) void seed_sad_kernel(SeedParams p) {
  __shared__ uint4 s_strip[kCtu * kSeedPitch / 8];
  __shared__ int s_sat[kSeedBatch][17][17];  // row 0 and column 0 stay zero
  __shared__ int s_rate[2 * kSeedMaxRadius + 1];
  const int tid = threadIdx.x, bx = tid & 15, by = tid >> 4;
  const int ctu = blockIdx.x, r = blockIdx.y, R = p.radius, dy = (int)blockIdx.z - R;
  const int W = p.W, H = p.H, span = 2 * R + 1;
  const int x0 = (ctu % p.ctusPerRow) * kCtu, y0 = (ctu / p.ctusPerRow) * kCtu;
  const uint16_t* __restrict__ ref = r == 0 ? p.refs[0] : r == 1 ? p.refs[1] : r == 2 ? p.refs[2] : p.refs[3];

  // the strip: sample c of row j is ref[clamp(y0 + dy + j)][clamp(x0 - R + c)]
  {
    unsigned* s32 = reinterpret_cast<unsigned*>(s_strip);
    const int ncw = (kCtu + 2 * R + 8) / 2;  // dwords per row that are read for a dx in range
    for (int idx = tid; idx < kCtu * ncw; idx += kSeedThreads) {
      const int j = idx / ncw, cw = idx - j * ncw;
      const int gy = clampi(y0 + dy + j, 0, H - 1), gx = x0 - R + 2 * cw;
      const uint16_t* row = ref + (size_t)gy * W;
      unsigned v;
      if (!(gx & 1) && gx >= 0 && gx + 1 < W)
        v = *reinterpret_cast<const unsigned*>(row + gx);  // frames are 4-byte aligned, W is even
      else
        v = (unsigned)row[clampi(gx, 0, W - 1)] | (unsigned)row[clampi(gx + 1, 0, W - 1)] << 16;
      s32[j * (kSeedPitch / 2) + cw] = v;
    }
    for (int idx = tid; idx < kSeedBatch * 17 * 17; idx += kSeedThreads) (&s_sat[0][0][0])[idx] = 0;
    if (tid < span) {
      const int d = shl(tid - R, 4);
      const int cp[6] = {d, shl(dy, 4), d, shl(dy, 4), 0, 0};
      s_rate[tid] = (int)mc_rate(p.lambda, affine_bits(cp, 2) + kRuiBits);
    }
  }

  // the lane's 8x8 block of cur; a block that leaves the frame counts 0 (no
  // candidate in the frame holds it)
  const bool blockIn = x0 + bx * 8 + 8 <= W && y0 + by * 8 + 8 <= H;
  unsigned C[8][4] = {};
  if (blockIn) {
    const char* base = reinterpret_cast<const char*>(p.cur);  // 8-byte aligned, x a multiple of 8
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const size_t off = ((size_t)(y0 + by * 8 + j) * W + x0 + bx * 8) * 2u;
      const uint2 a = *reinterpret_cast<const uint2*>(base + off), b = *reinterpret_cast<const uint2*>(base + off + 8);
      C[j][0] = a.x; C[j][1] = a.y; C[j][2] = b.x; C[j][3] = b.y;
    }
  }

  // the lane's two candidates
  int cx0[2], cy0[2], cx1[2], cy1[2], dxMax[2];
  long long* dst[2];
  long long best[2] = {kSeedInf, kSeedInf};
#pragma unroll
  for (int q = 0; q < 2; q++) {
    const int k = tid + q * kSeedThreads;
    const unsigned e = kSeedTab.v[min(k, kSeedCands - 1)];
    const int align = (int)(e >> 27) & 1;
    cx0[q] = (int)(e & 15);
    cy0[q] = (int)(e >> 4) & 15;
    cx1[q] = cx0[q] + ((int)(e >> 8) & 31);
    cy1[q] = cy0[q] + ((int)(e >> 13) & 31);
    const int x = x0 + cx0[q] * 8, y = y0 + cy0[q] * 8;
    int64_t* c = seed_sel(p.cost, r, align);
    const bool ok = k < kSeedCands && c && x0 + cx1[q] * 8 <= W && y0 + cy1[q] * 8 <= H && dy <= H + 7 - y;
    dxMax[q] = W + 7 - x;
    dst[q] = ok ? reinterpret_cast<long long*>(c) + ((size_t)ctu * (align ? kHalfCusPerCtu : kFullCusPerCtu) + ((e >> 18) & 511)) : nullptr;
  }
  __syncthreads();

  const int nb = (span + kSeedBatch - 1) / kSeedBatch;
#pragma unroll 1
  for (int kb = 0; kb < nb; kb++) {
    int acc[kSeedBatch] = {};
#pragma unroll
    for (int j = 0; j < 8; j++) {
      // samples (bx + kb) * 8 .. + 15 of strip row by * 8 + j: block column bx at offsets 8 kb .. 8 kb + 7
      const uint4* rp = s_strip + ((by * 8 + j) * (kSeedPitch / 8) + bx + kb);
      const uint4 lo = rp[0], hi = rp[1];
      const unsigned D[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
      unsigned Dodd[7];
#pragma unroll
      for (int m = 0; m < 7; m++) Dodd[m] = __builtin_amdgcn_alignbit(D[m + 1], D[m], 16);
#pragma unroll
      for (int o = 0; o < kSeedBatch; o++)
#pragma unroll
        for (int q = 0; q < 4; q++)
          acc[o] = (int)__builtin_amdgcn_sad_u16(C[j][q], (o & 1) ? Dodd[(o >> 1) + q] : D[(o >> 1) + q], (unsigned)acc[o]);
    }
#pragma unroll
    for (int o = 0; o < kSeedBatch; o++) s_sat[o][by + 1][bx + 1] = seed_row_prefix(blockIn ? acc[o] : 0);
    __syncthreads();
    if (tid < kSeedBatch * 16) {
      int* col = &s_sat[tid >> 4][0][(tid & 15) + 1];
      int run = 0;
#pragma unroll
      for (int j = 1; j <= 16; j++) {
        run += col[j * 17];
        col[j * 17] = run;
      }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 2; q++) {
      if (!dst[q]) continue;
#pragma unroll
      for (int o = 0; o < kSeedBatch; o++) {
        const int oo = kb * kSeedBatch + o, dx = oo - R;
        if (oo >= span || dx > dxMax[q]) continue;
        const int sad = s_sat[o][cy1[q]][cx1[q]] - s_sat[o][cy0[q]][cx1[q]] - s_sat[o][cy1[q]][cx0[q]] +
                        s_sat[o][cy0[q]][cx0[q]];
        const long long cost = (long long)sad + s_rate[oo];
        const int order = (dx | dy) == 0 ? 0 : 1 + (dy + R) * span + oo;  // (0, 0) first, then dy outer, dx inner
        best[q] = min(best[q], cost * 8192 + order);
      }
    }
    __syncthreads();  // the table is free again
  }
#pragma unroll
  for (int q = 0; q < 2; q++)
    if (dst[q] && best[q] != kSeedInf) atomicMin(dst[q], best[q]);
}

__global__ __launch_bounds__(kSeedThreads) void seed_close_kernel(SeedParams p) {
  const int i = blockIdx.x * kSeedThreads + threadIdx.x;
  const int span = 2 * p.radius + 1;
#pragma unroll
  for (int r = 0; r < 4; r++)
#pragma unroll
    for (int a = 0; a < 2; a++)
      if (p.cost[r][a] && i < p.nCtus * (a ? kHalfCusPerCtu : kFullCusPerCtu)) {
        const long long key = p.cost[r][a][i];
        if (key == kSeedInf) continue;
        const int order = (int)(key & 8191);
        p.cost[r][a][i] = key >> 13;
        if (order) {
          const int t = order - 1, oy = t / span;
          p.mv[r][a][2 * i] = shl(t - oy * span - p.radius, 4);
          p.mv[r][a][2 * i + 1] = shl(oy - p.radius, 4);
        }
      }
}

hipError_t seed_launch(const SeedParams& p, hipStream_t stream) {
  const int rows = p.nCtus * kHalfCusPerCtu;
  const dim3 grid((rows + kSeedThreads - 1) / kSeedThreads), block(kSeedThreads);
  hipLaunchKernelGGL(seed_init_kernel, grid, block, 0, stream, p);
  hipLaunchKernelGGL(seed_sad_kernel, dim3(p.nCtus, p.nrefs, 2 * p.radius + 1), block, 0, stream, p);
  hipLaunchKernelGGL(seed_close_kernel, grid, block, 0, stream, p);
  return hipGetLastError();
}

}  // namespace vame

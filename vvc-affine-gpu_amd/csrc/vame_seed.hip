// vame_seed.hip -- the integer-pel seed searches (include/vame.h):
//   vame_seed_search: for every candidate CU of a CTU the
//   integer displacement of the smallest SAD + rate inside +-radius;
//   vame_seed_pyramid, vame_seed_search_wide (§16): the same search at the top
//   level L of a 2:1 mean pyramid, then +-1 around twice the winner at every
//   level below, down to the frame.
//
// Every candidate CU, aligned or half-aligned, is a union of 8x8 blocks on the
// CTU's 8-sample grid (blocks of B = 8 >> L samples at level L), so one
// displacement costs the CTU's 256 block SADs once and every CU is four reads
// of their 16x16 summed-area table.
//
//   seed_pyr_down_kernel  one lane per 8x4 samples of the frame: four dwords
//                         per row in, its 4x2 samples of level 1 (two 8-byte
//                         stores) and, from those values, its 2x1 samples
//                         of level 2 (one dword) out
//   seed_init_kernel      INT64_MAX / (0, 0) into every row of the (refIdx,
//                         alignment) pairs in the mask
//   seed_grid_kernel<L>   the exhaustive search at level L (0: the frames).
//                         One workgroup per (CTU, refIdx, dy), one lane per
//                         block.  The lane holds its B x B cur samples in
//                         registers (packed dwords: 32 at level 0); the
//                         reference strip of the CTU's N = 128 >> L rows at
//                         dy, N + 2 radius samples wide, clamped to the
//                         level's edges while staged, lies in LDS (50 KB at
//                         level 0).  The dx run in batches of eight: per row
//                         the B + 8 samples that serve all eight (two 16-byte
//                         LDS reads at level 0; the odd dx through
//                         v_alignbit), 4 B v_sad_u16 per row.  Per batch: row
//                         prefix in a DPP row (a block row is one), column
//                         prefix by 128 lanes, then every lane prices its two
//                         candidates (485 per CTU) for the eight dx and keeps
//                         the minimum of value << 15 | order index in
//                         registers.  At the end one 64-bit atomic minimum per
//                         candidate into its cost entry: the minimum over the
//                         dy workgroups in any order is the first minimum of
//                         the rule's order.
//   seed_close_kernel     levels = 0.  One lane per row: key -> cost and mv
//   seed_refine_kernel    levels > 0.  One workgroup per (16 slots of the
//                         CTU's plan, CTU, refIdx); a slot is a DPP row of 16
//                         lanes.  A candidate of 64x64 samples or more takes a
//                         whole wave, one of 64x32 / 32x64 two rows, every
//                         smaller one a single row: four small CUs to a
//                         wave, and the longest chain of dependent loads
//                         (the 128x128 CU's) a quarter of what 16 lanes
//                         would leave.  The candidate decodes its key, then
//                         for l = L-1 .. 0 sums the nine SADs around twice
//                         the winner above (at level 0 also the SAD of
//                         (0, 0)), takes the first minimum of the rule's
//                         order and finally writes cost and mv.  The lanes
//                         stride over (reference row, group of 8 columns):
//                         one reference segment of ten samples serves the
//                         three ex and, against the cur rows above, at and
//                         below it, the three ey.  No LDS: the window is
//                         read from the frame, clamped sample by sample
//                         only where it touches the frame's edge.
//
// Bounds: a strip row of the grid kernel holds N + 2 Rmax(L) + 8 samples
// (Rmax = 32, 64, 32 at L = 0, 1, 2: the largest radius >> L; the last batch's
// reads run up to 7 samples past the widest window); a lane's reads end at
// sample N + 8 nb - 1 <= N + 2 R + 7, all staged.  Values stay below
// 2^25 + |rate| < 2^32, keys below 2^47; the order index is at most
// 129^2 = 16641 < 2^15.
#include "vame_seed.h"

#include "vame_mc_core.h"

namespace vame {

constexpr int kSeedThreads = 256;
constexpr int kSeedBatch = 8;  // dx per batch
constexpr int kSeedCands = kFullCusPerCtu + kHalfCusPerCtu;
constexpr int kSeedKeyBits = 15;
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

// The refine kernel's plan of a CTU: slot = one DPP row of 16 lanes.  A
// candidate of at least 64x64 samples takes four slots (a whole wave), one of
// 64x32 or 32x64 two, every smaller one a single slot; the four-slot
// candidates come first, then the two-slot ones, so a candidate never
// straddles a wave.  Entry: candidate | slot of the candidate << 9 | its slots << 11.
constexpr int kPyrSlots = 544;  // 9 * 4 + 24 * 2 + 452 = 536, rounded up to whole workgroups of 16
struct SeedPyrPlan {
  uint16_t v[kPyrSlots];
  int n;
};
constexpr int pyr_cand_slots(uint32_t e) {
  const int area = (int)((e >> 8) & 31) * (int)((e >> 13) & 31);  // in 8x8 blocks
  return area >= 64 ? 4 : area >= 32 ? 2 : 1;
}
constexpr SeedPyrPlan make_seed_pyr_plan() {
  SeedPyrPlan t{};
  const SeedTab tab = make_seed_tab();
  for (int want = 4; want >= 1; want >>= 1)
    for (int k = 0; k < kSeedCands; k++)
      if (pyr_cand_slots(tab.v[k]) == want)
        for (int sub = 0; sub < want; sub++) t.v[t.n++] = (uint16_t)(k | sub << 9 | want << 11);
  for (int i = t.n; i < kPyrSlots; i++) t.v[i] = 0;  // no slots: idle
  return t;
}
static_assert(make_seed_pyr_plan().n == 536, "the plan's slots");
static __constant__ SeedPyrPlan kSeedPyrPlan = make_seed_pyr_plan();

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
__device__ __forceinline__ const uint16_t* seed_ref(const uint16_t* const (&a)[4], int r) {
  return r == 0 ? a[0] : r == 1 ? a[1] : r == 2 ? a[2] : a[3];
}

// ------------------------------------------------------------------ pyramid
// mean of the two samples of a and the two of b, rounded: (a.lo + a.hi + b.lo + b.hi + 2) >> 2
__device__ __forceinline__ unsigned pyr_mean(unsigned a, unsigned b) {
  return ((a & 0xFFFFu) + (a >> 16) + (b & 0xFFFFu) + (b >> 16) + 2u) >> 2;
}

__global__ __launch_bounds__(kSeedThreads) void seed_pyr_down_kernel(SeedPyrDownParams p) {
  const int perRow = p.W >> 3, i = blockIdx.x * kSeedThreads + threadIdx.x;
  if (i >= perRow * (p.H >> 2)) return;
  const int py = i / perRow, px = i - py * perRow;
  const int W1 = p.W >> 1, W2 = p.W >> 2;
  unsigned m[2][4];  // level 1: rows 2 py, 2 py + 1, samples 4 px .. 4 px + 3
#pragma unroll
  for (int rr = 0; rr < 2; rr++) {
    // frames are 4-byte aligned, W is a multiple of 8
    const unsigned* a = reinterpret_cast<const unsigned*>(p.frame + (size_t)(4 * py + 2 * rr) * p.W + 8 * px);
    const unsigned* b = reinterpret_cast<const unsigned*>(p.frame + (size_t)(4 * py + 2 * rr + 1) * p.W + 8 * px);
#pragma unroll
    for (int k = 0; k < 4; k++) m[rr][k] = pyr_mean(a[k], b[k]);
    *reinterpret_cast<uint2*>(p.pyr + (size_t)(2 * py + rr) * W1 + 4 * px) =
        make_uint2(m[rr][0] | m[rr][1] << 16, m[rr][2] | m[rr][3] << 16);
  }
  const unsigned lo = (m[0][0] + m[0][1] + m[1][0] + m[1][1] + 2u) >> 2;
  const unsigned hi = (m[0][2] + m[0][3] + m[1][2] + m[1][3] + 2u) >> 2;
  *reinterpret_cast<unsigned*>(p.pyr + pyr_level1_samples(p.W, p.H) + (size_t)py * W2 + 2 * px) = lo | hi << 16;
}

hipError_t seed_pyr_down_launch(const SeedPyrDownParams& p, hipStream_t stream) {
  const int n = (p.W >> 3) * (p.H >> 2);
  hipLaunchKernelGGL(seed_pyr_down_kernel, dim3((n + kSeedThreads - 1) / kSeedThreads), dim3(kSeedThreads), 0, stream, p);
  return hipGetLastError();
}

// ------------------------------------------------------------------ the search
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

// floor(lambda * (bits + 2)) of the 2-CP CPMVs LT = RT = (16 Dx, 16 Dy)
__device__ __forceinline__ long long seed_rate(float lambda, int Dx, int Dy) {
  const int cp[6] = {shl(Dx, 4), shl(Dy, 4), shl(Dx, 4), shl(Dy, 4), 0, 0};
  return mc_rate(lambda, affine_bits(cp, 2) + kRuiBits);
}

// the largest radius >> L: 32, 64, 32
constexpr int seed_rmax(int L) { return L ? kSeedWideMaxRadius >> L : kSeedMaxRadius; }

template <int L>
__global__ __launch_bounds__(kSeedThreads) void seed_grid_kernel(SeedParams p) {
  constexpr int B = 8 >> L;                               // samples per grid block side
  constexpr int N = kCtu >> L;                            // the CTU's side
  constexpr int PITCH = N + 2 * seed_rmax(L) + 8;         // samples per strip row
  constexpr int ND = 4 + B / 2;                           // dwords a lane reads per row and batch
  __shared__ uint4 s_strip4[N * PITCH / 8];  // 16-byte units: level 0 reads it so
  unsigned* const s_strip = reinterpret_cast<unsigned*>(s_strip4);
  __shared__ int s_sat[kSeedBatch][17][17];  // row 0 and column 0 stay zero
  __shared__ int s_rate[2 * seed_rmax(L) + 1];
  const int tid = threadIdx.x, bx = tid & 15, by = tid >> 4;
  const int ctu = blockIdx.x, r = blockIdx.y, R = p.radius >> L, dy = (int)blockIdx.z - R;
  const int W = p.W, H = p.H, Wl = W >> L, Hl = H >> L, span = 2 * R + 1;
  const int x0 = (ctu % p.ctusPerRow) * kCtu, y0 = (ctu / p.ctusPerRow) * kCtu;
  const int x0l = x0 >> L, y0l = y0 >> L;
  const size_t lvl = L == 2 ? pyr_level1_samples(W, H) : 0;
  const uint16_t* __restrict__ ref;
  const uint16_t* __restrict__ cur;
  if constexpr (L == 0) {
    // The three L == 0 places of this kernel (here, the cur address, the strip read) keep the level-0
    // instance at the code of the kernel it replaced (profiles/seed_unify_ab.txt, "what that took").
    // Here: written out, not seed_ref, through which the pointer is loaded from a selected address,
    // one dependent scalar load more per workgroup (measured there: 0.4-1.2 % of vame_seed_search).
    ref = r == 0 ? p.refs[0] : r == 1 ? p.refs[1] : r == 2 ? p.refs[2] : p.refs[3];
    cur = p.cur;
  } else {
    ref = seed_ref(p.refPyrs, r) + lvl;
    cur = p.curPyr + lvl;
  }

  // the strip: sample c of row j is ref[clamp(y0l + dy + j)][clamp(x0l - R + c)]
  {
    const int ncw = (N + 2 * R + 8) / 2;  // dwords per row that are read for a dx in range
    for (int idx = tid; idx < N * ncw; idx += kSeedThreads) {
      const int j = idx / ncw, cw = idx - j * ncw;
      const int gy = clampi(y0l + dy + j, 0, Hl - 1), gx = x0l - R + 2 * cw;
      const uint16_t* row = ref + (size_t)gy * Wl;
      unsigned v;
      if (!(gx & 1) && gx >= 0 && gx + 1 < Wl)
        v = *reinterpret_cast<const unsigned*>(row + gx);  // levels are 4-byte aligned, Wl is even
      else
        v = (unsigned)row[clampi(gx, 0, Wl - 1)] | (unsigned)row[clampi(gx + 1, 0, Wl - 1)] << 16;
      s_strip[j * (PITCH / 2) + cw] = v;
    }
    for (int idx = tid; idx < kSeedBatch * 17 * 17; idx += kSeedThreads) (&s_sat[0][0][0])[idx] = 0;
    if (tid < span) s_rate[tid] = (int)seed_rate(p.lambda, shl(tid - R, L), shl(dy, L));
  }

  // the lane's block of cur; a block that leaves the frame counts 0 (no
  // candidate in the frame holds it)
  const bool blockIn = x0 + bx * 8 + 8 <= W && y0 + by * 8 + 8 <= H;
  unsigned C[B][B / 2] = {};
  if (blockIn) {
#pragma unroll
    for (int j = 0; j < B; j++) {
      const size_t row = (size_t)(y0l + by * B + j) * Wl;
      const unsigned* a;
      if constexpr (L == 0)  // the same address from a byte offset: reproduces the replaced kernel's code, not timed alone
        a = reinterpret_cast<const unsigned*>(reinterpret_cast<const char*>(cur) + (row + x0l + bx * B) * 2u);
      else
        a = reinterpret_cast<const unsigned*>(cur + row + x0l + bx * B);
#pragma unroll
      for (int q = 0; q < B / 2; q++) C[j][q] = a[q];
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
    // admissible: Dy = dy << L <= H + 7 - y (|Dy| <= radius holds for every dy of the grid)
    const bool ok = k < kSeedCands && c && x0 + cx1[q] * 8 <= W && y0 + cy1[q] * 8 <= H && shl(dy, L) <= H + 7 - y;
    dxMax[q] = (W + 7 - x) >> L;  // dx << L <= W + 7 - x
    dst[q] = ok ? reinterpret_cast<long long*>(c) + ((size_t)ctu * (align ? kHalfCusPerCtu : kFullCusPerCtu) + ((e >> 18) & 511)) : nullptr;
  }
  __syncthreads();

  const int nb = (span + kSeedBatch - 1) / kSeedBatch;
#pragma unroll 1
  for (int kb = 0; kb < nb; kb++) {
    int acc[kSeedBatch] = {};
#pragma unroll
    for (int j = 0; j < B; j++) {
      // samples bx * B + 8 kb .. + B + 7 of strip row by * B + j: block column bx at offsets 8 kb .. 8 kb + 7
      unsigned D[ND];
      if constexpr (L == 0) {  // two 16-byte reads (as eight dwords the reads are the same, the address set-up is not)
        const uint4* rp = s_strip4 + ((by * 8 + j) * (PITCH / 8) + bx + kb);
        const uint4 lo = rp[0], hi = rp[1];
        D[0] = lo.x; D[1] = lo.y; D[2] = lo.z; D[3] = lo.w; D[4] = hi.x; D[5] = hi.y; D[6] = hi.z; D[7] = hi.w;
      } else {
        const unsigned* rp = s_strip + ((by * B + j) * (PITCH / 2) + (bx * B) / 2 + 4 * kb);
#pragma unroll
        for (int m = 0; m < ND; m++) D[m] = rp[m];
      }
      unsigned Dodd[ND - 1];
#pragma unroll
      for (int m = 0; m < ND - 1; m++) Dodd[m] = __builtin_amdgcn_alignbit(D[m + 1], D[m], 16);
#pragma unroll
      for (int o = 0; o < kSeedBatch; o++)
#pragma unroll
        for (int q = 0; q < B / 2; q++)
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
        const long long value = ((long long)sad << (2 * L)) + s_rate[oo];
        const int order = (dx | dy) == 0 ? 0 : 1 + (dy + R) * span + oo;  // (0, 0) first, then dy outer, dx inner
        best[q] = min(best[q], value * (1 << kSeedKeyBits) + order);
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
        const int order = (int)(key & ((1 << kSeedKeyBits) - 1));
        p.cost[r][a][i] = key >> kSeedKeyBits;
        if (order) {
          const int t = order - 1, oy = t / span;
          p.mv[r][a][2 * i] = shl(t - oy * span - p.radius, 4);
          p.mv[r][a][2 * i + 1] = shl(oy - p.radius, 4);
        }
      }
}

// Ten samples gx - 1 .. gx + 8 of a reference row of Wl samples, clamped to the
// row, as E = (s0 s1, s2 s3, .. s8 s9).
__device__ __forceinline__ void pyr_segment(const uint16_t* __restrict__ row, int gx, int Wl, unsigned (&E)[5]) {
  const int s = gx - 1, a = s & ~1;
  if (s >= 0 && a + 11 < Wl) {
    const unsigned* q = reinterpret_cast<const unsigned*>(row + a);  // rows are 4-byte aligned, a is even
    unsigned t[6];
#pragma unroll
    for (int m = 0; m < 6; m++) t[m] = q[m];
    const bool odd = s & 1;
#pragma unroll
    for (int m = 0; m < 5; m++) E[m] = odd ? __builtin_amdgcn_alignbit(t[m + 1], t[m], 16) : t[m];
  } else {
#pragma unroll
    for (int m = 0; m < 5; m++)
      E[m] = (unsigned)row[clampi(s + 2 * m, 0, Wl - 1)] | (unsigned)row[clampi(s + 2 * m + 1, 0, Wl - 1)] << 16;
  }
}

// acc + the SAD of the eight samples c against r0 .. r3
__device__ __forceinline__ int pyr_sad8(uint2 c0, uint2 c1, unsigned r0, unsigned r1, unsigned r2, unsigned r3, int acc) {
  unsigned v = __builtin_amdgcn_sad_u16(c0.x, r0, (unsigned)acc);
  v = __builtin_amdgcn_sad_u16(c0.y, r1, v);
  v = __builtin_amdgcn_sad_u16(c1.x, r2, v);
  return (int)__builtin_amdgcn_sad_u16(c1.y, r3, v);
}

// The sum over the lanes of a candidate (1, 2 or 4 DPP rows of one wave), in
// every one of them.  The rows of a candidate run the same control flow, so
// the lanes a lane reads from are active.
__device__ __forceinline__ int pyr_cand_sum(int v, int nslots) {
  v = row_sum16(v);
  if (nslots >= 2) v += __shfl_xor(v, 16);
  if (nslots == 4) v += __shfl_xor(v, 32);
  return v;
}

__global__ __launch_bounds__(kSeedThreads) void seed_refine_kernel(SeedParams p) {
  const int ctu = blockIdx.y, r = blockIdx.z, t = threadIdx.x & 15;
  const unsigned plan = kSeedPyrPlan.v[blockIdx.x * (kSeedThreads / 16) + (threadIdx.x >> 4)];
  const int nslots = (int)(plan >> 11);
  if (!nslots) return;  // a DPP row leaves as a whole, here and below
  const unsigned e = kSeedTab.v[plan & 511];
  const int align = (int)(e >> 27) & 1;
  const int x = (ctu % p.ctusPerRow) * kCtu + (int)(e & 15) * 8, y = (ctu / p.ctusPerRow) * kCtu + (int)((e >> 4) & 15) * 8;
  const int w = (int)((e >> 8) & 31) * 8, h = (int)((e >> 13) & 31) * 8;
  int64_t* costp = seed_sel(p.cost, r, align);
  int32_t* mvp = seed_sel(p.mv, r, align);
  if (!costp || x + w > p.W || y + h > p.H) return;  // outside the mask, or not wholly in the frame
  const int row = ctu * (align ? kHalfCusPerCtu : kFullCusPerCtu) + (int)((e >> 18) & 511);
  const int lw = 31 - __clz(w), lane = (int)((plan >> 9) & 3) * 16 + t, nlanes = nslots * 16;
  const int W = p.W, H = p.H, L = p.levels, radius = p.radius;
  const uint16_t* __restrict__ ref0 = seed_ref(p.refs, r);
  const uint16_t* __restrict__ ref1 = seed_ref(p.refPyrs, r);

  // the top level's winner (every in-frame row holds a key: (0, 0) is admissible)
  int dx = 0, dy = 0;
  {
    const int order = (int)(costp[row] & ((1 << kSeedKeyBits) - 1));
    if (order) {
      const int Rc = radius >> L, span = 2 * Rc + 1, k = order - 1, oy = k / span;
      dx = k - oy * span - Rc;
      dy = oy - Rc;
    }
  }
  long long bv = 0;
#pragma unroll 1
  for (int l = L - 1; l >= 0; l--) {
    const uint16_t* __restrict__ cl = l ? p.curPyr : p.cur;
    const uint16_t* __restrict__ rl = l ? ref1 : ref0;
    const int Wl = W >> l, Hl = H >> l, xl = x >> l, yl = y >> l, hl = h >> l;
    const int lcw = lw - l - 3, items = (hl + 2) << lcw;  // groups of 8 columns per row: 1 << lcw (w >> l >= 8)
    const int cx = 2 * dx, cy = 2 * dy;
    int acc[3][3] = {};
    int acc0 = 0;
    for (int i = lane; i < items; i += nlanes) {
      const int jr = (i >> lcw) - 1, k8 = (i & ((1 << lcw) - 1)) * 8;
      unsigned E[5], O[4];
      pyr_segment(rl + (size_t)clampi(yl + cy + jr, 0, Hl - 1) * Wl, xl + cx + k8, Wl, E);
#pragma unroll
      for (int m = 0; m < 4; m++) O[m] = __builtin_amdgcn_alignbit(E[m + 1], E[m], 16);
#pragma unroll
      for (int ey = -1; ey <= 1; ey++) {
        const int j = jr - ey;  // the cur row this reference row meets at ey
        if (j < 0 || j >= hl) continue;
        // cur and the pyramid are 8-byte aligned, rows and x + k8 multiples of 8 bytes
        const uint2* c = reinterpret_cast<const uint2*>(cl + (size_t)(yl + j) * Wl + xl + k8);
        const uint2 c0 = c[0], c1 = c[1];
        acc[ey + 1][0] = pyr_sad8(c0, c1, E[0], E[1], E[2], E[3], acc[ey + 1][0]);
        acc[ey + 1][1] = pyr_sad8(c0, c1, O[0], O[1], O[2], O[3], acc[ey + 1][1]);
        acc[ey + 1][2] = pyr_sad8(c0, c1, E[1], E[2], E[3], E[4], acc[ey + 1][2]);
        if (l == 0 && ey == 0) {  // the SAD of (0, 0): the block itself lies in the frame
          const unsigned* z = reinterpret_cast<const unsigned*>(ref0 + (size_t)(y + j) * W + x + k8);
          acc0 = pyr_sad8(c0, c1, z[0], z[1], z[2], z[3], acc0);
        }
      }
    }
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
      for (int b = 0; b < 3; b++) acc[a][b] = pyr_cand_sum(acc[a][b], nslots);
    acc0 = pyr_cand_sum(acc0, nslots);

    // the first minimum in the order: at level 0 (0, 0), then the centre, then ey outer, ex inner
    int bx = cx, by = cy;
    bv = ((long long)acc[1][1] << (2 * l)) + seed_rate(p.lambda, shl(cx, l), shl(cy, l));
    if (l == 0) {
      const long long v0 = acc0 + seed_rate(p.lambda, 0, 0);
      if (!(bv < v0)) {
        bv = v0;
        bx = by = 0;
      }
    }
#pragma unroll
    for (int ey = -1; ey <= 1; ey++)
#pragma unroll
      for (int ex = -1; ex <= 1; ex++) {
        if (ex == 0 && ey == 0) continue;
        const int Dx = shl(cx + ex, l), Dy = shl(cy + ey, l);
        if (abs(Dx) > radius || abs(Dy) > radius || Dx > W + 7 - x || Dy > H + 7 - y) continue;
        const long long v = ((long long)acc[ey + 1][ex + 1] << (2 * l)) + seed_rate(p.lambda, Dx, Dy);
        if (v < bv) {
          bv = v;
          bx = cx + ex;
          by = cy + ey;
        }
      }
    dx = bx;
    dy = by;
  }
  if (lane == 0) {
    costp[row] = bv;
    mvp[2 * row] = shl(dx, 4);
    mvp[2 * row + 1] = shl(dy, 4);
  }
}

hipError_t seed_launch(const SeedParams& p, hipStream_t stream) {
  const int rows = p.nCtus * kHalfCusPerCtu, R = p.radius >> p.levels;
  const dim3 block(kSeedThreads), perRow((rows + kSeedThreads - 1) / kSeedThreads), grid(p.nCtus, p.nrefs, 2 * R + 1);
  hipLaunchKernelGGL(seed_init_kernel, perRow, block, 0, stream, p);
  if (p.levels == 0)
    hipLaunchKernelGGL(seed_grid_kernel<0>, grid, block, 0, stream, p);
  else if (p.levels == 1)
    hipLaunchKernelGGL(seed_grid_kernel<1>, grid, block, 0, stream, p);
  else
    hipLaunchKernelGGL(seed_grid_kernel<2>, grid, block, 0, stream, p);
  if (p.levels == 0)
    hipLaunchKernelGGL(seed_close_kernel, perRow, block, 0, stream, p);
  else
    hipLaunchKernelGGL(seed_refine_kernel, dim3(kPyrSlots * 16 / kSeedThreads, p.nCtus, p.nrefs), block, 0, stream, p);
  return hipGetLastError();
}

}  // namespace vame

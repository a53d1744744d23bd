// vame_partition.hip -- on-device CU partition decision (vame_partition,
// include/vame.h): from the search's result arrays of one POC, the cheapest
// tiling of every CTU by candidate CUs under binary and ternary splits, and the
// chosen leaves as vame_mc_cu descriptors that stay on the device.
//
// The rule.  A node is a CTU-relative rectangle with w, h in
// {16, 32, 64, 128} at a multiple of 16 that lies in the CTU: 1024 slots
// ((lh*4 + lw)*8 + y/16)*8 + x/16.  Its value, at frame position (X, Y):
//   outside (X >= W or Y >= H)            0, nothing emitted
//   hole    (16x16 crossing the edge)     0, nothing emitted
//   else the first minimum, under strict <, of
//     leaf   (the node lies in the frame and is a candidate CU of a PRED in the
//            mask): min over refIdx (outer) and 2-CP, 3-CP (inner) of its cost
//     BT-H, BT-V, TT-H, TT-V: penalty + the children's values (TT only with a
//            HALF PRED in the mask); infeasible with an infeasible child
// Two launches on the caller's stream, neither of which reads anything on the
// host:
//   part_decide_kernel  one 256-thread workgroup per CTU: the leaf minima into
//                       LDS, the values bottom-up over the 7 area levels, the
//                       chosen tree top-down over the same levels; the leaves
//                       (by top-left 16x16 block) and every block's owner go to
//                       the context's scratch with the CTU's leaf count
//   part_emit_kernel    one wave per CTU: the sum of the counts before it,
//                       each leaf's place by ballot + popcount over the 64
//                       blocks, the descriptors with the chosen row's CPMVs
// Both kernels are templates on BI: <false> is vame_partition; <true> is
// vame_partition_bi, whose leaf may be the row's bi-predicted
// candidate (vame_bipred's bi_cost + bi_penalty) and whose descriptors are the
// 20-word vame_mc_bicu.
#include <hip/hip_runtime.h>

#include "../../include/vame.h"
#include "vame_mc_core.h"
#include "vame_partition.h"

namespace vame {

// ---- slot -> candidate: align*512 + output offset, or -1 (compile-time data)
struct PartTable {
  int16_t v[kPartSlots];
};
constexpr int part_log16(int s) { return s == 16 ? 0 : s == 32 ? 1 : s == 64 ? 2 : 3; }
constexpr int part_slot(int lw, int lh, int y16, int x16) { return ((lh * 4 + lw) * 8 + y16) * 8 + x16; }
constexpr PartTable make_part_table() {
  PartTable t{};
  for (int i = 0; i < kPartSlots; i++) t.v[i] = -1;
  // aligned CU k of group g sits at raster position k
  for (int g = 0; g < kFullGroups; g++) {
    const int w = kFullW[g], h = kFullH[g], cols = kCtu / w;
    for (int k = 0; k < kFullStride[g + 1] - kFullStride[g]; k++)
      t.v[part_slot(part_log16(w), part_log16(h), (k / cols) * h / 16, (k % cols) * w / 16)] =
          (int16_t)(kFullStride[g] + k);
  }
  // half-aligned CUs whose position is a multiple of 16 in x and y (the others
  // would need an 8-sample sibling and are no nodes)
  for (int g = 0; g < kHalfGroups; g++)
    for (int k = 0; k < kHalfN[g]; k++) {
      const int x8 = kHalfX8[g][k], y8 = kHalfY8[g][k];
      if ((x8 | y8) & 1) continue;
      t.v[part_slot(part_log16(kHalfW[g]), part_log16(kHalfH[g]), y8 / 2, x8 / 2)] =
          (int16_t)(512 + kHalfStride[g] + k);
    }
  return t;
}
constexpr int part_count(const PartTable& t, int align) {
  int n = 0;
  for (int i = 0; i < kPartSlots; i++) n += t.v[i] >= 0 && (t.v[i] >> 9) == align;
  return n;
}
constexpr PartTable kPartTableHost = make_part_table();
// no rectangle is both an aligned and a half-aligned candidate: every aligned
// one kept its slot
static_assert(part_count(kPartTableHost, 0) == kFullCusPerCtu, "aligned candidates are nodes, none shadowed");
static __constant__ PartTable kPartTable = make_part_table();

constexpr int kPartThreads = 256;
constexpr long long kPartInf = 0x7fffffffffffffffll;  // infeasible
// decisions of a node
enum : unsigned char { kDecLeaf = 0, kDecBtH = 1, kDecBtV = 2, kDecTtH = 3, kDecTtV = 4, kDecOutside = 5, kDecHole = 6, kDecNone = 7 };

__device__ __forceinline__ long long part_add(long long a, long long b) {
  return (a == kPartInf || b == kPartInf) ? kPartInf : a + b;
}

// BI (vame_partition_bi): the leaf value is the first minimum of the uni leaf
// minimum and bi_cost + bi_penalty, the latter only where bi_sel names two
// hypotheses the call holds (refIdx < nrefs, PREDs in the mask).
template <bool BI>
__global__ __launch_bounds__(kPartThreads) void part_decide_kernel(PartParams p) {
  __shared__ long long s_val[kPartSlots];
  __shared__ unsigned char s_dec[kPartSlots];
  __shared__ unsigned char s_sel[kPartSlots];   // leaf: refIdx | (nCPs - 2) << 2; bit 7: a bi leaf
  __shared__ unsigned char s_mark[kPartSlots];
  __shared__ int s_leaf[64];                    // by top-left block: the leaf's code, or -1
  __shared__ int s_owner[64];                   // by block: the top-left block of its leaf, or -1
  __shared__ int s_holes, s_splits;

  const int tid = threadIdx.x, ctu = blockIdx.x;
  const int X0 = (ctu % p.ctusPerRow) * kCtu, Y0 = (ctu / p.ctusPerRow) * kCtu;
  const bool tt = (p.predMask & 12) != 0;
  // this thread's nodes: (lw, y16, x16) with lh = 0..3, slot = tid + 256 * lh
  const int x16 = tid & 7, y16 = (tid >> 3) & 7, lw = tid >> 6;
  const int wN = 1 << lw;

  if (tid < 64) {
    s_leaf[tid] = -1;
    s_owner[tid] = -1;
  }
  if (tid == 0) s_holes = s_splits = 0;

  // ---- leaf minima
#pragma unroll
  for (int lh = 0; lh < 4; lh++) {
    const int slot = tid + 256 * lh, hN = 1 << lh;
    s_mark[slot] = 0;
    long long best = kPartInf;
    unsigned char dec = kDecNone, sel = 0;
    if (x16 + wN <= 8 && y16 + hN <= 8) {
      const int X = X0 + x16 * 16, Y = Y0 + y16 * 16;
      if (X >= p.W || Y >= p.H) {
        dec = kDecOutside;
        best = 0;
      } else if (lw == 0 && lh == 0 && (X + 16 > p.W || Y + 16 > p.H)) {
        dec = kDecHole;
        best = 0;
      } else if (X + wN * 16 <= p.W && Y + hN * 16 <= p.H) {
        const int e = kPartTable.v[slot];
        const int align = e >> 9;
        if (e >= 0 && ((p.predMask >> (2 * align)) & 3)) {
          const size_t row = (size_t)ctu * (align ? kHalfCusPerCtu : kFullCusPerCtu) + (e & 511);
          for (int r = 0; r < p.nrefs; r++)
#pragma unroll
            for (int m = 0; m < 2; m++) {
              if (!((p.predMask >> (2 * align + m)) & 1)) continue;
              const long long c = p.cost[r][2 * align + m][row];
              if (c < best) {
                best = c;
                sel = (unsigned char)(r | (m << 2));
                dec = kDecLeaf;
              }
            }
          if (BI) {
            const int s = p.biSel[align][row];
            const int pm = (p.predMask >> (2 * align)) & 3;
            if (s >= 0 && s < 64 && (s & 3) < p.nrefs && ((s >> 3) & 3) < p.nrefs && ((pm >> ((s >> 2) & 1)) & 1) &&
                ((pm >> ((s >> 5) & 1)) & 1)) {
              const long long c = p.biCost[align][row] + p.biPenalty;
              if (c < best) {
                best = c;
                sel = 0x80;
                dec = kDecLeaf;
              }
            }
          }
        }
      }
    }
    s_val[slot] = best;
    s_dec[slot] = dec;
    s_sel[slot] = sel;
  }
  __syncthreads();

  // ---- values, bottom-up over the area levels lw + lh = 1 .. 6
  for (int level = 1; level <= 6; level++) {
    const int lh = level - lw, hN = 1 << (lh & 3);
    if (lh >= 0 && lh <= 3 && x16 + wN <= 8 && y16 + hN <= 8) {
      const int slot = tid + 256 * lh;
      unsigned char dec = s_dec[slot];
      if (dec != kDecOutside && dec != kDecHole) {
        long long best = s_val[slot];
        if (lh >= 1) {
          const long long v = part_add(part_add(s_val[part_slot(lw, lh - 1, y16, x16)],
                                                s_val[part_slot(lw, lh - 1, y16 + hN / 2, x16)]), p.penalty);
          if (v < best) best = v, dec = kDecBtH;
        }
        if (lw >= 1) {
          const long long v = part_add(part_add(s_val[part_slot(lw - 1, lh, y16, x16)],
                                                s_val[part_slot(lw - 1, lh, y16, x16 + wN / 2)]), p.penalty);
          if (v < best) best = v, dec = kDecBtV;
        }
        if (tt && lh >= 2) {
          const long long v = part_add(part_add(part_add(s_val[part_slot(lw, lh - 2, y16, x16)],
                                                         s_val[part_slot(lw, lh - 1, y16 + hN / 4, x16)]),
                                                s_val[part_slot(lw, lh - 2, y16 + 3 * hN / 4, x16)]), p.penalty);
          if (v < best) best = v, dec = kDecTtH;
        }
        if (tt && lw >= 2) {
          const long long v = part_add(part_add(part_add(s_val[part_slot(lw - 2, lh, y16, x16)],
                                                         s_val[part_slot(lw - 1, lh, y16, x16 + wN / 4)]),
                                                s_val[part_slot(lw - 2, lh, y16, x16 + 3 * wN / 4)]), p.penalty);
          if (v < best) best = v, dec = kDecTtV;
        }
        s_val[slot] = best;
        s_dec[slot] = dec;
      }
    }
    __syncthreads();
  }

  // ---- the chosen tree, top-down: the children of a marked node belong to
  // it alone (marked nodes of one level are disjoint)
  if (tid == 0) s_mark[part_slot(3, 3, 0, 0)] = 1;
  __syncthreads();
  for (int level = 6; level >= 1; level--) {
    const int lh = level - lw, hN = 1 << (lh & 3);
    if (lh >= 0 && lh <= 3) {
      const int slot = tid + 256 * lh;
      if (s_mark[slot]) {  // a marked slot is a valid node
        switch (s_dec[slot]) {
          case kDecBtH:
            s_mark[part_slot(lw, lh - 1, y16, x16)] = 1;
            s_mark[part_slot(lw, lh - 1, y16 + hN / 2, x16)] = 1;
            break;
          case kDecBtV:
            s_mark[part_slot(lw - 1, lh, y16, x16)] = 1;
            s_mark[part_slot(lw - 1, lh, y16, x16 + wN / 2)] = 1;
            break;
          case kDecTtH:
            s_mark[part_slot(lw, lh - 2, y16, x16)] = 1;
            s_mark[part_slot(lw, lh - 1, y16 + hN / 4, x16)] = 1;
            s_mark[part_slot(lw, lh - 2, y16 + 3 * hN / 4, x16)] = 1;
            break;
          case kDecTtV:
            s_mark[part_slot(lw - 2, lh, y16, x16)] = 1;
            s_mark[part_slot(lw - 1, lh, y16, x16 + wN / 4)] = 1;
            s_mark[part_slot(lw - 2, lh, y16, x16 + 3 * wN / 4)] = 1;
            break;
          default:
            break;
        }
      }
    }
    __syncthreads();
  }

  // ---- the marked nodes: leaves own their blocks, holes and splits are counted
#pragma unroll
  for (int lh = 0; lh < 4; lh++) {
    const int slot = tid + 256 * lh;
    if (!s_mark[slot]) continue;
    const unsigned char dec = s_dec[slot];
    if (dec == kDecLeaf) {
      const int b0 = y16 * 8 + x16;
      s_leaf[b0] = slot | ((int)s_sel[slot] << 10);
      for (int dy = 0; dy < (1 << lh); dy++)
        for (int dx = 0; dx < wN; dx++) s_owner[b0 + dy * 8 + dx] = b0;
    } else if (dec == kDecHole) {
      atomicAdd(&s_holes, 1);
    } else if (dec >= kDecBtH && dec <= kDecTtV) {
      atomicAdd(&s_splits, 1);
    }
  }
  __syncthreads();

  if (tid < 64) {
    const int code = s_leaf[tid];
    const int count = __popcll(__builtin_amdgcn_ballot_w64(code >= 0));
    p.scratch[p.nCtus + ctu * 64 + tid] = code;
    p.scratch[p.nCtus * 65 + ctu * 64 + tid] = s_owner[tid];
    if (tid == 0) {
      p.scratch[ctu] = count;
      if (p.ctuInfo) {
        p.ctuInfo[ctu * 4 + 1] = count;
        p.ctuInfo[ctu * 4 + 2] = s_holes;
        p.ctuInfo[ctu * 4 + 3] = s_splits;
      }
      if (p.ctuCost) p.ctuCost[ctu] = s_val[part_slot(3, 3, 0, 0)];
    }
  }
}

template <bool BI>
__global__ __launch_bounds__(64) void part_emit_kernel(PartParams p) {
  const int lane = threadIdx.x, ctu = blockIdx.x;
  // the leaves of the CTUs before this one (at most 510 counts)
  int first = 0;
  for (int i = lane; i < ctu; i += 64) first += p.scratch[i];
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) first += __shfl_xor(first, d, 64);

  const int code = p.scratch[p.nCtus + ctu * 64 + lane];
  const int owner = p.scratch[p.nCtus * 65 + ctu * 64 + lane];
  const unsigned long long leaves = __builtin_amdgcn_ballot_w64(code >= 0);
  if (code >= 0) {
    const int idx = first + __popcll(leaves & ((1ull << lane) - 1));
    const int slot = code & 1023;
    const int e = kPartTable.v[slot];
    const int align = e >> 9;
    const int row = ctu * (align ? kHalfCusPerCtu : kFullCusPerCtu) + (e & 511);
    const int bsel = BI && ((code >> 17) & 1) ? p.biSel[align][row] : -1;
    const int r = bsel >= 0 ? bsel & 3 : (code >> 10) & 3, m = bsel >= 0 ? (bsel >> 2) & 1 : (code >> 12) & 1;
    const int32_t* cp = p.cpmv[r][2 * align + m] + (size_t)row * 7;
    McCu cu;
    cu.x = (ctu % p.ctusPerRow) * kCtu + (slot & 7) * 16;
    cu.y = (ctu / p.ctusPerRow) * kCtu + ((slot >> 3) & 7) * 16;
    cu.w = 16 << ((slot >> 6) & 3);
    cu.h = 16 << ((slot >> 8) & 3);
    cu.ref = r;
    cu.ncps = 2 + m;
    cu.ltx = cp[1]; cu.lty = cp[2]; cu.rtx = cp[3]; cu.rty = cp[4]; cu.lbx = cp[5]; cu.lby = cp[6];
    if (BI) {
      int32_t* d = reinterpret_cast<int32_t*>(p.cus) + (size_t)idx * 20;
      *reinterpret_cast<McCu*>(d) = cu;
      if (bsel >= 0) {
        const int r1 = (bsel >> 3) & 3, m1 = (bsel >> 5) & 1;
        const int32_t* cp1 = p.cpmv[r1][2 * align + m1] + (size_t)row * 7;
        d[12] = r1;
        d[13] = 2 + m1;
#pragma unroll
        for (int k = 0; k < 6; k++) d[14 + k] = cp1[1 + k];
      } else {
        d[12] = -1;
#pragma unroll
        for (int k = 13; k < 20; k++) d[k] = 0;
      }
      if (p.sel) p.sel[idx] = bsel;
    } else {
      p.cus[idx] = cu;
    }
    if (p.rows) p.rows[idx] = row;
  }
  if (p.blockCu)
    p.blockCu[ctu * 64 + lane] = owner < 0 ? -1 : first + __popcll(leaves & ((1ull << owner) - 1));
  if (lane == 0) {
    if (p.ctuInfo) p.ctuInfo[ctu * 4] = first;
    if (ctu == p.nCtus - 1) *p.ncus = first + __popcll(leaves);
  }
}

hipError_t partition_launch(const PartParams& p, hipStream_t stream, bool bi) {
  if (bi) {
    hipLaunchKernelGGL(part_decide_kernel<true>, dim3(p.nCtus), dim3(kPartThreads), 0, stream, p);
    hipLaunchKernelGGL(part_emit_kernel<true>, dim3(p.nCtus), dim3(64), 0, stream, p);
  } else {
    hipLaunchKernelGGL(part_decide_kernel<false>, dim3(p.nCtus), dim3(kPartThreads), 0, stream, p);
    hipLaunchKernelGGL(part_emit_kernel<false>, dim3(p.nCtus), dim3(64), 0, stream, p);
  }
  return hipGetLastError();
}

// ------------------------------------------------------------- vame_mvp_gather
// One lane per bi descriptor: a rectangle that is a candidate CU of its CTU
// (kPartTable) takes, per hypothesis, the predictor of its row in the arrays of
// (ref, alignment), expanded to LT = RT = LB; anything else -- no candidate,
// outside the CTU grid, a reference without an array -- the zero predictor.
// The second entry is written for uni descriptors too (zero).
__global__ __launch_bounds__(kPartThreads) void mvp_gather_kernel(MvpGatherParams p) {
  const int i = blockIdx.x * kPartThreads + threadIdx.x;
  if (i >= mc_ncus(p.ncusDev, p.maxCus)) return;
  const McBiCu cu = p.cus[i];
  int align = -1, row = 0;
  if (mc_size_ok(cu.w) && mc_size_ok(cu.h) && cu.x >= 0 && cu.y >= 0 && ((cu.x | cu.y) & 15) == 0 &&
      (cu.x >> 7) < p.ctusPerRow) {
    const int ctu = (cu.y >> 7) * p.ctusPerRow + (cu.x >> 7);
    const int e = kPartTable.v[part_slot(part_log16(cu.w), part_log16(cu.h), (cu.y & 127) >> 4, (cu.x & 127) >> 4)];
    if (ctu < p.nCtus && e >= 0) {
      align = e >> 9;
      row = ctu * (align ? kHalfCusPerCtu : kFullCusPerCtu) + (e & 511);
    }
  }
  const int refs[2] = {cu.ref0, cu.ref1};
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const int32_t* mvp = nullptr;
#pragma unroll
    for (int rr = 0; rr < 4; rr++)
#pragma unroll
      for (int aa = 0; aa < 2; aa++)
        if (rr == refs[h] && aa == align) mvp = p.mvp[rr][aa];
    const int qx = mvp ? mvp[2 * (size_t)row] : 0, qy = mvp ? mvp[2 * (size_t)row + 1] : 0;
    int32_t* P = p.preds + ((size_t)i * 2 + h) * kMvpWords;
    P[0] = 3;
    P[1] = P[3] = P[5] = qx;
    P[2] = P[4] = P[6] = qy;
  }
}

hipError_t mvp_gather_launch(const MvpGatherParams& p, hipStream_t stream) {
  hipLaunchKernelGGL(mvp_gather_kernel, dim3((p.maxCus + kPartThreads - 1) / kPartThreads), dim3(kPartThreads), 0, stream,
                     p);
  return hipGetLastError();
}

}  // namespace vame

extern "C" int vame_partition_table(int32_t* table) {
  if (!table) return VAME_E_INVALID;
  for (int i = 0; i < vame::kPartSlots; i++) table[i] = vame::kPartTableHost.v[i];
  return VAME_OK;
}

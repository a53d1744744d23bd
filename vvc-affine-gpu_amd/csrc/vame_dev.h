// vame_dev.h -- the device-function library of the affine search: what its
// kernels (vame_kernel.h) and the prediction-side and list-form units
// (vame_mc_core.h, vame_refine_core.h) build on.  Integer helpers and the
// reference's small functions (clipMv, rate bits, scaleDeltaMvs), the filter
// tap table, the MV field, the 6-tap window filter from the LDS tile or the
// frame, SATD, PROF, one sub-block's prediction (predict_sb) and gradient sums
// (grad_sb), the shared-segment solveEqual (seg_solve) and a sub-block's
// contribution to the normal equations (eq_value).  No kernel, no LDS layout
// and no launch parameters: those are the search kernel's (vame_kernel.h).
#pragma once
#include <hip/hip_runtime.h>

#include "vame_instr.h"
#include "vame_tables.h"

namespace vame {

constexpr int kNumMom = 24;   // 3 CP: {1,u,v,uu,uv,vv} x {xx,xy,yy} + {1,u,v} x {xe,ye}
constexpr int kNumVal2 = 14;  // 2 CP: 10 distinct matrix entries + 4 right-hand sides

// device view of vame_cpmvs / typedef.h Cpmvs (28 bytes)
struct vame_cpmvs_dev {
  int32_t ncps, ltx, lty, rtx, rty, lbx, lby;
};

// ------------------------------------------------------------------ helpers
typedef short short2v __attribute__((ext_vector_type(2)));

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }
__device__ __forceinline__ int shl(int a, int s) { return (int)((unsigned)a << s); }
__device__ __forceinline__ short2v as_s2(unsigned v) { return __builtin_bit_cast(short2v, v); }
__device__ __forceinline__ unsigned as_u(short2v v) { return __builtin_bit_cast(unsigned, v); }
// v_dot2_i32_i16: a.lo*b.lo + a.hi*b.hi + acc (signed 16-bit halves, no clamp)
__device__ __forceinline__ int dot2(unsigned a, unsigned b, int acc) {
  return __builtin_amdgcn_sdot2(as_s2(a), as_s2(b), acc, false);
}
// low 16 bits of lo | low 16 bits of hi << 16
__device__ __forceinline__ unsigned pack16(int lo, int hi) {
  return __builtin_amdgcn_perm((unsigned)hi, (unsigned)lo, 0x05040100u);
}

// LDS ordering between the lanes of one wave (a wave's LDS ops execute in order)
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ void phase_sync(bool coop) {
  if (coop)
    __syncthreads();
  else
    wave_sync();
}

// aux_functions.cl:51-67 clipMv: one component, for a block at `pos` on the
// component's axis in a frame of extent `lim` along it
__device__ __forceinline__ int clip_mv_axis(int v, int pos, int lim) {
  return clampi(v, shl(-128 - 8 - pos + 1, 4), shl(lim + 8 - pos - 1, 4));
}
__device__ __forceinline__ void clip_mv(int& x, int& y, int bx, int by, int W, int H) {
  x = clip_mv_axis(x, bx, W);
  y = clip_mv_axis(y, by, H);
}

// aux_functions.cl:106-141 (bipred == 0)
__device__ __forceinline__ bool spread_over_limit(int a, int b, int c, int d, bool six) {
  const int s4 = 4 << 11;
  int w = (abs(4 * a + s4) >> 11) + 9, h = (abs(4 * b) >> 11) + 9;
  if (w * h > 165) return true;
  // 2 CP: (c, d) = (-b, a), so the second test's w and h are the first's h and
  // w -- the same product
  if (!six) return false;
  w = (abs(4 * c) >> 11) + 9;
  h = (abs(4 * d + s4) >> 11) + 9;
  return w * h > 165;
}

// aux_functions.cl:2057-2075 (1/16 -> 1/4 pel)
__device__ __forceinline__ int to_quarter(int v) { return v >= 0 ? (v + 1) >> 2 : (v + 2) >> 2; }

// aux_functions.cl:2117-2129
__device__ __forceinline__ int eg_bits(int value) {
  unsigned t = value <= 0 ? ((unsigned)(-value) << 1) + 1u : (unsigned)value << 1;
  int len = 1;
  while (t > 128u) {
    len += 14;
    t >>= 7;
  }
  return len + ((31 - __clz((int)t)) << 1);
}

// aux_functions.cl:2140-2189 with zero predictors (affine.cl:431-434)
__device__ __forceinline__ int affine_bits(const int* c, int ncp) {
  int ltx = to_quarter(c[0]), lty = to_quarter(c[1]);
  int b = eg_bits(ltx) + eg_bits(lty) + eg_bits(to_quarter(c[2]) - ltx) +
          eg_bits(to_quarter(c[3]) - lty);
  if (ncp == 3) b += eg_bits(to_quarter(c[4]) - ltx) + eg_bits(to_quarter(c[5]) - lty);
  return b;
}

// aux_functions.cl:2140-2189 against the predictor P (LT, RT, LB as c; QUARTER
// precision, cost_scale 0, imvShift 0): LT against P's LT, RT and LB against
// P's moved by the LT difference.  Components of c and P within [kMvMin,
// kMvMax]: the composed predictor stays within 3 * 2^17.  P = 0 gives
// affine_bits(c, ncp).
__device__ __forceinline__ int affine_bits_p(const int* c, const int* P, int ncp) {
  const int dx = c[0] - P[0], dy = c[1] - P[1];
  int b = eg_bits(to_quarter(c[0]) - to_quarter(P[0])) + eg_bits(to_quarter(c[1]) - to_quarter(P[1])) +
          eg_bits(to_quarter(c[2]) - to_quarter(P[2] + dx)) + eg_bits(to_quarter(c[3]) - to_quarter(P[3] + dy));
  if (ncp == 3) b += eg_bits(to_quarter(c[4]) - to_quarter(P[4] + dx)) + eg_bits(to_quarter(c[5]) - to_quarter(P[5] + dy));
  return b;
}
// The predictor of a rate site: in the kernels of the calls without predictors
// (MVP = false) an empty object whose bits() is affine_bits -- those kernels
// hold no predictor code or state; with MVP the six components, loaded from a
// vame_cpmvs (7 int32: nCPs, ignored, then LT, RT, LB), and affine_bits_p.
template <bool MVP>
struct MvPred {
  __device__ __forceinline__ void load(const int32_t*) {}
  __device__ __forceinline__ int bits(const int* c, int ncp) const { return affine_bits(c, ncp); }
};
template <>
struct MvPred<true> {
  int p[6];
  __device__ __forceinline__ void load(const int32_t* P) {
#pragma unroll
    for (int k = 0; k < 6; k++) p[k] = P[1 + k];
  }
  __device__ __forceinline__ int bits(const int* c, int ncp) const { return affine_bits_p(c, p, ncp); }
};

// (int)double with the semantics the reference's kernels get from the GPU:
// truncation, NaN -> 0, out-of-range values saturate -- exactly what
// v_cvt_i32_f64 does, so it is issued directly (a C++ cast of an out-of-range
// value is undefined and would need explicit checks).
__device__ __forceinline__ int cvt_i32_f64(double d) {
  int r;
  asm("v_cvt_i32_f64 %0, %1" : "=v"(r) : "v"(d));
  return r;
}

// aux_functions.cl:2194-2215
__device__ __forceinline__ int scale_delta(double d) {
  double s = d >= 0 ? 1.0 : -1.0;
  return shl(cvt_i32_f64(d * 4.0 + s * 0.5), 2);
}

// One CPMV component's update (affine.cl:860-893): scaleDeltaMvs of its delta,
// the wrapping add, clampCpmvs to [kMvMin, kMvMax], clipCpmvs for the CU at
// `pos` on the component's axis (x for even components, y for odd ones) in a
// frame of extent `lim` along it.
__device__ __forceinline__ int update_cpmv(int c, double d, int pos, int lim) {
  const int v = (int)((unsigned)c + (unsigned)scale_delta(d));
  return clip_mv_axis(clampi(v, kMvMin, kMvMax), pos, lim);
}

// The LB control point of the 3-CP start (affine.cl:81-105): the 2-CP model
// (LT, RT) of a 2^lw x 2^lh CU at frame position (cx, cy) evaluated at its
// bottom-left corner, rounded (roundMv), clamped to [kMvMin, kMvMax], rounded to
// quarter pel and clipped (clipMv).
__device__ __forceinline__ void derive_lb(int ltx, int lty, int rtx, int rty, int lw, int lh, int cx, int cy,
                                          int W, int H, int& lbx, int& lby) {
  const int sh = 7 + lh - lw;
  int vx2 = shl(ltx, 7) - shl(rty - lty, sh);
  int vy2 = shl(lty, 7) + shl(rtx - ltx, sh);
  vx2 = (vx2 + 64 - (vx2 >= 0)) >> 7;
  vy2 = (vy2 + 64 - (vy2 >= 0)) >> 7;
  lbx = shl(to_quarter(clampi(vx2, kMvMin, kMvMax)), 2);
  lby = shl(to_quarter(clampi(vy2, kMvMin, kMvMax)), 2);
  clip_mv(lbx, lby, cx, cy, W, H);
}

// floor(lambda * bits), the search's rate term (affine.cl:442-446)
__device__ __forceinline__ long long mc_rate(float lambda, int bits) {
  return (long long)(int)floorf(__fmul_rn(lambda, (float)bits));
}
// A candidate's cost (affine.cl:416-446): its SATD plus the rate term of its
// CPMVs' bits (affine_bits) and the reference index's kRuiBits.
__device__ __forceinline__ long long price(int satd, float lambda, int rate) {
  return (long long)satd + mc_rate(lambda, rate + kRuiBits);
}

// DPP lane shift with zero fill for lanes whose source is outside the pattern
// (bound_ctrl) or whose row is masked off (old = 0).
template <int CTRL, int ROWMASK>
__device__ __forceinline__ int dpp32(int v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, ROWMASK, 0xF, true);
}

// ---------------------------------------------------------- filter tap pairs
// kLuma6 (constants.cl:40-58) re-packed for v_dot2_i32_i16.  A 4-wide output
// row reads 5 dwords D[0..4] of its window row (two samples each); output c
// applies set s' + (c & 1) to D[(c >> 1) .. (c >> 1) + 3], where s' is the
// parity of the window start inside the dword stream:
//   set 0: (f0,f1) (f2,f3) (f4,f5) (0,0)     set 1: (0,f0) (f1,f2) (f3,f4) (f5,0)
//   set 2: (0,0) (f0,f1) (f2,f3) (f4,f5)
// The vertical pass uses sets 0/1 on row pairs (t[2k], t[2k+1]) the same way.
struct CoefTab {
  uint32_t v[16][3][4];
};
constexpr uint32_t pk16c(int lo, int hi) {
  return (uint32_t)(uint16_t)(int16_t)lo | ((uint32_t)(uint16_t)(int16_t)hi << 16);
}
constexpr CoefTab make_coef_tab() {
  CoefTab t{};
  for (int f = 0; f < 16; f++) {
    const int8_t* c = kLuma6[f];
    const uint32_t s0[4] = {pk16c(c[0], c[1]), pk16c(c[2], c[3]), pk16c(c[4], c[5]), 0u};
    const uint32_t s1[4] = {pk16c(0, c[0]), pk16c(c[1], c[2]), pk16c(c[3], c[4]), pk16c(c[5], 0)};
    const uint32_t s2[4] = {0u, pk16c(c[0], c[1]), pk16c(c[2], c[3]), pk16c(c[4], c[5])};
    for (int k = 0; k < 4; k++) {
      t.v[f][0][k] = s0[k];
      t.v[f][1][k] = s1[k];
      t.v[f][2][k] = s2[k];
    }
  }
  return t;
}
static __constant__ CoefTab kCoefTab = make_coef_tab();  // one copy per translation unit

// ------------------------------------------------------------- motion field
struct MvField {
  int bx, by, hx, hy, vx, vy;
  bool spread;
};

// deriveMv{2,3}Cps_and_spread (aux_functions.cl:146-212), once per CU and iteration
__device__ __forceinline__ MvField mv_field(const int* cp, int ncp, int lw, int lh) {
  MvField f;
  f.hx = shl(cp[2] - cp[0], 7 - lw);
  f.hy = shl(cp[3] - cp[1], 7 - lw);
  if (ncp == 3) {
    f.vx = shl(cp[4] - cp[0], 7 - lh);
    f.vy = shl(cp[5] - cp[1], 7 - lh);
  } else {
    f.vx = -f.hy;
    f.vy = f.hx;
  }
  f.spread = spread_over_limit(f.hx, f.hy, f.vx, f.vy, ncp == 3);
  f.bx = shl(cp[0], 7);
  f.by = shl(cp[1], 7);
  return f;
}

struct Geo {       // a lane's CU
  int x, y;        // frame position
  int lw, lh, w, h;
};

// Hide a value's origin from the optimizer: per-lane geometry is loop-invariant
// for a whole work item, and hoisting every address derived from it out of the
// iteration loop would pin ~60 VGPRs; recomputing them per phase is a few adds.
__device__ __forceinline__ void opaque(int& v) { asm volatile("" : "+v"(v)); }
__device__ __forceinline__ void opaque_geo(Geo& g, int& sx, int& sy) {
  opaque(g.x); opaque(g.y); opaque(sx); opaque(sy);
  opaque(g.lw); opaque(g.lh);
}


// Horizontal 6-tap pass of one window row (5 dwords = samples 0..9 of the row
// in dword order), offset -IF_INTERNAL_OFFS << 2 = -32768, shift 2
// (aux_functions.cl:1128-1161).  |t| < 2^14, so rows pack into int16 pairs.
__device__ __forceinline__ void hrow(const unsigned (&D)[5], const uint4& KA, const uint4& KB,
                                     int (&t)[4]) {
  t[0] = dot2(D[0], KA.x, dot2(D[1], KA.y, dot2(D[2], KA.z, dot2(D[3], KA.w, -32768)))) >> 2;
  t[1] = dot2(D[0], KB.x, dot2(D[1], KB.y, dot2(D[2], KB.z, dot2(D[3], KB.w, -32768)))) >> 2;
  t[2] = dot2(D[1], KA.x, dot2(D[2], KA.y, dot2(D[3], KA.z, dot2(D[4], KA.w, -32768)))) >> 2;
  t[3] = dot2(D[1], KB.x, dot2(D[2], KB.y, dot2(D[3], KB.z, dot2(D[4], KB.w, -32768)))) >> 2;
}
// The same row before the >> 2 (the shift happens while packing, pack_shr2),
// with the offsets re-based so that no accumulator needs a non-inline
// constant: the six taps of every phase sum to 64, so
//   sum_v f_v * ((S_v - 32768) >> 2) + 512 + (8192 << 6)
//     = sum_v f_v * ((S_v - 32768) >> 2 + 8192 + 8)
//     = sum_v f_v * ((S_v + 32) >> 2)
// (32768 is a multiple of 4, so the floor shifts by exactly 8192): the rows
// start from +32 and the vertical accumulators from 0.  (S_v + 32) >> 2 stays
// within [-5619, 22008], so the packed int16 pairs are exact.
// a.lo*b.lo + a.hi*b.hi + K for an inline constant K, as the VOP3 form (the
// compiler picks the accumulate-in-place v_dot2c form and a v_mov of K)
template <int K>
__device__ __forceinline__ int dot2k(unsigned a, unsigned b) {
  int r;
  asm("v_dot2_i32_i16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "i"(K));
  return r;
}
__device__ __forceinline__ void hrow_raw(const unsigned (&D)[5], const uint4& KA, const uint4& KB,
                                         int (&t)[4]) {
  t[0] = dot2(D[0], KA.x, dot2(D[1], KA.y, dot2(D[2], KA.z, dot2k<32>(D[3], KA.w))));
  t[1] = dot2(D[0], KB.x, dot2(D[1], KB.y, dot2(D[2], KB.z, dot2k<32>(D[3], KB.w))));
  t[2] = dot2(D[1], KA.x, dot2(D[2], KA.y, dot2(D[3], KA.z, dot2k<32>(D[4], KA.w))));
  t[3] = dot2(D[1], KB.x, dot2(D[2], KB.y, dot2(D[3], KB.z, dot2k<32>(D[4], KB.w))));
}
// (lo >> 2) | (hi >> 2) << 16 in two instructions: the second shift writes its
// low 16 bits straight into the upper half (SDWA dst_sel:WORD_1, preserve).
__device__ __forceinline__ unsigned pack_shr2(int lo, int hi) {
  unsigned d = (unsigned)(lo >> 2);
  asm("v_ashrrev_i32_sdwa %0, 2, %1 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD "
      "src1_sel:DWORD"
      : "+v"(d)
      : "v"(hi));
  return d;
}
// (lo >> 10) | (hi >> 10) << 16, the same way (arithmetic shifts).
__device__ __forceinline__ unsigned pack_sra10(int lo, int hi) {
  unsigned d = (unsigned)(lo >> 10);
  asm("v_ashrrev_i32_sdwa %0, 10, %1 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD "
      "src1_sel:DWORD"
      : "+v"(d)
      : "v"(hi));
  return d;
}
// Vertical pass, streamed: row pair k = (t[2k], t[2k+1]) (pair 4 = (t[8], 0))
// feeds output row r through tap-pair set G_{r&1}, entry k - (r >> 1)
// (aux_functions.cl:1182-1223); integer sums, so the order is free.
// t0/t1 are the raw horizontal sums (before >> 2).
__device__ __forceinline__ void vpair(int k, const int (&t0)[4], const int (&t1)[4],
                                      const uint4& G0, const uint4& G1, int (&acc)[4][4]) {
#pragma unroll
  for (int c = 0; c < 4; c++) {
    const unsigned P = pack_shr2(t0[c], t1[c]);
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int m = k - (r >> 1);
      if (m < 0 || m > 3 || ((r & 1) == 0 && m == 3)) continue;  // set 0 ends with (0,0)
      const uint4& G = (r & 1) ? G1 : G0;
      const unsigned g = m == 0 ? G.x : m == 1 ? G.y : m == 2 ? G.z : G.w;
      acc[r][c] = m == 0 ? dot2k<0>(P, g) : dot2(P, g, acc[r][c]);  // first tap pair starts the sum
    }
  }
}
// Window rows from the LDS tile, one row pair at a time (software-pipelining
// the reads one pair ahead held ~20 more VGPRs for no measurable gain: the
// other waves hide the LDS latency).
template <int PITCH_DW>
__device__ __forceinline__ void filter_rows(const unsigned* src, const uint4& KA, const uint4& KB,
                                            const uint4& G0, const uint4& G1, int (&acc)[4][4]) {
#pragma unroll
  for (int k = 0; k < 5; k++) {
    unsigned E[2][5];
#pragma unroll
    for (int h = 0; h < 2; h++)
      if (2 * k + h < 9) {  // row 9 does not exist
#pragma unroll
        for (int q = 0; q < 5; q++) E[h][q] = src[(2 * k + h) * PITCH_DW + q];
      }
    int t0[4], t1[4] = {0, 0, 0, 0};
    hrow_raw(E[0], KA, KB, t0);
    if (k < 4) hrow_raw(E[1], KA, KB, t1);
    vpair(k, t0, t1, G0, G1, acc);
    __builtin_amdgcn_sched_barrier(0);
  }
}
// A wave some of whose windows leave the LDS tile: every lane runs the one
// filter_rows computation, its window rows from the tile (in-tile lanes, taps
// of their start parity) or from the frame (the others, re-aligned to an even
// start, parity-0 taps), so such a wave computes its predictions once instead
// of once per path.  The frame rows come in two batches (rows 0-3, rows 4-8,
// each batch's loads in flight together): 6 dwords per row from the uniform
// frame base, re-aligned by v_alignbit, or -- a window crossing the left /
// right frame edge -- per-sample clamped loads; rows clamp to the frame
// (clamp-to-edge, affine.cl:254-326).
// One window row from the frame, as 5 dwords of sample pairs from an even
// start: 6 dwords from the uniform frame base re-aligned by v_alignbit, or --
// a window crossing the left / right frame edge -- per-sample clamped loads.
__device__ __forceinline__ void frame_row(const uint16_t* __restrict__ ref, int wx, int y, int W,
                                          bool wide, unsigned (&D)[5]) {
  if (wide) {
    const char* base = reinterpret_cast<const char*>(ref);
    const unsigned a = (unsigned)wx * 2u, b = a & ~3u, sh = (a & 2u) << 3;  // sh: 0 or 16 bits
    const unsigned off = (unsigned)y * (unsigned)W * 2u + b;
    unsigned raw[6];
    // dword-aligned 16 + 8 byte loads (global_load_dwordx4 / x2 need only dword alignment)
    typedef unsigned u32x4a4 __attribute__((ext_vector_type(4), aligned(4)));
    typedef unsigned u32x2a4 __attribute__((ext_vector_type(2), aligned(4)));
    const u32x4a4 v4 = *reinterpret_cast<const u32x4a4*>(base + off);
    const u32x2a4 v2 = *reinterpret_cast<const u32x2a4*>(base + (off + 16u));
    raw[0] = v4.x; raw[1] = v4.y; raw[2] = v4.z; raw[3] = v4.w; raw[4] = v2.x; raw[5] = v2.y;
#pragma unroll
    for (int q = 0; q < 5; q++) D[q] = __builtin_amdgcn_alignbit(raw[q + 1], raw[q], sh);
  } else {
    const uint16_t* row = ref + (size_t)y * W;
#pragma unroll
    for (int q = 0; q < 5; q++)
      D[q] = (unsigned)row[clampi(wx + 2 * q, 0, W - 1)] | ((unsigned)row[clampi(wx + 2 * q + 1, 0, W - 1)] << 16);
  }
}
// A wave some of whose windows leave the LDS tile: every lane runs the one
// filter_rows computation, its window rows from the tile (in-tile lanes, taps
// of their start parity) or from the frame (the others: rows clamped to the
// frame, clamp-to-edge as affine.cl:254-326, re-aligned to an even start,
// parity-0 taps), one row pair per step -- so such a wave computes its
// predictions once, not once per path, and waits for 5 rounds of frame
// loads instead of 9.
template <int PITCH_DW>
__device__ __forceinline__ void filter_rows_mixed(const unsigned* src, bool inTile,
                                                  const uint16_t* __restrict__ ref, int wx, int wy, int W,
                                                  int H, const uint4& KA, const uint4& KB, const uint4& G0,
                                                  const uint4& G1, int (&acc)[4][4]) {
  const bool wide = wx >= 0 && wx + 12 <= W;
#pragma unroll
  for (int k = 0; k < 5; k++) {
    unsigned E[2][5];
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int row = 2 * k + h;
      if (row < 9) {
        if (inTile) {
#pragma unroll
          for (int q = 0; q < 5; q++) E[h][q] = src[row * PITCH_DW + q];
        } else {
          frame_row(ref, wx, clampi(wy + row, 0, H - 1), W, wide, E[h]);
        }
      }
    }
    int t0[4], t1[4] = {0, 0, 0, 0};
    hrow_raw(E[0], KA, KB, t0);
    if (k < 4) hrow_raw(E[1], KA, KB, t1);
    vpair(k, t0, t1, G0, G1, acc);
    __builtin_amdgcn_sched_barrier(0);
  }
}
// Window leaves the LDS tile: clamp-to-edge loads from the frame
// (affine.cl:254-326), one row at a time (a rare path, kept register-lean:
// scalar vertical taps read from the LDS tap table).
// Vertical taps of window row i into the output rows it feeds.
__device__ __forceinline__ void vrow_acc(int i, const int (&t)[4], const unsigned* s_coef_dw, int fy,
                                         int (&acc)[4][4]) {
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int m = i - r;  // vertical tap of window row i for output row r
    if (m < 0 || m > 5) continue;
    const unsigned pr = s_coef_dw[fy * 12 + (m >> 1)];  // set 0: (f0,f1) (f2,f3) (f4,f5)
    const int cf = (int)(short)(m & 1 ? pr >> 16 : pr & 0xFFFF);
#pragma unroll
    for (int c = 0; c < 4; c++) acc[r][c] += t[c] * cf;
  }
}

// The window read from the frame (it left the staged tile): rows clamped to
// the frame.  A window whose samples wx .. wx + 11 lie inside its rows is
// read as 6 dwords per row from the uniform frame base (32-bit offsets), the
// loads of three rows in flight together, and re-aligned by v_alignbit; one
// that crosses the left / right frame edge takes the per-sample clamped loads.
// (The rows' latency dominates this path: 9 dependent round trips cost the
// 2160p configs 10-20 % of their time.)
__device__ __forceinline__ void filter_rows_global(const uint16_t* __restrict__ ref, int wx, int wy,
                                                   int W, int H, const uint4& KA, const uint4& KB,
                                                   const unsigned* s_coef_dw, int fy,
                                                   int (&acc)[4][4]) {
  if (wx >= 0 && wx + 12 <= W) {
    const char* base = reinterpret_cast<const char*>(ref);
    const unsigned a = (unsigned)wx * 2u, b = a & ~3u, sh = (a & 2u) << 3;  // sh: 0 or 16 bits
    constexpr int NB = 5;  // rows whose loads are in flight together
#pragma unroll 1
    for (int i0 = 0; i0 < 9; i0 += NB) {
      unsigned raw[NB][6];
#pragma unroll
      for (int j = 0; j < NB; j++) {
        if (i0 + j >= 9) break;
        const unsigned off = (unsigned)clampi(wy + i0 + j, 0, H - 1) * (unsigned)W * 2u + b;
#pragma unroll
        for (int k = 0; k < 6; k++) raw[j][k] = *reinterpret_cast<const unsigned*>(base + (off + 4u * k));
      }
#pragma unroll
      for (int j = 0; j < NB; j++) {
        if (i0 + j >= 9) break;
        unsigned D[5];
#pragma unroll
        for (int q = 0; q < 5; q++) D[q] = __builtin_amdgcn_alignbit(raw[j][q + 1], raw[j][q], sh);
        D[4] &= 0xFFFFu;  // sample wx + 9 meets a zero tap (as in the clamped path)
        int t[4];
        hrow(D, KA, KB, t);
        vrow_acc(i0 + j, t, s_coef_dw, fy, acc);
      }
    }
    return;
  }
#pragma unroll 1
  for (int i = 0; i < 9; i++) {
    const uint16_t* row = ref + (size_t)clampi(wy + i, 0, H - 1) * W;
    unsigned D[5];
#pragma unroll
    for (int q = 0; q < 5; q++) {
      const unsigned lo = row[clampi(wx + 2 * q, 0, W - 1)];
      const unsigned hi = q < 4 ? row[clampi(wx + 2 * q + 1, 0, W - 1)] : 0u;
      D[q] = lo | (hi << 16);
    }
    int t[4];
    hrow(D, KA, KB, t);
    vrow_acc(i, t, s_coef_dw, fy, acc);
  }
}

// xCalcHADs4x4 with the JVET_R0164 DC weighting (aux_functions.cl:1940-2043)
// on packed int16 pairs: the residual o - p is within +-1023, so every stage
// of the 4x4 Hadamard stays within +-16368 and the packed 16-bit adds are
// exact.  Rows are transformed first (elementwise on row vectors), then each
// row vector (c0,c1)(c2,c3); the outputs are the same 16 Walsh-Hadamard
// coefficients as the reference's butterfly (in another order -- the sum of
// magnitudes does not depend on it), the DC term being the first lane of row
// vector 0.  |.| sums run on v_dot2 against (1,1).
__device__ __forceinline__ int satd_4x4(const uint2 (&O)[4], const uint2 (&P)[4]) {
  short2v a[4][2];
#pragma unroll
  for (int r = 0; r < 4; r++) {
    a[r][0] = as_s2(O[r].x) - as_s2(P[r].x);
    a[r][1] = as_s2(O[r].y) - as_s2(P[r].y);
  }
  short2v d[4][2];
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const short2v m0 = a[0][k] + a[3][k], m1 = a[1][k] + a[2][k];
    const short2v m2 = a[1][k] - a[2][k], m3 = a[0][k] - a[3][k];
    d[0][k] = m0 + m1;
    d[1][k] = m2 + m3;
    d[2][k] = m0 - m1;
    d[3][k] = m3 - m2;
  }
  const short2v pm = {1, -1}, z = {0, 0};
  int sum = 0, dc = 0;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const short2v X = d[r][0], Ys = __builtin_shufflevector(d[r][1], d[r][1], 1, 0);
    const short2v mm = X + Ys, nn = X - Ys;  // (c0+c3, c1+c2), (c0-c3, c1-c2)
    // (u + v, u - v) of each pair, one v_pk_mad_i16 with op_sel
    const short2v e0 = __builtin_shufflevector(mm, mm, 1, 1) * pm + __builtin_shufflevector(mm, mm, 0, 0);
    const short2v e1 = __builtin_shufflevector(nn, nn, 1, 1) * pm + __builtin_shufflevector(nn, nn, 0, 0);
    const short2v a0 = __builtin_elementwise_max(e0, z - e0), a1 = __builtin_elementwise_max(e1, z - e1);
    if (r == 0) {
      dc = (unsigned short)a0[0];
      sum = dot2(as_u(a0), 0x00010000u, sum);
    } else {
      sum = dot2(as_u(a0), 0x00010001u, sum);
    }
    sum = dot2(as_u(a1), 0x00010001u, sum);
  }
  sum += dc >> 2;
  return (sum + 1) >> 1;
}

// PROF, the reference's hard-disabled refinement (enablePROF = 0 at
// affine.cl:168 / :1132), offered as an option (vame_set_prof).  Per sample,
// the MV offset from the sub-block centre (aux_functions.cl:218-404,
// get{Horizontal,Vertical}DeltasPROF{2,3}Cps), linear in (r, c) before its
// rounding: m(r, c) = 2 (h + v) - 2 (4h + 4v) + 4h c + 4v r, rounded by 8 bits
// (roundValue16) and clamped to +-31.  Recomputed per sample from six
// registers instead of holding 32 deltas.
__device__ __forceinline__ int prof_delta(int base, int q4h, int q4v, int r, int c) {
  const int m = base + q4h * c + q4v * r;
  return clampi((m + 128 - (m >= 0)) >> 8, -31, 31);
}
// PROF proper (aux_functions.cl:471-605) on the vertical pass taken as not
// the last one (shift 6, no offset, no clip: aux_functions.cl:1163-1174):
// the block padded to 6x6 with the reference samples around the integer
// position nearest the fractional MV (xFrac >> 3, yFrac >> 3), scaled to the
// internal precision, gradients of the >> 6 samples, dI = gx dH + gy dV
// clamped to [-8192, 8191], then (p + dI + 8 + 8192) >> 4 clipped to 10 bits.
// acc holds the vertical sums + 524800 (the re-based filter offsets);
// smp(row, col) reads the 9x9 filter window (origin two samples above-left
// of the integer-MV corner).
template <typename Smp>
__device__ __forceinline__ void prof_refine(const int (&acc)[4][4], const MvField& f, int fx, int fy,
                                            Smp smp, int (&pr)[4][4]) {
  const int xo = fx >> 3, yo = fy >> 3;
  int L[4], R[4], T[4], B[4];  // padding columns / rows, >> 6 of the scaled samples
#pragma unroll
  for (int k = 0; k < 4; k++) {
    L[k] = ((smp(yo + 2 + k, xo + 1) << 4) - 8192) >> 6;
    R[k] = ((smp(yo + 2 + k, xo + 6) << 4) - 8192) >> 6;
    T[k] = ((smp(yo + 1, xo + 2 + k) << 4) - 8192) >> 6;
    B[k] = ((smp(yo + 6, xo + 2 + k) << 4) - 8192) >> 6;
  }
  int p[4][4], q[4][4];
#pragma unroll
  for (int r = 0; r < 4; r++)
#pragma unroll
    for (int c = 0; c < 4; c++) {
      p[r][c] = (acc[r][c] - 524800) >> 6;
      q[r][c] = p[r][c] >> 6;
    }
  const int q4hx = shl(f.hx, 2), q4vx = shl(f.vx, 2), q4hy = shl(f.hy, 2), q4vy = shl(f.vy, 2);
  const int bh = shl(f.hx + f.vx, 1) - shl(q4hx + q4vx, 1);
  const int bv = shl(f.hy + f.vy, 1) - shl(q4hy + q4vy, 1);
#pragma unroll
  for (int r = 0; r < 4; r++)
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const int gx = (c == 3 ? R[r] : q[r][c + 1]) - (c == 0 ? L[r] : q[r][c - 1]);
      const int gy = (r == 3 ? B[c] : q[r + 1][c]) - (r == 0 ? T[c] : q[r - 1][c]);
      const int di = clampi(gx * prof_delta(bh, q4hx, q4vx, r, c) + gy * prof_delta(bv, q4hy, q4vy, r, c),
                            -8192, 8191);
      pr[r][c] = clampi((p[r][c] + di + 8 + 8192) >> 4, 0, 1023);
    }
}

// One 4x4 sub-block: affine MV (affine.cl:215-252), 9x9 window with
// clamp-to-edge (affine.cl:254-326), separable 6-tap filter (aux_functions.cl
// :1096-1239, PROF off), SATD against the original (aux_functions.cl:1940-2043).
// The prediction stays in registers (P[r] = packed sample pairs of row r) for
// the gradient step, and so do the original samples (O[r]).
template <int TILE, int TP, bool PROF, bool FORCE_TILE = false, int NCP = 3>
__device__ __forceinline__ int predict_sb(const MvField& f, int sx, int sy, const Geo& g,
                                          const uint16_t* s_tile, int tx0, int ty0, int tmx, int tmy,
                                          const uint16_t* __restrict__ ref,
                                          const uint16_t* __restrict__ cur, int W, int H,
                                          const uint4* s_coef, uint2 (&P)[4], uint2 (&O)[4],
                                          bool& outside) {
  {  // 32-bit byte offsets from the uniform frame base (frames < 4 GiB): the
     // saddr form of global_load, no 64-bit address arithmetic per row
    const unsigned b0 = (unsigned)((g.y + sy) * W + g.x + sx) * 2u, bw = (unsigned)W * 2u;
    const char* base = reinterpret_cast<const char*>(cur);
#pragma unroll
    for (int r = 0; r < 4; r++) O[r] = *reinterpret_cast<const uint2*>(base + (b0 + (unsigned)r * bw));
  }
  const int px = f.spread ? (g.w >> 1) : sx + 2, py = f.spread ? (g.h >> 1) : sy + 2;
  // |h|, |v| < 2^22 (clamped CPMVs, << (7 - log2 size)), px, py <= 128: 24-bit products are exact
  int mx, my;
  if constexpr (NCP == 2) {  // (vx, vy) = (-hy, hx): no negated operand
    mx = f.bx + __mul24(f.hx, px) - __mul24(f.hy, py);
    my = f.by + __mul24(f.hy, px) + __mul24(f.hx, py);
  } else {
    mx = f.bx + __mul24(f.hx, px) + __mul24(f.vx, py);
    my = f.by + __mul24(f.hy, px) + __mul24(f.vy, py);
  }
  mx = (mx + 64 - (mx >= 0)) >> 7;  // roundMv (aux_functions.cl:38-47)
  my = (my + 64 - (my >= 0)) >> 7;
  // clipMv (aux_functions.cl:51-67) on the frame position of the MV's target,
  // 16 x the CU position + mv: its bounds [(-135 - x) << 4, (W + 7 - x) << 4]
  // shifted by x << 4 become the frame constants [-135 << 4, (W + 7) << 4]
  // (the shift is a multiple of 16: the fractional phase is unchanged)
  const int ax = clampi(mx + shl(g.x, 4), -135 * 16, (W + 7) * 16);
  const int ay = clampi(my + shl(g.y, 4), -135 * 16, (H + 7) * 16);
  const int fx = ax & 15, fy = ay & 15;
  const int wx = (ax >> 4) + sx - 2, wy = (ay >> 4) + sy - 2;  // window origin (frame)
  int tx = wx - tx0, ty = wy - ty0;
  if ((VAME_ABLATE & 512) || FORCE_TILE) {  // timing-only: every window read from the tile (wrong results)
    tx = clampi(tx, 0, tmx);
    ty = clampi(ty, 0, tmy);
  }
  // tmx / tmy: the largest window origin inside the staged tile (its extent - 9)
  const bool inTile = (unsigned)tx <= (unsigned)tmx && (unsigned)ty <= (unsigned)tmy;
  outside = !inTile;
#if VAME_COUNT_PRED
  {  // instrumentation: outside windows that a 4 / 8 / 16 px wider margin would hold
#pragma unroll
    for (int e = 0; e < 3; e++) {
      const int x = 4 << e;
      const bool in = (unsigned)(tx + x) <= (unsigned)(tmx + 2 * x) && (unsigned)(ty + x) <= (unsigned)(tmy + 2 * x);
      const unsigned long long m = __builtin_amdgcn_ballot_w64(!inTile && in);
      if (m && __lane_id() == __builtin_ctzll(__builtin_amdgcn_ballot_w64(true)))
        atomicAdd(&g_pred_count[6 + 3 * (TILE > 100) + e], (unsigned long long)__popcll(m));
    }
  }
#endif
  if (!PROF && __builtin_amdgcn_ballot_w64(!(inTile && (fx | fy) == 0)) == 0) {
    // Every active lane has an integer MV inside the tile (e.g. every sub-block
    // of the first 2-CP prediction, from zero CPMVs): the phase-0 filter is the
    // identity -- (64 s - 32768) >> 2 = 16 s - 8192, then
    // (64 (16 s - 8192) + 512 + (8192 << 6)) >> 10 = s, within [0, 1023] (KAT-1)
    // -- so the prediction is the window's inner 4x4, copied from the tile.
    const int i0 = (ty + 2) * TP + tx + 2;  // the block's first sample in the tile
    const unsigned* s32 = reinterpret_cast<const unsigned*>(s_tile) + (i0 >> 1);
    const unsigned sh = (unsigned)(i0 & 1) << 4;  // 0 or 16: its half of the dword
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const unsigned d0 = s32[r * (TP / 2)], d1 = s32[r * (TP / 2) + 1], d2 = s32[r * (TP / 2) + 2];
      P[r].x = __builtin_amdgcn_alignbit(d1, d0, sh);
      P[r].y = __builtin_amdgcn_alignbit(d2, d1, sh);
    }
    return satd_4x4(O, P);
  }
  const int sp = inTile ? (tx & 1) : 0;
  const uint4 KA = s_coef[fx * 3 + sp], KB = s_coef[fx * 3 + sp + 1];
  const uint4 G0 = s_coef[fy * 3 + 0], G1 = s_coef[fy * 3 + 1];
  int acc[4][4];
  if (!PROF) {
    // offsets folded into the rows (hrow_raw); the first tap pair overwrites acc (vpair)
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
      for (int c = 0; c < 4; c++) acc[r][c] = 0;
    const unsigned* src = reinterpret_cast<const unsigned*>(s_tile) + ((ty * TP + tx) >> 1);  // in-tile lanes
    if (__builtin_amdgcn_ballot_w64(!inTile) == 0)
      filter_rows<TP / 2>(src, KA, KB, G0, G1, acc);
    else  // a wave with windows outside the tile: one filter pass for every lane
      filter_rows_mixed<TP / 2>(src, inTile, ref, wx, wy, W, H, KA, KB, G0, G1, acc);
  } else if (inTile) {
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
      for (int c = 0; c < 4; c++) acc[r][c] = 0;  // offsets folded into the rows (hrow_raw);
                                                  // the first tap pair overwrites it (vpair)
    const unsigned* src = reinterpret_cast<const unsigned*>(s_tile) + ((ty * TP + tx) >> 1);
    filter_rows<TP / 2>(src, KA, KB, G0, G1, acc);
  } else {
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
      for (int c = 0; c < 4; c++) acc[r][c] = 524800;  // (1 << 9) + (8192 << 6)
    filter_rows_global(ref, wx, wy, W, H, KA, KB, reinterpret_cast<const unsigned*>(s_coef), fy,
                       acc);
  }
  int pr[4][4];
  if (PROF && !f.spread) {  // applyPROF = enablePROF && !isSpread (aux_functions.cl:1101)
    if (inTile) {
      const uint16_t* win = s_tile + ty * TP + tx;
      prof_refine(acc, f, fx, fy, [&](int r, int c) { return (int)win[r * TP + c]; }, pr);
    } else {
      prof_refine(acc, f, fx, fy,
                  [&](int r, int c) {
                    return (int)ref[(size_t)clampi(wy + r, 0, H - 1) * W + clampi(wx + c, 0, W - 1)];
                  },
                  pr);
    }
  } else {
    // clipPel on packed pairs: acc >> 10 lies well inside int16 (the taps'
    // absolute sums are below 2^7 per pass), so pack first, then clamp both
    // halves at once (4 instructions per pair instead of 5)
    const short2v lo = {0, 0}, hi = {1023, 1023};
#pragma unroll
    for (int r = 0; r < 4; r++) {
      P[r].x = as_u(__builtin_elementwise_min(
          __builtin_elementwise_max(as_s2(pack_sra10(acc[r][0], acc[r][1])), lo), hi));
      P[r].y = as_u(__builtin_elementwise_min(
          __builtin_elementwise_max(as_s2(pack_sra10(acc[r][2], acc[r][3])), lo), hi));
    }
    return satd_4x4(O, P);
  }
#pragma unroll
  for (int r = 0; r < 4; r++) {
    P[r].x = pack16(pr[r][0], pr[r][1]);
    P[r].y = pack16(pr[r][2], pr[r][3]);
  }
  return satd_4x4(O, P);
}

// Extended prediction row of a sub-block: columns -1..4 as the packed pairs
// (c-1,c0) (c0,c1) (c2,c3) (c3,c4); (c1,c2) is re-derived where needed.
// Column -1 comes from the left lane's column 3 and column 4 from the right
// lane's column 0 (DPP wave_shr:1 / wave_shl:1 -- lanes of a CU row are
// consecutive; at CU edges the values are never used, see grad_sb).
__device__ __forceinline__ uint4 ext_row(const uint2& p, unsigned left, unsigned right) {
  return make_uint4(__builtin_amdgcn_alignbit(p.x, left, 16), p.x, p.y,
                    __builtin_amdgcn_alignbit(right, p.y, 16));
}

// One 4x4 sub-block of the gradient step (affine.cl:477-708): 3x3 Sobel on the
// 6x6 prediction patch (own rows as extended rows X[1..4], the neighbours' edge
// rows X[0] above and X[5] below) with the CU-border replication of
// affine.cl:506-540 (rows first, then columns) -- so patch samples outside the
// CU are never used -- the residual orig - pred (affine.cl:547-579) and the five
// sums S = (gx.gx, gx.gy, gy.gy, gx.e, gy.e).  Samples are handled as packed
// int16 pairs: |g| <= 4092 and |e| <= 1023 fit, and v_dot2_i32_i16 sums stay
// below 2^28 (exact).
// 2 a + b on both int16 halves in one v_pk_mad_i16 (op_sel_hi:0 on the inline
// constant: its low half, 2, multiplies the high halves too)
__device__ __forceinline__ short2v twice_plus(short2v a, short2v b) {
  unsigned r;
  asm("v_pk_mad_i16 %0, %1, 2, %2 op_sel_hi:[1,0,1]" : "=v"(r) : "v"(as_u(a)), "v"(as_u(b)));
  return as_s2(r);
}
__device__ __forceinline__ void grad_sb(int sx, int sy, const Geo& g, const uint4 (&X)[6],
                                        const uint2 (&Orig)[4], int S[5]) {
  short2v O[6][3], E[6][2];
#pragma unroll
  for (int i = 0; i < 6; i++) {
    O[i][0] = as_s2(X[i].x);                                      // (sx-1, sx)
    O[i][1] = as_s2(__builtin_amdgcn_alignbit(X[i].z, X[i].y, 16));  // (sx+1, sx+2)
    O[i][2] = as_s2(X[i].w);                                      // (sx+3, sx+4)
    E[i][0] = as_s2(X[i].y);                                      // (sx, sx+1)
    E[i][1] = as_s2(X[i].z);                                      // (sx+2, sx+3)
  }
  short2v gx[4][2], gy[4][2];
#pragma unroll
  for (int k = 0; k < 2; k++) {
    short2v Hd[6], Vs[6];
#pragma unroll
    for (int i = 0; i < 6; i++) {
      Hd[i] = O[i][k + 1] - O[i][k];                       // p(c+1) - p(c-1)
      Vs[i] = twice_plus(E[i][k], O[i][k] + O[i][k + 1]);  // p(c-1) + 2 p(c) + p(c+1)
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
      gx[r][k] = twice_plus(Hd[r + 1], Hd[r] + Hd[r + 2]);
      gy[r][k] = Vs[r + 2] - Vs[r];
    }
  }
  if (sy == 0) {
#pragma unroll
    for (int k = 0; k < 2; k++) { gx[0][k] = gx[1][k]; gy[0][k] = gy[1][k]; }
  }
  if (sy + 4 == g.h) {
#pragma unroll
    for (int k = 0; k < 2; k++) { gx[3][k] = gx[2][k]; gy[3][k] = gy[2][k]; }
  }
  if (sx == 0) {  // column 0 <- column 1: low half <- high half of pair 0
#pragma unroll
    for (int r = 0; r < 4; r++) {
      gx[r][0] = as_s2(__builtin_amdgcn_perm(as_u(gx[r][0]), as_u(gx[r][0]), 0x03020302u));
      gy[r][0] = as_s2(__builtin_amdgcn_perm(as_u(gy[r][0]), as_u(gy[r][0]), 0x03020302u));
    }
  }
  if (sx + 4 == g.w) {  // column 3 <- column 2: high half <- low half of pair 1
#pragma unroll
    for (int r = 0; r < 4; r++) {
      gx[r][1] = as_s2(__builtin_amdgcn_perm(as_u(gx[r][1]), as_u(gx[r][1]), 0x01000100u));
      gy[r][1] = as_s2(__builtin_amdgcn_perm(as_u(gy[r][1]), as_u(gy[r][1]), 0x01000100u));
    }
  }
  int sxx = 0, sxy = 0, syy = 0, sxe = 0, sye = 0;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const uint2 o = Orig[r];
    const unsigned e0 = as_u(as_s2(o.x) - E[r + 1][0]), e1 = as_u(as_s2(o.y) - E[r + 1][1]);
    const unsigned x0 = as_u(gx[r][0]), x1 = as_u(gx[r][1]);
    const unsigned y0 = as_u(gy[r][0]), y1 = as_u(gy[r][1]);
    sxx = dot2(x0, x0, dot2(x1, x1, sxx));
    sxy = dot2(x0, y0, dot2(x1, y1, sxy));
    syy = dot2(y0, y0, dot2(y1, y1, syy));
    sxe = dot2(x0, e0, dot2(x1, e1, sxe));
    sye = dot2(y0, e0, dot2(y1, e1, sye));
  }
  S[0] = sxx; S[1] = sxy; S[2] = syy; S[3] = sxe; S[4] = sye;
}

// VTM solveEqual (affine.cl:782-856), forward elimination shared by the lanes
// of a CU's segment (li = lane in the segment, Ls = segment size) on the CU's
// matrix M (row r = private_dEqualCoeff[r + 1], N + 1 columns) in LDS:
// every lane repeats the pivot search (sequential strict '>' scan, NaN never
// wins); the row swap and then each element a[j][k] -= a[i][k] * a[j][i-1] /
// a[i][i-1] of the step (no zero-pivot guard) is done by one lane, with the
// reference's operation order.  Columns left of the pivot are dead and skipped.
// Called by every lane of the wave (act: lane works on a live CU).
template <int N>
__device__ __forceinline__ void seg_eliminate(double* M, int li, int Ls, bool act) {
  constexpr int NC = N + 1;
#pragma unroll
  for (int i = 1; i < N; i++) {
    if (act) {
      double temp = fabs(M[(i - 1) * NC + i - 1]);
      int idx = i - 1;
#pragma unroll
      for (int r = i; r < N; r++) {
        const double f = fabs(M[r * NC + i - 1]);
        if (f > temp) {
          temp = f;
          idx = r;
        }
      }
      if (idx != i - 1 && li < N + 2 - i) {
        const int c = i - 1 + li;
        const double a = M[(i - 1) * NC + c], b = M[idx * NC + c];
        M[(i - 1) * NC + c] = b;
        M[idx * NC + c] = a;
      }
    }
    wave_sync();
    const int cols = N + 1 - i, E = (N - i) * cols;  // constants after unrolling
    if (act) {
      // at most two elements per lane (E <= 30, Ls >= 16); e / cols for e < 64
      // by a multiply-shift (exact for these small operands)
      constexpr int kMagic[7] = {0, 0, 513, 342, 257, 206, 171};  // ceil(1024 / cols)
#pragma unroll
      for (int q = 0; q < 2; q++) {
        const int e = li + q * Ls;
        if (e < E) {
          const int dr = (e * kMagic[N + 1 - i]) >> 10, r = i + dr, k = i + e - dr * cols;
          M[r * NC + k] = __dsub_rn(M[r * NC + k], __ddiv_rn(__dmul_rn(M[(i - 1) * NC + k], M[r * NC + i - 1]),
                                                             M[(i - 1) * NC + i - 1]));
        }
      }
    }
    wave_sync();
  }
}

// Back-substitution of solveEqual (affine.cl:832-856): fma where the
// reference's FP_CONTRACT fuses, all-zero result on a zero pivot; then the
// deltas fed to scaleDeltaMvs (affine.cl:860-883).
template <int NCP>
__device__ __forceinline__ void back_substitute(const double* M, int lw, int lh, double dd[6]) {
  constexpr int N = 2 * NCP, NC = N + 1;
  double p[N];
#pragma unroll
  for (int k = 0; k < N; k++) p[k] = 0.;
  p[N - 1] = __ddiv_rn(M[(N - 1) * NC + N], M[(N - 1) * NC + N - 1]);
  bool zero = false;
#pragma unroll
  for (int i = N - 2; i >= 0; i--) {
    if (!zero) {
      const double piv = M[i * NC + i];
      if (piv == 0.) {
        zero = true;
      } else {
        double temp = 0;
#pragma unroll
        for (int j = i + 1; j < N; j++) temp = fma(M[i * NC + j], p[j], temp);
        p[i] = __ddiv_rn(__dsub_rn(M[i * NC + N], temp), piv);
      }
    }
  }
  if (zero) {
#pragma unroll
    for (int k = 0; k < N; k++) p[k] = 0.;
  }
  const double w = (double)(1 << lw), h = (double)(1 << lh);
  dd[0] = p[0];
  dd[2] = p[2];
  dd[1] = __dadd_rn(__dmul_rn(p[1], w), p[0]);  // exact scaling by a power of two
  if constexpr (NCP == 3) {
    dd[3] = __dadd_rn(__dmul_rn(p[3], w), p[2]);
    dd[4] = __dadd_rn(__dmul_rn(p[4], h), p[0]);
    dd[5] = __dadd_rn(__dmul_rn(p[5], h), p[2]);
  } else {
    dd[3] = __dadd_rn(__dmul_rn(-p[3], w), p[2]);
    dd[4] = dd[5] = 0.;
  }
}

// Which reduced value feeds matrix element e = r * (N + 1) + c (eq_element's
// mapping as a table): bits 0-6 the value index, bit 7 set on the right-hand
// side column (scaled by 8).  2 CP: elements 0..19, 3 CP: 32..73.
struct EqMap {
  uint8_t v[80];
};
constexpr uint8_t eq_map_entry(int ncp, int r, int c) {
  if (ncp == 2) {
    if (c == 4) return (uint8_t)(0x80 | (10 + r));
    const int lo = r < c ? r : c, hi = r < c ? c : r;
    return (uint8_t)(lo == 0 ? hi : lo == 1 ? 3 + hi : lo == 2 ? 5 + hi : 9);
  }
  const int tr = (r == 2 || r == 3 || r == 5) ? 1 : 0, mr = (r == 1 || r == 3) ? 1 : (r >= 4 ? 2 : 0);
  if (c == 6) return (uint8_t)(0x80 | (18 + 3 * tr + mr));
  const int tc = (c == 2 || c == 3 || c == 5) ? 1 : 0, mc = (c == 1 || c == 3) ? 1 : (c >= 4 ? 2 : 0);
  const int prod = mr == 0 ? mc : mc == 0 ? mr : (mr == 1 && mc == 1) ? 3 : (mr == 2 && mc == 2) ? 5 : 4;
  return (uint8_t)(6 * (tr + tc) + prod);
}
constexpr EqMap make_eq_map() {
  EqMap m{};
  for (int e = 0; e < 20; e++) m.v[e] = eq_map_entry(2, e / 5, e % 5);
  for (int e = 0; e < 42; e++) m.v[32 + e] = eq_map_entry(3, e / 7, e % 7);
  return m;
}
static __constant__ EqMap kEqMap = make_eq_map();

// Build, eliminate and back-substitute one CU's system with its segment; the
// segment's first lane returns the deltas.  The int64 sums convert exactly
// (|value| < 2^53); the right-hand side is scaled by 8 exactly.
template <int NCP, bool KEEP_V = false>
__device__ __forceinline__ void seg_solve(long long* V, double* M, const uint8_t* eqmap, int li,
                                          int Ls, bool act, bool coop, int lw, int lh,
                                          double dd[6]) {
  constexpr int N = 2 * NCP, NC = N + 1;
  if (act) {
    for (int e = li; e < N * NC; e += Ls) {
      const int m = eqmap[(NCP == 2 ? 0 : 32) + e];
      const double sc = (m & 0x80) ? 8.0 : 1.0;
      M[e] = (double)V[m & 0x7F] * sc;
    }
    if (!KEEP_V && coop && li < kNumMom) {  // cooperative items accumulate with atomics
      int z = 0;
      opaque(z);  // a fresh zero, not a loop-carried (spilled) constant
      reinterpret_cast<int2*>(V)[li] = make_int2(z, z);
    }
  }
  wave_sync();
  seg_eliminate<N>(M, li, Ls, act);
  if (act && li == 0) {
    back_substitute<NCP>(M, lw, lh, dd);
    // the deltas for the CU's update lanes (M is dead now)
#pragma unroll
    for (int i = 0; i < 2 * NCP; i++) M[i] = dd[i];
  }
  wave_sync();
}

// Value i of a sub-block's contribution to its CU's normal equations
// (affine.cl:683-707: every sample of a sub-block uses the sub-block centre
// (u, v)), from the sub-block's five sums S.
//   2 CP, iC = (gx, u gx + v gy, gy, v gx - u gy) (affine.cl:691-694): the 10
//        distinct entries A00 A01 A02 A03 A11 A12 A13 A22 A23 A33 of the
//        symmetric matrix, then b0..b3 (before the << 3);
//   3 CP (affine.cl:684-689): the moments {1,u,v,uu,uv,vv} x {xx,xy,yy}, then
//        {1,u,v} x {xe,ye}; solve_cu forms the matrix from them.
__device__ __forceinline__ long long mul64(int a, int b) { return (long long)a * (long long)b; }

template <int NCP>
__device__ __forceinline__ long long eq_value(int i, const int (&S)[5], int u, int v) {
  // monomials fit int32 (u, v <= 126); every product is one i32 x i32 -> i64
  const int xx = S[0], xy = S[1], yy = S[2], xe = S[3], ye = S[4];
  const int uu = u * u, uv = u * v, vv = v * v;
  if constexpr (NCP == 2) {
    switch (i) {
      case 0: return xx;
      case 1: return mul64(u, xx) + mul64(v, xy);
      case 2: return xy;
      case 3: return mul64(v, xx) - mul64(u, xy);
      case 4: return mul64(uu, xx) + mul64(2 * uv, xy) + mul64(vv, yy);
      case 5: return mul64(u, xy) + mul64(v, yy);
      case 6: return mul64(uv, xx) + mul64(vv - uu, xy) - mul64(uv, yy);
      case 7: return yy;
      case 8: return mul64(v, xy) - mul64(u, yy);
      case 9: return mul64(vv, xx) - mul64(2 * uv, xy) + mul64(uu, yy);
      case 10: return xe;
      case 11: return mul64(u, xe) + mul64(v, ye);
      case 12: return ye;
      default: return mul64(v, xe) - mul64(u, ye);
    }
  } else {
    const int sidx = i < 18 ? i / 6 : (i < 21 ? 3 : 4);
    const int mono = i < 18 ? i % 6 : (i - 18) % 3;
    const int m = mono == 0 ? 1 : mono == 1 ? u : mono == 2 ? v : mono == 3 ? uu : mono == 4 ? uv : vv;
    return mul64(m, S[sidx]);
  }
}

}  // namespace vame

// vame_search.h -- the search's iteration from caller-given CPMVs on a CU list
// (vame_affine_search) and the seeded improvement of a POC's search results
// (vame_affine_me_seeded); include/vame.h, DESIGN.md §15: the parameter blocks
// and launch functions of vame_search.hip.
#pragma once
#include "vame_bipred.h"

namespace vame {

struct SearchParams {
  const uint16_t* cur;
  const uint16_t* refs[4];
  const McCu* cus;
  McCu* out;       // may be `cus`
  int64_t* cost;   // [maxCus]
  int32_t* bad;
  int maxCus, nrefs, W, H, extra;
  float lambda;
  const int32_t* ncusDev;  // or NULL: the count is maxCus
};
// The launches of one vame_affine_search call on `stream` (maxCus >= 1): one
// per size class, no scratch.
hipError_t search_launch(const SearchParams& p, hipStream_t stream);

// vame_affine_search_p: the same block and one predictor per
// descriptor; its kernels are instances of their own, vame_affine_search's hold
// no predictor code.
struct SearchParamsP : SearchParams {
  const int32_t* preds;  // vame_cpmvs (7 int32) [maxCus]
};
hipError_t search_p_launch(const SearchParamsP& p, hipStream_t stream);

// vame_affine_me_seeded's work buffer: the count of seeded rows, then per slot
// (capacity = refs x in-frame candidates of the alignments in the mask) the
// 2-CP descriptor, its cost, where it goes (refIdx | align << 2, row) and, with
// 3-CP in the mask, the 3-CP descriptor and its cost.
struct SeededWork {
  int32_t* count;
  McCu* cus2;
  McCu* cus3;
  int64_t* cost2;
  int64_t* cost3;
  int32_t* slot;  // [cap][2]
};
constexpr size_t kSeededHead = 64;  // bytes in front of the lists (the count)
inline size_t seeded_work_bytes(size_t cap, bool with3) {
  return kSeededHead + cap * ((with3 ? 2 : 1) * (sizeof(McCu) + sizeof(int64_t)) + 2 * sizeof(int32_t));
}
inline SeededWork seeded_work(void* base, size_t cap, bool with3) {
  char* b = static_cast<char*>(base);
  SeededWork w;
  w.count = reinterpret_cast<int32_t*>(b);
  b += kSeededHead;
  w.cost2 = reinterpret_cast<int64_t*>(b);
  b += cap * sizeof(int64_t);
  w.cost3 = with3 ? reinterpret_cast<int64_t*>(b) : nullptr;
  b += with3 ? cap * sizeof(int64_t) : 0;
  w.cus2 = reinterpret_cast<McCu*>(b);
  b += cap * sizeof(McCu);
  w.cus3 = with3 ? reinterpret_cast<McCu*>(b) : nullptr;
  b += with3 ? cap * sizeof(McCu) : 0;
  w.slot = reinterpret_cast<int32_t*>(b);
  return w;
}

struct SeededParams {
  SearchParams search;           // cur, refs, bad, nrefs, W, H, extra, lambda
  const BiCand* cands;           // vame_create's table of the in-frame candidates
  int candBegin, candEnd;        // those of the alignments in the mask
  const int32_t* seed[4][2];     // vame_mv [rows], [refIdx][align]
  int64_t* cost[4][4];           // the results to improve, [refIdx][PRED]
  int32_t* cpmv[4][4];           // vame_cpmvs, 7 int32 per row
  SeededWork work;
  int cap;
  bool with3;
};
// The launches of one vame_affine_me_seeded call on `stream`.
hipError_t seeded_launch(const SeededParams& p, hipStream_t stream);

// vame_affine_me_seeded_p: the rows' translational predictors
// in the seed layout; the build kernel expands a row's to LT = RT = LB in
// `preds` (the work buffer's tail, one vame_cpmvs per slot), which both
// searches price against.
struct SeededParamsP : SeededParams {
  const int32_t* mvp[4][2];  // vame_mv [rows], [refIdx][align]
  int32_t* preds;            // [cap][7]
};
inline size_t seeded_p_work_bytes(size_t cap, bool with3) {
  return seeded_work_bytes(cap, with3) + cap * 7 * sizeof(int32_t);
}
hipError_t seeded_p_launch(const SeededParamsP& p, hipStream_t stream);

// vame_reprice: the zero-predictor rate of every in-frame row's CPMVs replaced
// by the rate against the row's predictor.
struct RepriceParams {
  const BiCand* cands;
  int candBegin, candEnd;    // the in-frame candidates of the alignments in the mask
  const int32_t* mvp[4][2];  // vame_mv [rows], [refIdx][align]
  int64_t* cost[4][4];       // [refIdx][PRED]; NULL outside the mask
  const int32_t* cpmv[4][4];
  int32_t* bad;
  int nrefs;
  float lambda;
};
hipError_t reprice_launch(const RepriceParams& p, hipStream_t stream);

}  // namespace vame

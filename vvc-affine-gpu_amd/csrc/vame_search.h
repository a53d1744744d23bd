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

}  // namespace vame

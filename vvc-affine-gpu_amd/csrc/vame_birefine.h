// vame_birefine.h -- refinement of bi-predicted CUs (vame_bipred_refine;
// include/vame.h): the parameter block and the launch function
// of vame_birefine.hip.
#pragma once
#include "vame_mc_core.h"

namespace vame {

struct BiRefineParams {
  const uint16_t* cur;
  const uint16_t* refs[4];
  const McBiCu* cus;
  McBiCu* out;     // may be `cus`
  int64_t* cost;   // [maxCus]
  int32_t* bad;
  int maxCus, nrefs, W, H, rounds;
  float lambda;
  const int32_t* ncusDev;  // or NULL: the count is maxCus
};
// The launches of one vame_bipred_refine call on `stream` (maxCus >= 1): one
// per size class, no scratch.
hipError_t birefine_launch(const BiRefineParams& p, hipStream_t stream);

// vame_bipred_refine_p: the same block and the predictors; its
// kernels are instances of their own, vame_bipred_refine's hold no predictor
// code.
struct BiRefineParamsP : BiRefineParams {
  const int32_t* preds;  // vame_cpmvs (7 int32): hypothesis h of descriptor i at 2i + h
};
hipError_t birefine_p_launch(const BiRefineParamsP& p, hipStream_t stream);

}  // namespace vame

// vame_bipred.h -- affine bi-prediction (vame_affine_mc_bi, vame_bipred;
// include/vame.h): vame_bipred's parameter block and launch
// function (vame_affine_mc_bi's are vame_mc_core.h's McBiParams, mc_bi_launch).
#pragma once
#include "vame_items.h"
#include "vame_mc_core.h"

namespace vame {

constexpr int kBiPairs = 6;  // (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)

struct BiRowsParams {
  const uint16_t* cur;
  const uint16_t* refs[4];
  const int64_t* cost[4][4];  // [refIdx][PRED], as vame_poc_result
  const int32_t* cpmv[4][4];  // vame_cpmvs, 7 int32 per row
  int64_t* biCost[2];         // [align], or NULL outside the mask
  int32_t* biSel[2];
  const BiCand* cands;
  const int32_t* groupCand;   // group of 16 sub-blocks -> candidate
  int64_t* pairSatd;          // [candidates][kBiPairs]
  int candBegin, candEnd;     // the candidates of the alignments in the mask
  int groupBegin, groupEnd;   // and their groups
  int rowsOf[2];              // nCtus * {201 | 284}
  int nrefs, predMask, W, H;
  float lambda;
};
// The launches of one vame_bipred call on `stream`.
hipError_t bipred_launch(const BiRowsParams& p, hipStream_t stream);

// vame_bipred_p: the rows' translational predictors in the seed
// layout.  Only the closing kernel reads them (the pair SATDs do not depend on
// a predictor): it is an instance of its own.
struct BiRowsParamsP : BiRowsParams {
  const int32_t* mvp[4][2];  // vame_mv [rows], [refIdx][align]
};
hipError_t bipred_p_launch(const BiRowsParamsP& p, hipStream_t stream);

}  // namespace vame

// vame_bipred.h -- affine bi-prediction (vame_affine_mc_bi, vame_bipred;
// include/vame.h): the parameter blocks and launch functions of
// vame_bipred.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace vame {

// device view of vame_mc_bicu (include/vame.h): 20 int32; the first 12 are a McCu
struct McBiCu {
  int32_t x, y, w, h, ref0;
  int32_t ncps0, c0[6];  // LTx, LTy, RTx, RTy, LBx, LBy
  int32_t ref1;          // -1: uni-predicted from (ref0, c0)
  int32_t ncps1, c1[6];
};

struct McBiParams {
  const uint16_t* cur;  // NULL when cost is
  const uint16_t* refs[4];
  const McBiCu* cus;
  uint16_t* pred;    // or NULL
  int64_t* cost;     // or NULL
  int32_t* bad;
  int32_t* offs;     // [ncus + 1]: first sub-block of each descriptor; the total
  int32_t* blockSum; // [1024]: sub-blocks per scan block
  int ncus, nrefs, W, H;
  float lambda;
  const int32_t* ncusDev;  // or NULL: the count is ncus
};
// The three launches of one vame_affine_mc_bi call on `stream` (ncus >= 1).
hipError_t mc_bi_launch(const McBiParams& p, hipStream_t stream);

// A candidate CU of the frame's fixed geometry that lies wholly in the frame
// (vame_create builds the table: the aligned candidates first, CTUs ascending,
// rows ascending, then the half-aligned ones).
struct BiCand {
  int32_t xy;     // frame x | y << 16
  int32_t shape;  // log2 w | log2 h << 4 | align << 8
  int32_t row;    // ctu * {201 | 284} + offset: the row in its alignment's arrays
  int32_t first;  // its first group of 16 sub-blocks (over both alignments)
};
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

}  // namespace vame

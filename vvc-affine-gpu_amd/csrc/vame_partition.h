// vame_partition.h -- the partition decision's parameter block and launch
// (vame_partition.hip; called by vame_stages.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace vame {

struct McCu;                      // the descriptor it emits (vame_mc_core.h)
constexpr int kPartSlots = 1024;  // nodes of a CTU: ((lh*4 + lw)*8 + y/16)*8 + x/16
// int32 words of a context's scratch per CTU: the leaf count, the leaf code of
// each of the 64 top-left blocks, the owner of each of the 64 blocks
constexpr size_t kPartScratchWords = 1 + 64 + 64;
struct PartParams {
  const int64_t* cost[4][4];  // [refIdx][PRED], as vame_poc_result
  const int32_t* cpmv[4][4];  // vame_cpmvs, 7 int32 per row
  McCu* cus;
  int32_t* rows;              // or NULL
  int32_t* ncus;
  int32_t* ctuInfo;           // or NULL
  int64_t* ctuCost;           // or NULL
  int32_t* blockCu;           // or NULL
  int32_t* scratch;           // nCtus * kPartScratchWords
  long long penalty;
  int nrefs, predMask, W, H, nCtus, ctusPerRow;
  // vame_partition_bi only: the bi cost / selection of every row per alignment
  // (vame_bipred's outputs), the penalty of a bi leaf; `cus` then holds 20-word
  // vame_mc_bicu descriptors, `sel` (or NULL) each leaf's bi_sel or -1
  const int64_t* biCost[2];
  const int32_t* biSel[2];
  long long biPenalty;
  int32_t* sel;
};
// The two launches of one vame_partition call on `stream`; bi: of one
// vame_partition_bi call (the leaf may be a bi-predicted one).
hipError_t partition_launch(const PartParams& p, hipStream_t stream, bool bi = false);

// vame_mvp_gather: per bi descriptor and hypothesis the
// predictor of the candidate row the descriptor's rectangle is, or zero.
struct McBiCu;
struct MvpGatherParams {
  const int32_t* mvp[4][2];  // vame_mv [rows], [refIdx][align]; NULL: that array is not given
  const McBiCu* cus;
  int32_t* preds;            // vame_cpmvs (7 int32), two per descriptor
  const int32_t* ncusDev;    // or NULL: the count is maxCus
  int maxCus, ctusPerRow, nCtus;
};
hipError_t mvp_gather_launch(const MvpGatherParams& p, hipStream_t stream);

}  // namespace vame

// vame_birefine.hip -- refinement of bi-predicted CUs (vame_bipred_refine,
// include/vame.h): one hypothesis of a bi descriptor is held,
// the other runs the search's gradient iteration against what the held one
// leaves to explain, e = 2 cur - P_fixed - P_moving; then the roles swap.
//
// Work mapping: one workgroup per descriptor, one lane per 4x4 sub-block, in
// three size classes -- 64, 256 and 1024 lanes for CUs of up to 64, 256 and
// 1024 sub-blocks.  The count of descriptors lives on the device, so every
// class is launched over the whole capacity and a workgroup whose descriptor
// is past the count or of another class leaves at once.  Per lane, in
// registers: the original block, the fixed hypothesis' 16 accumulators and
// 2 cur - P_fixed; in LDS: the moving hypothesis' samples P_m as int16 [h][w]
// (2 / 8 / 32 KB) for the Sobel neighbourhood, the 24 int64 moments and the
// 6x7 FP64 system.  Every step of the iteration is the search's device
// function (vame_dev.h): mv_field, filter_rows_global, satd_4x4, grad_sb,
// eq_value, seg_solve, scale_delta; the gradient step and the workgroup sums
// are vame_refine_core.h's, shared with vame_search.hip.
//
// Operand widths with |e| <= 2046 (the search has |e| <= 1023): e and
// 2 cur - P_fixed (-1023 .. 2046) fit the packed int16 lanes of grad_sb; its
// five sums over 16 samples stay below 16 * 4092^2 < 2^29; eq_value
// multiplies them by monomials <= 126^2 in int64 (< 2^43 per sub-block,
// < 2^53 per CU); the right-hand side's * 8 happens in FP64 (exact).
#include <hip/hip_runtime.h>

#include "vame_birefine_kernel.h"

namespace vame {

hipError_t birefine_launch(const BiRefineParams& p, hipStream_t stream) { return birefine_launch_t(p, stream); }

}  // namespace vame

// vame_birefine_p.hip -- the instances of birefine_kernel
// (vame_birefine_kernel.h) that price against predictors: vame_bipred_refine_p
// (include/vame.h).  A unit of its own: instantiated beside
// vame_bipred_refine's instances they changed how those were scheduled.
#include <hip/hip_runtime.h>

#include "vame_birefine_kernel.h"

namespace vame {

hipError_t birefine_p_launch(const BiRefineParamsP& p, hipStream_t stream) { return birefine_launch_t(p, stream); }

}  // namespace vame

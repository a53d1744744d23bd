// vame_search_p.hip -- the instances of search_kernel (vame_search_kernel.h)
// that price against a predictor: vame_affine_search_p and the two searches of
// vame_affine_me_seeded_p (include/vame.h).  A unit of its own:
// instantiated beside vame_affine_search's instances they changed how those
// were scheduled.
#include <hip/hip_runtime.h>

#include "vame_search_kernel.h"

namespace vame {

hipError_t search_p_launch(const SearchParamsP& p, hipStream_t stream) { return search_launch_t(p, stream); }

}  // namespace vame

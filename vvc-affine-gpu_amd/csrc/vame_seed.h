// vame_seed.h -- the integer-pel seed searches (vame_seed_search, DESIGN.md
// §15; vame_seed_pyramid, vame_seed_search_wide, §16; include/vame.h): the
// parameter blocks and launch functions of vame_seed.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace vame {

constexpr int kSeedMaxRadius = 32;
constexpr int kSeedWideMaxRadius = 128;
constexpr int kSeedWideMaxLevels = 2;

// samples of levels 1 and 2 of a W x H frame; level 2 starts at pyr + pyr_level1_samples
__host__ __device__ inline size_t pyr_level1_samples(int W, int H) { return (size_t)(W / 2) * (H / 2); }
__host__ __device__ inline size_t pyr_samples(int W, int H) { return pyr_level1_samples(W, H) + (size_t)(W / 4) * (H / 4); }

struct SeedPyrDownParams {
  const uint16_t* frame;
  uint16_t* pyr;
  int W, H;
};
// The launch of one vame_seed_pyramid call on `stream`.
hipError_t seed_pyr_down_launch(const SeedPyrDownParams& p, hipStream_t stream);

// levels = 0: the exhaustive search on the frames, the pyramids NULL;
// levels = 1, 2: the search from that level of the pyramids down.
// The order of the fields counts: what level 0 reads comes first, cur and refs
// adjacent, so that its kernels load the block as they did before the pyramid
// fields existed (profiles/seed_unify_ab.txt, "the parameter block").
struct SeedParams {
  const uint16_t* cur;
  const uint16_t* refs[4];
  int64_t* cost[4][2];  // [refIdx][align], NULL outside the mask
  int32_t* mv[4][2];    // vame_mv, 2 int32 per row
  int nrefs, W, H, nCtus, ctusPerRow, radius;
  float lambda;
  int levels;
  const uint16_t* curPyr;
  const uint16_t* refPyrs[4];
};
// The launches of one vame_seed_search or vame_seed_search_wide call on `stream`.
hipError_t seed_launch(const SeedParams& p, hipStream_t stream);

}  // namespace vame

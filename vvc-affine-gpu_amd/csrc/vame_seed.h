// vame_seed.h -- integer-pel seed search (vame_seed_search; include/vame.h,
// DESIGN.md §15): the parameter block and launch function of vame_seed.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace vame {

constexpr int kSeedMaxRadius = 32;

struct SeedParams {
  const uint16_t* cur;
  const uint16_t* refs[4];
  int64_t* cost[4][2];  // [refIdx][align], NULL outside the mask
  int32_t* mv[4][2];    // vame_mv, 2 int32 per row
  int nrefs, W, H, nCtus, ctusPerRow, radius;
  float lambda;
};
// The launches of one vame_seed_search call on `stream`.
hipError_t seed_launch(const SeedParams& p, hipStream_t stream);

}  // namespace vame

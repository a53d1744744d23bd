// vame_templates.h -- everything vame_create uploads, built on the host alone
// (vame_templates.cpp; no HIP include, so tests/native/templates_check.cpp
// builds and checks it as a plain C++ program): the search's work-item
// templates, the block order and vame_bipred's candidate table.
#pragma once
#include <vector>

#include "vame_items.h"
#include "vame_tables.h"

namespace vame {

struct CuDesc {
  int x, y, w, h, align, outOff;
};
using Tasks = std::vector<std::vector<CuDesc>>;  // CUs of one size per task

// The item builders: false (and `it` unspecified) when the tasks break what
// the kernels rely on -- see the definitions.
bool make_coop_item(Item& it, int rx, int ry, const Tasks& tasks, int threads);
bool make_auto_item(Item& it, int rx, int ry, const Tasks& tasks, int sbl);

// The work-item templates (identical for every CTU), as uploaded.  The
// quadrant items of four sets [s][FULL | HALF | both alignments] at
// quad[quadOff[s][a] .. + quadN[s][a]): 0 / 1 the items with one / two
// sub-blocks per lane apart (affine_me_quad beside affine_me_quad2: the
// 2+3-CP launches), 2 the PROF packing (every quadrant CU one sub-block per
// lane, affine_me_quad_prof), 3 the items of 0 and 1 together (one
// affine_me_quad launch: the 2-CP-only launches).  The 128-class CUs, each an
// item of its own: the 128x128 CU (big1), every 128x64 / 64x128 CU in the
// tables' order (half: affine_me_half_prof) and by orientation, the nHalfW
// 128x64 items then the nHalfH 64x128 ones (halfWH: affine_me_half2w / _half2h,
// or both in one affine_me_half2 launch).
struct Templates {
  std::vector<Item> quad;
  int quadOff[4][3], quadN[4][3];
  std::vector<Item> big1, half, halfWH;
  int nHalfW, nHalfH;
};
bool build_templates(Templates& t);

std::vector<int32_t> build_order(int nCtus, int cols, int groupCombos, int& nChunks, int& cpp);

// vame_bipred's tables for a supported resolution: the in-frame candidate CUs
// (aligned first; cands[0 .. nCand[0]) aligned, then nCand[1] half-aligned) and
// the map group of 16 sub-blocks -> candidate (nGroup[a] groups per alignment).
struct BiTable {
  std::vector<BiCand> cands;
  std::vector<int32_t> groupCand;
  int nCand[2], nGroup[2];
};
BiTable build_bi_table(int width, int height);

}  // namespace vame

// vame_items.h -- the layout of what the host hands the kernels as tables: the
// search's work items (CuSlot, Item), the kernel kinds with their per-kind
// constants (Cfg) and vame_bipred's candidate rows (BiCand).  Plain C++ with no
// HIP include: vame_templates.cpp builds the tables on the host alone,
// vame_kernel.h and vame_bipred.h read them on the device.
#pragma once
#include <stdint.h>

namespace vame {

constexpr int kMaxCu = 16;    // CU state slots per workgroup (LDS)
constexpr int kMaxTasks = 16;  // autonomous items: wave tasks (wave w runs tasks w, w + 4, ...)
constexpr int kTaskCu = 4;    // CUs per wave task (<= 64 sub-blocks, >= 16 each)
constexpr int kItemCu = kMaxTasks * kTaskCu;  // CU slots per work item
constexpr int kThreads = 256;  // quadrant workgroups

struct CuSlot {          // 8 bytes
  uint8_t x, y;          // CTU-relative position
  uint8_t lw : 4, lh : 4;  // log2 width / height
  uint8_t align : 1;     // 0 FULL, 1 HALF
  uint8_t taskCus : 5;   // a task's first slot: CUs in the task (0 elsewhere)
  uint16_t outOff : 9;   // RETURN_STRIDE[group] + cuIdx
  uint16_t taskLogL : 4;  // a task's first slot: log2 lanes per CU
  uint16_t pad;
};
static_assert(sizeof(CuSlot) == 8, "CuSlot packing");

// An item's CUs come in tasks of one CU size each, run over the item's one
// staged tile: a cooperative item's tasks one after another by the whole
// workgroup, an autonomous item's tasks by its waves (wave w: tasks w, w + 4).
// Task t holds CU slots t * kTaskCu .. (a single-task cooperative item: up to
// kMaxCu slots from 0).
struct Item {
  int16_t nCu;      // CU slots (host view; unused slots have lw 0)
  int16_t rx, ry;   // region origin (CTU-relative)
  int16_t coop;     // bit 0: cooperative (a task's CUs span waves); bit 1: autonomous waves claim tasks;
                    // bit 2: two stacked sub-blocks per lane (affine_me_quad's SBL2 items)
  int16_t nTasks;
  int16_t rw, rh;   // affine_me_half items: the region's extent (the CU's); 0 elsewhere
  int16_t pad;
  CuSlot cu[kItemCu];
};

// Work-item classes (kernels): 0 affine_me_quad -- a 64x64 quadrant, 256
// threads; 1 affine_me_ctu -- a whole 128x128 CTU, 1024 threads; 2
// affine_me_half -- ONE 128x64 or 64x128 CU, 512 threads (two workgroups per
// CU: one's single-wave solve overlaps the other's prediction), its tile
// staged over the CU's extent only (160 x 96 or 96 x 160 of the square
// storage).
// 3 affine_me_ctu2 -- ONE 128x128 CU per 512-thread workgroup, two
// vertically adjacent sub-blocks per lane, two workgroups per CU (one's
// single-wave cost and solve phases overlap the other's prediction).
// 4 / 5 affine_me_half2w / affine_me_half2h -- ONE 128x64 / 64x128 CU per
// 256-thread workgroup, two stacked sub-blocks per lane, its tile staged over
// the CU's extent (160 x 96 / 96 x 160, sized for it), four workgroups per CU.
// 6 affine_me_quad2 -- a 64x64 quadrant's CUs of 32 to 128 sub-blocks, 256
// threads, two stacked sub-blocks per lane, autonomous wave tasks only (a CU
// of 32 / 64 / 128 sub-blocks on 16 / 32 / 64 lanes, four / two / one per
// wave): every per-wave step of an iteration (MV field, cost, equation
// reduction, solve, update) covers twice the sub-blocks it does in
// affine_me_quad, which keeps the 16-sub-block CUs and the 64x64 CUs.
enum { kKindQuad = 0, kKindCtu = 1, kKindHalf = 2, kKindCtu2 = 3, kKindHalf2W = 4, kKindHalf2H = 5, kKindQuad2 = 6 };
template <int KIND>
struct Cfg {
  static constexpr bool HALF2 = KIND == kKindHalf2W || KIND == kKindHalf2H;
  static constexpr bool QUAD = KIND == kKindQuad || KIND == kKindQuad2;  // quadrant work items
  static constexpr int REGION = QUAD ? 64 : 128;  // largest region edge
  static constexpr int THREADS = QUAD || HALF2 ? 256 : KIND == kKindCtu ? 1024 : 512;
  static constexpr int SBL = KIND == kKindCtu2 || HALF2 || KIND == kKindQuad2 ? 2 : 1;  // sub-blocks per lane (stacked vertically)
  static constexpr int MAXCU = (KIND == kKindHalf || KIND == kKindCtu2 || HALF2) ? 1 : kMaxCu;  // CU state slots (LDS)
  static constexpr int ITEMCU = QUAD ? kItemCu : MAXCU;  // CU slots per item
  static constexpr bool AUTO = QUAD;                    // holds autonomous items
  static constexpr bool COOP = KIND != kKindQuad2;      // holds cooperative items
  static constexpr int MARGIN = 16;                     // reference-tile margin (samples)
  static constexpr int TILE = REGION + 2 * MARGIN;      // tile edge (samples; the staged extent's largest)
  static constexpr int TILE_W = KIND == kKindHalf2H ? 64 + 2 * MARGIN : TILE;  // allocated tile extent
  static constexpr int TILE_H = KIND == kKindHalf2W ? 64 + 2 * MARGIN : TILE;
  // tile pitch (samples) == 8 (mod 16): the window rows of sub-blocks 4 rows
  // apart land 16 banks apart (2-way at most for the packed-pair reads)
  static constexpr int TP = (TILE_W + 7) / 16 * 16 + 8;
  static constexpr int TILE_ELEMS = TILE_H * TP + 16;
  static constexpr int NSB = THREADS * SBL;             // sub-blocks per work item (max)
  // SBL = 2: the upper sub-block's prediction parked in LDS across the lower
  // one's (held in registers: +3 % time at c4); affine_me_half2* keep it in
  // registers, so that four workgroups fit a CU's LDS (parked in LDS, three
  // per CU: 8 % slower, HISTORY.md), and so does affine_me_quad2 (parked in
  // LDS it loses a workgroup per CU: 3 % slower at c2, 5 % at c4, HISTORY.md)
  static constexpr bool STASH = KIND != kKindQuad2 && !HALF2;
};

// The hand-over of a two-sub-block wave task (affine_me_quad in 2-CP-only
// launches, vame_kernel.h): once the task's live CUs together hold <= 64
// sub-blocks, the wave's 64 lanes run them one sub-block per lane.  liveCus has
// bit k set for a live CU in slot k of the task (k < kTaskCu), logNsb is log2
// of a CU's sub-blocks (5 or 6; a task holds CUs of one size).  Live CU number
// r (slots ascending) takes the aligned segment of 2^logNsb lanes from
// r << logNsb, its sub-blocks in raster order.
constexpr bool relayout_fits(unsigned liveCus, int logNsb) {
  return liveCus != 0 && (__builtin_popcount(liveCus) << logNsb) <= 64;
}
struct RelayoutLane {
  int cu;  // the lane's CU: its slot in the task, or -1 for a lane without one
  int sb;  // its sub-block in the CU (raster order)
};
constexpr RelayoutLane relayout_lane(int lane, unsigned liveCus, int logNsb) {
  // at most two segments fit a wave: the lane's rank among the live CUs is 0 or 1
  const unsigned m = (lane >> logNsb) ? liveCus & (liveCus - 1) : liveCus;
  return {m ? __builtin_ctz(m) : -1, lane & ((1 << logNsb) - 1)};
}

// A candidate CU of the frame's fixed geometry that lies wholly in the frame
// (vame_templates.cpp builds the table: the aligned candidates first, CTUs
// ascending, rows ascending, then the half-aligned ones).
struct BiCand {
  int32_t xy;     // frame x | y << 16
  int32_t shape;  // log2 w | log2 h << 4 | align << 8
  int32_t row;    // ctu * {201 | 284} + offset: the row in its alignment's arrays
  int32_t first;  // its first group of 16 sub-blocks (over both alignments)
};

}  // namespace vame

// relayout_check.cpp -- stand-alone check of the hand-over's lane mapping
// (relayout_fits / relayout_lane in vame_items.h), the one the quadrant kernel
// of the 2-CP-only launches uses when a two-sub-block wave task's live CUs fit
// the wave one sub-block per lane.  Built with vame_templates.cpp alone (g++
// -std=c++17 -fsanitize=address,undefined; tests/test_relayout_map.py), it
// exits non-zero unless, for every two-sub-block task the product templates
// build and every subset of its CUs that meets the hand-over's condition,
//   * the mapping covers each sub-block of each live CU exactly once;
//   * each live CU keeps an aligned segment of 32 or 64 consecutive lanes, its
//     sub-blocks in raster order, and no lane lands on a settled CU;
//   * the lanes a sub-block reads its neighbours from (left / right by DPP,
//     above / below at -/+ sbCols in the wave's prediction rows) are lanes of
//     the same CU inside the wave's 64 rows;
// and unless the condition refuses every subset that does not fit.
#include <cstdarg>
#include <cstdio>
#include <vector>

#include "../../vvc-affine-gpu_amd/csrc/vame_templates.h"

using namespace vame;

static int g_fails = 0;
static void fail(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  fprintf(stderr, "FAIL: ");
  vfprintf(stderr, fmt, ap);
  fprintf(stderr, "\n");
  va_end(ap);
  g_fails++;
}
#define CHECK(cond, ...) \
  do {                   \
    if (!(cond)) fail(__VA_ARGS__); \
  } while (0)

// usable in constant expressions, on the host as on the device
static_assert(relayout_fits(0x5, 5) && !relayout_fits(0x7, 5) && !relayout_fits(0, 5) && !relayout_fits(0x3, 6), "fits");
static_assert(relayout_lane(40, 0xA, 5).cu == 3 && relayout_lane(40, 0xA, 5).sb == 8 && relayout_lane(40, 0x2, 5).cu == -1,
              "lane map");

static int g_tasks = 0, g_subsets = 0;

// One task (its n CU slots from `cu`) with the live CUs of `mask`.
static void check_subset(const CuSlot* cu, int n, int logNsb, unsigned mask, const char* what) {
  const int nsb = 1 << logNsb;
  int rankOf[kTaskCu], live = 0;
  for (int k = 0; k < kTaskCu; k++) rankOf[k] = (mask >> k) & 1 ? live++ : -1;
  std::vector<int> hits((size_t)kTaskCu * nsb, 0);
  RelayoutLane at[64];
  for (int lane = 0; lane < 64; lane++) {
    const RelayoutLane r = at[lane] = relayout_lane(lane, mask, logNsb);
    if (r.cu < 0) {
      CHECK(lane >= live * nsb, "%s mask %x: lane %d of a live segment has no CU", what, mask, lane);
      continue;
    }
    CHECK(r.cu < n && ((mask >> r.cu) & 1), "%s mask %x: lane %d on slot %d, not a live CU", what, mask, lane, r.cu);
    if (r.cu >= n || !((mask >> r.cu) & 1)) continue;
    CHECK(r.sb >= 0 && r.sb < nsb, "%s mask %x: lane %d sub-block %d", what, mask, lane, r.sb);
    if (r.sb < 0 || r.sb >= nsb) continue;
    hits[(size_t)r.cu * nsb + r.sb]++;
    // the CU's segment: aligned, consecutive, in raster order
    CHECK(lane == rankOf[r.cu] * nsb + r.sb, "%s mask %x: lane %d holds sub-block %d of live CU number %d", what, mask,
          lane, r.sb, rankOf[r.cu]);
  }
  for (int k = 0; k < kTaskCu; k++)
    for (int s = 0; s < nsb; s++)
      CHECK(hits[(size_t)k * nsb + s] == ((mask >> k) & 1 ? 1 : 0), "%s mask %x: sub-block %d of slot %d covered %d times",
            what, mask, s, k, hits[(size_t)k * nsb + s]);
  // neighbour lanes
  for (int lane = 0; lane < 64; lane++) {
    const RelayoutLane r = at[lane];
    if (r.cu < 0 || r.cu >= n) continue;
    const int cols = 1 << (cu[r.cu].lw - 2), rows = 1 << (cu[r.cu].lh - 2);
    CHECK(cols * rows == nsb, "%s: slot %d is %d x %d sub-blocks in a task of %d", what, r.cu, cols, rows, nsb);
    const int c = r.sb % cols, row = r.sb / cols;
    const auto same = [&](int l, int sb) { return l >= 0 && l < 64 && at[l].cu == r.cu && at[l].sb == sb; };
    if (c > 0) CHECK(same(lane - 1, r.sb - 1), "%s mask %x: lane %d, left neighbour", what, mask, lane);
    if (c + 1 < cols) CHECK(same(lane + 1, r.sb + 1), "%s mask %x: lane %d, right neighbour", what, mask, lane);
    if (row > 0) CHECK(same(lane - cols, r.sb - cols), "%s mask %x: lane %d, row above", what, mask, lane);
    if (row + 1 < rows) CHECK(same(lane + cols, r.sb + cols), "%s mask %x: lane %d, row below", what, mask, lane);
  }
}

static void check_item(const Item& it, const char* what) {
  for (int t = 0; t < it.nTasks; t++) {
    const CuSlot* cu = it.cu + t * kTaskCu;
    const int n = cu[0].taskCus, logNsb = cu[0].taskLogL + 1;  // two sub-blocks per lane
    CHECK(n >= 1 && n <= kTaskCu && logNsb >= 5 && logNsb <= 7, "%s task %d: %d CUs of 2^%d sub-blocks", what, t, n, logNsb);
    if (n < 1 || n > kTaskCu) continue;
    g_tasks++;
    for (unsigned mask = 0; mask < (1u << n); mask++) {
      const int live = __builtin_popcount(mask);
      const bool fits = live > 0 && live * (1 << logNsb) <= 64;
      CHECK(relayout_fits(mask, logNsb) == fits, "%s task %d mask %x: relayout_fits", what, t, mask);
      if (!fits) continue;
      g_subsets++;
      check_subset(cu, n, logNsb, mask, what);
    }
  }
}

int main() {
  Templates t;
  if (!build_templates(t)) {
    fail("build_templates failed");
    return 1;
  }
  int items = 0;
  for (int set : {1, 3})  // the two-sub-block items alone, and the 2-CP-only launches' merged set
    for (int a = 0; a < 3; a++)
      for (int i = 0; i < t.quadN[set][a]; i++) {
        const Item& it = t.quad[(size_t)t.quadOff[set][a] + i];
        if (!(it.coop & 4)) continue;
        char what[64];
        snprintf(what, sizeof(what), "set %d alignment %d item %d", set, a, i);
        check_item(it, what);
        items++;
      }
  CHECK(items > 0 && g_subsets > 0, "no two-sub-block task checked (%d items, %d subsets)", items, g_subsets);
  if (g_fails) {
    fprintf(stderr, "relayout_check: %d check(s) failed\n", g_fails);
    return 1;
  }
  printf("relayout_check ok: %d items, %d tasks, %d live subsets\n", items, g_tasks, g_subsets);
  return 0;
}

// vame_templates.cpp -- builds, on the host alone, everything vame_create
// uploads: the work-item templates of the search kernels (which lane works on
// which CU), the block order and vame_bipred's candidate table; and the
// geometry queries of include/vame.h that need no context.  Plain C++ over
// the constant tables of vame_tables.h: no HIP, so a stand-alone program can
// check it (tests/native/templates_check.cpp).
#include "vame_templates.h"

#include <algorithm>
#include <cstring>

#include "../../include/vame.h"

// the one instrumentation switch the host side reads (vame_instr.h, which
// needs HIP): bit 8, timing-only builds without the 128x64 / 64x128 items
#ifndef VAME_ABLATE
#define VAME_ABLATE 0
#endif

namespace vame {

static_assert(kFullCusPerCtu <= 512 && kHalfCusPerCtu <= 512, "CuSlot::outOff");

namespace {

// The quadrant packing (measured alternatives in HISTORY.md): autonomous items
// of kMaxTasks wave tasks over one staged tile, waves claiming the next task
// from an LDS counter as they finish; one cooperative item per quadrant
// chaining its cooperative groups; a launch of both alignments on items
// mixing them, every quadrant's first (largest-task) autonomous item first.

int ilog2(int v) {
  int l = 0;
  while ((1 << (l + 1)) <= v) l++;
  return l;
}

int nsb_of(const CuDesc& c) { return c.w * c.h / 16; }

void set_slot(CuSlot& s, const CuDesc& c) {
  s.x = (uint8_t)c.x;
  s.y = (uint8_t)c.y;
  s.lw = (uint8_t)ilog2(c.w);
  s.lh = (uint8_t)ilog2(c.h);
  s.align = (uint8_t)c.align;
  s.outOff = (uint16_t)c.outOff;
}

// What both kinds of item share: 1 .. kMaxTasks tasks, none empty, one CU
// size per task.
bool tasks_ok(const Tasks& tasks) {
  if (tasks.empty() || (int)tasks.size() > kMaxTasks) return false;
  for (auto& t : tasks) {
    if (t.empty()) return false;
    for (auto& c : t)
      if (nsb_of(c) != nsb_of(t[0])) return false;
  }
  return true;
}

// Every HALF CU lies inside one 64x64 quadrant: the quadrant items stage the
// quadrant's tile alone.
constexpr bool half_cus_inside_quadrants() {
  for (int g = 0; g < kHalfGroups; g++)
    for (int k = 0; k < kHalfN[g]; k++) {
      const int x = kHalfX8[g][k] * 8, y = kHalfY8[g][k] * 8;
      if (x % 64 + kHalfW[g] > 64 || y % 64 + kHalfH[g] > 64) return false;
    }
  return true;
}
static_assert(half_cus_inside_quadrants(), "a HALF CU crosses a quadrant border");

}  // namespace

// Cooperative item: tasks of CUs of one size, each CU spanning nsb >= 64
// lanes (one per sub-block) of the workgroup (workgroup barriers per phase,
// LDS atomics), run one after another over the item's one staged tile.  A
// single task holds slots 0 .. (up to kMaxCu), a chain's task t slots
// t * kTaskCu ...
bool make_coop_item(Item& it, int rx, int ry, const Tasks& tasks, int threads) {
  memset(&it, 0, sizeof(it));
  it.rx = (int16_t)rx;
  it.ry = (int16_t)ry;
  it.coop = 1;
  if (!tasks_ok(tasks)) return false;
  it.nTasks = (int16_t)tasks.size();
  const int stride = tasks.size() > 1 ? kTaskCu : kMaxCu;
  for (size_t t = 0; t < tasks.size(); t++) {
    const int nsb = nsb_of(tasks[t][0]);
    const int n = (int)tasks[t].size();
    if (nsb < 64 || n * nsb > threads || n > stride) return false;
    for (int i = 0; i < n; i++) set_slot(it.cu[t * stride + i], tasks[t][i]);
    it.cu[t * stride].taskCus = (uint8_t)n;
    it.cu[t * stride].taskLogL = (uint16_t)ilog2(nsb);
    it.nCu = (int16_t)(t * stride + n);
  }
  return true;
}

// Autonomous item: up to kMaxTasks wave tasks, each CUs of ONE size (one lane
// per sub-block, or per two stacked sub-blocks with sbl = 2: 16, 32 or 64
// lanes per CU), so a task's segment size is uniform.  Wave w runs task w,
// then claims the next unclaimed one as it finishes, over the one staged
// tile: task t holds CU slots t * kTaskCu .. (its first slot carries the
// task's CU count and lanes per CU) and the running wave's prediction rows.
// Unused slots stay zero (lw 0).
bool make_auto_item(Item& it, int rx, int ry, const Tasks& tasks, int sbl) {
  memset(&it, 0, sizeof(it));
  it.rx = (int16_t)rx;
  it.ry = (int16_t)ry;
  it.coop = sbl == 2 ? 2 | 4 : 2;  // bit 1: waves claim tasks; bit 2: two sub-blocks per lane
  if (!tasks_ok(tasks)) return false;
  it.nTasks = (int16_t)tasks.size();
  it.nCu = (int16_t)(tasks.size() * kTaskCu);
  for (size_t t = 0; t < tasks.size(); t++) {
    const int lanes = nsb_of(tasks[t][0]) / sbl;
    const int n = (int)tasks[t].size();
    if (n * lanes > 64 || lanes < 16 || n > kTaskCu) return false;  // the kernel's segment sums handle 16 / 32 / 64
    for (int i = 0; i < n; i++) set_slot(it.cu[t * kTaskCu + i], tasks[t][i]);
    it.cu[t * kTaskCu].taskCus = (uint8_t)n;
    it.cu[t * kTaskCu].taskLogL = (uint16_t)ilog2(lanes);
  }
  return true;
}

namespace {

// CUs of one quadrant: wave tasks of one size class (largest first, at most
// kTaskCu CUs and 64 lanes each), then items of kMaxTasks consecutive tasks,
// appended to `out`.
bool pack_autonomous(int qx, int qy, std::vector<CuDesc> cus, std::vector<Item>& out, int sbl) {
  std::stable_sort(cus.begin(), cus.end(),
                   [](const CuDesc& a, const CuDesc& b) { return nsb_of(a) > nsb_of(b); });
  Tasks waves;
  for (auto& c : cus) {
    if (waves.empty() || nsb_of(waves.back()[0]) != nsb_of(c) || (int)waves.back().size() == kTaskCu ||
        (int)(waves.back().size() + 1) * nsb_of(c) / sbl > 64)
      waves.push_back({});
    waves.back().push_back(c);
  }
  for (size_t w = 0; w < waves.size(); w += kMaxTasks) {
    const Tasks grp(waves.begin() + w, waves.begin() + std::min(waves.size(), w + kMaxTasks));
    Item it;
    if (!make_auto_item(it, qx, qy, grp, sbl)) return false;
    out.push_back(it);
  }
  return true;
}

// The CUs of group g of an alignment that pass `keep`.
template <typename Keep>
std::vector<CuDesc> group_descs(int align, int g, Keep keep) {
  std::vector<CuDesc> c;
  for (int k = 0; k < group_cus(align, g); k++) {
    const CuGeom cu = cu_geom(align, g, k);
    if (keep(cu)) c.push_back({cu.x, cu.y, cu.w, cu.h, align, group_stride(align, g) + k});
  }
  return c;
}

// The 128-class items: the FULL 128x128 CU, whole CTU, cooperative (big); each
// 128x64 / 64x128 CU alone, the region = the CU (half).
bool build_big(std::vector<Item>& big, std::vector<Item>& half) {
  for (int g = 0; g < kFullGroups; g++) {
    const int w = kFullW[g], h = kFullH[g];
    if (w != 128 && h != 128) continue;
    const std::vector<CuDesc> c = group_descs(0, g, [](const CuGeom&) { return true; });
    Item it;
    if (w == h) {
      if (!make_coop_item(it, 0, 0, {c}, Cfg<kKindCtu>::THREADS)) return false;
      big.push_back(it);
      continue;
    }
    if (VAME_ABLATE & 256) continue;  // timing-only builds: no 128x64 / 64x128 items
    for (auto& cu : c) {
      if (!make_coop_item(it, cu.x, cu.y, {{cu}}, Cfg<kKindHalf>::THREADS)) return false;
      it.rw = (int16_t)w;
      it.rh = (int16_t)h;
      half.push_back(it);
    }
  }
  return true;
}

// The quadrant items of one kernel, by alignment set: for launches of FULL
// CUs only, HALF CUs only, and both alignments.
typedef std::vector<Item> QuadSet[3];

// The quadrant items (identical for every CTU), per 64x64 quadrant:
//   q1       : affine_me_quad (one sub-block per lane): the cooperative CUs
//              (FULL 64x64; without q2 also FULL 64x32 / 32x64 and HALF 64x32 +
//              32x64) chained in one item, then autonomous items of kMaxTasks
//              wave tasks over the CUs of 16 sub-blocks (without q2: of <= 64)
//   q2       : (nullptr: not used, the PROF packing) affine_me_quad2 (two
//              stacked sub-blocks per lane): autonomous items over the CUs of
//              32 to 128 sub-blocks
// In the items of a launch of both alignments the alignments mix: every
// quadrant's cooperative chain first, then every quadrant's first
// (largest-task) autonomous item, then the seconds, ...: the kernel's last
// workgroups are its shortest.
bool build_quads(QuadSet& q1, QuadSet* q2) {
  // the largest CU an autonomous task of each kernel holds (sub-blocks)
  const int max1 = q2 ? 16 : 64, min2 = 32, max2 = 128;
  struct Both {
    std::vector<Item> coop, autos;
    std::vector<int> rank;  // an autonomous item's index within its quadrant
  } both1, both2;
  for (int q = 0; q < 4; q++) {
    const int qx = (q & 1) * 64, qy = (q >> 1) * 64;
    auto inq = [&](const CuGeom& c) { return c.x >= qx && c.x < qx + 64 && c.y >= qy && c.y < qy + 64; };
    std::vector<CuDesc> a1[2], a2[2];  // autonomous CUs per alignment, per kernel
    Tasks coop[2];                     // cooperative tasks (q1), per alignment
    auto place = [&](const std::vector<CuDesc>& c, int align) {
      if (c.empty()) return;
      const int nsb = nsb_of(c[0]);
      if (nsb <= max1)
        a1[align].insert(a1[align].end(), c.begin(), c.end());
      else if (q2 && nsb >= min2 && nsb <= max2)
        a2[align].insert(a2[align].end(), c.begin(), c.end());
      else
        coop[align].push_back(c);  // a task per group
    };
    for (int g = 0; g < kFullGroups; g++)
      if (kFullW[g] != 128 && kFullH[g] != 128) place(group_descs(0, g, inq), 0);
    std::vector<CuDesc> halfBig;  // the HALF 64x32 + 32x64 CUs: one cooperative task
    for (int g = 0; g < kHalfGroups; g++) {
      const std::vector<CuDesc> c = group_descs(1, g, inq);
      if (!c.empty() && nsb_of(c[0]) > max1 && !(q2 && nsb_of(c[0]) <= max2))
        halfBig.insert(halfBig.end(), c.begin(), c.end());
      else
        place(c, 1);
    }
    if (!halfBig.empty()) coop[1].push_back(halfBig);
    Item it;
    // one-alignment sets: the cooperative chain, then the autonomous items
    for (int al = 0; al < 2; al++) {
      if (!coop[al].empty()) {
        if (!make_coop_item(it, qx, qy, coop[al], Cfg<kKindQuad>::THREADS)) return false;
        q1[al].push_back(it);
      }
      if (!pack_autonomous(qx, qy, a1[al], q1[al], 1)) return false;
      if (q2 && !pack_autonomous(qx, qy, a2[al], (*q2)[al], 2)) return false;
    }
    // both alignments
    Tasks t(coop[0]);
    t.insert(t.end(), coop[1].begin(), coop[1].end());
    if (!t.empty()) {
      if (!make_coop_item(it, qx, qy, t, Cfg<kKindQuad>::THREADS)) return false;
      both1.coop.push_back(it);
    }
    for (int k = 0; k < (q2 ? 2 : 1); k++) {
      Both& b = k ? both2 : both1;
      std::vector<CuDesc> cus(k ? a2[0] : a1[0]);
      const std::vector<CuDesc>& h = k ? a2[1] : a1[1];
      cus.insert(cus.end(), h.begin(), h.end());
      const size_t before = b.autos.size();
      if (!pack_autonomous(qx, qy, cus, b.autos, k ? 2 : 1)) return false;
      for (size_t i = before; i < b.autos.size(); i++) b.rank.push_back((int)(i - before));
    }
  }
  for (int k = 0; k < (q2 ? 2 : 1); k++) {
    Both& b = k ? both2 : both1;
    std::vector<Item>& out = k ? (*q2)[2] : q1[2];
    out = b.coop;
    std::vector<size_t> idx(b.autos.size());
    for (size_t i = 0; i < idx.size(); i++) idx[i] = i;
    std::stable_sort(idx.begin(), idx.end(), [&](size_t x, size_t y) { return b.rank[x] < b.rank[y]; });
    for (size_t i : idx) out.push_back(b.autos[i]);
  }
  return true;
}

}  // namespace

bool build_templates(Templates& t) {
  t = Templates();
  QuadSet qs[4];  // SBL1 items, SBL2 items; the PROF packing; the product's merged set
  if (!build_big(t.big1, t.half) || !build_quads(qs[0], &qs[1]) || !build_quads(qs[2], nullptr)) return false;
  // one affine_me_quad launch over both: the cooperative (64x64) items first,
  // then the SBL2 items, then the 16-sub-block items (the shortest last)
  for (int a = 0; a < 3; a++) {
    std::vector<Item>& m = qs[3][a];
    for (const Item& it : qs[0][a])
      if (it.coop & 1) m.push_back(it);
    m.insert(m.end(), qs[1][a].begin(), qs[1][a].end());
    for (const Item& it : qs[0][a])
      if (!(it.coop & 1)) m.push_back(it);
  }
  for (int k = 0; k < 4; k++)
    for (int a = 0; a < 3; a++) {
      t.quadOff[k][a] = (int)t.quad.size();
      t.quadN[k][a] = (int)qs[k][a].size();
      t.quad.insert(t.quad.end(), qs[k][a].begin(), qs[k][a].end());
    }
  // the single-CU half items by orientation: the 128x64 items, then the 64x128
  // ones, adjacent (affine_me_half2 runs both)
  for (int wide = 1; wide >= 0; wide--)
    for (const Item& it : t.half)
      if ((it.cu[0].lw > it.cu[0].lh) == (wide != 0)) t.halfWH.push_back(it);
  t.nHalfW = (int)std::count_if(t.half.begin(), t.half.end(), [](const Item& it) { return it.cu[0].lw > it.cu[0].lh; });
  t.nHalfH = (int)t.half.size() - t.nHalfW;
  // the kernels index their seed-reuse sums by these counts (best_layout in
  // vame_engine.hip): one 128x128 item and two of each orientation
  return t.big1.size() == 1 && ((VAME_ABLATE & 256) || (t.nHalfW == 2 && t.nHalfH == 2));
}

// The slot -> CTU table of the block order: the frame's CTU rows cut into
// chunks of at most groupCombos CTUs; within a chunk the CTUs in raster order,
// padded to a multiple of 8 slots, so slot j runs on XCD j % 8 (workgroups
// are dealt round-robin over the XCDs) and raster neighbours sit on different
// XCDs: the per-XCD load follows the frame's content evenly.  (Runs of
// adjacent CTUs per XCD and compact per-XCD strips measured slower or equal:
// HISTORY.md.)
std::vector<int32_t> build_order(int nCtus, int cols, int groupCombos, int& nChunks, int& cpp) {
  const int rows = nCtus / cols;
  nChunks = (nCtus + groupCombos - 1) / groupCombos;
  const int rowsPer = (rows + nChunks - 1) / nChunks;
  nChunks = (rows + rowsPer - 1) / rowsPer;
  cpp = (rowsPer * cols + 7) / 8 * 8;
  std::vector<int32_t> order((size_t)nChunks * cpp, -1);
  for (int ch = 0; ch < nChunks; ch++) {
    const int r0 = ch * rowsPer, r1 = std::min(rows, r0 + rowsPer);
    int32_t* o = order.data() + (size_t)ch * cpp;
    for (int k = 0; k < (r1 - r0) * cols; k++) o[k] = r0 * cols + k;
  }
  return order;
}

BiTable build_bi_table(int width, int height) {
  BiTable t;
  const int nCtus = num_ctus(width, height), ctusPerRow = (width + kCtu - 1) / kCtu;
  for (int align = 0; align < 2; align++) {
    const int per = align ? kHalfCusPerCtu : kFullCusPerCtu;
    const size_t cand0 = t.cands.size(), group0 = t.groupCand.size();
    for (int ctu = 0; ctu < nCtus; ctu++) {
      const int X0 = (ctu % ctusPerRow) * kCtu, Y0 = (ctu / ctusPerRow) * kCtu;
      for (int g = 0; g < (align ? kHalfGroups : kFullGroups); g++)
        for (int k = 0; k < group_cus(align, g); k++) {
          const CuGeom cu = cu_geom(align, g, k);
          const int x = X0 + cu.x, y = Y0 + cu.y;
          if (x + cu.w > width || y + cu.h > height) continue;
          BiCand cd;
          cd.xy = x | (y << 16);
          cd.shape = ilog2(cu.w) | (ilog2(cu.h) << 4) | (align << 8);
          cd.row = ctu * per + group_stride(align, g) + k;
          cd.first = (int32_t)t.groupCand.size();
          t.groupCand.insert(t.groupCand.end(), (size_t)(cu.w * cu.h) >> 8, (int32_t)t.cands.size());
          t.cands.push_back(cd);
        }
    }
    t.nCand[align] = (int)(t.cands.size() - cand0);
    t.nGroup[align] = (int)(t.groupCand.size() - group0);
  }
  return t;
}

}  // namespace vame

using namespace vame;

extern "C" {

int vame_num_ctus(int width, int height) { return num_ctus(width, height); }
int vame_cus_per_ctu(int align) {
  return align == 0 ? kFullCusPerCtu : align == 1 ? kHalfCusPerCtu : 0;
}
int vame_num_groups(int align) { return align == 0 ? kFullGroups : align == 1 ? kHalfGroups : 0; }

int vame_group_geometry(int align, int g, int* w, int* h, int* ncu, int* stride, int* xs, int* ys) {
  if (!w || !h || !ncu || !stride || !xs || !ys) return VAME_E_INVALID;
  if ((align != 0 && align != 1) || g < 0 || g >= vame_num_groups(align)) return VAME_E_INVALID;
  *w = cu_geom(align, g, 0).w;
  *h = cu_geom(align, g, 0).h;
  *ncu = group_cus(align, g);
  *stride = group_stride(align, g);
  for (int k = 0; k < *ncu; k++) {
    xs[k] = cu_geom(align, g, k).x;
    ys[k] = cu_geom(align, g, k).y;
  }
  return VAME_OK;
}

// Over the arrays vame_create uploads, combined as the launcher combines them
// (launch_plan in vame_engine.hip): a 2-CP-only launch runs quadrant set 3, a
// launch with 3-CP sets 0 and 1, both with the 128x128 item and the half
// items by orientation; PROF runs set 2 with the half items in table order.
// The 128-class items launch with the FULL alignment.  Each of the three, over
// the items of `align` alone and over those of both alignments, must cover the
// CUs of `align` alike, and a one-alignment set holds no CU of the other.
int vame_template_coverage(int half128, int align, int32_t* hits, int32_t* items3) {
  if (!hits || (align != 0 && align != 1) || half128 == 0) return VAME_E_INVALID;
  Templates t;
  if (!build_templates(t)) return VAME_E_INVALID;
  const int n = align ? kHalfCusPerCtu : kFullCusPerCtu;
  std::vector<int32_t> cover;
  for (int launch = 0; launch < 3; launch++)
    for (int a : {align, 2}) {
      std::vector<int32_t> h((size_t)n, 0);
      const auto count = [&](const Item* items, size_t nItems) {
        for (size_t i = 0; i < nItems; i++)
          for (int k = 0; k < items[i].nCu; k++) {
            const CuSlot& s = items[i].cu[k];
            if (s.lw == 0) continue;  // an unused slot
            if ((a < 2 && s.align != a) || s.outOff >= (s.align ? kHalfCusPerCtu : kFullCusPerCtu)) return false;
            if (s.align == align) h[s.outOff]++;
          }
        return true;
      };
      bool ok = true;
      for (int s : {launch == 0 ? 3 : launch == 1 ? 0 : 2, launch == 1 ? 1 : -1})
        if (s >= 0) ok = ok && count(t.quad.data() + t.quadOff[s][a], (size_t)t.quadN[s][a]);
      if (a != 1) {
        const std::vector<Item>& halves = launch == 2 ? t.half : t.halfWH;
        ok = ok && count(t.big1.data(), t.big1.size()) && count(halves.data(), halves.size());
      }
      if (!ok || (!cover.empty() && h != cover)) return VAME_E_INVALID;
      cover = h;
    }
  std::copy(cover.begin(), cover.end(), hits);
  if (items3) {
    items3[0] = t.quadN[0][2] + t.quadN[1][2];  // affine_me_quad + affine_me_quad2 items of a both-alignment launch
    items3[1] = (int32_t)t.big1.size();
    items3[2] = (int32_t)t.half.size();
  }
  return VAME_OK;
}

int vame_pred_mask(int mode_mask) {
  const int ncp = (mode_mask & VAME_MODE_3CP) ? 3 : 1;  // 2CP [+ 3CP] per alignment
  const int sel = (mode_mask >> 2) & 3;                  // neither selection bit: both
  return ((sel == 0 || (sel & 1)) ? ncp : 0) | ((sel == 0 || (sel & 2)) ? ncp << 2 : 0);
}

}  // extern "C"

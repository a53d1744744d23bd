// templates_check.cpp -- stand-alone check of vame_templates.cpp, the host-only
// unit that builds everything vame_create uploads.  Built with that unit alone
// (g++ -std=c++17 -fsanitize=address,undefined; tests/test_host.py), it exits
// non-zero unless
//   * the uploaded work items, combined as the launcher combines them
//     (launch_plan in vame_engine.hip), cover every CU of every selected
//     alignment exactly once, in all three launch forms;
//   * every item keeps what the kernel that runs it relies on;
//   * the item builders refuse every input that breaks one of those rules;
//   * the block order and vame_bipred's candidate table are what their
//     consumers index, for the five supported resolutions.
#include <algorithm>
#include <array>
#include <cstdarg>
#include <cstdio>
#include <set>
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

// What an item has to respect in the kernel that runs it (Cfg<KIND>).
struct Kind {
  const char* name;
  int itemCu, nsb;  // CU slots per item; sub-blocks a workgroup holds (THREADS x SBL)
  bool quad, autoOk, coopOk, sbl2Only;
};
template <int K>
Kind kind_of(const char* name) {
  return {name, Cfg<K>::ITEMCU, Cfg<K>::NSB, Cfg<K>::QUAD, Cfg<K>::AUTO, Cfg<K>::COOP, K == kKindQuad2};
}

struct Span {
  const Item* items;
  int n;
  Kind kind;
};

// Every former abort() condition, on one built item.
static void check_item(const Item& it, const Kind& k, const char* what, int idx) {
  const bool coop = (it.coop & 1) != 0, autonomous = (it.coop & 2) != 0;
  CHECK(coop != autonomous, "%s[%d] %s: coop bits %d", what, idx, k.name, it.coop);
  CHECK(coop ? k.coopOk : k.autoOk, "%s[%d]: kernel %s does not run this kind of item", what, idx, k.name);
  CHECK(it.nTasks >= 1 && it.nTasks <= kMaxTasks, "%s[%d]: nTasks %d", what, idx, it.nTasks);
  if (it.nTasks < 1 || it.nTasks > kMaxTasks) return;
  const int sbl = (it.coop & 4) ? 2 : 1;
  CHECK(!(it.coop & 4) || autonomous, "%s[%d]: two sub-blocks per lane in a cooperative item", what, idx);
  CHECK(!k.sbl2Only || sbl == 2, "%s[%d]: a one-sub-block item in %s", what, idx, k.name);
  const int stride = coop && it.nTasks == 1 ? kMaxCu : kTaskCu;
  std::vector<bool> used(kItemCu, false);
  for (int t = 0; t < it.nTasks; t++) {
    const CuSlot& first = it.cu[t * stride];
    const int n = first.taskCus;
    CHECK(n >= 1 && n <= stride, "%s[%d] task %d: %d CUs", what, idx, t, n);
    const int nsb = 1 << (first.lw + first.lh - 4), lanes = nsb / sbl;
    CHECK((1 << first.taskLogL) == lanes, "%s[%d] task %d: taskLogL %d for %d lanes", what, idx, t, first.taskLogL, lanes);
    if (coop) {
      CHECK(nsb >= 64, "%s[%d] task %d: cooperative CU of %d sub-blocks", what, idx, t, nsb);
      CHECK(n * nsb <= k.nsb, "%s[%d] task %d: %d x %d sub-blocks in %s", what, idx, t, n, nsb, k.name);
    } else {
      CHECK(lanes == 16 || lanes == 32 || lanes == 64, "%s[%d] task %d: %d lanes per CU", what, idx, t, lanes);
      CHECK(n * lanes <= 64 && n <= kTaskCu, "%s[%d] task %d: %d CUs x %d lanes", what, idx, t, n, lanes);
    }
    for (int i = 0; i < n && i < stride; i++) {
      const int slot = t * stride + i;
      const CuSlot& s = it.cu[slot];
      CHECK(slot < k.itemCu, "%s[%d]: slot %d beyond the %d of %s", what, idx, slot, k.itemCu, k.name);
      CHECK(s.lw + s.lh == first.lw + first.lh, "%s[%d] task %d: mixed CU sizes", what, idx, t);
      CHECK(i == 0 || (s.taskCus == 0 && s.taskLogL == 0), "%s[%d] slot %d: task fields outside a first slot", what, idx, slot);
      used[slot] = true;
      if (k.quad) {  // the item stages its quadrant's tile alone
        const int w = 1 << s.lw, h = 1 << s.lh;
        CHECK(it.rx % 64 == 0 && it.ry % 64 == 0 && s.x >= it.rx && s.x + w <= it.rx + 64 && s.y >= it.ry &&
                  s.y + h <= it.ry + 64,
              "%s[%d] slot %d: CU %dx%d at (%d, %d) outside quadrant (%d, %d)", what, idx, slot, w, h, s.x, s.y, it.rx, it.ry);
      }
    }
  }
  int last = -1;
  for (int s = 0; s < kItemCu; s++) {
    CHECK(used[s] == (it.cu[s].lw != 0), "%s[%d] slot %d: used %d, lw %d", what, idx, s, (int)used[s], it.cu[s].lw);
    if (used[s]) last = s;
  }
  CHECK(it.nCu > last && it.nCu <= kItemCu, "%s[%d]: nCu %d, last used slot %d", what, idx, it.nCu, last);
}

static void check_templates() {
  Templates t;
  if (!build_templates(t)) {
    fail("build_templates failed");
    return;
  }
  CHECK(t.big1.size() == 1 && t.nHalfW == 2 && t.nHalfH == 2 && t.half.size() == 4 && t.halfWH.size() == 4,
        "128-class items: big1 %zu halfW %d halfH %d half %zu", t.big1.size(), t.nHalfW, t.nHalfH, t.half.size());
  CHECK(t.quadN[0][2] + t.quadN[1][2] == 16 && t.quadN[3][2] == 16, "both-alignment quadrant items: %d + %d, merged %d",
        t.quadN[0][2], t.quadN[1][2], t.quadN[3][2]);
  for (int i = 0; i < t.nHalfW; i++) CHECK(t.halfWH[i].rw == 128 && t.halfWH[i].rh == 64, "halfW[%d] is not 128x64", i);
  for (int i = 0; i < t.nHalfH; i++)
    CHECK(t.halfWH[t.nHalfW + i].rw == 64 && t.halfWH[t.nHalfW + i].rh == 128, "halfH[%d] is not 64x128", i);
  const char* launchName[3] = {"2-CP-only", "2+3-CP", "PROF"};
  const int perAlign[2] = {kFullCusPerCtu, kHalfCusPerCtu};
  for (int launch = 0; launch < 3; launch++)
    for (int a = 0; a < 3; a++) {  // alignment selection: FULL, HALF, both
      const auto quad = [&](int set, const Kind& k) { return Span{t.quad.data() + t.quadOff[set][a], t.quadN[set][a], k}; };
      std::vector<Span> spans;
      if (launch == 0) {
        spans.push_back(quad(3, kind_of<kKindQuad>("affine_me_quad")));
      } else if (launch == 1) {
        spans.push_back(quad(1, kind_of<kKindQuad2>("affine_me_quad2")));
        spans.push_back(quad(0, kind_of<kKindQuad>("affine_me_quad")));
      } else {
        spans.push_back(quad(2, kind_of<kKindQuad>("affine_me_quad_prof")));
      }
      if (a != 1) {  // the 128-class items launch with the FULL alignment
        const Item* hw = t.halfWH.data();
        if (launch == 0) {
          spans.push_back({t.big1.data(), (int)t.big1.size(), kind_of<kKindCtu2>("affine_me_ctu2")});
          spans.push_back({hw, t.nHalfW + t.nHalfH, kind_of<kKindHalf2W>("affine_me_half2")});
        } else if (launch == 1) {
          spans.push_back({t.big1.data(), (int)t.big1.size(), kind_of<kKindCtu2>("affine_me_ctu2")});
          spans.push_back({hw, t.nHalfW, kind_of<kKindHalf2W>("affine_me_half2w")});
          spans.push_back({hw + t.nHalfW, t.nHalfH, kind_of<kKindHalf2H>("affine_me_half2h")});
        } else {
          spans.push_back({t.big1.data(), (int)t.big1.size(), kind_of<kKindCtu>("affine_me_ctu_prof")});
          spans.push_back({t.half.data(), (int)t.half.size(), kind_of<kKindHalf>("affine_me_half_prof")});
        }
      }
      char what[64];
      snprintf(what, sizeof(what), "%s launch, alignment set %d", launchName[launch], a);
      std::vector<int> hits[2] = {std::vector<int>(kFullCusPerCtu, 0), std::vector<int>(kHalfCusPerCtu, 0)};
      for (const Span& sp : spans)
        for (int i = 0; i < sp.n; i++) {
          const Item& it = sp.items[i];
          check_item(it, sp.kind, what, i);
          for (int s = 0; s < kItemCu; s++) {
            const CuSlot& cu = it.cu[s];
            if (cu.lw == 0) continue;
            CHECK(a == 2 || cu.align == a, "%s: item %d of %s holds a CU of alignment %d", what, i, sp.kind.name, cu.align);
            if (cu.outOff < perAlign[cu.align])
              hits[cu.align][cu.outOff]++;
            else
              fail("%s: output offset %d", what, cu.outOff);
          }
        }
      for (int al = 0; al < 2; al++) {
        const int want = a == 2 || a == al ? 1 : 0;
        for (int o = 0; o < perAlign[al]; o++)
          CHECK(hits[al][o] == want, "%s: alignment %d offset %d hit %d times, want %d", what, al, o, hits[al][o], want);
      }
    }
}

// The item builders called with one violating input per rule: each refuses it
// (and accepts its nearest valid neighbour).
static void check_error_paths() {
  const auto cu = [](int w, int h, int k = 0) { return CuDesc{0, 0, w, h, 0, k}; };
  const auto n_of = [&](int n, int w, int h) { return std::vector<CuDesc>((size_t)n, cu(w, h)); };
  Item it;
  // cooperative items
  CHECK(make_coop_item(it, 0, 0, {n_of(1, 64, 64)}, 256), "coop: one 64x64 CU refused");
  CHECK(make_coop_item(it, 0, 0, Tasks(16, n_of(1, 64, 16)), 256), "coop: 16 tasks refused");
  CHECK(!make_coop_item(it, 0, 0, {}, 256), "coop: no task accepted");
  CHECK(!make_coop_item(it, 0, 0, Tasks(17, n_of(1, 64, 16)), 256), "coop: 17 tasks accepted");
  CHECK(!make_coop_item(it, 0, 0, {{}}, 256), "coop: an empty task accepted");
  CHECK(!make_coop_item(it, 0, 0, {{cu(64, 32), cu(64, 16)}}, 256), "coop: mixed sizes in a task accepted");
  CHECK(!make_coop_item(it, 0, 0, {n_of(1, 32, 16)}, 256), "coop: a CU of 32 sub-blocks accepted");
  CHECK(!make_coop_item(it, 0, 0, {n_of(3, 64, 32)}, 256), "coop: 3 x 128 sub-blocks on 256 threads accepted");
  CHECK(make_coop_item(it, 0, 0, {n_of(16, 64, 16)}, 1024), "coop: 16 CUs in a single task refused");
  CHECK(!make_coop_item(it, 0, 0, {n_of(17, 64, 16)}, 2048), "coop: 17 CUs in a single task accepted");
  CHECK(!make_coop_item(it, 0, 0, {n_of(5, 64, 16), n_of(1, 64, 16)}, 1024), "coop: 5 CUs in a chained task accepted");
  // autonomous items
  CHECK(make_auto_item(it, 0, 0, Tasks(16, n_of(4, 16, 16)), 1), "auto: 16 tasks of 4 x 16 sub-blocks refused");
  CHECK(make_auto_item(it, 0, 0, {n_of(1, 64, 32)}, 2), "auto: 128 sub-blocks on 64 lanes refused");
  CHECK(!make_auto_item(it, 0, 0, {}, 1), "auto: no task accepted");
  CHECK(!make_auto_item(it, 0, 0, Tasks(17, n_of(1, 16, 16)), 1), "auto: 17 tasks accepted");
  CHECK(!make_auto_item(it, 0, 0, {{}}, 1), "auto: an empty task accepted");
  CHECK(!make_auto_item(it, 0, 0, {{cu(16, 16), cu(32, 16)}}, 1), "auto: mixed sizes in a task accepted");
  CHECK(!make_auto_item(it, 0, 0, {n_of(5, 16, 16)}, 1), "auto: five CUs of 16 sub-blocks accepted");
  CHECK(!make_auto_item(it, 0, 0, {n_of(3, 32, 16)}, 1), "auto: 3 x 32 lanes accepted");
  CHECK(!make_auto_item(it, 0, 0, {n_of(1, 16, 8)}, 1), "auto: 8 lanes per CU accepted");
  CHECK(!make_auto_item(it, 0, 0, {n_of(1, 16, 16)}, 2), "auto: 16 sub-blocks on 8 lanes accepted");
  CHECK(!make_auto_item(it, 0, 0, {n_of(1, 64, 32)}, 1), "auto: 128 lanes per CU accepted");
}

static const int kRes[5][2] = {{416, 240}, {832, 480}, {1280, 720}, {1920, 1080}, {3840, 2160}};

static void check_order() {
  for (auto& r : kRes)
    for (int combos : {8, 408}) {
      const int nCtus = num_ctus(r[0], r[1]), cols = (r[0] + kCtu - 1) / kCtu;
      int nChunks = -1, cpp = -1;
      const std::vector<int32_t> order = build_order(nCtus, cols, combos, nChunks, cpp);
      CHECK(nChunks >= 1 && cpp >= 8 && cpp % 8 == 0 && order.size() == (size_t)nChunks * cpp,
            "order %dx%d/%d: %d chunks of %d, %zu entries", r[0], r[1], combos, nChunks, cpp, order.size());
      if (order.size() != (size_t)nChunks * cpp || cpp <= 0) continue;
      int next = 0;  // chunks hold whole CTU rows in raster order, then padding
      for (int ch = 0; ch < nChunks; ch++) {
        int n = 0;
        while (n < cpp && order[(size_t)ch * cpp + n] >= 0) n++;
        CHECK(n > 0 && n % cols == 0, "order %dx%d/%d chunk %d: %d CTUs, rows of %d", r[0], r[1], combos, ch, n, cols);
        for (int k = 0; k < cpp; k++) {
          const int32_t v = order[(size_t)ch * cpp + k];
          CHECK(v == (k < n ? next + k : -1), "order %dx%d/%d chunk %d slot %d: %d", r[0], r[1], combos, ch, k, v);
        }
        next += n;
      }
      CHECK(next == nCtus, "order %dx%d/%d: %d CTUs of %d", r[0], r[1], combos, next, nCtus);
    }
}

static void check_bi_table() {
  for (auto& r : kRes) {
    const int W = r[0], H = r[1], nCtus = num_ctus(W, H), cols = (W + kCtu - 1) / kCtu;
    const BiTable t = build_bi_table(W, H);
    CHECK(t.cands.size() == (size_t)t.nCand[0] + t.nCand[1] && t.groupCand.size() == (size_t)t.nGroup[0] + t.nGroup[1],
          "bi table %dx%d: sizes", W, H);
    if (W == 1920) CHECK(t.cands.size() == 60810, "bi table 1920x1080: %zu candidates", t.cands.size());
    size_t i = 0, group = 0;
    for (int al = 0; al < 2; al++) {
      const int per = al ? kHalfCusPerCtu : kFullCusPerCtu;
      // the in-frame CUs straight from the tables: (row, x, y, w, h)
      std::set<std::array<int, 5>> want, got;
      for (int ctu = 0; ctu < nCtus; ctu++)
        for (int g = 0; g < (al ? kHalfGroups : kFullGroups); g++) {
          const int w = al ? kHalfW[g] : kFullW[g], h = al ? kHalfH[g] : kFullH[g];
          const int n = al ? kHalfN[g] : kCtu / w * (kCtu / h), off = al ? kHalfStride[g] : kFullStride[g];
          for (int k = 0; k < n; k++) {
            const int x = ctu % cols * kCtu + (al ? kHalfX8[g][k] * 8 : k * w % kCtu);
            const int y = ctu / cols * kCtu + (al ? kHalfY8[g][k] * 8 : k * w / kCtu * h);
            if (x + w <= W && y + h <= H) want.insert({ctu * per + off + k, x, y, w, h});
          }
        }
      for (int n = 0; n < t.nCand[al] && i < t.cands.size(); n++, i++) {
        const BiCand& c = t.cands[i];
        const int w = 1 << (c.shape & 15), h = 1 << ((c.shape >> 4) & 15);
        CHECK((c.shape >> 8) == al, "bi table %dx%d cand %zu: alignment %d", W, H, i, c.shape >> 8);
        CHECK(c.row >= 0 && c.row < nCtus * per, "bi table %dx%d cand %zu: row %d", W, H, i, c.row);
        CHECK(got.insert({c.row, c.xy & 0xFFFF, c.xy >> 16, w, h}).second, "bi table %dx%d cand %zu: row %d twice", W, H, i, c.row);
        CHECK((size_t)c.first == group, "bi table %dx%d cand %zu: first %d, want %zu", W, H, i, c.first, group);
        for (int k = 0; k < (w * h) >> 8; k++, group++)
          CHECK(group < t.groupCand.size() && (size_t)t.groupCand[group] == i, "bi table %dx%d group %zu: not cand %zu", W, H, group, i);
      }
      CHECK(got == want, "bi table %dx%d alignment %d: %zu candidates, %zu in-frame CUs", W, H, al, got.size(), want.size());
      std::set<int> rows;
      for (auto& c : got) rows.insert(c[0]);
      CHECK(rows.size() == got.size(), "bi table %dx%d alignment %d: rows not unique", W, H, al);
      CHECK(group == (size_t)t.nGroup[0] + (al ? t.nGroup[1] : 0), "bi table %dx%d alignment %d: %zu groups", W, H, al, group);
    }
  }
}

int main() {
  check_templates();
  check_error_paths();
  check_order();
  check_bi_table();
  if (g_fails) {
    fprintf(stderr, "templates_check: %d check(s) failed\n", g_fails);
    return 1;
  }
  printf("templates_check ok: sizeof(Item) = %zu\n", sizeof(Item));
  return 0;
}

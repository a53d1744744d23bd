// cli_check.cpp -- stand-alone check of the `vame` CLI's host-only units,
// cli_options.cpp and cli_plan.cpp.  Built with them, vame_hostlogic.cpp and
// vame_templates.cpp alone (g++ -std=c++17 -fsanitize=address,undefined;
// tests/test_host.py), it exits non-zero unless
//   * the option parser accepts and refuses what boost's would, and the
//     Settings come out as the command line says;
//   * deal_pocs / plan_batches partition the POCs as their comments say, no
//     batch beyond kMaxBatchPairs pairs;
//   * recon_labels is the first-seen union of the POCs' reference lists;
//   * Layout's 32 blocks are disjoint, ordered, aligned and inside `bytes`;
//   * the apportioned per-PRED times sum to the fused time, masked PREDs 0.
// It prints the pred_work values that the test compares with an independent
// count (vame.metrics.pair_accounting).
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <vector>

#include "../../include/vame.h"
#include "../../vvc-affine-gpu_amd/host/cli_options.h"
#include "../../vvc-affine-gpu_amd/host/cli_plan.h"

using namespace vame_cli;

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
#define CHECK(cond, ...)            \
  do {                              \
    if (!(cond)) fail(__VA_ARGS__); \
  } while (0)

// ---------------------------------------------------------------- options
static int parse_args(Cli& c, std::initializer_list<const char*> args) {
  std::vector<const char*> argv{"vame"};
  argv.insert(argv.end(), args);
  return parse(c, (int)argv.size(), argv.data());
}

// A complete command line plus `args`: read_settings' exit code, or, where it
// goes on (-1), check_settings'.
static int settings(Settings& s, std::initializer_list<const char*> args, const char* qp = "32",
                    const char* frames = "3", const char* res = "416x240") {
  std::vector<const char*> argv{"vame", "-q", qp, "-f", frames, "-s", res, "-o", "orig.csv", "-r", "recon.csv"};
  argv.insert(argv.end(), args);
  const int rc = read_settings((int)argv.size(), argv.data(), s);
  return rc >= 0 ? rc : check_settings(s);
}

static void check_options() {
  {
    Cli c;
    for (auto& o : c.opts) CHECK(o.name && o.help, "option table has an empty entry");
    CHECK(std::string(c.opts[kDevices].name) == "devices" && std::string(c.opts[kQP].name) == "QP" &&
              std::string(c.opts[kLogFile].name) == "CpmvLogFile",
          "option table out of step with OptId");
    CHECK(parse_args(c, {"-q32"}) == 0 && c.has(kQP) && c.num(kQP) == 32, "-q32");
    CHECK(c.defaulted(kFrames) && c.str(kGpus) == "1" && c.num(kThreads) == 0, "defaults");
  }
  {
    Cli c;
    CHECK(parse_args(c, {"--QP=32", "--Frames=3"}) == 0 && c.num(kQP) == 32 && c.num(kFrames) == 3,
          "--QP=32 --Frames=3 (unique prefix)");
  }
  {
    Cli c;
    CHECK(parse_args(c, {"--per-launch", "--prof", "-f", "2"}) == 0 && c.flag("per-launch") && c.flag("prof") &&
              !c.flag("help") && c.num(kFrames) == 2,
          "value-less flags");
  }
  const std::initializer_list<const char*> errors[] = {
      {"--R", "1"},  // Resolution or ReferenceFrames
      {"-f", "1", "-q"}, {"stray"}, {"--bogus", "1"}, {"-x", "1"}, {"--QP"}};
  for (auto& e : errors) {
    Cli c;
    CHECK(parse_args(c, e) == 2, "'%s ...' must be a parse error", *e.begin());
  }
  for (auto& h : {std::initializer_list<const char*>{"-h"}, {"--help"}, {"-q", "3", "--help"}}) {
    Cli c;
    CHECK(parse_args(c, h) == 1, "help");
  }

  Settings s;
  CHECK(settings(s, {}) == -1, "a complete command line is accepted");
  CHECK(s.frames == 3 && s.qp == 32 && s.extra == 0 && s.W == 416 && s.H == 240 && s.orig_path == "orig.csv" &&
            s.recon_path == "recon.csv" && s.prefix.empty() && !s.per_launch && !s.prof && s.threads == 0 &&
            s.mode_mask == (VAME_MODE_2CP | VAME_MODE_3CP) && s.devices == std::vector<int>{0},
        "default settings");
  CHECK(settings(s, {"--devices", "0,0,0"}) == -1 && s.devices == std::vector<int>({0, 0, 0}), "--devices 0,0,0");
  CHECK(settings(s, {"--gpus", "2", "--DeviceIndex", "1"}) == -1 && s.devices == std::vector<int>({1, 2}),
        "--gpus 2 --DeviceIndex 1");
  CHECK(settings(s, {"--modes", "2cp", "--align", "half"}) == -1 && s.mode_mask == (VAME_MODE_2CP | VAME_MODE_HALF),
        "--modes 2cp --align half");
  CHECK(settings(s, {"--align", "full", "--per-launch", "--prof", "--threads", "5", "-l", "out/log",
                     "--ExtraGradientIter", "2"}) == -1 &&
            s.mode_mask == (VAME_MODE_2CP | VAME_MODE_3CP | VAME_MODE_FULL) && s.per_launch && s.prof &&
            s.threads == 5 && s.prefix == "out/log" && s.extra == 2,
        "the extension options");
  CHECK(settings(s, {"--align", "diag"}) == 1, "--align diag");
  CHECK(settings(s, {"--modes", "x"}) == 1, "--modes x");
  CHECK(settings(s, {"--bogus", "1"}) == 1 && settings(s, {"--help"}) == 1, "parse error / help exit with 1");
  CHECK(settings(s, {}, "32", "3", "416") == 0, "-s 416 (the reference returns 0 here)");
  CHECK(settings(s, {}, "32", "3", "417x240") == 0, "unsupported resolution");
  CHECK(settings(s, {}, "32", "0") == 1, "-f 0");
  CHECK(settings(s, {}, "70") == 1 && settings(s, {}, "-20") == 1, "QP outside the lambda table");
  const char* no_qp[] = {"vame", "-f", "1"};
  CHECK(read_settings(3, no_qp, s) == 1, "missing required options");
}

// ---------------------------------------------------------------- plan
static int pairs_of(const std::vector<int>& batch) {
  int n = 0;
  for (int p : batch) n += std::min(4, p);
  return n;
}

static void check_deal_and_batches() {
  for (int N = 1; N <= 40; N++)
    for (int workers = 1; workers <= 5; workers++) {
      const auto deal = deal_pocs(N, workers);
      CHECK((int)deal.size() == workers, "deal_pocs(%d, %d): %zu lists", N, workers, deal.size());
      std::vector<int> seen(N + 1, 0);
      for (int w = 0; w < (int)deal.size(); w++) {
        CHECK(std::is_sorted(deal[w].begin(), deal[w].end()), "deal_pocs(%d, %d): worker %d not ascending", N,
              workers, w);
        for (int p : deal[w]) {
          CHECK(p >= 1 && p <= N, "deal_pocs(%d, %d): POC %d", N, workers, p);
          if (p < 1 || p > N) continue;
          seen[p]++;
          CHECK(w == ((p - 1) / 4) % workers, "deal_pocs(%d, %d): POC %d with worker %d", N, workers, p, w);
        }
        for (bool per_launch : {false, true}) {
          const auto batches = plan_batches(deal[w], per_launch);
          std::vector<int> cat;
          for (auto& b : batches) {
            CHECK(!b.empty() && (per_launch ? b.size() == 1 : b.size() <= (size_t)kBatchPocs),
                  "plan_batches: a batch of %zu POCs (per_launch %d)", b.size(), per_launch);
            CHECK(pairs_of(b) <= kMaxBatchPairs, "plan_batches: %d pairs in a batch", pairs_of(b));
            cat.insert(cat.end(), b.begin(), b.end());
          }
          CHECK(cat == deal[w], "plan_batches(%d POCs, %d) is no partition in order", (int)deal[w].size(),
                per_launch);
        }
      }
      for (int p = 1; p <= N; p++) CHECK(seen[p] == 1, "deal_pocs(%d, %d): POC %d dealt %d times", N, workers, p, seen[p]);
    }
  const auto d13 = deal_pocs(13, 3);
  CHECK(d13[0] == std::vector<int>({1, 2, 3, 4, 13}) && d13[1] == std::vector<int>({5, 6, 7, 8}) &&
            d13[2] == std::vector<int>({9, 10, 11, 12}),
        "deal_pocs(13, 3)");
  const auto d4 = deal_pocs(4, 3);
  CHECK(d4[0].size() == 4 && d4[1].empty() && d4[2].empty(), "deal_pocs(4, 3): two idle workers");
  CHECK(plan_batches({}, false).empty(), "no POCs, no batches");
  // a contiguous run is cut every kBatchPocs POCs
  std::vector<int> run;
  for (int p = 1; p <= 10; p++) run.push_back(p);
  const auto b10 = plan_batches(run, false);
  CHECK(b10.size() == 3 && b10[0].size() == 4 && b10[1].size() == 4 && b10[2] == std::vector<int>({9, 10}),
        "plan_batches(1..10)");
  CHECK(kMaxBatchPairs == 4 * kBatchPocs && kMaxBatchPairs <= 32, "kMaxBatchPairs within vame_set_max_pairs' range");
  CHECK(slabs_per_worker(false) == 2 * kBatchPocs + 2 && slabs_per_worker(true) == 3, "slabs_per_worker");
}

// true if one of the lists holds a reference older than the four frames before its POC
static bool check_labels(const std::vector<int>& pocs) {
  const std::vector<int> labels = recon_labels(pocs);
  std::vector<int> expect;
  bool long_term = false;
  for (int p : pocs) {
    int refs[4];
    const int n = vame_ref_list(p, refs);
    CHECK(n >= 1 && n <= 4, "vame_ref_list(%d) = %d", p, n);
    for (int r = 0; r < n; r++) {
      if (std::find(expect.begin(), expect.end(), refs[r]) == expect.end()) expect.push_back(refs[r]);
      CHECK(std::find(labels.begin(), labels.end(), refs[r]) != labels.end(), "label %d of POC %d missing", refs[r], p);
      long_term |= p - refs[r] > 4;
    }
  }
  CHECK(labels == expect, "recon_labels: not the first-seen union (%zu POCs)", pocs.size());
  std::vector<int> sorted = labels;
  std::sort(sorted.begin(), sorted.end());
  CHECK(std::adjacent_find(sorted.begin(), sorted.end()) == sorted.end(), "recon_labels: a label twice");
  return long_term;
}

static void check_recon_labels() {
  CHECK(recon_labels({}).empty(), "no POCs, no labels");
  CHECK(recon_labels({1}) == std::vector<int>{0}, "POC 1 refers to frame 0");
  CHECK(!check_labels({1, 2, 3, 4}), "POCs 1-4 refer to the frames before them");
  check_labels({1, 2, 3, 4, 5, 6});
  check_labels(deal_pocs(13, 3)[0]);
  std::vector<int> late;  // their lists hold a long-term reference
  for (int p = 211; p <= 240; p++) late.push_back(p);
  CHECK(check_labels(late), "POCs 211-240 hold a long-term reference");
  for (int w = 0; w < 3; w++) check_labels(deal_pocs(240, 3)[w]);
}

static void check_layout() {
  const int sizes[3][2] = {{416, 240}, {1920, 1080}, {3840, 2160}};
  for (auto& wh : sizes) {
    const int nCtus = vame_num_ctus(wh[0], wh[1]);
    CHECK(nCtus > 0, "%dx%d", wh[0], wh[1]);
    const Layout L(nCtus);
    size_t at = 0, formula = 0;
    for (int r = 0; r < 4; r++)
      for (int m = 0; m < 4; m++) {
        const size_t n = (size_t)nCtus * ((m >> 1) ? 284 : 201);  // the sizes the CLI used to restate
        const size_t cp_len = (n * sizeof(vame_cpmvs) + 255) & ~size_t(255);
        CHECK(L.off_cost[r][m] == at && L.off_cost[r][m] % 8 == 0, "%dx%d cost[%d][%d] at %zu, expected %zu", wh[0],
              wh[1], r, m, L.off_cost[r][m], at);
        at += n * sizeof(int64_t);
        CHECK(L.off_cp[r][m] == at, "%dx%d cpmvs[%d][%d] at %zu, expected %zu", wh[0], wh[1], r, m, L.off_cp[r][m], at);
        CHECK(cp_len % 256 == 0 && cp_len >= n * sizeof(vame_cpmvs), "cpmvs block length %zu", cp_len);
        at += cp_len;
        formula += n * sizeof(int64_t) + cp_len;
      }
    CHECK(L.bytes == at && L.bytes == formula, "%dx%d: %zu bytes, expected %zu", wh[0], wh[1], L.bytes, formula);
  }
  CHECK(vame_cus_per_ctu(0) == 201 && vame_cus_per_ctu(1) == 284, "vame_cus_per_ctu");
}

static void check_apportioning() {
  const int sizes[2][2] = {{416, 240}, {1920, 1080}};
  for (auto& wh : sizes)
    for (int extra : {0, 2}) {
      double w[4];
      for (int m = 0; m < 4; m++) w[m] = pred_work(wh[0], wh[1], m >> 1, (m & 1) ? 3 : 2, extra);
      printf("pred_work %dx%d extra %d: %.0f %.0f %.0f %.0f\n", wh[0], wh[1], extra, w[0], w[1], w[2], w[3]);
      CHECK(w[0] > w[1] && w[2] > w[3] && w[3] > 0, "pred_work: 2 CP is 6 predictions per sub-block, 3 CP 5");
      for (int mask : {15, 5, 3, 12, 1, 4}) {
        const float fused = 123456792.f;
        float ns[4] = {-1, -1, -1, -1};
        apportion(fused, wh[0], wh[1], mask, extra, ns);
        double sum = 0, wsum = 0;
        for (int m = 0; m < 4; m++) {
          sum += ns[m];
          if ((mask >> m) & 1) wsum += w[m];
        }
        for (int m = 0; m < 4; m++) {
          if (!((mask >> m) & 1)) CHECK(ns[m] == 0, "masked-out PRED %d gets %f", m, (double)ns[m]);
          else CHECK(ns[m] == (float)((double)fused * w[m] / wsum), "PRED %d of mask %d: %f", m, mask, (double)ns[m]);
        }
        // four values rounded to float: each within half an ulp of its share
        CHECK(std::fabs(sum - fused) <= 4 * fused * 6e-8, "mask %d: the parts sum to %f, fused %f", mask, sum,
              (double)fused);
      }
    }
}

int main() {
  check_options();
  check_deal_and_batches();
  check_recon_labels();
  check_layout();
  check_apportioning();
  if (g_fails) {
    fprintf(stderr, "cli_check: %d check(s) failed\n", g_fails);
    return 1;
  }
  printf("cli_check ok\n");
  return 0;
}

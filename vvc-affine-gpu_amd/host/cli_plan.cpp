// cli_plan.cpp -- see cli_plan.h.
#include "cli_plan.h"

#include <algorithm>
#include <cstdint>

#include "../../include/vame.h"

namespace vame_cli {

Layout::Layout(int nCtus) {
  size_t o = 0;
  for (int r = 0; r < 4; r++)
    for (int m = 0; m < 4; m++) {
      const size_t n = (size_t)nCtus * vame_cus_per_ctu(m >> 1);
      off_cost[r][m] = o;
      o += n * sizeof(int64_t);
      off_cp[r][m] = o;
      o += (n * sizeof(vame_cpmvs) + 255) & ~size_t(255);
    }
  bytes = o;
}

std::vector<std::vector<int>> deal_pocs(int N, int workers) {
  std::vector<std::vector<int>> pocs(workers);
  for (int p = 1; p <= N; p++) pocs[((p - 1) / kBatchPocs) % workers].push_back(p);
  return pocs;
}

std::vector<std::vector<int>> plan_batches(const std::vector<int>& pocs, bool per_launch) {
  const size_t B = per_launch ? 1 : kBatchPocs;
  std::vector<std::vector<int>> batches;
  for (int p : pocs) {
    if (batches.empty() || batches.back().size() == B) batches.push_back({});
    batches.back().push_back(p);
  }
  return batches;
}

std::vector<int> recon_labels(const std::vector<int>& pocs) {
  std::vector<int> labels;
  for (int p : pocs) {
    int refs[4];
    const int n = vame_ref_list(p, refs);
    for (int r = 0; r < n; r++)
      if (std::find(labels.begin(), labels.end(), refs[r]) == labels.end()) labels.push_back(refs[r]);
  }
  return labels;
}

double pred_work(int W, int H, int align, int ncp, int extra) {
  const int cols = (W + 127) / 128, rows = (H + 127) / 128;
  double sb = 0;
  int w, h, n, stride, xs[64], ys[64];
  for (int g = 0; g < vame_num_groups(align); g++) {
    if (vame_group_geometry(align, g, &w, &h, &n, &stride, xs, ys)) continue;
    for (int ctu = 0; ctu < cols * rows; ctu++)
      for (int k = 0; k < n; k++) {
        const int x = (ctu % cols) * 128 + xs[k], y = (ctu / cols) * 128 + ys[k];
        if (x + w <= W && y + h <= H) sb += (double)(w / 4) * (h / 4);
      }
  }
  return sb * ((ncp == 2 ? 6 : 5) + extra);
}

void apportion(float fused_ns, int W, int H, int pred_mask, int extra, float pred_ns[4]) {
  double wgt[4], sum = 0;
  for (int m = 0; m < 4; m++) {
    wgt[m] = !((pred_mask >> m) & 1) ? 0 : pred_work(W, H, m >> 1, (m & 1) ? 3 : 2, extra);
    sum += wgt[m];
  }
  for (int m = 0; m < 4; m++) pred_ns[m] = (float)((double)fused_ns * wgt[m] / sum);
}

}  // namespace vame_cli

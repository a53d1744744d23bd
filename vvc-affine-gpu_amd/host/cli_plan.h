// cli_plan.h -- the `vame` CLI's host arithmetic: where one POC's results lie,
// which worker codes which POCs in which batches, which recon frames a worker
// holds, and how a fused launch's time is shared among the reference's
// per-PRED keys.  Host-only (no HIP): tests/native/cli_check.cpp runs it
// under ASan + UBSan.
#pragma once
#include <cstddef>
#include <vector>

namespace vame_cli {

constexpr int kBatchPocs = 4;  // POCs per vame_affine_me_batch call
// A POC has at most 4 (POC, refIdx) pairs, so a batch never holds more than
// this many: what plan_batches guarantees and what the worker sizes its
// context's seed-reuse scratch for (vame_set_max_pairs; half of the default).
constexpr int kMaxBatchPairs = 4 * kBatchPocs;

struct Layout {  // one POC's results: [ref][pred] cost block, then cpmvs block
  size_t off_cost[4][4], off_cp[4][4], bytes;
  explicit Layout(int nCtus);
};

// POCs 1..N in chunks of kBatchPocs consecutive POCs, dealt to the workers in
// turn.  The writer takes POCs in order and each worker holds at most
// slabs_per_worker unwritten slabs, so the workers must advance through the
// sequence together: with one contiguous block per worker, worker 1 would
// stall after its first slabs until the writer had drained worker 0's block.
std::vector<std::vector<int>> deal_pocs(int N, int workers);

// A worker's POCs cut into batches: the fused path hands up to kBatchPocs POCs
// (<= kMaxBatchPairs pairs) to one vame_affine_me_batch call, so they share
// launches; --per-launch keeps the reference's one launch per (refIdx, PRED).
std::vector<std::vector<int>> plan_batches(const std::vector<int>& pocs, bool per_launch);

// The recon labels a worker's reference rings hold (vame_ref_list), each once,
// in first-seen order -- the order of the frames in its device block.
std::vector<int> recon_labels(const std::vector<int>& pocs);

// Pinned result slabs per worker: two batches in flight plus two POCs' worth
// for the writer.
inline int slabs_per_worker(bool per_launch) { return per_launch ? 3 : 2 * kBatchPocs + 2; }

// Algorithmic work of one PRED of one (POC, ref) pair: sub-block predictions
// over the in-frame CUs (affine.cl:192-193; n_pred 6 / 5 for 2 / 3 CP, + extra
// iterations, affine.cl:172-177) -- the weights that apportion a fused
// launch's kernel time to the reference's per-PRED keys.
double pred_work(int W, int H, int align, int ncp, int extra);
// fused_ns shared among the PREDs of pred_mask by pred_work; 0 for the others.
void apportion(float fused_ns, int W, int H, int pred_mask, int extra, float pred_ns[4]);

}  // namespace vame_cli

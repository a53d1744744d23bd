// vame_stages.hip -- the C entry points of the stages after the fused search
// (include/vame.h): affine MC, partition, bi-prediction and its refinement,
// the seed searches, the search on a CU list and the seeded search.  Each
// checks its arguments, fills the stage's parameter block and calls the
// stage's launch function; the kernels are in the stages' own units, none is
// here.
#include <hip/hip_runtime.h>

#include <cstring>
#include <type_traits>

#include "../../include/vame.h"
#include "vame_ctx.h"
#include "vame_mc_core.h"
#include "vame_partition.h"
#include "vame_bipred.h"
#include "vame_birefine.h"
#include "vame_search.h"
#include "vame_seed.h"

using namespace vame;

static_assert(sizeof(vame_mc_cu) == sizeof(McCu) && VAME_MC_MAX_CUS == kMcMaxCus, "vame_mc_cu layout");
static_assert(sizeof(vame_mc_bicu) == sizeof(McBiCu) && sizeof(McBiCu) == 80, "vame_mc_bicu layout");

namespace {

// vame_affine_mc (ncus_dev NULL), vame_affine_mc_dev (ncus = the capacity)
// and, over bi descriptors (CU = vame_mc_bicu), vame_affine_mc_bi
// and vame_affine_mc_bi_p (preds non-NULL: the MVP instances of its kernels)
template <typename CU>
int affine_mc(vame_ctx* c, const uint16_t* cur, const uint16_t* const* refs, int nrefs, const CU* cus,
              int ncus, const int32_t* ncus_dev, float lambda, uint16_t* pred, int64_t* cost, int32_t* bad,
              void* stream, const vame_cpmvs* preds = nullptr) {
  constexpr bool bi = std::is_same<CU, vame_mc_bicu>::value;
  if (!c || !refs || nrefs < 1 || nrefs > 4 || ncus < 0 || ncus > VAME_MC_MAX_CUS || !bad) return VAME_E_INVALID;
  if ((!pred && !cost) || (cost && !cur)) return VAME_E_INVALID;
  // the kernel reads window rows as dwords and moves block rows as 8-byte words
  if ((reinterpret_cast<uintptr_t>(cur) | reinterpret_cast<uintptr_t>(pred)) & 7) return VAME_E_INVALID;
  typename std::conditional<bi, McBiParams, McParams>::type p;
  memset(&p, 0, sizeof(p));
  if (!set_refs(p.refs, refs, nrefs)) return VAME_E_INVALID;
  if (bi && c->prof) return VAME_E_UNSUPPORTED;  // PROF has no bi form
  if (ncus == 0) return VAME_OK;
  if (!cus) return VAME_E_INVALID;
  DeviceGuard guard(c->device);
  VAME_HIP(guard.err);
  p.cur = cur;
  p.cus = reinterpret_cast<decltype(p.cus)>(cus);
  p.pred = pred;
  p.cost = cost;
  p.bad = bad;
  p.offs = c->mcScratch;
  p.blockSum = c->mcScratch + kMcMaxCus + 1;
  p.ncus = ncus;
  p.nrefs = nrefs;
  p.W = c->W;
  p.H = c->H;
  p.lambda = lambda;
  p.ncusDev = ncus_dev;
  if constexpr (bi) {
    if (preds) {
      McBiParamsP pp;
      static_cast<McBiParams&>(pp) = p;
      pp.preds = reinterpret_cast<const int32_t*>(preds);
      VAME_HIP(mc_bi_p_launch(pp, (hipStream_t)stream));
    } else {
      VAME_HIP(mc_bi_launch(p, (hipStream_t)stream));
    }
  } else {
    VAME_HIP(mc_launch(p, c->prof, (hipStream_t)stream));
  }
  return VAME_OK;
}

// vame_partition and (bi: leaves may be bi-predicted, `cus` holds vame_mc_bicu
// descriptors) vame_partition_bi
int partition(vame_ctx* c, const vame_poc_result* res, int nrefs, int pred_mask, int64_t split_penalty, bool bi,
              const int64_t* const* bi_cost, const int32_t* const* bi_sel, int64_t bi_penalty, void* cus,
              int32_t* rows, int32_t* sel, int32_t* ncus, int32_t* ctu_info, int64_t* ctu_cost,
              int32_t* block_cu, void* stream) {
  if (!c || !res || nrefs < 1 || nrefs > 4 || !cus || !ncus || (bi && (!bi_cost || !bi_sel))) return VAME_E_INVALID;
  if ((pred_mask & ~15) || !(pred_mask & 3)) return VAME_E_INVALID;  // at least one FULL PRED
  if (split_penalty < 0 || split_penalty > (int64_t(1) << 40)) return VAME_E_INVALID;
  if (bi_penalty < 0 || bi_penalty > (int64_t(1) << 40)) return VAME_E_INVALID;
  PartParams p;
  memset(&p, 0, sizeof(p));
  if (!set_result(p.cost, p.cpmv, res, nrefs, pred_mask)) return VAME_E_INVALID;
  for (int a = 0; bi && a < 2; a++) {
    if (!((pred_mask >> (2 * a)) & 3)) continue;
    if (!bi_cost[a] || !bi_sel[a]) return VAME_E_INVALID;
    p.biCost[a] = bi_cost[a];
    p.biSel[a] = bi_sel[a];
  }
  if (bi && c->prof) return VAME_E_UNSUPPORTED;  // PROF has no bi form
  DeviceGuard guard(c->device);
  VAME_HIP(guard.err);
  p.cus = reinterpret_cast<McCu*>(cus);
  p.rows = rows;
  p.sel = sel;
  p.ncus = ncus;
  p.ctuInfo = ctu_info;
  p.ctuCost = ctu_cost;
  p.blockCu = block_cu;
  p.scratch = c->partScratch;
  p.penalty = split_penalty;
  p.biPenalty = bi_penalty;
  p.nrefs = nrefs;
  p.predMask = pred_mask;
  p.W = c->W;
  p.H = c->H;
  p.nCtus = c->nCtus;
  p.ctusPerRow = c->ctusPerRow;
  VAME_HIP(partition_launch(p, (hipStream_t)stream, bi));
  return VAME_OK;
}

// What vame_seed_search and vame_seed_search_wide share, after their own
// argument checks: the references and the (refIdx, alignment) output mask into
// the zeroed block, then its common fields and the launches.
int seed_search(vame_ctx* c, SeedParams& p, const uint16_t* cur, const uint16_t* const* refs, int nrefs,
                float lambda, int align_mask, int radius, const vame_seed_result* out, void* stream) {
  if (!set_refs(p.refs, refs, nrefs)) return VAME_E_INVALID;
  for (int r = 0; r < nrefs; r++)
    for (int a = 0; a < 2; a++) {
      if (!((align_mask >> a) & 1)) continue;
      if (!out->mv[r][a] || !out->cost[r][a]) return VAME_E_INVALID;
      p.cost[r][a] = out->cost[r][a];
      p.mv[r][a] = reinterpret_cast<int32_t*>(out->mv[r][a]);
    }
  DeviceGuard guard(c->device);
  VAME_HIP(guard.err);
  p.cur = cur;
  p.nrefs = nrefs;
  p.W = c->W;
  p.H = c->H;
  p.nCtus = c->nCtus;
  p.ctusPerRow = c->ctusPerRow;
  p.radius = radius;
  p.lambda = lambda;
  VAME_HIP(seed_launch(p, (hipStream_t)stream));
  return VAME_OK;
}

// vame_affine_search and vame_bipred_refine: the same checks in the same
// order and the same parameter block, but for the CU descriptor, the name of
// the iteration count (P::*iters, at most maxIters) and the launch function.
// `launch` is any callable (const P&, hipStream_t) -> hipError_t: the stage's
// launch function, or with_preds (below) for the _p forms.
template <typename P, typename CU, typename Launch>
int refine_cus(vame_ctx* c, const uint16_t* cur, const uint16_t* const* refs, int nrefs, const CU* cus, int max_cus,
               const int32_t* ncus_dev, float lambda, int P::*iters, int niters, int maxIters, CU* out, int64_t* cost,
               int32_t* bad, Launch launch, void* stream) {
  if (!c || !cur || !refs || !cus || !out || !cost || !bad) return VAME_E_INVALID;
  if (nrefs < 1 || nrefs > 4 || niters < 0 || niters > maxIters || max_cus < 0 || max_cus > VAME_MC_MAX_CUS)
    return VAME_E_INVALID;
  // the kernel reads window rows as dwords and block rows as 8-byte words
  if (reinterpret_cast<uintptr_t>(cur) & 7) return VAME_E_INVALID;
  P p;
  memset(&p, 0, sizeof(p));
  if (!set_refs(p.refs, refs, nrefs)) return VAME_E_INVALID;
  if (c->prof) return VAME_E_UNSUPPORTED;  // no PROF form (PROF has no bi form)
  if (max_cus == 0) return VAME_OK;
  DeviceGuard guard(c->device);
  VAME_HIP(guard.err);
  p.cur = cur;
  p.cus = reinterpret_cast<decltype(p.cus)>(cus);
  p.out = reinterpret_cast<decltype(p.out)>(out);
  p.cost = cost;
  p.bad = bad;
  p.maxCus = max_cus;
  p.nrefs = nrefs;
  p.W = c->W;
  p.H = c->H;
  p.*iters = niters;
  p.lambda = lambda;
  p.ncusDev = ncus_dev;
  VAME_HIP(launch(p, (hipStream_t)stream));
  return VAME_OK;
}

// The launch of a _p call on a CU list: the block with the predictors and the
// launch of their instances, or -- preds NULL, the zero predictor -- the
// counterpart's own launch.
template <typename PP, typename P>
auto with_preds(const vame_cpmvs* preds, hipError_t (*launch)(const P&, hipStream_t),
                hipError_t (*launch_p)(const PP&, hipStream_t)) {
  return [=](const P& p, hipStream_t stream) {
    if (!preds) return launch(p, stream);
    PP pp;
    static_cast<P&>(pp) = p;
    pp.preds = reinterpret_cast<const int32_t*>(preds);
    return launch_p(pp, stream);
  };
}

// The in-frame candidates of the alignments a valid mode mask codes: their
// range in the context's table.
bool seeded_range(vame_ctx* c, int mode_mask, int& begin, int& end) {
  if (!(mode_mask & VAME_MODE_2CP) || (mode_mask & ~15)) return false;
  const int preds = vame_pred_mask(mode_mask);
  begin = (preds & 3) ? 0 : c->biNCand[0];
  end = (preds & 12) ? c->biNCand[0] + c->biNCand[1] : c->biNCand[0];
  return true;
}

// The predictor arrays of refIdx 0 .. nrefs-1 for the alignments with a PRED
// in `preds` into a parameter block: each non-null.
bool set_mvp(const int32_t* (&dst)[4][2], const vame_mvp* mvp, int nrefs, int preds) {
  for (int r = 0; r < nrefs; r++)
    for (int a = 0; a < 2; a++) {
      if (!((preds >> (2 * a)) & 3)) continue;
      if (!mvp->mv[r][a]) return false;
      dst[r][a] = reinterpret_cast<const int32_t*>(mvp->mv[r][a]);
    }
  return true;
}

// vame_affine_me_seeded (mvp NULL) and vame_affine_me_seeded_p (which rejects a NULL mvp itself)
int affine_me_seeded(vame_ctx* c, const uint16_t* cur, const uint16_t* const* refs, int nrefs, float lambda,
                     int mode_mask, int extra_grad_iter, vame_mv* const seed_mv[4][2],
                     const vame_mvp* mvp, const vame_poc_result* res, void* work, size_t work_bytes, int32_t* bad,
                     void* stream) {
  if (!c || !cur || !refs || !seed_mv || !res || !work || !bad || nrefs < 1 || nrefs > 4) return VAME_E_INVALID;
  if (extra_grad_iter < 0 || extra_grad_iter > 64) return VAME_E_INVALID;
  if ((reinterpret_cast<uintptr_t>(cur) | reinterpret_cast<uintptr_t>(work)) & 7) return VAME_E_INVALID;
  SeededParamsP p;
  memset(&p, 0, sizeof(p));
  if (!seeded_range(c, mode_mask, p.candBegin, p.candEnd)) return VAME_E_INVALID;
  const int preds = vame_pred_mask(mode_mask);
  if (!set_refs(p.search.refs, refs, nrefs)) return VAME_E_INVALID;
  if (!set_result(p.cost, p.cpmv, res, nrefs, preds)) return VAME_E_INVALID;
  for (int r = 0; r < nrefs; r++)
    for (int a = 0; a < 2; a++) {
      if (!((preds >> (2 * a)) & 3)) continue;
      if (!seed_mv[r][a]) return VAME_E_INVALID;
      p.seed[r][a] = reinterpret_cast<const int32_t*>(seed_mv[r][a]);
    }
  if (mvp && !set_mvp(p.mvp, mvp, nrefs, preds)) return VAME_E_INVALID;
  p.with3 = (mode_mask & VAME_MODE_3CP) != 0;
  p.cap = nrefs * (p.candEnd - p.candBegin);
  if (work_bytes < (mvp ? seeded_p_work_bytes((size_t)p.cap, p.with3) : seeded_work_bytes((size_t)p.cap, p.with3)))
    return VAME_E_INVALID;
  if (c->prof) return VAME_E_UNSUPPORTED;  // no PROF form
  DeviceGuard guard(c->device);
  VAME_HIP(guard.err);
  p.cands = c->biCands;
  p.work = seeded_work(work, (size_t)p.cap, p.with3);
  p.preds = reinterpret_cast<int32_t*>(static_cast<char*>(work) + seeded_work_bytes((size_t)p.cap, p.with3));
  p.search.cur = cur;
  p.search.bad = bad;
  p.search.nrefs = nrefs;
  p.search.W = c->W;
  p.search.H = c->H;
  p.search.extra = extra_grad_iter;
  p.search.lambda = lambda;
  if (mvp)
    VAME_HIP(seeded_p_launch(p, (hipStream_t)stream));
  else
    VAME_HIP(seeded_launch(p, (hipStream_t)stream));
  return VAME_OK;
}

// vame_bipred (mvp NULL) and vame_bipred_p (which rejects a NULL mvp itself)
int bipred(vame_ctx* c, const uint16_t* cur, const uint16_t* const* refs, int nrefs, float lambda,
           const vame_poc_result* res, int pred_mask, const vame_mvp* mvp, int64_t* const bi_cost[2],
           int32_t* const bi_sel[2], void* stream) {
  if (!c || !cur || !refs || !res || nrefs < 1 || nrefs > 4 || !bi_cost || !bi_sel) return VAME_E_INVALID;
  if ((pred_mask & ~15) || !pred_mask) return VAME_E_INVALID;
  if (reinterpret_cast<uintptr_t>(cur) & 7) return VAME_E_INVALID;
  BiRowsParamsP p;
  memset(&p, 0, sizeof(p));
  if (!set_refs(p.refs, refs, nrefs)) return VAME_E_INVALID;
  if (!set_result(p.cost, p.cpmv, res, nrefs, pred_mask)) return VAME_E_INVALID;
  const bool on[2] = {(pred_mask & 3) != 0, (pred_mask & 12) != 0};
  for (int a = 0; a < 2; a++) {
    if (!on[a]) continue;
    if (!bi_cost[a] || !bi_sel[a]) return VAME_E_INVALID;
    p.biCost[a] = bi_cost[a];
    p.biSel[a] = bi_sel[a];
  }
  if (mvp && !set_mvp(p.mvp, mvp, nrefs, pred_mask)) return VAME_E_INVALID;
  if (c->prof) return VAME_E_UNSUPPORTED;  // PROF has no bi form
  DeviceGuard guard(c->device);
  VAME_HIP(guard.err);
  p.cur = cur;
  p.cands = c->biCands;
  p.groupCand = c->biGroupCand;
  p.pairSatd = c->biPairSatd;
  p.candBegin = on[0] ? 0 : c->biNCand[0];
  p.candEnd = on[1] ? c->biNCand[0] + c->biNCand[1] : c->biNCand[0];
  p.groupBegin = on[0] ? 0 : c->biNGroup[0];
  p.groupEnd = on[1] ? c->biNGroup[0] + c->biNGroup[1] : c->biNGroup[0];
  p.rowsOf[0] = c->nCtus * kFullCusPerCtu;
  p.rowsOf[1] = c->nCtus * kHalfCusPerCtu;
  p.nrefs = nrefs;
  p.predMask = pred_mask;
  p.W = c->W;
  p.H = c->H;
  p.lambda = lambda;
  if (mvp)
    VAME_HIP(bipred_p_launch(p, (hipStream_t)stream));
  else
    VAME_HIP(bipred_launch(p, (hipStream_t)stream));
  return VAME_OK;
}

}  // namespace

extern "C" {

int vame_affine_mc(vame_ctx* c, const uint16_t* cur, const uint16_t* const* refs, int nrefs,
                   const vame_mc_cu* cus, int ncus, float lambda, uint16_t* pred, int64_t* cost,
                   int32_t* bad, void* stream) {
  return affine_mc(c, cur, refs, nrefs, cus, ncus, nullptr, lambda, pred, cost, bad, stream);
}

int vame_affine_mc_dev(vame_ctx* c, const uint16_t* cur, const uint16_t* const* refs, int nrefs,
                       const vame_mc_cu* cus, int max_cus, const int32_t* ncus_dev, float lambda,
                       uint16_t* pred, int64_t* cost, int32_t* bad, void* stream) {
  if (!ncus_dev) return VAME_E_INVALID;
  return affine_mc(c, cur, refs, nrefs, cus, max_cus, ncus_dev, lambda, pred, cost, bad, stream);
}

int vame_partition(vame_ctx* c, const vame_poc_result* res, int nrefs, int pred_mask, int64_t split_penalty,
                   vame_mc_cu* cus, int32_t* rows, int32_t* ncus, int32_t* ctu_info, int64_t* ctu_cost,
                   int32_t* block_cu, void* stream) {
  return partition(c, res, nrefs, pred_mask, split_penalty, false, nullptr, nullptr, 0, cus, rows, nullptr, ncus,
                   ctu_info, ctu_cost, block_cu, stream);
}

int vame_affine_mc_bi(vame_ctx* c, const uint16_t* cur, const uint16_t* const* refs, int nrefs,
                      const vame_mc_bicu* cus, int max_cus, const int32_t* ncus_dev, float lambda,
                      uint16_t* pred, int64_t* cost, int32_t* bad, void* stream) {
  return affine_mc(c, cur, refs, nrefs, cus, max_cus, ncus_dev, lambda, pred, cost, bad, stream);
}

int vame_bipred(vame_ctx* c, const uint16_t* cur, const uint16_t* const* refs, int nrefs, float lambda,
                const vame_poc_result* res, int pred_mask, int64_t* const bi_cost[2], int32_t* const bi_sel[2],
                void* stream) {
  return bipred(c, cur, refs, nrefs, lambda, res, pred_mask, nullptr, bi_cost, bi_sel, stream);
}

int vame_partition_bi(vame_ctx* c, const vame_poc_result* res, int nrefs, int pred_mask, int64_t split_penalty,
                      const int64_t* const bi_cost[2], const int32_t* const bi_sel[2], int64_t bi_penalty,
                      vame_mc_bicu* cus, int32_t* rows, int32_t* sel, int32_t* ncus, int32_t* ctu_info,
                      int64_t* ctu_cost, int32_t* block_cu, void* stream) {
  return partition(c, res, nrefs, pred_mask, split_penalty, true, bi_cost, bi_sel, bi_penalty, cus, rows, sel, ncus,
                   ctu_info, ctu_cost, block_cu, stream);
}

int vame_bipred_refine(vame_ctx* c, const uint16_t* cur, const uint16_t* const* refs, int nrefs,
                       const vame_mc_bicu* cus, int max_cus, const int32_t* ncus_dev, float lambda, int rounds,
                       vame_mc_bicu* out, int64_t* cost, int32_t* bad, void* stream) {
  return refine_cus(c, cur, refs, nrefs, cus, max_cus, ncus_dev, lambda, &BiRefineParams::rounds, rounds, 4, out, cost, bad,
                    birefine_launch, stream);
}

int vame_seed_search(vame_ctx* c, const uint16_t* cur, const uint16_t* const* refs, int nrefs, float lambda,
                     int align_mask, int radius, const vame_seed_result* out, void* stream) {
  if (!c || !cur || !refs || !out || nrefs < 1 || nrefs > 4) return VAME_E_INVALID;
  if ((align_mask & ~3) || !align_mask || radius < 0 || radius > kSeedMaxRadius) return VAME_E_INVALID;
  // the kernel reads block rows of cur as 8-byte words and reference rows as dwords
  if (reinterpret_cast<uintptr_t>(cur) & 7) return VAME_E_INVALID;
  SeedParams p;
  memset(&p, 0, sizeof(p));  // levels 0, no pyramids
  return seed_search(c, p, cur, refs, nrefs, lambda, align_mask, radius, out, stream);
}

size_t vame_seed_pyramid_bytes(vame_ctx* c) { return c ? 2 * pyr_samples(c->W, c->H) : 0; }

int vame_seed_pyramid(vame_ctx* c, const uint16_t* frame, uint16_t* pyr, void* stream) {
  if (!c || !frame || !pyr) return VAME_E_INVALID;
  // the kernel reads frame rows as dwords and stores level-1 rows as 8-byte words
  if ((reinterpret_cast<uintptr_t>(frame) & 3) || (reinterpret_cast<uintptr_t>(pyr) & 7)) return VAME_E_INVALID;
  DeviceGuard guard(c->device);
  VAME_HIP(guard.err);
  SeedPyrDownParams p;
  p.frame = frame;
  p.pyr = pyr;
  p.W = c->W;
  p.H = c->H;
  VAME_HIP(seed_pyr_down_launch(p, (hipStream_t)stream));
  return VAME_OK;
}

int vame_seed_search_wide(vame_ctx* c, const uint16_t* cur, const uint16_t* cur_pyr, const uint16_t* const* refs,
                          const uint16_t* const* ref_pyrs, int nrefs, float lambda, int align_mask, int radius,
                          int levels, const vame_seed_result* out, void* stream) {
  if (!c || !cur || !cur_pyr || !refs || !ref_pyrs || !out || nrefs < 1 || nrefs > 4) return VAME_E_INVALID;
  if ((align_mask & ~3) || !align_mask || radius < 0 || radius > kSeedWideMaxRadius || levels < 1 ||
      levels > kSeedWideMaxLevels)
    return VAME_E_INVALID;
  // the kernels read block rows of cur and of the pyramids as 8-byte words and reference rows as dwords
  if ((reinterpret_cast<uintptr_t>(cur) | reinterpret_cast<uintptr_t>(cur_pyr)) & 7) return VAME_E_INVALID;
  SeedParams p;
  memset(&p, 0, sizeof(p));
  // all pyramids before refs and the output mask (once per reference in between them): every one of
  // these returns VAME_E_INVALID before anything is launched, so the order cannot be seen
  for (int r = 0; r < nrefs; r++) {
    if (!ref_pyrs[r] || (reinterpret_cast<uintptr_t>(ref_pyrs[r]) & 7)) return VAME_E_INVALID;
    p.refPyrs[r] = ref_pyrs[r];
  }
  p.curPyr = cur_pyr;
  p.levels = levels;
  return seed_search(c, p, cur, refs, nrefs, lambda, align_mask, radius, out, stream);
}

int vame_affine_search(vame_ctx* c, const uint16_t* cur, const uint16_t* const* refs, int nrefs,
                       const vame_mc_cu* cus, int max_cus, const int32_t* ncus_dev, float lambda,
                       int extra_grad_iter, vame_mc_cu* out, int64_t* cost, int32_t* bad, void* stream) {
  return refine_cus(c, cur, refs, nrefs, cus, max_cus, ncus_dev, lambda, &SearchParams::extra, extra_grad_iter, 64, out,
                    cost, bad, search_launch, stream);
}

size_t vame_seeded_work_bytes(vame_ctx* c, int nrefs, int mode_mask) {
  int begin, end;
  if (!c || nrefs < 1 || nrefs > 4 || !seeded_range(c, mode_mask, begin, end)) return 0;
  return seeded_work_bytes((size_t)nrefs * (end - begin), (mode_mask & VAME_MODE_3CP) != 0);
}

int vame_affine_me_seeded(vame_ctx* c, const uint16_t* cur, const uint16_t* const* refs, int nrefs, float lambda,
                          int mode_mask, int extra_grad_iter, vame_mv* const seed_mv[4][2],
                          const vame_poc_result* res, void* work, size_t work_bytes, int32_t* bad, void* stream) {
  return affine_me_seeded(c, cur, refs, nrefs, lambda, mode_mask, extra_grad_iter, seed_mv, nullptr, res, work,
                          work_bytes, bad, stream);
}

// ---- rates against a predictor
int vame_affine_mc_bi_p(vame_ctx* c, const uint16_t* cur, const uint16_t* const* refs, int nrefs,
                        const vame_mc_bicu* cus, const vame_cpmvs* preds, int max_cus, const int32_t* ncus_dev,
                        float lambda, uint16_t* pred, int64_t* cost, int32_t* bad, void* stream) {
  return affine_mc(c, cur, refs, nrefs, cus, max_cus, ncus_dev, lambda, pred, cost, bad, stream, preds);
}

int vame_affine_search_p(vame_ctx* c, const uint16_t* cur, const uint16_t* const* refs, int nrefs,
                         const vame_mc_cu* cus, const vame_cpmvs* preds, int max_cus, const int32_t* ncus_dev,
                         float lambda, int extra_grad_iter, vame_mc_cu* out, int64_t* cost, int32_t* bad,
                         void* stream) {
  return refine_cus(c, cur, refs, nrefs, cus, max_cus, ncus_dev, lambda, &SearchParams::extra, extra_grad_iter, 64, out,
                    cost, bad, with_preds(preds, search_launch, search_p_launch), stream);
}

int vame_bipred_refine_p(vame_ctx* c, const uint16_t* cur, const uint16_t* const* refs, int nrefs,
                         const vame_mc_bicu* cus, const vame_cpmvs* preds, int max_cus, const int32_t* ncus_dev,
                         float lambda, int rounds, vame_mc_bicu* out, int64_t* cost, int32_t* bad, void* stream) {
  return refine_cus(c, cur, refs, nrefs, cus, max_cus, ncus_dev, lambda, &BiRefineParams::rounds, rounds, 4, out, cost,
                    bad, with_preds(preds, birefine_launch, birefine_p_launch), stream);
}

int vame_reprice(vame_ctx* c, int nrefs, float lambda, int pred_mask, const vame_mvp* mvp, const vame_poc_result* res,
                 int32_t* bad, void* stream) {
  if (!c || !mvp || !res || !bad || nrefs < 1 || nrefs > 4) return VAME_E_INVALID;
  if ((pred_mask & ~15) || !pred_mask) return VAME_E_INVALID;
  RepriceParams p;
  memset(&p, 0, sizeof(p));
  if (!set_result(p.cost, p.cpmv, res, nrefs, pred_mask)) return VAME_E_INVALID;
  if (!set_mvp(p.mvp, mvp, nrefs, pred_mask)) return VAME_E_INVALID;
  DeviceGuard guard(c->device);
  VAME_HIP(guard.err);
  p.cands = c->biCands;
  p.candBegin = (pred_mask & 3) ? 0 : c->biNCand[0];
  p.candEnd = (pred_mask & 12) ? c->biNCand[0] + c->biNCand[1] : c->biNCand[0];
  p.bad = bad;
  p.nrefs = nrefs;
  p.lambda = lambda;
  VAME_HIP(reprice_launch(p, (hipStream_t)stream));
  return VAME_OK;
}

size_t vame_seeded_p_work_bytes(vame_ctx* c, int nrefs, int mode_mask) {
  int begin, end;
  if (!c || nrefs < 1 || nrefs > 4 || !seeded_range(c, mode_mask, begin, end)) return 0;
  return seeded_p_work_bytes((size_t)nrefs * (end - begin), (mode_mask & VAME_MODE_3CP) != 0);
}

int vame_affine_me_seeded_p(vame_ctx* c, const uint16_t* cur, const uint16_t* const* refs, int nrefs, float lambda,
                            int mode_mask, int extra_grad_iter, vame_mv* const seed_mv[4][2], const vame_mvp* mvp,
                            const vame_poc_result* res, void* work, size_t work_bytes, int32_t* bad, void* stream) {
  if (!mvp) return VAME_E_INVALID;
  return affine_me_seeded(c, cur, refs, nrefs, lambda, mode_mask, extra_grad_iter, seed_mv, mvp, res, work,
                          work_bytes, bad, stream);
}

int vame_bipred_p(vame_ctx* c, const uint16_t* cur, const uint16_t* const* refs, int nrefs, float lambda,
                  const vame_poc_result* res, int pred_mask, const vame_mvp* mvp, int64_t* const bi_cost[2],
                  int32_t* const bi_sel[2], void* stream) {
  if (!mvp) return VAME_E_INVALID;
  return bipred(c, cur, refs, nrefs, lambda, res, pred_mask, mvp, bi_cost, bi_sel, stream);
}

int vame_mvp_gather(vame_ctx* c, const vame_mvp* mvp, const vame_mc_bicu* cus, int max_cus, const int32_t* ncus_dev,
                    vame_cpmvs* preds, void* stream) {
  if (!c || !mvp || !cus || !preds || max_cus < 0 || max_cus > VAME_MC_MAX_CUS) return VAME_E_INVALID;
  if (max_cus == 0) return VAME_OK;
  DeviceGuard guard(c->device);
  VAME_HIP(guard.err);
  MvpGatherParams p;
  memset(&p, 0, sizeof(p));
  for (int r = 0; r < 4; r++)
    for (int a = 0; a < 2; a++) p.mvp[r][a] = reinterpret_cast<const int32_t*>(mvp->mv[r][a]);
  p.cus = reinterpret_cast<const McBiCu*>(cus);
  p.preds = reinterpret_cast<int32_t*>(preds);
  p.ncusDev = ncus_dev;
  p.maxCus = max_cus;
  p.ctusPerRow = c->ctusPerRow;
  p.nCtus = c->nCtus;
  VAME_HIP(mvp_gather_launch(p, (hipStream_t)stream));
  return VAME_OK;
}

}  // extern "C"

/*
 * vame.h -- C ABI of the MI355X affine motion-estimation engine (libvame.so).
 *
 * Drop-in boundary for the reference's hot path (iagostorch/VVC-Affine-GPU):
 * what the reference host does with clSetKernelArg + clEnqueueNDRangeKernel on
 *   affine_gradient_mult_sizes     (affine.cl:11,  aligned CUs)      and
 *   affine_gradient_mult_sizes_HA  (affine.cl:960, half-aligned CUs)
 * compiled with -DnCP=2|3 (main.cpp:389-392) and launched at main.cpp:827-966
 * is one call of vame_affine_me() here.  The gradient / equation scratch
 * buffers of the reference signature (args 5-7) and its unused debug args
 * (11-12) disappear: all scratch lives in LDS and registers.
 *
 * Plain pointers and sizes only.  Frame / result pointers are DEVICE pointers
 * (hipMalloc'd or torch.cuda tensors) unless a function says otherwise; every
 * call is asynchronous on `stream` (a hipStream_t, NULL = default stream).
 * Results use the reference's return-array layout (affine.cl:936, :1929):
 *   index = ctu * {201 | 284} + RETURN_STRIDE[group] + cuIdx
 * so the host's decision-log writer (main_aux_functions.h:387-525) is unchanged.
 * A context is bound to one device and is not thread-safe; use one per GPU per
 * host thread.  Functions return 0 or a negative VAME_E* code.
 */
#ifndef VAME_H
#define VAME_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* typedef.h:1-8 Mv / Cpmvs, same 28-byte layout.  1/16-pel units. */
typedef struct { int32_t x, y; } vame_mv;
typedef struct { int32_t nCPs; vame_mv LT, RT, LB; } vame_cpmvs;

enum { VAME_ALIGN_FULL = 0, VAME_ALIGN_HALF = 1 };
/* mode_mask bits of the fused calls: 2CP (required), 3CP (seeded by 2CP), and
 * an optional alignment selection -- FULL and/or HALF; neither bit = both, as
 * the reference codes them (the vame CLI's --align) */
enum { VAME_MODE_2CP = 1, VAME_MODE_3CP = 2, VAME_MODE_FULL = 4, VAME_MODE_HALF = 8 };
/* The PREDs (bit m = FULL_2CP, FULL_3CP, HALF_2CP, HALF_3CP) a valid mode_mask
 * codes: the vame_poc_result entries it writes, the log files it feeds. */
int vame_pred_mask(int mode_mask);

enum {
  VAME_OK = 0,
  VAME_E_INVALID = -1,     /* bad argument (resolution, nCP, align, null pointer ...) */
  VAME_E_DEVICE = -2,      /* HIP runtime error (see vame_last_hip_error) */
  VAME_E_NOMEM = -3,
  VAME_E_UNSUPPORTED = -4  /* e.g. more than 4 reference frames */
};

typedef struct vame_ctx vame_ctx;

/* Output slots of the fused per-POC call: [ref][FULL_2CP, FULL_3CP, HALF_2CP, HALF_3CP].
 * cost/cpmvs of slot (r, m) must hold nCtus*{201|284} entries (or be NULL when the
 * mode is not requested).  Mirrors the four return_* memory objects per refIdx
 * of main.cpp:484-504. */
typedef struct {
  int64_t* cost[4][4];
  vame_cpmvs* cpmvs[4][4];
} vame_poc_result;

/* Create a context on HIP device `device` for frames of width x height (one of
 * the reference's resolutions: constants.h:73-79 / main.cpp:257-265).
 * Every device buffer the launches use is allocated here (the reference
 * allocates its buffers before the POC loop, main.cpp:473-552), among them the
 * 3-CP seed-reuse scratch for 32 pairs per launch (~1 GB at 3840x2160; see
 * vame_set_max_pairs): no launch allocates, so a call may be captured into a
 * hipGraph on the caller's stream.  Runtime knobs, read here (results are
 * bit-identical under every setting; the defaults are the measured best on
 * MI355X):
 *   VAME_STREAMS       2 (default): the quadrant kernel on a side stream of the
 *                      context, forked from and joined into the caller's stream;
 *                      1: every kernel on the caller's stream
 *   VAME_SYNC          1 (default): the join as a stream memory operation;
 *                      0: an event
 *   VAME_GROUP_COMBOS  (CTU, pair) combinations per block-order group (408) */
int vame_create(vame_ctx** out, int device, int width, int height);
void vame_destroy(vame_ctx* ctx);
/* (POC, refIdx) pairs per launch of the fused calls, 1..32 (default 32): the
 * seed-reuse scratch is re-sized for it (synchronizes the device; outside any
 * capture), batches are cut into launches of at most that many pairs.  A
 * caller coding a few pairs per call (the CLI: one POC, <= 4 pairs) keeps the
 * scratch at 1/8 of the default.  vame_get_max_pairs returns the setting. */
int vame_set_max_pairs(vame_ctx* ctx, int max_pairs);
int vame_get_max_pairs(vame_ctx* ctx);

/* One reference launch (affine.cl:11 or :960 built with -DnCP=nCP).
 *   ref, cur : W*H uint16 samples (10-bit), device memory
 *   lambda   : motion lambda (float kernel arg 4, main.cpp:585/831)
 *   prev     : nCP==3 only: the same-alignment 2-CP result of this (POC, ref)
 *              (gPrevCpmvs, main.cpp:777/908); NULL for nCP==2
 *   cost     : nCtus*{201|284} int64 best RD cost per candidate CU
 *   cpmvs    : same count, best CPMVs (LB = 0 for 2 CPs)                       */
int vame_affine_me(vame_ctx* ctx, const uint16_t* ref, const uint16_t* cur, float lambda,
                   int align, int nCP, int extra_grad_iter, const vame_cpmvs* prev,
                   int64_t* cost, vame_cpmvs* cpmvs, void* stream);

/* Fused per-POC call: every ref x {FULL, HALF} x {2CP -> 3CP} in one pass
 * (the whole refIdx loop of main.cpp:746-966).  3-CP seeds come from the 2-CP
 * result of the same CU inside the kernel (no round trip through memory). */
int vame_affine_me_poc(vame_ctx* ctx, const uint16_t* cur, const uint16_t* const* refs,
                       int nrefs, float lambda, int mode_mask, int extra_grad_iter,
                       const vame_poc_result* out, void* stream);

/* Batched fused call: several POCs (each one vame_affine_me_poc) in as few
 * launches as possible (vame_get_max_pairs() (POC, refIdx) pairs per launch,
 * default 32), so consecutive
 * POCs share one grid -- no launch gaps or tails between them.  Results are
 * identical to one vame_affine_me_poc per job. */
typedef struct {
  const uint16_t* cur;              /* orig of the POC */
  const uint16_t* const* refs;      /* its nrefs (1..4) reference frames, refIdx order */
  int nrefs;
  float lambda;
  const vame_poc_result* out;
} vame_poc_job;
int vame_affine_me_batch(vame_ctx* ctx, const vame_poc_job* jobs, int njobs, int mode_mask,
                         int extra_grad_iter, void* stream);

/* The compact wire form of the jobs' decision records, for the frame-shard
 * gather into rank 0 (vame/shard.py pack() is its
 * specification): for each job in order, refIdx 0..nrefs-1, each PRED of
 * vame_pred_mask(mode_mask) in PRED order: the nCtus*{201|284} costs as
 * int32, then the records' CPMV components (LT, RT, and LB for 3-CP: 4 or 6
 * int32 each).  `slab` (device, `words` int32) is zero-filled past the
 * records; `*bad` (device int32) is OR-ed with 1 when a record does not fit
 * the form (cost outside [0, 2^31), 2-CP LB != 0).  One kernel on `stream`;
 * the jobs' cur / refs / lambda are not read.  VAME_E_INVALID when the records
 * exceed `words`. */
int vame_pack_records(vame_ctx* ctx, const vame_poc_job* jobs, int njobs, int mode_mask, int32_t* slab,
                      long long words, int32_t* bad, void* stream);

/* Affine motion compensation: the prediction and / or the cost of CPMVs the
 * caller already has (a chosen CU's winner, merge or inherited candidates),
 * computed exactly as one prediction step of the search computes them.
 * A descriptor (12 int32, device memory) is a CU at frame position (x, y) of
 * size w x h, predicted from frame refs[ref] with the CPMVs cp: cp.nCPs = 2 or
 * 3 selects the 4- or 6-parameter model (LB is ignored for 2).  Every 4x4
 * sub-block: sub-block MV and spread test, roundAndClipMv against the CU
 * position, clamp-to-edge window, 6-tap filter with the reference's rounding
 * and clipPel (aux_functions.cl:146-212, :90-101, affine.cl:254-326,
 * aux_functions.cl:1096-1239); PROF as vame_set_prof sets it, where the search
 * applies it (the spread test passes).
 *   pred : W*H device frame or NULL: receives the samples of the valid
 *          descriptors' CUs and nothing else (where two CUs overlap, a sample
 *          holds the result of one of them)
 *   cost : ncus int64 (device) or NULL: sum of satd_4x4 against `cur` over the
 *          CU + floor(lambda * (bits + 2)), the search's cost with its zero
 *          predictor and ruiBits = 2 (affine.cl:416-446); lambda = 0: the SATD
 *   bad  : device int32, OR-ed with 1 when a descriptor is invalid
 * At least one of pred and cost is given; cur may be NULL when cost is.
 * A valid descriptor has w, h in {16, 32, 64, 128}; x, y >= 0 and multiples
 * of 4; x + w <= W, y + h <= H; 0 <= ref < nrefs; nCPs in {2, 3}; every used
 * CPMV component in [-2^17, 2^17 - 1] (the range the search clamps to).  An
 * invalid one writes nothing to pred, gets cost 0, sets bit 0 of *bad and does
 * not disturb the others.
 * The descriptors are not read on the host; the call allocates and
 * synchronizes nothing and runs on `stream` alone (never the side stream), so
 * it can be captured into a hipGraph.  Its offset table is the context's:
 * calls on one context must be ordered one after the other (one stream, or
 * events between streams).  ncus <= VAME_MC_MAX_CUS; ncus = 0 is a no-op.
 * Frames are 8-byte aligned (refs: 4).  Argument errors: VAME_E_INVALID. */
typedef struct { int32_t x, y, w, h, ref; vame_cpmvs cp; } vame_mc_cu;
enum { VAME_MC_MAX_CUS = 1 << 20 };
int vame_affine_mc(vame_ctx* ctx, const uint16_t* cur, const uint16_t* const* refs, int nrefs,
                   const vame_mc_cu* cus, int ncus, float lambda, uint16_t* pred, int64_t* cost,
                   int32_t* bad, void* stream);

/* vame_affine_mc on the first min(*ncus_dev, max_cus) descriptors, the count
 * read on the device (a negative count is 0): descriptors and cost entries
 * past it are neither read nor written.  The launches are sized from max_cus
 * (<= VAME_MC_MAX_CUS; 0 is a no-op); every other guarantee of vame_affine_mc
 * holds -- the partner of vame_partition, whose leaf count stays on the device. */
int vame_affine_mc_dev(vame_ctx* ctx, const uint16_t* cur, const uint16_t* const* refs, int nrefs,
                       const vame_mc_cu* cus, int max_cus, const int32_t* ncus_dev, float lambda,
                       uint16_t* pred, int64_t* cost, int32_t* bad, void* stream);

/* CU partition decision: per CTU the cheapest tiling by candidate CUs of the
 * search's results of one POC, under VVC-style binary and ternary splits, and
 * for every leaf its best (refIdx, 2-CP | 3-CP) candidate; the leaves come out
 * as descriptors for vame_affine_mc(_dev).  The rule:
 *   node   a CTU-relative rectangle (x, y, w, h), w, h in {16, 32, 64, 128},
 *          x, y multiples of 16, inside the CTU; at frame position (X, Y)
 *   value  X >= W or Y >= H: 0, nothing emitted.  A 16x16 node crossing the
 *          frame edge (the last 8 rows at 1080p): 0, a hole.  Else the first
 *          minimum, under strict <, of leaf, BT-H, BT-V, TT-H, TT-V:
 *   leaf   only a node wholly in the frame that is a candidate CU of a PRED in
 *          pred_mask: min of cost[r][m][ctu*{201|284} + offset] over
 *          r = 0..nrefs-1 (outer) and m = 2-CP, 3-CP (inner), first minimum
 *   split  split_penalty + the children's values (top to bottom / left to
 *          right): BT-H two (w, h/2), h >= 32; BT-V two (w/2, h), w >= 32;
 *          TT-H (w, h/4) (w, h/2) (w, h/4), h >= 64; TT-V the same in x; the TT
 *          splits only with a HALF PRED in the mask
 * Half-aligned candidates at an odd multiple of 8 are no nodes and never leaves.
 *   res        device pointers; entries of PREDs outside pred_mask may be NULL
 *   pred_mask  bits of vame_pred_mask(); at least one FULL PRED (so that every
 *              CTU has a tiling)
 *   split_penalty  0 .. 2^40
 *   cus        nCtus*64 descriptors: frame x, y, w, h, ref, cp = the chosen
 *              row's CPMVs with nCPs = 2 or 3.  CTUs ascending, a CTU's leaves
 *              in raster order of their top-left 16x16 block
 *   rows       or NULL: the row's index in its PRED array (PRED = 2*align + nCPs - 2)
 *   ncus       device int32: the total number of leaves; entries of cus / rows
 *              at or past it are not written
 *   ctu_info   or NULL, [nCtus][4]: first leaf, leaves, holes, splits
 *   ctu_cost   or NULL, [nCtus]: the root's value (split penalties included)
 *   block_cu   or NULL, [nCtus*64] at ctu*64 + (y/16)*8 + x/16: the index into
 *              cus of the leaf that covers the block, or -1
 * Reads nothing on the host, allocates and synchronizes nothing, runs on
 * `stream` alone and can be captured.  Its scratch is the context's: calls on
 * one context are ordered one after the other.  Argument errors (nrefs outside
 * 1..4, no FULL bit, a NULL array of a PRED in the mask, a penalty outside the
 * range, NULL cus / ncus): VAME_E_INVALID, nothing written. */
int vame_partition(vame_ctx* ctx, const vame_poc_result* res, int nrefs, int pred_mask,
                   int64_t split_penalty, vame_mc_cu* cus, int32_t* rows, int32_t* ncus,
                   int32_t* ctu_info, int64_t* ctu_cost, int32_t* block_cu, void* stream);
/* The rule's candidate map (no device work): slot ((lh*4 + lw)*8 + y/16)*8 + x/16,
 * lw = log2(w/16), lh = log2(h/16), of table[1024] holds align*512 + the
 * candidate's output offset (RETURN_STRIDE[group] + cuIdx), or -1. */
int vame_partition_table(int32_t* table);

/* ---- Affine bi-prediction: a CU predicted as the average of
 * two hypotheses from two reference frames.  A hypothesis is one prediction of
 * vame_affine_mc up to its second-stage accumulator acc = sum + 512 +
 * (8192 << 6), whose uni sample is clip(acc >> 10); the bi sample is
 *   clip((acc0 + acc1) >> 11, 0, 1023)
 * (the unrounded values summed, one rounding; two identical hypotheses give
 * the uni sample), and the bi cost the sum of satd_4x4 of the bi block against
 * `cur` + floor(lambda * (bits(cp0) + bits(cp1) + 4)): each hypothesis carries
 * its own ruiBits = 2.  PROF has no bi form: while vame_set_prof(ctx, 1) is in
 * force the three calls return VAME_E_UNSUPPORTED and write nothing. */

/* first 12 int32 are a vame_mc_cu; ref1 < 0: uni-predicted from (ref0, cp0) */
typedef struct { int32_t x, y, w, h, ref0; vame_cpmvs cp0; int32_t ref1; vame_cpmvs cp1; } vame_mc_bicu; /* 80 B */

/* vame_affine_mc_dev on bi descriptors: the first min(*ncus_dev, max_cus) of
 * them (ncus_dev NULL: max_cus).  vame_affine_mc's validity rules hold per
 * hypothesis; ref1 == -1 is the only negative value allowed (cp1 is then not
 * read, samples and cost equal vame_affine_mc's bit for bit), ref1 == ref0 is
 * allowed.  Every guarantee of vame_affine_mc(_dev) carries over: an invalid
 * descriptor writes nothing, costs 0 and sets *bad; descriptors and costs at
 * or past the count are untouched; nothing is read on the host, allocated or
 * synchronized; `stream` alone, capturable; the context's offset table (calls
 * on one context are ordered one after the other); max_cus <= VAME_MC_MAX_CUS. */
int vame_affine_mc_bi(vame_ctx* ctx, const uint16_t* cur, const uint16_t* const* refs, int nrefs,
                      const vame_mc_bicu* cus, int max_cus, const int32_t* ncus_dev, float lambda,
                      uint16_t* pred, int64_t* cost, int32_t* bad, void* stream);

/* The best reference pair of every candidate CU of the search's results `res`
 * of one POC.  For every alignment a with a PRED in pred_mask and every row
 * whose CU lies wholly in the frame: the hypothesis of refIdx r is the first
 * minimum under strict < over m = 2-CP, 3-CP of cost[r][2a + m][row] among the
 * PREDs in the mask, with that row's CPMVs; the candidates are the pairs
 * r0 < r1 in the order (0,1) (0,2) (0,3) (1,2) (1,3) (2,3);
 *   bi_cost[a][row]  the first minimum of the bi cost over the pairs
 *   bi_sel[a][row]   r0 + 4*m0 + 8*r1 + 32*m1 of that pair
 * Rows of CUs that leave the frame get INT64_MAX and -1; with nrefs == 1 every
 * row does.  bi_cost[a] / bi_sel[a]: nCtus*{201|284} entries (device), NULL
 * allowed for an alignment without a PRED in the mask.  Every entry is written
 * by the call's kernels (no host memset); integer sums: identical from run to
 * run.  Reads nothing on the host, allocates and synchronizes nothing, runs on
 * `stream` alone and can be captured; its scratch is the context's.  Argument
 * errors (nrefs outside 1..4, an empty or unknown mask, a NULL array of a PRED
 * in the mask, NULL outputs of an alignment in the mask): VAME_E_INVALID,
 * nothing written. */
int vame_bipred(vame_ctx* ctx, const uint16_t* cur, const uint16_t* const* refs, int nrefs, float lambda,
                const vame_poc_result* res, int pred_mask, int64_t* const bi_cost[2], int32_t* const bi_sel[2],
                void* stream);

/* vame_partition with a leaf that may be bi-predicted: the leaf value is the
 * first minimum, under strict <, of the uni leaf minimum of vame_partition and
 * bi_cost[a][row] + bi_penalty, the latter only where bi_sel[a][row] >= 0 (and
 * names hypotheses the call holds: refIdx < nrefs, PREDs in pred_mask).
 * Everything else is vame_partition's rule, word for word.
 *   bi_cost, bi_sel  vame_bipred's outputs; needed for every alignment with a
 *                    PRED in pred_mask
 *   bi_penalty       0 .. 2^40
 *   cus    nCtus*64 descriptors: a uni leaf is vame_partition's descriptor,
 *          ref1 = -1 and a zero cp1; a bi leaf holds both hypotheses
 *   rows   or NULL: the row inside its alignment's arrays
 *   sel    or NULL: bi_sel of a bi leaf, -1 of a uni leaf
 * ncus, ctu_info, ctu_cost, block_cu, the order of the leaves: vame_partition's. */
int vame_partition_bi(vame_ctx* ctx, const vame_poc_result* res, int nrefs, int pred_mask,
                      int64_t split_penalty, const int64_t* const bi_cost[2], const int32_t* const bi_sel[2],
                      int64_t bi_penalty, vame_mc_bicu* cus, int32_t* rows, int32_t* sel, int32_t* ncus,
                      int32_t* ctu_info, int64_t* ctu_cost, int32_t* block_cu, void* stream);

/* Refinement of bi-predicted CUs: one hypothesis is held, the
 * other re-estimated against what the held one leaves to explain, then the
 * roles swap.  Works on the first min(*ncus_dev, max_cus) descriptors
 * (ncus_dev NULL: max_cus; a negative count is 0); entries of cus, out and
 * cost at or past the count are neither read nor written.
 * A valid bi descriptor (vame_affine_mc_bi's rules, ref1 >= 0, ref1 == ref0
 * allowed): out[i] is the descriptor with its refined CPMVs and cost[i] its bi
 * cost, bit for bit vame_affine_mc_bi's cost of out[i].  The rule is the
 * search's iteration (oracle/vame_oracle.c:run_cu) with two references:
 *   state   best = (cp0, cp1) as given, bestCost = the bi cost of the input
 *   round   t = 0 .. rounds-1 moves hypothesis m = 1 - (t & 1) and holds
 *           f = 1 - m; both start at best.  acc_f and P_f = clip(acc_f >> 10)
 *           are taken once per round.  The moving hypothesis runs the search's
 *           loop with its own nCPs, niter = 5 (2-CP) or 4 (3-CP); for it =
 *           0 .. niter: predict it as vame_affine_mc does (acc_m, P_m); the
 *           bi cost of (curr, best[f]); under strict < against bestCost take
 *           curr as best[m]; unless it == niter, one gradient step on P_m --
 *           Sobel gradients, normal equations, solveEqual, scaleDeltaMvs, the
 *           wrapping add, clamp to +-2^17 and clipMv -- with the error term
 *           e = 2 cur - P_f - P_m.  A 2-CP hypothesis never changes its LB.
 *   rounds  0 .. 4; 0 copies the descriptors and returns their costs
 * The cost never rises.  A uni descriptor (ref1 == -1) is copied through with
 * its uni cost; an invalid one is copied through, costs 0 and ORs 1 into *bad.
 * out may be cus; cost holds max_cus entries.  All sums are integer or run in
 * solveEqual's fixed order: identical from run to run.
 * Reads nothing on the host, allocates and synchronizes nothing, runs on
 * `stream` alone and can be captured.  It uses no scratch of the context:
 * calls on one context need no ordering among themselves.  Frames are 8-byte
 * aligned (refs: 4).  While vame_set_prof(ctx, 1) is in force:
 * VAME_E_UNSUPPORTED, nothing written.  Argument errors (NULL cur, refs, cus,
 * out, cost or bad; nrefs outside 1..4; rounds outside 0..4; max_cus outside
 * 0..VAME_MC_MAX_CUS; a misaligned frame): VAME_E_INVALID, nothing written.
 * max_cus = 0 is a no-op. */
int vame_bipred_refine(vame_ctx* ctx, const uint16_t* cur, const uint16_t* const* refs, int nrefs,
                       const vame_mc_bicu* cus, int max_cus, const int32_t* ncus_dev, float lambda,
                       int rounds, vame_mc_bicu* out, int64_t* cost, int32_t* bad, void* stream);

/* ---- Seeding the affine search.  The search starts every
 * 2-CP candidate at zero CPMVs and follows motion of a few samples; these
 * calls give it the translational start an encoder has.  All three read
 * nothing on the host, allocate and synchronize nothing, run on `stream` alone
 * (never the side stream) and can be captured; every output entry is written
 * by the call's kernels; all sums are integer or run in solveEqual's fixed
 * order: identical from run to run. */

/* The best integer displacement of every candidate CU.  For every r < nrefs,
 * every alignment in align_mask (bit 0 FULL, bit 1 HALF) and every row
 * ctu*{201|284} + offset, whose CU is (x, y, w, h) at frame position:
 *   CU not wholly in the frame: mv = (0, 0), cost = INT64_MAX.
 *   candidates  integer d = (dx, dy), |dx|, |dy| <= radius, dx <= W+7-x and
 *               dy <= H+7-y: the displacements whose MV (16dx, 16dy) clipMv
 *               leaves unchanged at the CU's position
 *   value       SAD(d) + floor(lambda * (bits + 2)): SAD(d) = sum |cur[y+j][x+i]
 *               - ref[clamp(y+dy+j, 0, H-1)][clamp(x+dx+i, 0, W-1)]|, bits = the
 *               search's bits of the 2-CP CPMVs LT = RT = (16dx, 16dy) -- the
 *               block is vame_affine_mc's prediction of those CPMVs, the rate
 *               the search's rate of them
 *   selection   mv = (16dx, 16dy) of the first minimum under strict <, in the
 *               order (0, 0), then dy = -radius..radius (outer), dx =
 *               -radius..radius (inner); cost = that value
 * radius 0..32 (0: mv 0 and the value of (0, 0)).  mv / cost of (r, alignment):
 * nCtus*{201|284} entries (device); entries outside the mask may be NULL and
 * are not touched.  PROF does not enter.  Argument errors (nrefs outside 1..4,
 * an empty or unknown mask, a radius outside 0..32, a NULL output of an
 * (r, alignment) in the mask, a misaligned frame: cur 8 bytes, refs 4):
 * VAME_E_INVALID, nothing written. */
typedef struct { vame_mv* mv[4][2]; int64_t* cost[4][2]; } vame_seed_result;   /* [ref][align] */
int vame_seed_search(vame_ctx* ctx, const uint16_t* cur, const uint16_t* const* refs, int nrefs,
                     float lambda, int align_mask, int radius, const vame_seed_result* out, void* stream);

/* The same seeds over a wide range, coarse to fine on a picture pyramid
 * (DESIGN.md §16).  Level 0 of a frame is the frame; level l+1 at (x, y) is
 * (a + b + c + d + 2) >> 2 of level l's samples at (2x, 2y), (2x+1, 2y),
 * (2x, 2y+1), (2x+1, 2y+1); level l is (W >> l) x (H >> l).
 * vame_seed_pyramid writes levels 1 and 2 of `frame` into pyr: caller memory
 * (device, 8-byte aligned) of vame_seed_pyramid_bytes = 2*((W/2)*(H/2) +
 * (W/4)*(H/4)) bytes (0 for a NULL context), level 1 directly followed by
 * level 2, both dense and row-major.  A frame's pyramid is built once and
 * reused for as long as the frame serves as cur or as a reference.  Argument
 * errors (NULL, frame not 4-byte or pyr not 8-byte aligned): VAME_E_INVALID,
 * nothing written.
 *
 * vame_seed_search_wide: outputs, masks, NULL rules and row layout as
 * vame_seed_search; cur_pyr / ref_pyrs[r] are the pyramids of cur / refs[r].
 * A row whose CU (x, y, w, h) is not wholly in the frame: mv = (0, 0), cost =
 * INT64_MAX.  For the others, with L = levels:
 *   displacement  d = (dx, dy) at level l stands for D = (dx << l, dy << l)
 *   admissible    |Dx|, |Dy| <= radius, Dx <= W+7-x and Dy <= H+7-y; a
 *                 candidate that is not admissible is never taken
 *   value_l(d)    (SAD_l(d) << 2l) + floor(lambda * (bits + 2)): SAD_l over the
 *                 block (x>>l, y>>l, w>>l, h>>l) of level l of cur against
 *                 level l of the reference at the displaced position,
 *                 coordinates clamped to [0, (W>>l)-1] x [0, (H>>l)-1]; bits =
 *                 the search's bits of the 2-CP CPMVs LT = RT = (16Dx, 16Dy).
 *                 value_0 is vame_seed_search's value
 *   level L       candidates d in [-Rc, Rc]^2, Rc = radius >> L; the first
 *                 minimum under strict < in the order (0, 0), then dy outer,
 *                 dx inner
 *   level l < L   (L-1 down to 0) centre c = 2 * (the winner of level l+1);
 *                 candidates in order: at level 0 only D = (0, 0); then c;
 *                 then c + (ex, ey), ey = -1, 0, 1 (outer), ex = -1, 0, 1
 *                 (inner) without (0, 0); the first minimum under strict <
 *   output        mv = (16Dx, 16Dy) of level 0's winner, cost = its value_0:
 *                 what vame_seed_search assigns to that displacement, and
 *                 never above the value of (0, 0)
 * radius 0..128 (0: mv 0 and the value of (0, 0)), levels 1..2.  Reads nothing
 * on the host, allocates and synchronizes nothing, runs on `stream` alone and
 * can be captured; every output entry of an (r, alignment) in the mask is
 * written by the call's kernels; integer sums only.  PROF does not enter.
 * Argument errors (nrefs outside 1..4, an empty or unknown mask, radius or
 * levels out of range, a NULL pyramid, a NULL output of an (r, alignment) in
 * the mask, cur or a pyramid not 8-byte aligned, a reference not 4-byte
 * aligned): VAME_E_INVALID, nothing written. */
size_t vame_seed_pyramid_bytes(vame_ctx* ctx);
int vame_seed_pyramid(vame_ctx* ctx, const uint16_t* frame, uint16_t* pyr, void* stream);
int vame_seed_search_wide(vame_ctx* ctx, const uint16_t* cur, const uint16_t* cur_pyr,
                          const uint16_t* const* refs, const uint16_t* const* ref_pyrs, int nrefs,
                          float lambda, int align_mask, int radius, int levels,
                          const vame_seed_result* out, void* stream);

/* The search's iteration from caller-given CPMVs, on a CU list: the first
 * min(*ncus_dev, max_cus) descriptors (ncus_dev NULL: max_cus; a negative
 * count is 0); entries at or past the count are neither read nor written.
 * A valid descriptor (vame_affine_mc's rules): oracle/vame_oracle.c:run_cu
 * with init = its CPMVs, nCP = its nCPs, niter = (5 | 4) + extra_grad_iter,
 * PROF off; out[i] is the descriptor with the best CPMVs and cost[i] its cost,
 * bit for bit vame_affine_mc's cost of out[i].  Iteration 0's cost always
 * becomes the best; a 2-CP descriptor keeps its LB as given.  An invalid
 * descriptor is copied through, costs 0 and ORs 1 into *bad.  out may be cus.
 * It uses no scratch of the context.  extra_grad_iter 0..64.  While
 * vame_set_prof(ctx, 1) is in force: VAME_E_UNSUPPORTED, nothing written.
 * Argument errors as vame_bipred_refine's. */
int vame_affine_search(vame_ctx* ctx, const uint16_t* cur, const uint16_t* const* refs, int nrefs,
                       const vame_mc_cu* cus, int max_cus, const int32_t* ncus_dev, float lambda,
                       int extra_grad_iter, vame_mc_cu* out, int64_t* cost, int32_t* bad, void* stream);

/* Improve a POC's search results in place from seeds.  res holds the results
 * of vame_affine_me_poc for the same cur / refs / lambda / mode_mask / extra.
 * For every r, every alignment a in the mask and every row whose CU is wholly
 * in the frame and whose seed seed_mv[r][a][row] is not (0, 0):
 *   d2 = vame_affine_search's rule with nCPs = 2, LT = RT = seed, LB = 0;
 *   with 3-CP in the mask, d3 = that rule with nCPs = 3 from d2's best CPMVs
 *   and the LB the fused search derives from them (affine.cl:81-105);
 *   res[r][2a] takes d2's row where d2.cost < its cost, res[r][2a+1] d3's row
 *   where d3.cost < its cost: cost and CPMVs together, nCPs as the search
 *   writes it.
 * Every other row is untouched; with all seeds zero the call changes nothing.
 * Seeds need not come from vame_seed_search: any MV with components in
 * [-2^17, 2^17-1] is a start; a seed outside that range skips its row and ORs
 * 1 into *bad.  mode_mask as the fused calls take it (2-CP required).  work:
 * caller memory (device, 8-byte aligned) of at least vame_seeded_work_bytes
 * (0 for bad arguments): the descriptor lists and device counts the call
 * builds.  While PROF is on: VAME_E_UNSUPPORTED.  Argument errors:
 * VAME_E_INVALID, nothing written. */
size_t vame_seeded_work_bytes(vame_ctx* ctx, int nrefs, int mode_mask);
int vame_affine_me_seeded(vame_ctx* ctx, const uint16_t* cur, const uint16_t* const* refs, int nrefs,
                          float lambda, int mode_mask, int extra_grad_iter,
                          vame_mv* const seed_mv[4][2], const vame_poc_result* res /* in-out */,
                          void* work, size_t work_bytes, int32_t* bad, void* stream);

/* ---- Rates against a motion-vector predictor.  Every rate
 * above prices CPMVs against the all-zero predictor, the only one the
 * reference's callers pass (affine.cl:431-434); its rate function takes any
 * (calc_affine_bits, aux_functions.cl:2140-2189).  These calls expose it.  For
 * CPMVs c, a predictor P (LT, RT, LB) and n control points, with q = the
 * search's 1/16 -> 1/4 pel rounding and eg = its Exp-Golomb length:
 *   bits_p(c, P, n) = eg(q(c.LT.x) - q(P.LT.x)) + eg(q(c.LT.y) - q(P.LT.y))
 *                   + eg(q(c.RT.x) - q(P.RT.x + c.LT.x - P.LT.x)) + the same in y
 *                   + (n == 3) * [eg(q(c.LB.x) - q(P.LB.x + c.LT.x - P.LT.x)) + the same in y]
 * bits_p(c, 0, n) is the search's bits of c.  The rate term is floor(lambda *
 * (bits_p + 2)); a bi CU pays floor(lambda * (both hypotheses' bits_p + 4)).
 * Predictor components lie in [-2^17, 2^17 - 1].  The fused search
 * (vame_affine_me*) and the seed searches keep the zero predictor.
 *
 * Descriptor-list calls take `preds`, device memory: a general affine
 * predictor per hypothesis, nCPs ignored, all six components checked -- one
 * entry per vame_mc_cu, two per vame_mc_bicu (hypothesis h of descriptor i at
 * 2i + h; the second is not read when ref1 < 0).  preds == NULL is the zero
 * predictor: the call's outputs are then bit for bit its counterpart's.  A
 * predictor component out of range makes its descriptor invalid, with what
 * the counterpart does for an invalid descriptor.  Each call keeps every other
 * guarantee of its counterpart word for word: nothing read on the host,
 * allocated or synchronized; `stream` alone, capturable; the device-side
 * count; VAME_E_UNSUPPORTED under PROF; argument errors write nothing. */

/* vame_affine_mc_bi with bits_p in the cost.  The samples do not depend on the
 * predictor.  A uni descriptor (ref1 == -1) is the uni case: its cost is the
 * SATD + floor(lambda * (bits_p(cp0, preds[2i]) + 2)). */
int vame_affine_mc_bi_p(vame_ctx* ctx, const uint16_t* cur, const uint16_t* const* refs, int nrefs,
                        const vame_mc_bicu* cus, const vame_cpmvs* preds, int max_cus, const int32_t* ncus_dev,
                        float lambda, uint16_t* pred, int64_t* cost, int32_t* bad, void* stream);

/* vame_affine_search with bits_p(., preds[i]) in every iteration's cost, so
 * the predictor takes part in which iteration wins.  cost[i] is bit for bit
 * vame_affine_mc_bi_p's cost of out[i] (as a uni descriptor) with preds[i]. */
int vame_affine_search_p(vame_ctx* ctx, const uint16_t* cur, const uint16_t* const* refs, int nrefs,
                         const vame_mc_cu* cus, const vame_cpmvs* preds, int max_cus, const int32_t* ncus_dev,
                         float lambda, int extra_grad_iter, vame_mc_cu* out, int64_t* cost, int32_t* bad,
                         void* stream);

/* vame_bipred_refine with bits_p(., preds[2i + h]) for hypothesis h, in the
 * start cost and in every comparison.  The cost never rises; cost[i] is bit
 * for bit vame_affine_mc_bi_p's cost of out[i] with the same predictors. */
int vame_bipred_refine_p(vame_ctx* ctx, const uint16_t* cur, const uint16_t* const* refs, int nrefs,
                         const vame_mc_bicu* cus, const vame_cpmvs* preds, int max_cus, const int32_t* ncus_dev,
                         float lambda, int rounds, vame_mc_bicu* out, int64_t* cost, int32_t* bad, void* stream);

/* Row-layout calls take translational predictors in the seed layout, so the mv
 * arrays of a vame_seed_result can be passed as they are: the predictor of a
 * row is LT = RT = LB = mv[r][alignment][row].  An array of an (r, alignment)
 * the call uses must not be NULL (VAME_E_INVALID, nothing written). */
typedef struct { const vame_mv* mv[4][2]; } vame_mvp;   /* [ref][align], nCtus*{201|284} rows */

/* Re-price a POC's search results: for every r < nrefs, every PRED m in
 * pred_mask and every row whose CU lies wholly in the frame,
 *   cost <- cost - floor(lambda * (bits(cp) + 2)) + floor(lambda * (bits_p(cp, P, n) + 2)),
 * n = 2 + (m & 1), cp the row's CPMVs, P its predictor.  CPMVs and all other
 * rows are untouched; a row whose predictor is out of range is skipped and ORs
 * 1 into *bad.  res must hold zero-predictor costs of the same lambda (what the
 * fused search wrote): the call cannot tell, and a second call prices twice.
 * The new cost equals vame_affine_mc_bi_p's cost of the row's CPMVs with that
 * predictor; it is pure arithmetic, no prediction is made.  PROF does not
 * enter.  Reads nothing on the host, allocates and synchronizes nothing, runs
 * on `stream` alone and can be captured.  Argument errors (NULL ctx, mvp, res
 * or bad; nrefs outside 1..4; an empty or unknown mask; a NULL array of a PRED
 * or of an (r, alignment) in the mask): VAME_E_INVALID, nothing written. */
int vame_reprice(vame_ctx* ctx, int nrefs, float lambda, int pred_mask, const vame_mvp* mvp,
                 const vame_poc_result* res /* in-out, costs only */, int32_t* bad, void* stream);

/* vame_affine_me_seeded's rule with d2 and d3 run by vame_affine_search_p's
 * rule under the row's predictor (the 3-CP start still comes from
 * affine.cl:81-105).  res is expected re-priced under the same mvp
 * (vame_reprice); the merge is strict <.  A row whose predictor is out of
 * range is skipped and ORs 1 into *bad, as one whose seed is.  With an
 * all-zero mvp the call equals vame_affine_me_seeded bit for bit.  work: at
 * least vame_seeded_p_work_bytes (the seeded call's lists and one predictor
 * per slot). */
size_t vame_seeded_p_work_bytes(vame_ctx* ctx, int nrefs, int mode_mask);
int vame_affine_me_seeded_p(vame_ctx* ctx, const uint16_t* cur, const uint16_t* const* refs, int nrefs,
                            float lambda, int mode_mask, int extra_grad_iter, vame_mv* const seed_mv[4][2],
                            const vame_mvp* mvp, const vame_poc_result* res /* in-out */, void* work,
                            size_t work_bytes, int32_t* bad, void* stream);

/* vame_bipred's rule; only the bi cost changes.  The hypothesis of refIdx r is
 * still the first minimum of the given costs (which the caller has re-priced);
 * the bi cost is the SATD of the bi block + floor(lambda * (bits_p(cp0, P[r0])
 * + bits_p(cp1, P[r1]) + 4)), P[r] the row's predictor of refIdx r.  There is
 * no bad flag: a row with a predictor out of range, of any r < nrefs, keeps
 * INT64_MAX and -1. */
int vame_bipred_p(vame_ctx* ctx, const uint16_t* cur, const uint16_t* const* refs, int nrefs, float lambda,
                  const vame_poc_result* res, int pred_mask, const vame_mvp* mvp, int64_t* const bi_cost[2],
                  int32_t* const bi_sel[2], void* stream);

/* The predictors of a descriptor list, for vame_bipred_refine_p and
 * vame_affine_mc_bi_p on vame_partition_bi's leaves without a host read.  For
 * each of the first min(*ncus_dev, max_cus) descriptors (ncus_dev NULL:
 * max_cus) and each hypothesis h: if (x mod 128, y mod 128, w, h) is a
 * candidate per vame_partition_table, in a CTU of the frame, preds[2i + h] is
 * the mvp row of (ref_h, its alignment, ctu*{201|284} + offset) expanded to LT
 * = RT = LB; otherwise -- no candidate, ref_h outside 0..3 (a uni descriptor's
 * ref1), or a NULL array -- zero.  Both entries of a descriptor are written.
 * Nothing is validated here: the consuming call checks the ranges.  Reads
 * nothing on the host, allocates and synchronizes nothing, `stream` alone,
 * capturable.  Argument errors (NULL ctx, mvp, cus or preds; max_cus outside
 * 0..VAME_MC_MAX_CUS): VAME_E_INVALID, nothing written. */
int vame_mvp_gather(vame_ctx* ctx, const vame_mvp* mvp, const vame_mc_bicu* cus, int max_cus,
                    const int32_t* ncus_dev, vame_cpmvs* preds, void* stream);

/* PROF (prediction refinement with optical flow).  The reference carries the
 * code but hard-disables it (`int enablePROF=0`, affine.cl:168 / :1132;
 * aux_functions.cl:215-605, :1096-1239); enable != 0 turns it on for the
 * context's later launches (both entry points), exactly as the reference's
 * functions compute it with enablePROF = 1.  Default off = reference behaviour. */
int vame_set_prof(vame_ctx* ctx, int enable);

/* Device-side kernel timing (the reference's per-PRED kernelExecutionTime,
 * main.cpp:856-866): when enabled, every kernel launch carries hipEvents in its
 * own dispatch on the stream it runs on.  kernel_class 0 = quadrant work items
 * (affine_me_quad); 6 = those of 32 to 128 sub-blocks in launches with 3-CP
 * (affine_me_quad2; 2-CP-only launches run them in affine_me_quad); 3 = the
 * 128x128 CUs (affine_me_ctu2); 4 / 5 = the 128x64 / 64x128 CUs
 * (affine_me_half2w / _half2h) -- in 2-CP-only launches 4 = both, in one
 * affine_me_half2 launch, and 5 stays empty; under PROF 0 = every quadrant
 * work item (affine_me_quad_prof), 1 = the 128x128 CUs (affine_me_ctu_prof),
 * 2 = the 128x64 / 64x128 CUs (affine_me_half_prof).
 * enable = 2 times the quadrant kernels only (their dispatches carry the events;
 * the 128-class launches run untimed).  vame_get_timing waits for the recorded
 * launches and returns their summed duration and count since the last reset.
 * enable | VAME_TIMING_KEEP changes what later launches record without
 * dropping the launches recorded so far (timing a sample of a run's steps).
 * Launches on a stream under capture carry no events. */
enum { VAME_TIMING_KEEP = 16 };
int vame_set_timing(vame_ctx* ctx, int enable);
int vame_get_timing(vame_ctx* ctx, int kernel_class, double* total_ms, int* launches, int reset);

/* Work-item templates (no device work): how many times the engine's work
 * items -- quadrant, 128x128 and 128x64 / 64x128 items, as vame_create builds
 * them -- cover each of the CTU's candidate CUs of `align`: hits[0 ..
 * {201|284}) indexed by the output offset RETURN_STRIDE[group] + cuIdx
 * (affine.cl:936 / :1929).  A valid partition covers every CU exactly once
 * (the quadrant items of one-alignment launches; VAME_E_INVALID if those of
 * both-alignment launches cover differently).  half128 must be non-zero (the
 * one packing: every 128x64 / 64x128 CU a work item of its own).  Also returns
 * the item counts per kernel class (quad -- of a both-alignment launch --,
 * 128x128, 128x64 + 64x128) in items3 when non-NULL. */
int vame_template_coverage(int half128, int align, int32_t* hits, int32_t* items3);

/* Geometry / host helpers (no device work). */
int vame_num_ctus(int width, int height);   /* 0 if unsupported */
int vame_cus_per_ctu(int align);            /* 201 / 284 */
int vame_num_groups(int align);             /* 12 / 24 */
/* CU group g: size, count, return stride, CTU-relative positions (xs/ys >= 64 entries) */
int vame_group_geometry(int align, int g, int* w, int* h, int* ncu, int* stride, int* xs,
                        int* ys);
/* Motion lambda of a POC (main.cpp:585 -> main_aux_functions.h:1482-1497, constants.h:94-103) */
float vame_lambda(int qp, int poc);
int vame_poc_qp(int qp, int poc);
/* Reference-picture list of a POC (main.cpp:591-707): fills pocs[0..min(4,poc)-1]
 * with the POC held by each refIdx slot; returns the number of refs. */
int vame_ref_list(int poc, int* pocs);

/* ---- Host I/O contracts of the reference's ./main (no device work) ---- */

/* Frame ingest (main.cpp:293-330): reads `nframes` frames of width x height
 * samples into `out` (host, nframes*W*H uint16).  CSV layout as the reference
 * reads it: one frame line per text line, ',' separated, frames stacked; each
 * value parsed like stoi and stored as unsigned short.  Paths ending in .u16 /
 * .yuv are raw little-endian 16-bit frames.  nthreads <= 0: all host cores.
 * Returns 0, or VAME_E_INVALID for a missing file / short file / bad value. */
int vame_read_frames(const char* path, int width, int height, int nframes, uint16_t* out,
                     int nthreads);
/* The same for frames first .. first + nframes - 1 of the file (a frame-sharded
 * rank reads only the frames its POC block uses). */
int vame_read_frames_range(const char* path, int width, int height, int first, int nframes,
                           uint16_t* out, int nthreads);
/* The same, reading only the bytes [span_begin, span_end) of a CSV (span_end < 0:
 * to the end), which must hold every line of those frames, with lines_before =
 * the number of '\n' in [0, span_begin) -- so a rank whose frames lie deep in
 * a large file does not scan the bytes ahead of them.  vame_count_lines counts
 * the '\n' of [begin, end) (end < 0: to the end; ranks count disjoint chunks
 * and exchange the counts). */
long long vame_count_lines(const char* path, long long begin, long long end, int nthreads);
/* The '\n' counts of n byte ranges [begin[i], end[i]) of one file, into
 * counts[i], in one pass over one mapping with one set of threads (a rank's
 * chunks of a CSV: calling vame_count_lines per chunk paid a mapping and a
 * thread start per 16 MB chunk).  Returns VAME_OK, or VAME_E_INVALID for a
 * missing file, a negative or reversed range. */
int vame_count_lines_ranges(const char* path, const long long* begin, const long long* end, int n,
                            long long* counts, int nthreads);
int vame_read_frames_span(const char* path, int width, int height, int first, int nframes,
                          long long span_begin, long long lines_before, long long span_end,
                          uint16_t* out, int nthreads);

/* Decision log (main_aux_functions.h:387-525, 1547-1585).  pred = 0 FULL_2CP,
 * 1 FULL_3CP, 2 HALF_2CP, 3 HALF_3CP (constants.h:15-21).  Files are
 * <prefix>_<FULL|HALF>_<2|3>CPs_<W>x<H>.csv with the reference's header.
 *   vame_log_remove_old    : removeOldTraces (:1547) -- deletes the old files
 *   vame_log_write_headers : creates/truncates the files of one pred with the
 *                            header (done by the reference at POC 1, refIdx 0)
 *   vame_log_append        : appends the rows of one (POC, refIdx, pred) from
 *                            HOST result arrays in the reference's index layout;
 *                            returns the number of bytes written (< 0: error)
 *   vame_log_file_count    : distinct files of a pred (12 FULL, 8 HALF)        */
int vame_log_remove_old(const char* prefix);
int vame_log_write_headers(const char* prefix, int pred);
long long vame_log_append(const char* prefix, int pred, int width, int height, int poc, int ref,
                          const int64_t* cost, const vame_cpmvs* cpmvs, int nthreads);
int vame_log_file_count(int pred);

/* The same log, a whole POC per call (the CLI's path): a writer holds a
 * persistent thread pool and the open files of one prefix.  One call appends
 * the rows of every refIdx r < nrefs and PRED m in pred_mask (bit m), from the
 * host arrays cost[r*4 + m] / cpmvs[r*4 + m] (entries of PREDs outside the
 * mask may be NULL); the files receive exactly the bytes of the reference's
 * per-(POC, refIdx, PRED) appends in main.cpp:942-958 order (refIdx outer,
 * PRED inner).  Headers stay with vame_log_write_headers (POC 1, before the
 * first call).  Returns the bytes written (< 0: error).
 *   vame_log_writer_create : NULL on a bad prefix / unsupported resolution;
 *                            nthreads <= 0: all host cores                   */
typedef struct vame_log_writer vame_log_writer;
vame_log_writer* vame_log_writer_create(const char* prefix, int width, int height, int nthreads);
long long vame_log_writer_poc(vame_log_writer* w, int poc, int nrefs, int pred_mask,
                              const int64_t* const* cost, const vame_cpmvs* const* cpmvs);
/* The same for refIdx ref0 .. ref0 + nrefs - 1 only (arrays indexed
 * (r - ref0)*4 + m): a POC whose refIdx range is cut between two frame-shard
 * ranks is logged by each for its own refs, in the same order. */
long long vame_log_writer_refs(vame_log_writer* w, int poc, int ref0, int nrefs, int pred_mask,
                               const int64_t* const* cost, const vame_cpmvs* const* cpmvs);
int vame_log_writer_destroy(vame_log_writer* w);
/* Deferred mode, for a frame-shard rank whose rows belong in the middle of
 * the files: after vame_log_writer_set_deferred(w, 1) (before its first POC;
 * VAME_E_INVALID once rows were logged) the writer keeps each
 * file's rows in host memory instead of appending them.  Its files are
 * numbered 0 .. vame_log_writer_num_files - 1 (vame_log_writer_file_name);
 * vame_log_writer_sizes reports the bytes held per file, and
 * vame_log_writer_flush_at writes every file's rows at offsets[f] (pwrite;
 * the file is created if missing and never truncated), files in parallel,
 * returning the bytes written -- so the ranks of a node, once they know each
 * other's sizes, place their blocks into the one set of files at once. */
int vame_log_writer_set_deferred(vame_log_writer* w, int deferred);
int vame_log_writer_num_files(vame_log_writer* w);
int vame_log_writer_file_name(vame_log_writer* w, int f, char* buf, int buflen);
int vame_log_writer_sizes(vame_log_writer* w, long long* sizes);
long long vame_log_writer_flush_at(vame_log_writer* w, const long long* offsets);

const char* vame_strerror(int code);
const char* vame_last_hip_error(void);
const char* vame_version(void);

#ifdef __cplusplus
}
#endif
#endif /* VAME_H */

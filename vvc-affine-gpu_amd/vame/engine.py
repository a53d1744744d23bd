"""Device-side entry points (HIP kernels via libvame.so) on torch.cuda tensors.

Mirrors the reference's operator interface for this path:
  * `Engine.affine_me(ref, cur, lam, align, ncp, extra, prev)` == one launch of
    affine_gradient_mult_sizes(_HA) built with -DnCP=ncp (affine.cl:11/:960,
    args set at main.cpp:827-840), returning the gBestCost / gBestCpmvs arrays;
  * `Engine.affine_me_poc(cur, refs, lam, ...)` == the whole refIdx loop of one
    POC (main.cpp:746-966), fused into one pass;
  * `Engine.affine_me_batch([(cur, refs, lam, out), ...])` == several POCs'
    affine_me_poc calls in shared launches.
Frames are (H, W) int16/uint16 tensors of 10-bit samples on the engine's device.
"""
from __future__ import annotations

import ctypes

import torch

from . import bipred as B
from . import partition as P
from ._lib import (CUS_PER_CTU, MAX_PENALTY, MODE_2CP, MODE_3CP, MODE_FULL, MODE_HALF, MODES,  # noqa: F401
                   Mvp, PocJob, PocResult, SeedResult, check, lib)

CPMV_FIELDS = ("nCPs", "LTx", "LTy", "RTx", "RTy", "LBx", "LBy")


def pred_mask(modes: int) -> int:
    """vame_pred_mask: the PREDs (bit m of MODES) a mode mask codes."""
    ncp = 3 if modes & MODE_3CP else 1
    sel = (modes >> 2) & 3
    return (ncp if sel in (0, 1, 3) else 0) | ((ncp << 2) if sel in (0, 2, 3) else 0)


def _ptr(t: torch.Tensor | None):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _poc_result(res: dict) -> PocResult:
    """The vame_poc_result of an alloc_poc dict: the pointers of every
    (refIdx, MODE) entry it holds."""
    pr = PocResult()
    for (r, name), (cost, cpmv) in res.items():
        m = MODES.index(name)
        pr.cost[r][m] = cost.data_ptr()
        pr.cpmvs[r][m] = cpmv.data_ptr()
    return pr


class Engine:
    def __init__(self, width: int, height: int, device: int | torch.device = 0):
        if not torch.cuda.is_available():
            raise RuntimeError("vame.Engine needs a HIP device (no CPU fallback)")
        self.device = torch.device("cuda", device if isinstance(device, int) else device.index)
        self.W, self.H = width, height
        self.n_ctus = lib().vame_num_ctus(width, height)
        if not self.n_ctus:
            raise ValueError(f"unsupported resolution {width}x{height}")
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            check(lib().vame_create(ctypes.byref(h), self.device.index, width, height))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib().vame_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_prof(self, enable: bool) -> None:
        """PROF on/off for later launches (the reference hard-disables it,
        affine.cl:168); vame_set_prof."""
        check(lib().vame_set_prof(self._h, int(enable)))

    def set_max_pairs(self, n: int) -> None:
        """(POC, refIdx) pairs per launch, 1..32 (default 32): sizes the
        context's 3-CP seed-reuse scratch (vame_set_max_pairs)."""
        check(lib().vame_set_max_pairs(self._h, int(n)))

    @property
    def max_pairs(self) -> int:
        return lib().vame_get_max_pairs(self._h)

    def set_timing(self, enable, keep: bool = False) -> None:
        """True / 1: time every kernel class; 2: the quadrant kernel only; 0: off.
        keep: leave the launches recorded so far (VAME_TIMING_KEEP)."""
        check(lib().vame_set_timing(self._h, int(enable) | (16 if keep else 0)))

    def get_timing(self, kernel_class: int, reset: bool = True):
        """(total_ms, launches) of kernel class 0 (quadrant items, affine_me_quad) /
        6 (those of 32 to 128 sub-blocks in launches with 3-CP, affine_me_quad2) /
        3 (128x128 CUs, affine_me_ctu2) / 4, 5 (128x64 / 64x128 CUs,
        affine_me_half2w / affine_me_half2h; in 2-CP-only launches 4 is both, in
        one affine_me_half2 launch); under PROF 0 (affine_me_quad_prof) / 1
        (128x128 CUs, affine_me_ctu_prof) / 2 (128x64 and 64x128 CUs,
        affine_me_half_prof)."""
        t, n = ctypes.c_double(), ctypes.c_int()
        check(lib().vame_get_timing(self._h, kernel_class, ctypes.byref(t), ctypes.byref(n), int(reset)))
        return t.value, n.value

    def n_cus(self, align: int) -> int:
        return self.n_ctus * CUS_PER_CTU[bool(align)]

    def _frame(self, f: torch.Tensor) -> torch.Tensor:
        if f.shape != (self.H, self.W) or f.device != self.device or f.dtype not in (torch.int16, torch.uint16):
            raise ValueError(f"frame must be ({self.H},{self.W}) int16/uint16 on {self.device}")
        return f.contiguous()

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # ---- argument checks shared by the prediction-side entry points
    def _check_cus(self, t: torch.Tensor, cols: int, name: str = "cus", n: int | None = None) -> None:
        """A descriptor tensor: contiguous int32 [n, cols] on the engine's device."""
        if (t.dim() != 2 or t.shape[1] != cols or t.dtype != torch.int32 or t.device != self.device
                or not t.is_contiguous() or (n is not None and t.shape[0] != n)):
            raise ValueError(f"{name} must be a contiguous int32 [{'n' if n is None else n}, {cols}] tensor "
                             f"on {self.device}")

    def _refs(self, refs, what: str):
        """1..4 reference frames: (the frames, their pointer array)."""
        refs = [self._frame(r) for r in refs]
        if not 1 <= len(refs) <= 4:
            raise ValueError(f"{what} takes 1..4 reference frames")
        return refs, (ctypes.c_void_p * len(refs))(*[r.data_ptr() for r in refs])

    def _check_pred(self, pred: torch.Tensor | None) -> None:
        if pred is not None and (pred.shape != (self.H, self.W) or pred.device != self.device
                                 or pred.dtype not in (torch.int16, torch.uint16) or not pred.is_contiguous()):
            raise ValueError(f"pred must be a contiguous ({self.H},{self.W}) int16/uint16 frame on {self.device}")

    def _check_scalar(self, t: torch.Tensor | None, name: str) -> None:
        if t is not None and (t.numel() != 1 or t.dtype != torch.int32 or t.device != self.device):
            raise ValueError(f"{name} must be an int32 scalar on {self.device}")

    def _bad(self) -> torch.Tensor:
        """A cleared `bad` flag: the int32 device scalar the kernels OR into."""
        return torch.zeros((), dtype=torch.int32, device=self.device)

    @staticmethod
    def _preds(result: dict, preds: int | None, full: bool = False) -> int:
        """The PRED mask of a call on an alloc_poc dict: `preds`, or every PRED
        the dict holds; at least one PRED, with `full` a FULL one."""
        preds = P.result_preds(result) if preds is None else int(preds)
        if preds & ~15 or not preds & (3 if full else 15):
            raise ValueError(f"preds must hold a {'FULL PRED (bit 0 or 1)' if full else 'PRED'} and only bits 0..3")
        return preds

    def _mc(self, what: str, cols: int, cus, refs, lam: float, cur, pred, want_cost: bool, ncus):
        """What affine_mc (cols = 12), affine_mc_bi and affine_mc_p (20) share
        around their C call: the argument checks and the cost / bad buffers.
        Returns the call's leading arguments up to cus, its trailing ones from
        lambda on, and the (pred, cost, bad) to return."""
        self._check_cus(cus, cols)
        if pred is None and not want_cost:
            raise ValueError(f"{what} needs pred, want_cost or both")
        refs, ref_ptrs = self._refs(refs, what)
        if want_cost:
            if cur is None:
                raise ValueError("want_cost needs cur")
            cur = self._frame(cur)
        self._check_pred(pred)
        self._check_scalar(ncus, "ncus")
        cost = torch.empty(cus.shape[0], dtype=torch.int64, device=self.device) if want_cost else None
        bad = self._bad()
        return ((self._h, _ptr(cur if want_cost else None), ref_ptrs, len(refs), _ptr(cus)),
                (float(lam), _ptr(pred), _ptr(cost), _ptr(bad), self._stream()), (pred, cost, bad))

    def _refine(self, plain, with_preds, cols: int, per: int, it_name: str, it_max: int, cus, preds, refs, cur,
                lam: float, iters: int, count, out, cost):
        """affine_search(_p) and bipred_refine(_p), parametrised as the C side's
        refine_cus: descriptors of `cols` columns with `per` predictor rows
        each, `iters` (called `it_name`) in 0..it_max.  Calls the symbol
        `plain` without preds, `with_preds` with them."""
        self._check_cus(cus, cols)
        if not 0 <= int(iters) <= it_max:
            raise ValueError(f"{it_name} must be in 0..{it_max}")
        refs, ref_ptrs = self._refs(refs, plain.__name__)
        cur = self._frame(cur)
        n = cus.shape[0]
        self._check_preds(preds, per * n, with_preds.__name__)
        self._check_scalar(count, "the descriptor count")
        out, cost = self._refine_out(cus, out, cost)
        bad = self._bad()
        head = (self._h, _ptr(cur), ref_ptrs, len(refs), _ptr(cus))
        tail = (n, _ptr(count), float(lam), int(iters), _ptr(out), _ptr(cost), _ptr(bad), self._stream())
        check(plain(*head, *tail) if preds is None else with_preds(*head, _ptr(preds), *tail))
        return out, cost, bad

    def _refine_out(self, cus: torch.Tensor, out, cost):
        """The out / cost buffers of affine_search and bipred_refine for the
        descriptors `cus`: the caller's, checked, or new ones."""
        n, cols = cus.shape
        if out is None:
            out = torch.empty_like(cus)
        else:
            self._check_cus(out, cols, "out", n)
        if cost is None:
            cost = torch.empty(n, dtype=torch.int64, device=self.device)
        elif (cost.dtype != torch.int64 or cost.numel() != n or cost.device != self.device
              or not cost.is_contiguous()):
            raise ValueError(f"cost must be a contiguous int64 [{n}] tensor on {self.device}")
        return out, cost

    def _check_out(self, out, align: int):
        """Caller-supplied result buffers must hold exactly the launch's rows:
        int64 cost[n], int32 cpmv[n, 7], contiguous, on the engine's device."""
        cost, cpmv = out
        n = self.n_cus(align)
        ok = (cost.dtype == torch.int64 and cost.numel() == n and cost.is_contiguous()
              and cpmv.dtype == torch.int32 and tuple(cpmv.shape) == (n, 7) and cpmv.is_contiguous()
              and cost.device == self.device and cpmv.device == self.device)
        if not ok:
            raise ValueError(f"result buffers must be int64[{n}] and int32[{n}, 7], contiguous, "
                             f"on {self.device} (align={align})")
        return cost, cpmv

    def alloc_result(self, align: int):
        n = self.n_cus(align)
        return (torch.empty(n, dtype=torch.int64, device=self.device),
                torch.empty((n, 7), dtype=torch.int32, device=self.device))

    def affine_me(self, ref, cur, lam: float, align: int, ncp: int, extra: int = 0,
                  prev: torch.Tensor | None = None, out=None):
        ref, cur = self._frame(ref), self._frame(cur)
        if align not in (0, 1) or ncp not in (2, 3):
            raise ValueError("align must be 0/1 and ncp 2/3")
        cost, cpmv = self._check_out(out, align) if out is not None else self.alloc_result(align)
        if ncp == 3 and (prev is None or tuple(prev.shape) != (self.n_cus(align), 7)
                         or prev.dtype != torch.int32 or prev.device != self.device):
            raise ValueError("3-CP needs prev = the same-alignment 2-CP cpmvs, int32 [n, 7] on the device")
        check(lib().vame_affine_me(self._h, _ptr(ref), _ptr(cur), float(lam), align, ncp, extra,
                                   _ptr(prev.contiguous()) if prev is not None else None,
                                   _ptr(cost), _ptr(cpmv), self._stream()))
        return cost, cpmv

    def alloc_poc(self, nrefs: int, modes: int = 3):
        res = {}
        preds = pred_mask(modes)
        for r in range(nrefs):
            for m, name in enumerate(MODES):
                if (preds >> m) & 1:
                    res[(r, name)] = self.alloc_result(m >> 1)
        return res

    def _check_poc_out(self, out, nrefs: int, modes: int):
        preds = pred_mask(modes)
        need = {(r, name) for r in range(nrefs) for m, name in enumerate(MODES) if (preds >> m) & 1}
        missing = need - set(out)
        if missing:
            raise ValueError(f"result buffers missing for {sorted(missing)}")
        for (r, name), bufs in out.items():
            if r >= nrefs or name not in MODES:
                raise ValueError(f"unexpected result key {(r, name)}")
            self._check_out(bufs, MODES.index(name) >> 1)

    def affine_me_batch(self, jobs, modes: int = 3, extra: int = 0):
        """jobs: [(cur, refs, lam, out)] with out from alloc_poc; one
        vame_affine_me_batch call (max_pairs (POC, refIdx) pairs per launch,
        default 32)."""
        keep = []
        arr = (PocJob * len(jobs))()
        for j, (cur, refs, lam, out) in enumerate(jobs):
            cur = self._frame(cur)
            refs, ref_ptrs = self._refs(refs, "affine_me_batch")
            self._check_poc_out(out, len(refs), modes)
            pr = _poc_result(out)
            keep += [cur, refs, pr, ref_ptrs]
            arr[j].cur = cur.data_ptr()
            arr[j].refs = ctypes.cast(ref_ptrs, ctypes.c_void_p)
            arr[j].nrefs = len(refs)
            arr[j].lam = float(lam)
            arr[j].out = ctypes.cast(ctypes.pointer(pr), ctypes.c_void_p)
        check(lib().vame_affine_me_batch(self._h, arr, len(jobs), modes, extra, self._stream()))
        return [job[3] for job in jobs]

    def pack_records(self, results: list[dict], modes: int, words: int | None = None,
                     bad: torch.Tensor | None = None) -> torch.Tensor:
        """vame_pack_records: the POCs' results (alloc_poc dicts, POC order) in
        the compact wire form of shard.pack, one kernel, zero-padded to
        `words`; `bad` (int32 device scalar) is OR-ed with 1 when a record does
        not fit the form (shard.check_flag reads it)."""
        from .shard import slab_words
        need = slab_words([(max(r for r, _ in res) + 1, modes, (self.n_cus(0), self.n_cus(1)))
                           for res in results])
        words = need if words is None else words
        if words < need:
            raise ValueError("slab larger than the agreed size")
        slab = torch.empty(words, dtype=torch.int32, device=self.device)
        if bad is None:
            bad = self._bad()
        arr = (PocJob * max(len(results), 1))()
        keep = []
        for j, res in enumerate(results):
            nrefs = max(r for r, _ in res) + 1
            self._check_poc_out(res, nrefs, modes)
            pr = _poc_result(res)
            keep.append(pr)
            arr[j].nrefs = nrefs
            arr[j].out = ctypes.cast(ctypes.pointer(pr), ctypes.c_void_p)
        check(lib().vame_pack_records(self._h, arr, len(results), modes, slab.data_ptr(), words,
                                      bad.data_ptr(), self._stream()))
        return slab

    def affine_mc(self, cus: torch.Tensor, refs, lam: float = 0.0, cur: torch.Tensor | None = None,
                  pred: torch.Tensor | None = None, want_cost: bool = False, ncus: torch.Tensor | None = None):
        """vame_affine_mc: predict and / or cost caller-given CPMVs exactly as
        one prediction step of the search does.  cus: int32 [n, 12] on the
        engine's device, columns x, y, w, h, ref, nCPs, LTx, LTy, RTx, RTy,
        LBx, LBy (vame.mc.cus_from_result builds them from result arrays);
        refs: 1..4 frames, indexed by the ref column.  pred: a frame that
        receives the samples of the valid descriptors' CUs (other samples keep
        their value), or None; want_cost: return int64 cost[n] = SATD against
        `cur` + floor(lam * (bits + 2)).  Returns (pred, cost, bad): bad is an
        int32 device scalar, 1 when a descriptor was invalid (such a descriptor
        writes no sample and costs 0).  ncus: an int32 device scalar, the
        number of descriptors to run (vame_affine_mc_dev: min(ncus, n), read on
        the device; rows of cus and cost past it are neither read nor
        written).  Asynchronous on the current stream."""
        head, tail, ret = self._mc("affine_mc", 12, cus, refs, lam, cur, pred, want_cost, ncus)
        if ncus is not None:
            check(lib().vame_affine_mc_dev(*head, cus.shape[0], _ptr(ncus), *tail))
        else:
            check(lib().vame_affine_mc(*head, cus.shape[0], *tail))
        return ret

    def partition(self, result: dict, preds: int | None = None, split_penalty: int = 0, out: dict | None = None):
        """vame_partition: per CTU the cheapest tiling by the candidate CUs of
        `result` (an alloc_poc dict of one POC, as the search filled it) under
        binary and ternary splits, every leaf with its best (refIdx, 2-CP |
        3-CP) candidate.  preds: the PREDs that take
        part (bit m of MODES; None = every PRED the dict holds; at least one
        FULL PRED); split_penalty: added per split, 0 .. 2^40.  Returns device
        tensors: cus int32 [nCtus*64, 12] (descriptors for affine_mc; the
        first ncus rows are written), rows int32 [nCtus*64] (the chosen row in
        its PRED array), ncus int32 scalar, ctu_info int32 [nCtus, 4] (first,
        count, holes, splits), ctu_cost int64 [nCtus], block_cu int32
        [nCtus*64].  out: a dict of an earlier call to write into.  Reads
        nothing on the host; asynchronous on the current stream."""
        return self._partition(P, result, None, preds, split_penalty, 0, out)

    def _partition(self, form, result: dict, bi, preds, split_penalty: int, bi_penalty: int, out: dict | None):
        """partition() (form = vame.partition, which names its outputs) and
        partition_bi() (form = vame.bipred, with the bi arrays)."""
        what = "partition" if form is P else "partition_bi"
        preds = self._preds(result, preds, full=True)
        if not 0 <= int(split_penalty) <= MAX_PENALTY or not 0 <= int(bi_penalty) <= MAX_PENALTY:
            raise ValueError("split_penalty and bi_penalty must be in [0, 2^40]")
        nrefs, pr = self._check_result(result, preds, what)
        if form is B:
            bcost, bsel = self._check_bi(bi, preds)
        if out is None:
            out = form.alloc(self.n_ctus, self.device)
        for k, w in form.alloc(self.n_ctus, "meta").items():
            t = out[k]
            if t.shape != w.shape or t.dtype != w.dtype or t.device != self.device or not t.is_contiguous():
                raise ValueError(f"out[{k!r}] must be a contiguous {w.dtype} {tuple(w.shape)} tensor on {self.device}")
        head = (self._h, ctypes.byref(pr), nrefs, preds, int(split_penalty))
        ptrs = [_ptr(out[k]) for k in form.KEYS]
        if form is P:
            check(lib().vame_partition(*head, *ptrs, self._stream()))
        else:
            check(lib().vame_partition_bi(*head, bcost, bsel, int(bi_penalty), *ptrs, self._stream()))
        return out

    def predict_partition(self, part: dict, refs, lam: float = 0.0, cur: torch.Tensor | None = None,
                          pred: torch.Tensor | None = None, want_cost: bool = False):
        """affine_mc on the leaves of a partition() result, their count read on
        the device: (pred, cost, bad) as affine_mc, cost int64 [nCtus*64] with
        the first ncus entries written."""
        if part["cus"].dim() == 2 and part["cus"].shape[1] == 20:  # a partition_bi() result
            return self.affine_mc_bi(part["cus"], refs, lam, cur=cur, pred=pred, want_cost=want_cost,
                                     ncus=part["ncus"])
        return self.affine_mc(part["cus"], refs, lam, cur=cur, pred=pred, want_cost=want_cost, ncus=part["ncus"])

    # ---- bi-prediction
    def _check_result(self, result: dict, preds: int, what: str, refs=None):
        """An alloc_poc dict that holds every PRED of `preds` for refIdx
        0 .. nrefs-1, over the frames `refs` where given: (nrefs, its
        vame_poc_result)."""
        if not result:
            raise ValueError(f"{what} needs a result dict")
        nrefs = max(r for r, _ in result) + 1
        if not 1 <= nrefs <= 4:
            raise ValueError(f"{what} takes the results of 1..4 references")
        if refs is not None and nrefs != len(refs):
            raise ValueError(f"{what}: the result dict holds {nrefs} references, refs {len(refs)}")
        need = {}
        for r in range(nrefs):
            for m, name in enumerate(MODES):
                if (preds >> m) & 1:
                    if (r, name) not in result:
                        raise ValueError(f"result buffers missing for {(r, name)}")
                    need[(r, name)] = self._check_out(result[(r, name)], m >> 1)
        return nrefs, _poc_result(need)

    def _check_bi(self, bi: dict, preds: int):
        """vame_bipred's arrays of the alignments in `preds`: two 2-pointer arrays."""
        V = ctypes.c_void_p
        cost, sel = (V * 2)(), (V * 2)()
        for a in (0, 1):
            if not (preds >> (2 * a)) & 3:
                continue
            try:
                c, s = bi["cost"][a], bi["sel"][a]
            except (KeyError, IndexError, TypeError):
                c = s = None
            n = self.n_cus(a)
            if (c is None or s is None or c.dtype != torch.int64 or s.dtype != torch.int32 or c.numel() != n
                    or s.numel() != n or c.device != self.device or s.device != self.device
                    or not c.is_contiguous() or not s.is_contiguous()):
                raise ValueError(f"bi['cost'][{a}] / bi['sel'][{a}] must be contiguous int64[{n}] / int32[{n}] "
                                 f"on {self.device}")
            cost[a], sel[a] = c.data_ptr(), s.data_ptr()
        return cost, sel

    def affine_mc_bi(self, cus: torch.Tensor, refs, lam: float = 0.0, cur: torch.Tensor | None = None,
                     pred: torch.Tensor | None = None, want_cost: bool = False, ncus: torch.Tensor | None = None):
        """vame_affine_mc_bi: affine_mc on bi descriptors, int32 [n, 20] with
        the columns vame.bipred.BICU_FIELDS: a 12-column descriptor, then ref1
        and the second hypothesis' nCPs and CPMVs.  ref1 = -1: uni-predicted,
        exactly affine_mc; else the sample is the once-rounded average of the
        two hypotheses and the cost carries both rates.  Arguments and the
        returned (pred, cost, bad) as affine_mc.  Not available under PROF."""
        return self._mc_bi("affine_mc_bi", cus, None, refs, lam, cur, pred, want_cost, ncus)

    def _mc_bi(self, what: str, cus, preds, refs, lam: float, cur, pred, want_cost: bool, ncus):
        """affine_mc_bi, and with `preds` (int32 [2n, 7]) affine_mc_p."""
        head, tail, ret = self._mc(what, 20, cus, refs, lam, cur, pred, want_cost, ncus)
        n = cus.shape[0]
        self._check_preds(preds, 2 * n, what)
        if preds is None:
            check(lib().vame_affine_mc_bi(*head, n, _ptr(ncus), *tail))
        else:
            check(lib().vame_affine_mc_bi_p(*head, _ptr(preds), n, _ptr(ncus), *tail))
        return ret

    def bipred(self, cur, refs, lam: float, result: dict, preds: int | None = None, out: dict | None = None):
        """vame_bipred: for every candidate CU of `result` (an alloc_poc dict
        of one POC over the frames `refs`) the cheapest pair of two references'
        winners.  Returns {"cost": [FULL, HALF], "sel": [FULL, HALF]}: int64 /
        int32 arrays over the rows of each alignment (None for an alignment
        without a PRED in `preds`); rows of CUs that leave the frame, and every
        row with one reference, hold INT64_MAX and -1; sel = r0 + 4*m0 + 8*r1 +
        32*m1 (vame.bipred.decode_sel).  preds: None = every PRED the dict
        holds.  out: a dict of an earlier call to write into."""
        return self._bipred("bipred", cur, refs, lam, result, None, preds, out)

    def _bipred(self, what: str, cur, refs, lam: float, result: dict, mvp: dict | None, preds, out: dict | None):
        """bipred, and with `mvp` bipred_p."""
        cur = self._frame(cur)
        refs, ref_ptrs = self._refs(refs, what)
        preds = self._preds(result, preds)
        nrefs, pr = self._check_result(result, preds, what, refs)
        m = None if mvp is None else self._mv_table(mvp, nrefs, preds, f"{what}: mvp")
        if out is None:
            full = B.alloc_bi(self.n_ctus, self.device)
            out = {k: [t if (preds >> (2 * a)) & 3 else None for a, t in enumerate(full[k])] for k in ("cost", "sel")}
        cost, sel = self._check_bi(out, preds)
        head = (self._h, _ptr(cur), ref_ptrs, nrefs, float(lam), ctypes.byref(pr), preds)
        if m is None:
            check(lib().vame_bipred(*head, cost, sel, self._stream()))
        else:
            check(lib().vame_bipred_p(*head, ctypes.byref(m), cost, sel, self._stream()))
        return out

    def partition_bi(self, result: dict, bi: dict, preds: int | None = None, split_penalty: int = 0,
                     bi_penalty: int = 0, out: dict | None = None):
        """vame_partition_bi: partition() whose leaves may be bi-predicted: a
        leaf's value is the smaller of its uni minimum and bi cost + bi_penalty
        (bi: a bipred() result over the same `result`).  Returns the tensors of
        partition() with cus int32 [nCtus*64, 20] (vame.bipred.BICU_FIELDS;
        ref1 = -1 for a uni leaf) and sel int32 [nCtus*64] (bi_sel, or -1)."""
        return self._partition(B, result, bi, preds, split_penalty, bi_penalty, out)

    # ---- refinement of bi-predicted CUs
    def bipred_refine(self, cus: torch.Tensor, refs, cur, lam: float, rounds: int = 2,
                      count: torch.Tensor | None = None, out: torch.Tensor | None = None,
                      cost: torch.Tensor | None = None):
        """vame_bipred_refine: for every bi descriptor of cus (int32 [n, 20],
        vame.bipred.BICU_FIELDS) hold one hypothesis, re-estimate the other
        against what the held one leaves to explain, and swap, `rounds` times
        (0..4; round 0 moves the second hypothesis).  Returns (out, cost, bad):
        the descriptors with their refined CPMVs, int64 [n] their bi costs --
        exactly affine_mc_bi's costs of `out`, never above those of `cus` --
        and the int32 flag of an invalid descriptor (copied through, cost 0).
        Uni descriptors (ref1 = -1) pass through with their uni cost.  count:
        an int32 scalar on the device, the number of descriptors to work on
        (entries past it stay untouched); out may be cus.  Reads nothing on the
        host; asynchronous on the current stream.  Not available under PROF."""
        return self.bipred_refine_p(cus, None, refs, cur, lam, rounds, count, out, cost)

    def refine_partition(self, part: dict, refs, cur, lam: float, rounds: int = 2) -> dict:
        """bipred_refine on the leaves of a partition_bi() result, their count
        read on the device.  Returns a new dict for predict_partition: the
        entries of `part` with `cus` replaced by the refined descriptors, plus
        leaf_cost int64 [nCtus*64] (the first ncus entries written) and bad.
        `part` is not modified; no host read."""
        if part["cus"].dim() != 2 or part["cus"].shape[1] != 20:
            raise ValueError("refine_partition needs a partition_bi() result")
        cus, cost, bad = self.bipred_refine(part["cus"], refs, cur, lam, rounds, count=part["ncus"])
        out = dict(part)
        out["cus"], out["leaf_cost"], out["bad"] = cus, cost, bad
        return out

    def refine_bipred(self, cur, refs, lam: float, result: dict, bi: dict, rounds: int = 2,
                      preds: int | None = None) -> dict:
        """bipred_refine on every candidate CU with a pair (bi_sel >= 0) of a
        bipred() result `bi` over `result`.  Returns a new bi dict: cost with
        the refined costs scattered back, sel unchanged, and per alignment the
        refined descriptors `cus` and their `rows` (None for an alignment
        outside `preds`).  partition_bi() takes it as its bi argument; the bi
        leaves it emits still carry the search's CPMVs, and refine_partition()
        with the same `rounds` turns them into the descriptors refined here, at
        the costs the partition used.  `bi` is not modified.  Reads the
        selection on the host (synchronizes)."""
        preds = self._preds(result, preds)
        self._check_result(result, preds, "refine_bipred")
        self._check_bi(bi, preds)
        out = {"cost": [None, None], "sel": [None, None], "cus": [None, None], "rows": [None, None]}
        for a in (0, 1):
            if not (preds >> (2 * a)) & 3:
                continue
            sel = bi["sel"][a]
            rows = torch.nonzero(sel >= 0).reshape(-1)
            res_a = {k: v for k, v in result.items() if (preds >> MODES.index(k[1])) & 1}
            cus = B.bicus_from_sel(self.W, self.H, a, res_a, sel, rows)
            cost = bi["cost"][a].clone()
            if rows.numel():
                cus, c, _ = self.bipred_refine(cus, refs, cur, lam, rounds)
                cost[rows] = c
            out["cost"][a], out["sel"][a], out["cus"][a], out["rows"][a] = cost, sel, cus, rows.to(torch.int32)
        return out

    # ---- seeding the search
    def _check_seed(self, t, a: int, what: str, dtype, tail: tuple):
        n = self.n_cus(a)
        if (t is None or t.dtype != dtype or tuple(t.shape) != (n,) + tail or t.device != self.device
                or not t.is_contiguous()):
            raise ValueError(f"{what} must be a contiguous {dtype} {(n,) + tail} tensor on {self.device}")
        return t

    def _seed_out(self, nrefs: int, aligns: int, out: dict | None):
        """(out, its vame_seed_result) of seed_search / seed_search_wide."""
        if int(aligns) & ~3 or not int(aligns):
            raise ValueError("aligns must hold bit 0 (FULL), bit 1 (HALF) or both")
        keys = [(r, a) for r in range(nrefs) for a in (0, 1) if (aligns >> a) & 1]
        if out is None:
            out = {"mv": {k: torch.empty((self.n_cus(k[1]), 2), dtype=torch.int32, device=self.device) for k in keys},
                   "cost": {k: torch.empty(self.n_cus(k[1]), dtype=torch.int64, device=self.device) for k in keys}}
        sr = SeedResult()
        for r, a in keys:
            try:
                mv, cost = out["mv"][(r, a)], out["cost"][(r, a)]
            except (KeyError, TypeError):
                raise ValueError(f"out['mv'] / out['cost'] miss {(r, a)}") from None
            sr.mv[r][a] = self._check_seed(mv, a, f"out['mv'][{(r, a)}]", torch.int32, (2,)).data_ptr()
            sr.cost[r][a] = self._check_seed(cost, a, f"out['cost'][{(r, a)}]", torch.int64, ()).data_ptr()
        return out, sr

    def seed_search(self, cur, refs, lam: float, radius: int = 16, aligns: int = 3, out: dict | None = None):
        """vame_seed_search: the best integer displacement of every candidate
        CU inside +-radius (0..32) under SAD + the search's rate, first minimum
        in the order (0, 0), then dy outer, dx inner.  aligns: bit 0 FULL, bit
        1 HALF.  Returns {"mv": {(r, a): int32 [n, 2]}, "cost": {(r, a): int64
        [n]}} over the rows of each alignment: mv in 1/16 pel (a start for
        affine_me_seeded), cost its SAD + rate; rows of CUs that leave the
        frame hold (0, 0) and INT64_MAX.  out: a dict of an earlier call to
        write into.  Reads nothing on the host; asynchronous on the current
        stream."""
        cur = self._frame(cur)
        refs, ref_ptrs = self._refs(refs, "seed_search")
        if not 0 <= int(radius) <= 32:
            raise ValueError("radius must be in 0..32")
        out, sr = self._seed_out(len(refs), aligns, out)
        check(lib().vame_seed_search(self._h, _ptr(cur), ref_ptrs, len(refs), float(lam), int(aligns), int(radius),
                                     ctypes.byref(sr), self._stream()))
        return out

    def _pyr_samples(self) -> int:
        return (self.W // 2) * (self.H // 2) + (self.W // 4) * (self.H // 4)

    def _check_pyr(self, t, what: str):
        if (t is None or t.dtype not in (torch.int16, torch.uint16) or tuple(t.shape) != (self._pyr_samples(),)
                or t.device != self.device or not t.is_contiguous() or t.data_ptr() & 7):
            raise ValueError(f"{what} must be a contiguous, 8-byte aligned int16/uint16 [{self._pyr_samples()}] tensor "
                             f"on {self.device}")
        return t

    def seed_pyramid(self, frame, out=None):
        """vame_seed_pyramid: levels 1 and 2 of the frame's 2:1 mean pyramid
        (level l+1 = (a + b + c + d + 2) >> 2 of level l's 2x2 samples) as one
        tensor [(W/2)(H/2) + (W/4)(H/4)] of the frame's dtype, level 1 followed
        by level 2, both dense and row-major.  Build a frame's pyramid once and
        pass it to seed_search_wide for as long as the frame is cur or a
        reference.  out: a tensor of an earlier call to write into.
        Asynchronous on the current stream."""
        frame = self._frame(frame)
        if out is None:
            out = torch.empty(self._pyr_samples(), dtype=frame.dtype, device=self.device)
        self._check_pyr(out, "out")
        check(lib().vame_seed_pyramid(self._h, _ptr(frame), _ptr(out), self._stream()))
        return out

    def seed_search_wide(self, cur, refs, lam: float, radius: int = 64, levels: int = 2, aligns: int = 3,
                         cur_pyr=None, ref_pyrs=None, out: dict | None = None):
        """vame_seed_search_wide: seed_search's result over +-radius (0..128),
        coarse to fine: every displacement of the grid of 2^levels samples
        (levels 1..2) at the pyramid's top level, then +-1 around twice the
        winner at every level below, down to the frame; at the frame (0, 0)
        comes first, so a non-zero seed is strictly better than not moving.
        The cost is seed_search's value of the returned displacement.
        cur_pyr / ref_pyrs: the frames' seed_pyramid() tensors (ref_pyrs a
        list, entries may be None); what is missing is built here.  Returns
        the same dict as seed_search (affine_me_seeded takes out["mv"]).
        Reads nothing on the host; asynchronous on the current stream."""
        cur = self._frame(cur)
        refs, ref_ptrs = self._refs(refs, "seed_search_wide")
        if not 0 <= int(radius) <= 128:
            raise ValueError("radius must be in 0..128")
        if not 1 <= int(levels) <= 2:
            raise ValueError("levels must be 1 or 2")
        out, sr = self._seed_out(len(refs), aligns, out)
        ref_pyrs = [None] * len(refs) if ref_pyrs is None else list(ref_pyrs)
        if len(ref_pyrs) != len(refs):
            raise ValueError(f"ref_pyrs holds {len(ref_pyrs)} pyramids, refs {len(refs)} frames")
        cur_pyr = self.seed_pyramid(cur) if cur_pyr is None else self._check_pyr(cur_pyr, "cur_pyr")
        ref_pyrs = [self.seed_pyramid(f) if t is None else self._check_pyr(t, f"ref_pyrs[{r}]")
                    for r, (f, t) in enumerate(zip(refs, ref_pyrs))]
        pyr_ptrs = (ctypes.c_void_p * len(refs))(*[t.data_ptr() for t in ref_pyrs])
        check(lib().vame_seed_search_wide(self._h, _ptr(cur), _ptr(cur_pyr), ref_ptrs, pyr_ptrs, len(refs), float(lam),
                                          int(aligns), int(radius), int(levels), ctypes.byref(sr), self._stream()))
        return out

    def affine_search(self, cus: torch.Tensor, refs, cur, lam: float, extra: int = 0,
                      ncus: torch.Tensor | None = None, out: torch.Tensor | None = None,
                      cost: torch.Tensor | None = None):
        """vame_affine_search: the search's iteration (5 gradient steps for a
        2-CP, 4 for a 3-CP descriptor, + extra) started at the CPMVs of every
        descriptor of cus (int32 [n, 12], vame.mc.CU_FIELDS).  Returns (out,
        cost, bad): the descriptors with the best CPMVs met, int64 [n] their
        costs -- exactly affine_mc's costs of `out` -- and the int32 flag of an
        invalid descriptor (copied through, cost 0).  ncus: an int32 scalar on
        the device, the number of descriptors to work on (entries past it stay
        untouched); out may be cus.  Reads nothing on the host; asynchronous on
        the current stream.  Not available under PROF."""
        return self.affine_search_p(cus, None, refs, cur, lam, extra, ncus, out, cost)

    def affine_me_seeded(self, cur, refs, lam: float, result: dict, seeds: dict, modes: int = 3, extra: int = 0):
        """vame_affine_me_seeded: improve `result` (the alloc_poc dict
        affine_me_poc filled for the same cur, refs, lam, modes and extra) in
        place: every row with a non-zero seed runs the 2-CP search from LT =
        RT = seed and, with 3-CP in modes, the 3-CP search from that winner;
        a row takes the new cost and CPMVs where the cost is strictly lower.
        seeds: {(r, a): int32 [n, 2]} (seed_search()["mv"], or any MVs with
        components in [-2^17, 2^17 - 1]).  Returns (result, bad): bad is 1 when
        a seed was out of range (its row is skipped).  torch allocates the work
        buffer.  Reads nothing on the host; asynchronous on the current stream.
        Not available under PROF."""
        return self._seeded("affine_me_seeded", cur, refs, lam, result, seeds, None, modes, extra)

    def _seeded(self, what: str, cur, refs, lam: float, result: dict, seeds: dict, mvp: dict | None, modes: int,
                extra: int):
        """affine_me_seeded, and with `mvp` affine_me_seeded_p."""
        cur = self._frame(cur)
        refs, ref_ptrs = self._refs(refs, what)
        if not int(modes) & MODE_2CP or int(modes) & ~15:
            raise ValueError("modes must hold MODE_2CP and only bits 0..3")
        if not 0 <= int(extra) <= 64:
            raise ValueError("extra must be in 0..64")
        preds = pred_mask(modes)
        nrefs, pr = self._check_result(result, preds, what, refs)
        s = self._mv_table(seeds, nrefs, preds, f"{what}: seeds")
        m = None if mvp is None else self._mv_table(mvp, nrefs, preds, f"{what}: mvp")
        L = lib()
        nbytes = (L.vame_seeded_work_bytes if m is None else L.vame_seeded_p_work_bytes)(self._h, nrefs, int(modes))
        work = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=self.device)
        bad = self._bad()
        head = (self._h, _ptr(cur), ref_ptrs, nrefs, float(lam), int(modes), int(extra), s.mv)
        tail = (ctypes.byref(pr), _ptr(work), work.numel() * 8, _ptr(bad), self._stream())
        if m is None:
            check(L.vame_affine_me_seeded(*head, *tail))
        else:
            check(L.vame_affine_me_seeded_p(*head, ctypes.byref(m), *tail))
        return result, bad

    # ---- rates against a motion-vector predictor
    def _check_preds(self, preds: torch.Tensor | None, n: int, what: str):
        """The predictors of a descriptor-list call: None (the zero predictor)
        or a contiguous int32 [n, 7] tensor (vame_cpmvs; nCPs ignored)."""
        if preds is not None and (preds.dtype != torch.int32 or tuple(preds.shape) != (n, 7)
                                  or preds.device != self.device or not preds.is_contiguous()):
            raise ValueError(f"{what}: preds must be a contiguous int32 [{n}, 7] tensor on {self.device}")

    def _mv_table(self, mvs: dict, nrefs: int, preds: int, what: str) -> Mvp:
        """{(r, a): int32 [n, 2]} (seed_search()["mv"], region_predictors()) as a
        vame_mvp, whose .mv is the [4][2] pointer table the seeds travel in:
        every (r, alignment) with a PRED in `preds` must be there."""
        out = Mvp()
        for r in range(nrefs):
            for a in (0, 1):
                if (preds >> (2 * a)) & 3:
                    t = mvs.get((r, a)) if isinstance(mvs, dict) else None
                    out.mv[r][a] = self._check_seed(t, a, f"{what}[{(r, a)}]", torch.int32, (2,)).data_ptr()
        return out

    @staticmethod
    def _widen(cus: torch.Tensor, preds: torch.Tensor | None = None):
        """Uni descriptors [n, 12] as uni bi descriptors [n, 20] (ref1 = -1), and
        their predictors [n, 7] at the rows 2i of a [2n, 7] tensor."""
        wide = torch.zeros((cus.shape[0], 20), dtype=torch.int32, device=cus.device)
        wide[:, :12] = cus
        wide[:, 12] = -1
        if preds is not None:
            p2 = torch.zeros((cus.shape[0], 2, 7), dtype=torch.int32, device=cus.device)
            p2[:, 0] = preds
            preds = p2.reshape(-1, 7)
        return wide, preds

    def affine_mc_p(self, cus: torch.Tensor, preds: torch.Tensor | None, refs, lam: float = 0.0,
                    cur: torch.Tensor | None = None, pred: torch.Tensor | None = None, want_cost: bool = False,
                    ncus: torch.Tensor | None = None):
        """vame_affine_mc_bi_p: affine_mc_bi whose cost prices every hypothesis
        against a predictor, floor(lam * (bits_p + 2)) per hypothesis (include/
        vame.h).  cus: int32 [n, 20] (vame.bipred.BICU_FIELDS) with preds int32
        [2n, 7], hypothesis h of descriptor i at row 2i + h (the second is not
        read for a uni descriptor), or int32 [n, 12] (vame.mc.CU_FIELDS) with
        preds [n, 7]: those are widened to uni bi descriptors on the device.
        A predictor row is (nCPs -- ignored --, LTx, LTy, RTx, RTy, LBx, LBy),
        components in [-2^17, 2^17 - 1]; one out of range makes its descriptor
        invalid.  preds None: the zero predictor, affine_mc_bi's outputs bit
        for bit.  The samples do not depend on the predictor.  Returns (pred,
        cost, bad) as affine_mc.  Not available under PROF."""
        if cus.dim() == 2 and cus.shape[1] == 12:
            self._check_cus(cus, 12)
            self._check_preds(preds, cus.shape[0], "affine_mc_p")
            cus, preds = self._widen(cus, preds)
        return self._mc_bi("affine_mc_p", cus, preds, refs, lam, cur, pred, want_cost, ncus)

    def affine_search_p(self, cus: torch.Tensor, preds: torch.Tensor | None, refs, cur, lam: float, extra: int = 0,
                        ncus: torch.Tensor | None = None, out: torch.Tensor | None = None,
                        cost: torch.Tensor | None = None):
        """vame_affine_search_p: affine_search with the rate of every iteration
        taken against preds[i] (int32 [n, 7], as affine_mc_p), so the predictor
        takes part in which iteration wins.  cost is affine_mc_p's cost of out
        with the same predictors.  preds None: affine_search bit for bit."""
        L = lib()
        return self._refine(L.vame_affine_search, L.vame_affine_search_p, 12, 1, "extra", 64,
                            cus, preds, refs, cur, lam, extra, ncus, out, cost)

    def bipred_refine_p(self, cus: torch.Tensor, preds: torch.Tensor | None, refs, cur, lam: float, rounds: int = 2,
                        count: torch.Tensor | None = None, out: torch.Tensor | None = None,
                        cost: torch.Tensor | None = None):
        """vame_bipred_refine_p: bipred_refine with hypothesis h of descriptor i
        priced against preds[2i + h] (int32 [2n, 7]) in the start cost and in
        every comparison.  The cost never rises and is affine_mc_p's cost of
        out.  preds None: bipred_refine bit for bit."""
        L = lib()
        return self._refine(L.vame_bipred_refine, L.vame_bipred_refine_p, 20, 2, "rounds", 4,
                            cus, preds, refs, cur, lam, rounds, count, out, cost)

    def reprice(self, lam: float, result: dict, mvp: dict, preds: int | None = None):
        """vame_reprice: replace, in place, the zero-predictor rate in the costs
        of `result` (an alloc_poc dict as the search filled it, same lam) by
        the rate against each row's predictor mvp[(r, a)][row] (LT = RT = LB):
        every in-frame row of every PRED in `preds` (None: all the dict
        holds).  CPMVs are untouched.  A second call prices twice.  Returns
        (result, bad): bad is 1 when a predictor was out of range (its row is
        skipped).  Pure arithmetic; reads nothing on the host."""
        preds = self._preds(result, preds)
        nrefs, pr = self._check_result(result, preds, "reprice")
        m = self._mv_table(mvp, nrefs, preds, "reprice: mvp")
        bad = self._bad()
        check(lib().vame_reprice(self._h, nrefs, float(lam), preds, ctypes.byref(m), ctypes.byref(pr), _ptr(bad),
                                 self._stream()))
        return result, bad

    def affine_me_seeded_p(self, cur, refs, lam: float, result: dict, seeds: dict, mvp: dict, modes: int = 3,
                           extra: int = 0):
        """vame_affine_me_seeded_p: affine_me_seeded whose two searches price
        against the row's predictor mvp[(r, a)][row]; `result` is expected
        re-priced under the same mvp (reprice()).  With an all-zero mvp it is
        affine_me_seeded bit for bit.  Returns (result, bad): bad is 1 when a
        seed or a predictor was out of range (its row is skipped)."""
        if mvp is None:
            raise ValueError("affine_me_seeded_p needs mvp")
        return self._seeded("affine_me_seeded_p", cur, refs, lam, result, seeds, mvp, modes, extra)

    def bipred_p(self, cur, refs, lam: float, result: dict, mvp: dict, preds: int | None = None,
                 out: dict | None = None):
        """vame_bipred_p: bipred whose bi cost prices hypothesis r against the
        row's predictor mvp[(r, a)][row]; the hypotheses are still picked by
        the costs of `result`, which the caller has re-priced (reprice()).  A
        row with a predictor out of range keeps INT64_MAX and -1.  Arguments
        and the returned dict as bipred."""
        if mvp is None:
            raise ValueError("bipred_p needs mvp")
        return self._bipred("bipred_p", cur, refs, lam, result, mvp, preds, out)

    def leaf_predictors(self, part: dict, mvp: dict, out: torch.Tensor | None = None) -> torch.Tensor:
        """vame_mvp_gather on the leaves of a partition() or partition_bi()
        result, their count read on the device: int32 [2 * nCtus*64, 7], the
        predictor of hypothesis h of leaf i at row 2i + h -- the mvp row of
        (ref, alignment, candidate row) expanded to LT = RT = LB, zero where
        the leaf is no candidate CU or mvp holds no array for (ref,
        alignment).  Uni leaves of partition() (12 columns) are widened on the
        device; affine_mc_p takes cus[:, :12] with rows 0::2, or the widened
        form.  Rows of leaves past the count are not written (zero in a new
        tensor).  No host read; asynchronous on the current stream."""
        cus = part["cus"]
        if cus.dim() == 2 and cus.shape[1] == 12:
            self._check_cus(cus, 12)
            cus = self._widen(cus)[0]
        self._check_cus(cus, 20)
        n = cus.shape[0]
        self._check_scalar(part["ncus"], "ncus")
        if out is None:
            out = torch.zeros((2 * n, 7), dtype=torch.int32, device=self.device)
        self._check_preds(out, 2 * n, "leaf_predictors")
        m = Mvp()
        for (r, a), t in mvp.items():
            if not (0 <= r < 4 and a in (0, 1)):
                raise ValueError(f"unexpected mvp key {(r, a)}")
            m.mv[r][a] = self._check_seed(t, a, f"mvp[{(r, a)}]", torch.int32, (2,)).data_ptr()
        check(lib().vame_mvp_gather(self._h, ctypes.byref(m), _ptr(cus), n, _ptr(part["ncus"]), _ptr(out),
                                    self._stream()))
        return out

    def affine_me_poc(self, cur, refs, lam: float, modes: int = 3, extra: int = 0, out=None):
        """modes: 1 = 2-CP only, 3 = 2-CP then 3-CP, plus MODE_FULL / MODE_HALF to
        code one alignment only.  Returns {(refIdx, MODE): (cost, cpmv)}."""
        cur = self._frame(cur)
        refs, ref_ptrs = self._refs(refs, "affine_me_poc")
        out = out if out is not None else self.alloc_poc(len(refs), modes)
        self._check_poc_out(out, len(refs), modes)
        pr = _poc_result(out)
        check(lib().vame_affine_me_poc(self._h, _ptr(cur), ref_ptrs, len(refs), float(lam), modes,
                                       extra, ctypes.byref(pr), self._stream()))
        return out

"""Frame-sharded end-to-end run over N GPUs, one process per GPU (BASELINE
configs[4]): the reference's ./main contract -- CSV frames in,
the 40 per-CU decision-log CSVs out (main.cpp:293-330, :578-1003;
main_aux_functions.h:387-525) -- with the POC loop cut into contiguous
(POC, refIdx) pair blocks, one per rank (`shard.pair_shard`).

    python -m vame.distrun -f 240 -s 3840x2160 -q 32 -o orig.csv -r recon.csv \\
        -l logs/out [--gpus N] [--shard-logs [--merge-parts] | --gather-records]
        [--modes all|2cp] [--ExtraGradientIter E]

Every rank reads only the frames its block uses (`vame_read_frames_span`,
each launch's frames parsed just before they go up, beside the kernels of
the launches before), codes its block in launches of up to 32 pairs
(`vame_affine_me_batch`; the first launch small, so the GPU starts early),
and copies each launch's results to pinned host memory while the GPU runs the
next one.  The logs are written in the reference's order by one of three paths:

  default       the decision-log gather of byte counts: every rank formats
                its own block as it completes -- rank 0 into the final files,
                rank k into host memory (a deferred `vame_log_writer`) -- then
                the ranks gather their byte counts per file (one all_reduce,
                RCCL) and write their blocks into the final files at their
                offsets, all ranks in parallel (pwrite), so formatting and
                writing scale with the ranks.
  --shard-logs  per-rank files: rank 0 appends to the final files,
                rank k to its own part files `<log>.partK_*` (headerless), each
                as its launches complete, so nothing is left to write after a
                rank's last launch.  The final files are the `cat` of rank 0's
                and the parts in rank order (`vame.logs.merge_parts`, or
                `--merge-parts`: rank 0 appends them after the last rank ends).
  --gather-records  the records themselves to rank 0: every other rank packs
                its records compactly on its GPU (`shard.pack`), and after the
                last launch one gather (RCCL over xGMI) brings them to rank 0,
                which formats and writes them POC by POC (rank 0's CPU formats
                the whole log; for file systems the ranks do not share).

Blocks are contiguous in coding order, and a POC cut between two ranks is cut
at a refIdx boundary (refIdx is the outer loop of every file's rows), so both
paths give files byte-identical to a one-process run (tests/test_distrun.py).
Without a launcher, `--gpus N` starts the N ranks itself (vame.launch).
"""
from __future__ import annotations

import argparse
import contextlib
import json
import os
import queue
import sys
import threading
import time

import numpy as np
import torch

from . import logs, shard
from .engine import pred_mask
from .hostlogic import lambda_for_poc, ref_list

RESOLUTIONS = ((3840, 2160), (1920, 1080), (1280, 720), (832, 480), (416, 240))  # constants.h:73-79
MAX_PAIRS = 32  # pairs per launch (vame_affine_me_batch)


def parse_args(argv=None) -> argparse.Namespace:
    """The reference's options (main.cpp:58-69) plus the frame-shard ones."""
    ap = argparse.ArgumentParser(prog="vame.distrun")
    ap.add_argument("-f", "--FramesToBeEncoded", dest="frames", type=int, required=True)
    ap.add_argument("-s", "--Resolution", dest="res", required=True)
    ap.add_argument("-q", "--QP", dest="qp", type=int, required=True)
    ap.add_argument("-o", "--OriginalFrames", dest="orig", required=True)
    ap.add_argument("-r", "--ReferenceFrames", dest="recon", required=True)
    ap.add_argument("-l", "--CpmvLogFile", dest="log", default="")
    ap.add_argument("--ExtraGradientIter", dest="extra", type=int, default=0)
    ap.add_argument("--modes", choices=("all", "2cp"), default="all")
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--gather-records", action="store_true",
                    help="gather the decision records into rank 0, which formats the whole log")
    ap.add_argument("--shard-logs", action="store_true",
                    help="every rank appends its block to its own part files as it goes (<log>.partK_*)")
    ap.add_argument("--merge-parts", action="store_true",
                    help="with --shard-logs: rank 0 appends the part files to the final ones at the end")
    ap.add_argument("--rank-only", type=int, default=None, metavar="K",
                    help="run only rank K's share of a --gpus N job, alone on GPU 0 (no collective; "
                         "its logs stay part files): prices one rank of an N-GPU node on one GPU")
    a = ap.parse_args(argv)
    try:
        a.W, a.H = (int(v) for v in a.res.lower().split("x"))
    except ValueError:
        ap.error(f"bad resolution {a.res!r}")
    if (a.W, a.H) not in RESOLUTIONS:
        ap.error(f"unsupported resolution {a.W}x{a.H}")
    if a.frames < 1 or a.gpus < 1 or not 0 <= a.extra <= 64:
        ap.error("frames and gpus must be >= 1, ExtraGradientIter in 0..64")
    if a.rank_only is not None and not 0 <= a.rank_only < a.gpus:
        ap.error("--rank-only K needs 0 <= K < --gpus")
    if a.gather_records and a.shard_logs:
        ap.error("--gather-records and --shard-logs are two log paths: pick one")
    if a.merge_parts and not a.shard_logs:
        ap.error("--merge-parts goes with --shard-logs")
    a.log_path = "gather" if a.gather_records else "parts" if a.shard_logs else "place"
    if shard.sequence_pairs(a.frames) < a.gpus:  # every rank codes at least one pair
        ap.error(f"--gpus {a.gpus} needs at least as many (POC, refIdx) pairs "
                 f"({shard.sequence_pairs(a.frames)} in {a.frames} frames)")
    a.mode_mask = 3 if a.modes == "all" else 1
    return a


part_prefix = logs.part_prefix


def launch_batches(blocks, first: int = MAX_PAIRS):
    """The block's entries in launches of at most MAX_PAIRS pairs (entries
    whole); the first launches ramp up from `first` pairs, doubling (the GPU
    starts once the first launch's few frames are parsed, and each launch's
    kernels cover the parsing of the next, larger one's frames)."""
    out, cur, n = [], [], 0
    for poc, refs in blocks:
        if cur and n + len(refs) > min(MAX_PAIRS, first << len(out)):
            out.append(cur)
            cur, n = [], 0
        cur.append((poc, refs))
        n += len(refs)
    if cur:
        out.append(cur)
    return out


@contextlib.contextmanager
def _owned(*steps):
    """A scope that releases what it started: on every way out each of `steps`
    runs, in order, whatever the ones before it did.  The first error -- the
    body's, else the first a step raised -- is the one raised; a later one
    never replaces it."""
    err = None
    try:
        yield
    except BaseException as e:  # raised again below, after the steps
        err = e
    for step in steps:
        try:
            step()
        except BaseException as e:  # kept only if it is the first
            err = err or e
    if err is not None:
        raise err


class _Streams:
    """The caller's compute stream and the two copy streams of a rank (all None
    on a CPU rank).  Frames go up and results come back on streams of their
    own, and those take an explicit priority (VAME_COPY_PRIO, default -1): HIP
    maps streams onto 4 hardware queues in creation order, and a copy stream
    sharing the compute stream's queue puts each launch's result download in
    front of the next launch (the vame CLI measured 5.1 ms of idle GPU per
    4-POC 4K launch that way).  So: upload before download, both before the
    first launch, and no other stream."""

    def __init__(self, device):
        self.device, self.cuda = device, device.type == "cuda"
        self.compute = self.up = self.down = None
        if self.cuda:
            prio = int(os.environ.get("VAME_COPY_PRIO", "-1"))
            self.compute = torch.cuda.current_stream(device)
            self.up = torch.cuda.Stream(device, priority=prio)
            self.down = torch.cuda.Stream(device, priority=prio)

    def on(self, stream):
        return torch.cuda.stream(stream) if self.cuda else contextlib.nullcontext()

    def synchronize(self) -> None:
        """Wait for everything the rank has queued on its device."""
        if self.cuda:
            torch.cuda.synchronize(self.device)


class Ingest:
    """Frame ingest: only the frames this block reads (main.cpp:293-330).
    Text lines have no fixed length, so the ranks first index the CSVs
    together: rank r counts the newlines of chunks r, r + N, ... and one
    all_reduce shares the counts; each rank then parses only the chunks that
    hold its frames.  With the line index, each launch's frames are parsed just
    before they go up, by the uploader thread (`read_launch`), so the GPU starts
    after the first launch's frames only and the rest of the ingest runs beside
    the kernels (the reference reads every frame first); without it (a one-rank
    run, raw frames) the block's frames are read at once, here."""

    def __init__(self, a, world: int, rank: int, dist, blocks):
        t = time.perf_counter()
        self.W, self.H, self.paths = a.W, a.H, (a.orig, a.recon)
        self.orig, self.recon = {}, {}  # host frames by POC
        self.parse_s = 0.0  # time in read_into: the uploader thread's once it runs
        self.T = {}  # index_others_s (--rank-only), index_s, read_csv_s
        self.idx = {path: line_index(path, world, rank, dist, self.T) for path in self.paths}
        others = self.T.get("index_others_s", 0.0)
        self.T["index_s"] = time.perf_counter() - t - others
        self.overlap = bool(blocks) and all(i is not None for i in self.idx.values())
        if blocks and not self.overlap:
            self.read_launch(blocks)
        self.T["read_csv_s"] = time.perf_counter() - t - others

    def read_into(self, store: dict, path: str, frames) -> None:
        """Parse `frames` (POC numbers, 0-based frame index in the file) of
        `path` into `store`, one contiguous run of frames per read."""
        frames = sorted(f for f in set(frames) if f not in store)
        t0 = time.perf_counter()
        k = 0
        while k < len(frames):
            e = k
            while e + 1 < len(frames) and frames[e + 1] == frames[e] + 1:
                e += 1
            first, n = frames[k], frames[e] - frames[k] + 1
            idx = self.idx[path]
            span = None if idx is None else logs.line_span(*idx, first * self.H, (first + n) * self.H)
            got = logs.read_frames(path, self.W, self.H, n, first=first, span=span)
            for i in range(n):
                store[first + i] = got[i]
            k = e + 1
        self.parse_s += time.perf_counter() - t0

    def read_launch(self, batch) -> None:
        """The frames the pairs of `batch` read."""
        self.read_into(self.orig, self.paths[0], [p - 1 for p, _ in batch])
        self.read_into(self.recon, self.paths[1], [ref_list(p)[r] for p, refs in batch for r in refs])

    def drop_through(self, poc: int) -> None:
        """Forget the original frames of POCs up to `poc` (no later launch reads them)."""
        for q in [q for q in self.orig if q + 1 <= poc]:
            del self.orig[q]


class Uploader:
    """Frames go to the device launch by launch, ahead of the kernels, from a
    thread and on a stream of their own (copies from pageable memory block the
    calling thread, so the launching thread never waits for them); the compute
    stream waits for each launch's upload event (`wait`)."""

    def __init__(self, ingest: Ingest, batches, streams: _Streams, t_start: float):
        self.ingest, self.batches, self.streams, self.t_start = ingest, batches, streams, t_start
        self.d_orig, self.d_recon = {}, {}  # device frames by POC
        self.ready = [threading.Event() for _ in batches]
        self.events = [None] * len(batches)
        self.error = None  # what the thread raised
        self.first_frames_s = None  # launch 0's frames parsed, since t_start (overlapped ingest)
        self._halt = threading.Event()
        self._thread = threading.Thread(target=self._run, name="vame-distrun-uploader")

    def start(self) -> None:
        self._thread.start()

    def stop_and_join(self) -> None:
        self._halt.set()
        if self._thread.ident is not None:
            self._thread.join()

    def wait(self, b: int):
        """Block until launch b's frames are queued; its upload event (None on
        a CPU rank).  Raises what the thread raised."""
        self.ready[b].wait()
        if self.error is not None:
            raise self.error
        return self.events[b]

    def frames(self, poc: int, refs):
        """(current frame, [reference frames]) of one entry, on the device."""
        rl = ref_list(poc)
        return self.d_orig[poc], [self.d_recon[rl[r]] for r in refs]

    def _run(self) -> None:
        s = self.streams
        try:
            with (torch.cuda.device(s.device) if s.cuda else contextlib.nullcontext()), s.on(s.up):
                for b, batch in enumerate(self.batches):
                    if self._halt.is_set():
                        break
                    self._upload(b, batch)
        except Exception as e:  # surfaced by the launching thread (wait)
            self.error = e
        finally:
            for ev in self.ready:
                ev.set()

    def _upload(self, b: int, batch) -> None:
        ing, s = self.ingest, self.streams
        if ing.overlap:  # this launch's frames, parsed now
            ing.read_launch(batch)
            if b == 0:
                self.first_frames_s = time.perf_counter() - self.t_start
        for poc, refs in batch:
            rl = ref_list(poc)
            self._frame(self.d_orig, poc, ing.orig[poc - 1])
            for r in refs:
                self._frame(self.d_recon, rl[r], ing.recon[rl[r]])
        if ing.overlap:
            ing.drop_through(max(p for p, _ in batch))
        if s.cuda:
            self.events[b] = torch.cuda.Event()
            self.events[b].record(s.up)
        self.ready[b].set()

    def _frame(self, store: dict, key: int, host) -> None:
        if key not in store:
            t = torch.from_numpy(np.ascontiguousarray(host).view(np.int16))
            if self.streams.cuda:
                t = t.to(self.streams.device, non_blocking=True)
                t.record_stream(self.streams.compute)
            store[key] = t


class _HostSlots:
    """Pinned host copies of the results of a launch, one set per slot
    (reused when the writer has finished with it)."""

    def __init__(self, n_slots: int, pin: bool):
        self.free = queue.Queue()
        self.bufs = [dict() for _ in range(n_slots)]
        self.pin = pin
        for s in range(n_slots):
            self.free.put(s)

    def host_like(self, slot: int, key, t: torch.Tensor) -> torch.Tensor:
        b = self.bufs[slot].get(key)
        if b is None or b.shape != t.shape:
            b = torch.empty(t.shape, dtype=t.dtype, pin_memory=self.pin)
            self.bufs[slot][key] = b
        return b


def host_records(refs, res) -> dict:
    """One entry's records as `logs.write_poc` takes them: keyed by the true
    refIdx (refs[j]; `res` is keyed by the index within the entry), numpy."""
    return {(refs[j], name): (c.cpu().numpy(), p.cpu().numpy()) for (j, name), (c, p) in res.items()}


class LogSink:
    """Where a rank's records go on the host: its LogWriter (if `role` gives it
    one), the two pinned slots each launch's results are copied into on the
    download stream while the GPU runs the next launch, and the writer thread
    that formats a launch's POCs once its copy has landed."""

    def __init__(self, role: logs.LogRole, W: int, H: int, streams: _Streams):
        self.role, self.W, self.H, self.streams = role, W, H, streams
        self.writer = None
        self.slots = _HostSlots(2, streams.cuda)
        self.work: queue.Queue = queue.Queue()
        self.error = None  # what the thread raised
        self.log_bytes, self.log_write_s = 0, 0.0  # the thread's until it is joined, then the caller's
        self._thread = threading.Thread(target=self._run, name="vame-distrun-log-writer")

    def open(self) -> None:
        """Remove old files, create the writer, start the thread."""
        if self.role.remove_old:
            logs.remove_old(self.role.prefix)
        if self.role.writer != "none":
            self.writer = logs.LogWriter(self.role.prefix, self.W, self.H)
            if self.role.writer == "deferred":
                self.writer.defer()
        self._thread.start()

    def write(self, poc: int, refs, res) -> None:
        self.log_bytes += logs.write_poc(self.role.prefix, self.W, self.H, poc, host_records(refs, res),
                                         writer=self.writer)

    def _run(self) -> None:
        try:
            while (item := self.work.get()) is not None:
                ev, slot, batch, host = item
                if ev is not None:
                    ev.synchronize()
                t0 = time.perf_counter()
                for (poc, refs), res in zip(batch, host):
                    self.write(poc, refs, res)
                self.log_write_s += time.perf_counter() - t0
                self.slots.free.put(slot)
        except Exception as e:  # surfaced by end_and_join
            self.error = e
            self.slots.free.put(-1)

    def download(self, batch, outs) -> bool:
        """Queue the copy of one launch's results into a free slot and hand it
        to the thread; False once the thread has failed."""
        slot = self.slots.free.get()
        if slot < 0:
            return False
        s, host = self.streams, []
        if s.cuda:
            s.down.wait_stream(torch.cuda.current_stream(s.device))
        with s.on(s.down):
            for i, out in enumerate(outs):
                h = {}
                for key, (c, p) in out.items():
                    hc = self.slots.host_like(slot, (i, key, 0), c)
                    hp = self.slots.host_like(slot, (i, key, 1), p)
                    hc.copy_(c, non_blocking=s.cuda)
                    hp.copy_(p, non_blocking=s.cuda)
                    if s.cuda:  # the launch's buffers stay allocated until the copy ran
                        c.record_stream(s.down)
                        p.record_stream(s.down)
                    h[key] = (hc, hp)
                host.append(h)
            ev = None
            if s.cuda:
                ev = torch.cuda.Event()
                ev.record(s.down)
        self.work.put((ev, slot, batch, host))
        return True

    def end_and_join(self) -> None:
        """Let the thread finish what is queued; raises what it raised."""
        if self._thread.ident is not None:
            self.work.put(None)
            self._thread.join()
        if self.error is not None:
            raise self.error

    def close(self) -> None:
        if self.writer is not None:
            self.writer.close()


class PackedRecords:
    """The gather path's records: packed compactly per launch and kept on this
    GPU until the gather.  The compact-form check is collected on the device
    and read once after the last launch (`check`; a per-launch read would stall
    the launching thread until that launch finished)."""

    def __init__(self, engine, modes: int, device):
        self.engine, self.modes, self.device = engine, modes, device
        self.hip = hasattr(engine, "pack_records")  # the HIP engine packs in one kernel
        self.bad = torch.zeros((), dtype=torch.int32 if self.hip else torch.bool, device=device)
        self.parts = []

    def add(self, outs) -> None:
        if self.hip:
            self.parts.append(self.engine.pack_records(outs, self.modes, None, self.bad))
        else:
            self.parts.append(shard.pack(outs, None, self.device, modes=self.modes, validate=self.bad))

    def check(self) -> None:
        if self.parts:
            shard.check_flag(self.bad)

    def slab(self, words: int) -> torch.Tensor:
        mine = torch.cat(self.parts) if self.parts else torch.empty(0, dtype=torch.int32, device=self.device)
        return torch.cat([mine, mine.new_zeros(words - mine.numel())])


def _launch_all(a, engine, batches, uploader: Uploader, sink: LogSink, packed: PackedRecords,
                streams: _Streams) -> list:
    """The hot path: this block's launches.  Returns the timing event pair of
    each (none on a CPU rank); stops early once the writer thread has failed."""
    spans = []
    for b, batch in enumerate(batches):
        up_event = uploader.wait(b)
        jobs = [(*uploader.frames(poc, refs), lambda_for_poc(a.qp, poc),
                 engine.alloc_poc(len(refs), a.mode_mask)) for poc, refs in batch]
        if streams.cuda:
            streams.compute.wait_event(up_event)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        engine.affine_me_batch(jobs, a.mode_mask, a.extra)
        if streams.cuda:
            e1.record()
            spans.append((e0, e1))
        outs = [j[3] for j in jobs]
        if sink.role.download:
            if not sink.download(batch, outs):
                break
        elif sink.role.pack:
            packed.add(outs)
    return spans


def exchange_sizes(dist, world: int, rank: int, mine: list[int]) -> list[int]:
    """The byte counts per file of every rank's block, shared by one
    all_reduce; returns this rank's offsets: the sizes of the ranks before it."""
    sizes = torch.zeros((world, len(mine)), dtype=torch.int64)
    sizes[rank] = torch.tensor(mine, dtype=torch.int64)
    _all_reduce_cpu(dist, sizes)
    return sizes[:rank].sum(0).tolist()


def gather_records(a, world: int, n_cus, packed: PackedRecords, sink: LogSink, dist) -> float:
    """--gather-records: one gather of equal-size slabs brings every rank's
    packed records to rank 0, which formats and writes them POC by POC.
    Returns the time the gather took."""
    t = time.perf_counter()
    modes = a.mode_mask
    shards = [shard.pair_shard(a.frames, world, r) for r in range(world)]
    slab = packed.slab(max(shard.slab_words(shard.block_layout(s, modes, n_cus)) for s in shards))
    if dist.get_backend() == "gloo":
        slab = slab.cpu()
    slabs = shard.gather_to_root(slab, world, 0)
    sink.streams.synchronize()
    gather_s = time.perf_counter() - t
    if slabs is not None:  # rank 0
        t0 = time.perf_counter()
        for r in range(0 if sink.role.unpack_own else 1, world):
            o = 0
            for poc, refs in shards[r]:
                w = shard.poc_words(len(refs), modes, n_cus)
                sink.write(poc, refs, shard.unpack(slabs[r][o:o + w], [(len(refs), modes, n_cus)])[0])
                o += w
        sink.log_write_s += time.perf_counter() - t0
    return gather_s


def place_block(a, world: int, rank: int, sink: LogSink, dist) -> None:
    """The default path's end: every rank's block into the final files at its
    byte offsets (the sizes of the ranks before it), all ranks in parallel.
    Rank 0 has appended its block already and only reports its sizes; without
    the exchange (--rank-only K) the block goes into its part files alone."""
    role = sink.role
    mine = (sink.writer.held_sizes() if role.place else
            [os.path.getsize(n) if os.path.exists(n) else 0 for n in logs.log_names(a.log)])
    offsets = exchange_sizes(dist, world, rank, mine) if role.exchange else [0] * len(mine)
    if role.place:
        sink.writer.flush_at(offsets)
        sink.close()


def merge(a, world: int) -> float:
    """--merge-parts: rank 0 appends the part files; returns the time it took."""
    t = time.perf_counter()
    logs.merge_parts(a.log, world, pred_mask(a.mode_mask))
    return time.perf_counter() - t


def _end_phase(a, world: int, rank: int, n_cus, packed: PackedRecords, sink: LogSink, dist) -> dict:
    """What is left after the last launch, by the rank's role; the collectives
    in the same order on every rank (gather, or the size exchange; barrier)."""
    role, T = sink.role, {"gather_s": 0.0, "merge_s": 0.0}
    if role.gather:
        T["gather_s"] = gather_records(a, world, n_cus, packed, sink, dist)
    if not role.place:
        sink.close()  # rank 0's final files, or this rank's part files, are complete
    if role.place or role.exchange:
        t = time.perf_counter()
        place_block(a, world, rank, sink, dist)
        if role.place:
            T["merge_s"] = time.perf_counter() - t
    if role.barrier:
        dist.barrier()  # every block is in place (or in its part files)
    if role.merge:
        T["merge_s"] = merge(a, world)
    return T


def _timings(rank: int, blocks, ingest: Ingest, uploader: Uploader, sink: LogSink, spans, ends: dict,
             t_start: float) -> dict:
    """The rank's timing record, from what each step measured (all threads
    joined, the device idle)."""
    T = {"rank": rank, "pairs": sum(len(r) for _, r in blocks), "pocs": len(blocks),
         "read_csv_s": 0.0, "kernel_s": 0.0, "log_write_s": sink.log_write_s, "log_bytes": sink.log_bytes,
         **ends, **ingest.T}
    if uploader.first_frames_s is not None:
        T["first_frames_s"] = uploader.first_frames_s
    if ingest.overlap:  # parsed in the uploader thread, beside the launches
        T["read_csv_s"] += ingest.parse_s
        T["read_csv_overlapped"] = True
    if spans:
        T["kernel_s"] = sum(x.elapsed_time(y) for x, y in spans) * 1e-3
        # GPU idle between this rank's launches
        T["gpu_gaps_s"] = spans[0][0].elapsed_time(spans[-1][1]) * 1e-3 - T["kernel_s"]
    T["overall_s"] = time.perf_counter() - t_start
    return T


def run_rank(a, world: int, rank: int, engine, device, dist=None) -> dict:
    """One rank's whole run; returns its timings.  `engine` needs n_cus,
    alloc_poc and affine_me_batch (vame.engine.Engine on the GPU; the tests
    pass an oracle-backed stand-in on CPU ranks).  Whatever way it ends, the
    uploader is stopped and joined, the writer thread ended and joined, the
    device drained and the LogWriter closed, in that order, and the first
    error is the one raised."""
    t_start = time.perf_counter()
    n_cus = (engine.n_cus(0), engine.n_cus(1))
    role = logs.log_role(a.log, a.log_path, world, rank, dist is not None, a.merge_parts)
    blocks = shard.pair_shard(a.frames, world, rank)
    ingest = Ingest(a, world, rank, dist, blocks)
    batches = launch_batches(blocks, int(os.environ.get("VAME_FIRST_LAUNCH_PAIRS", "8")) if ingest.overlap
                             else MAX_PAIRS)
    streams = _Streams(device)
    uploader = Uploader(ingest, batches, streams, t_start)
    sink = LogSink(role, a.W, a.H, streams)
    with _owned(uploader.stop_and_join, sink.end_and_join, streams.synchronize, sink.close):
        uploader.start()
        sink.open()
        packed = PackedRecords(engine, a.mode_mask, device)
        spans = _launch_all(a, engine, batches, uploader, sink, packed, streams)
        uploader.stop_and_join()
        sink.end_and_join()
        packed.check()
        streams.synchronize()
        ends = _end_phase(a, world, rank, n_cus, packed, sink, dist)
    return _timings(rank, blocks, ingest, uploader, sink, spans, ends, t_start)


def line_index(path: str, world: int, rank: int, dist, T: dict):
    """(chunk byte bounds, newline prefix counts) of a CSV, or None for raw
    frames / a one-rank run (which reads its frames from the start).  Rank r
    counts chunks r, r + world, ...; an all_reduce sums the counts.  Without
    a process group (--rank-only) the other ranks' chunks are counted here too,
    and that time is kept apart (T["index_others_s"]): on a node those chunks
    are counted by the other ranks, at the same time."""
    if world == 1 or path.endswith((".u16", ".yuv")):
        return None
    size = os.path.getsize(path)
    K = max(world, min(64 * world, size >> 22))  # chunks of >= 4 MiB
    bounds = [size * k // K for k in range(K + 1)]
    counts = torch.zeros(K, dtype=torch.int64)
    mine = list(range(rank, K, world))  # one native pass over this rank's chunks
    counts[mine] = torch.tensor(logs.count_lines_ranges(path, [(bounds[k], bounds[k + 1]) for k in mine]))
    if dist is not None:
        _all_reduce_cpu(dist, counts)
    else:
        t = time.perf_counter()
        others = [k for k in range(K) if k % world != rank]
        if others:
            counts[others] = torch.tensor(logs.count_lines_ranges(path, [(bounds[k], bounds[k + 1])
                                                                         for k in others]))
        T["index_others_s"] = T.get("index_others_s", 0.0) + time.perf_counter() - t
    prefix = [0] + torch.cumsum(counts, 0).tolist()
    return bounds, prefix


def _all_reduce_cpu(dist, t: torch.Tensor) -> None:
    """Sum a small CPU tensor over the ranks (through the GPU under RCCL)."""
    if dist.get_backend() == "nccl":
        c = t.cuda()
        dist.all_reduce(c)
        t.copy_(c.cpu())
    else:
        dist.all_reduce(t)


def report(a, per_rank: list[dict]) -> str:
    """The reference's timing block (main_aux_functions.h:1416-1446) over the
    whole job: wall-clock figures are the max over ranks, kernel time summed."""
    mx = lambda k: max(t[k] for t in per_rank)  # noqa: E731
    lines = ["=-=-=-=-=-=-=-=-=-=-=-=-=-=-=-=-=-=-=-=-=-=-=", "TIMING RESULTS (nanoseconds)",
             f"TOTAL_EXEC_TIME({a.frames}x),{sum(t['kernel_s'] for t in per_rank) * 1e9:f}",
             f"MAX_RANK_EXEC_TIME,{mx('kernel_s') * 1e9:f}",
             f"OVERALL({a.frames}x),{mx('overall_s'):f}",
             f"READ_CSV_TIME,{mx('read_csv_s') * 1e9:f}",
             f"LOG_WRITE_TIME,{mx('log_write_s') * 1e9:f}",
             f"LOG_GATHER_TIME,{mx('gather_s') * 1e9:f}",
             f"LOG_MERGE_TIME,{mx('merge_s') * 1e9:f}",
             f"LOG_BYTES,{sum(t['log_bytes'] for t in per_rank)}",
             "=-=-=-=-=-=-=-=-=-=-=-=-=-=-=-=-=-=-=-=-=-=-=",
             "DISTRUN " + json.dumps({"ranks": len(per_rank), "log_path": a.log_path,
                                      "per_rank": per_rank})]
    return "\n".join(lines)


def main(argv=None) -> int:
    a = parse_args(argv)
    from .launch import init_rank, launch_ranks
    backend = os.environ.get("VAME_DIST_BACKEND", "nccl")
    if a.rank_only is not None:  # one rank of an N-rank job, alone (no process group)
        from .engine import Engine
        torch.cuda.set_device(0)
        dev = torch.device("cuda", 0)
        eng = Engine(a.W, a.H, 0)
        try:
            if a.log_path == "gather":  # no collective: its rows stay in its own (part) files
                a.log_path = "place"
            T = run_rank(a, a.gpus, a.rank_only, eng, dev)
        finally:
            eng.close()
        print(report(a, [T]), flush=True)
        return 0
    if "WORLD_SIZE" not in os.environ:
        if a.gpus > 1:  # no launcher: start the ranks (nothing has touched the GPU yet)
            return launch_ranks(a.gpus, ["-m", "vame.distrun"] + (sys.argv[1:] if argv is None else argv),
                                backend, "vame.distrun")
    elif int(os.environ["WORLD_SIZE"]) != a.gpus:
        print(f"vame.distrun: WORLD_SIZE={os.environ['WORLD_SIZE']} but --gpus {a.gpus}", file=sys.stderr)
        return 2
    dist, rank, dev = init_rank(a.gpus, backend)
    from .engine import Engine
    eng = Engine(a.W, a.H, dev.index)
    try:
        T = run_rank(a, a.gpus, rank, eng, dev, dist)
    finally:
        eng.close()
    per_rank = [T]
    if dist is not None:
        per_rank = [None] * a.gpus
        dist.all_gather_object(per_rank, T)
    if rank == 0:
        print(report(a, per_rank), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())

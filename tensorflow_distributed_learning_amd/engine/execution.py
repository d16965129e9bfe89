"""What the engines share about device-resident executions (engine/fused.py, engine/trainer.py,
engine/mirrored.py): the input iterator that hands out each execution's sample ids, the ring of
pinned buffers those ids are uploaded through, the bookkeeping of which K-step graphs a run replays
(one per starting accumulation phase), and the capture of such a graph.
"""
from __future__ import annotations

import contextlib
import os
import queue
import threading
from typing import List, Optional, Tuple

import numpy as np
import torch

from ..data import device as DD
from ..parallel import input_lib


class IndexRing:
    """``nslots`` pinned int32 staging buffers, one event each, handed out in rotation: the host fills
    slot i+1 while the copy out of slot i may still be in flight."""

    def __init__(self, device, nslots: int):
        self.device = device
        self.bufs: List[Optional[torch.Tensor]] = [None] * nslots
        self.events = [None] * nslots
        self._next = 0

    def next_slot(self) -> int:
        slot = self._next
        self._next = (slot + 1) % len(self.bufs)
        return slot

    def _buffer(self, slot: int, n: int) -> torch.Tensor:
        if self.events[slot] is not None:
            self.events[slot].synchronize()  # the previous copy out of this buffer has run
        buf = self.bufs[slot]
        if buf is None or buf.numel() < n:
            buf = self.bufs[slot] = torch.empty(max(n, 1024), dtype=torch.int32, pin_memory=True)
        return buf

    def reserve(self, n: int):
        """Every slot's buffer at ``n`` elements now: a pinned (hipHostMalloc) allocation inside the
        launch loop waited ~30 ms for the device."""
        for slot in range(len(self.bufs)):
            self._buffer(slot, n)

    def upload(self, idx_np: np.ndarray, dst: torch.Tensor, slot: int):
        """Asynchronous H2D copy of ``idx_np`` into ``dst[:n]`` on the current stream, through the
        slot's pinned buffer (no host synchronisation unless the slot's last copy is still running)."""
        n = int(idx_np.size)
        stage = self._buffer(slot, n)
        stage[:n].numpy()[:] = idx_np
        dst[:n].copy_(stage[:n], non_blocking=True)
        if self.events[slot] is None:
            self.events[slot] = torch.cuda.Event()
        self.events[slot].record(torch.cuda.current_stream(self.device))


def execution_starts(steps: int, K: int, accum_steps: int = 1) -> List[Tuple[int, int]]:
    """``[(K_i, t_add_i)]``: the distinct executions of a run of ``steps`` steps in executions of K, as
    (size, micro-steps from now to its start).  Without accumulation one full execution stands for
    all; an accumulating optimizer needs one per starting phase the run's executions will have.  The
    shorter last execution comes last."""
    starts = [(K, i * K) for i in range(min(steps // K, accum_steps))]
    if steps % K:
        starts.append((steps % K, steps - steps % K))
    return starts


def accum_key(opt, key: tuple, t_add: int = 0) -> tuple:
    """Key of the execution graph that starts ``t_add`` micro-steps from now; with gradient
    accumulation it carries the execution's starting phase (every step's mode is baked in).  With
    a weight EMA that overwrites every f steps (``ema_overwrite_frequency``) the phase is taken mod
    f: f is a multiple of the accumulation steps, so it tells both the accumulation phase and which
    steps of the execution overwrite.  Unchanged with EMA off."""
    if getattr(opt, "use_ema", False) and opt.ema_overwrite_frequency is not None:
        return key + (("ema", (int(opt.iterations) + int(t_add)) % opt.ema_overwrite_frequency),)
    return key + (opt._accum_phase(t_add),) if opt._accumulating else key


def weights_tag(sample_w: bool, class_w: bool) -> tuple:
    """Graph-key element of a step whose loss head reads a sample-weight column and / or the class-weight
    table: which of the two are present picks the head's kernel variant, which a capture bakes in.  Keys of
    unweighted steps carry no such element (they are what they were)."""
    return ("weights", bool(sample_w), bool(class_w))


def weights_key(key: tuple, sample_w: bool, class_w: bool) -> tuple:
    """``key`` of an execution graph, with the weights tag when the execution is weighted (it goes in front of
    the accumulation / EMA phase that ``accum_key`` appends)."""
    return key + (weights_tag(sample_w, class_w),) if sample_w or class_w else key


def has_class_weight(key: tuple) -> bool:
    return any(isinstance(e, tuple) and len(e) == 3 and e[0] == "weights" and e[2] for e in key)


def phase_period(opt, K: int = 1) -> int:
    """How many distinct starting phases the K-step executions of a run can have (the ``accum_steps``
    of ``execution_starts``): the accumulation steps, or, with EMA overwrites on, the number of
    distinct values of ``i K mod f``."""
    if getattr(opt, "use_ema", False) and opt.ema_overwrite_frequency is not None:
        import math

        f = opt.ema_overwrite_frequency
        return f // math.gcd(f, max(1, int(K)))
    return opt.gradient_accumulation_steps or 1


@contextlib.contextmanager
def capturing(device, optimizer, t_add: int = 0):
    """Capture the body of the ``with`` into the hipGraph it yields, on a fresh stream behind the
    current one.  The body is recorded as if it started ``t_add`` micro-steps from now (the
    accumulation phase of its step k: ``iterations + t_add + k``); capture records, it does not run a
    step, so ``iterations`` is restored.

    Keep this sequence (stream and its wait, then the synchronise, nothing on the capture stream afterwards):
    the fused engine's K=1000 benchmark ran 0.8 % slower from graphs captured after synchronise-then-stream
    with a ``wait_stream`` back onto the current stream at the end (profiles/engine_refactor_ab.txt)."""
    s = torch.cuda.Stream(device)
    s.wait_stream(torch.cuda.current_stream(device))
    torch.cuda.synchronize(device)
    graph = torch.cuda.CUDAGraph()
    it0 = optimizer.iterations
    optimizer.iterations = it0 + t_add
    try:
        with torch.cuda.graph(graph, stream=s):
            yield graph
    finally:
        optimizer.iterations = it0


class Prefetching:
    """Input prefetch of depth one execution for a trainer with ``_take_upload(handler, K)`` ->
    ``(handler, K, ...)`` or None, and ``K``."""

    _ready = None  # one execution's indices taken and uploaded ahead of its launch

    def prefetch(self, handler, K: int) -> bool:
        """tf.data ``prefetch`` semantics: take and upload the indices of the next K-step execution
        now, so the next ``run_train`` launches its first graph without waiting for the host's batch
        assembly.  Returns False at a ragged tail."""
        K = min(int(K), self.K)
        if self._ready is None:
            self._ready = self._take_upload(handler, K)
            return self._ready is not None
        return self._ready[1] == K

    def _next_execution(self, handler, K: int):
        """The prefetched execution (it must be the one asked for), else a fresh take + upload."""
        r, self._ready = self._ready, None
        if r is None:
            return self._take_upload(handler, K)
        if r[0] is not handler or r[1] != K:
            raise RuntimeError(f"{type(self).__name__}: prefetched execution does not match the requested steps")
        return r


class _IndexProducer:
    """Background thread producing the global-batch index arrays of an IndexStream into a bounded
    queue, so an epoch's shuffle (native, GIL released) never stalls the launch loop."""

    def __init__(self, stream: "DD.IndexStream", depth: int = 512):
        self.stream = stream
        self.q: "queue.Queue" = queue.Queue(maxsize=depth)
        self._stop = threading.Event()
        self._ended = False
        self.t = threading.Thread(target=self._run, name="tdl-index-producer", daemon=True)
        self.t.start()

    def _run(self):
        while not self._stop.is_set():
            g = self.stream.next_batch()
            item = (g, self.stream._epoch)  # epochs the stream had to generate to produce g
            while not self._stop.is_set():
                try:
                    self.q.put(item, timeout=0.1)
                    break
                except queue.Full:
                    continue
            if g is None:
                return

    def get(self):
        """(batch or None at the end, epochs generated up to it)."""
        if self._ended:
            return None, None
        g, ep = self.q.get()
        if g is None:
            self._ended = True
        return g, ep

    def close(self):
        self._stop.set()
        while True:
            try:
                self.q.get_nowait()
            except queue.Empty:
                break
        self.t.join(timeout=5)


class DeviceHandler:
    """Index vectors for this replica: its slice of every global batch."""

    def __init__(self, lp: DD.LoweredPipeline, seed: Optional[int], rank: int, R: int):
        self.lp = lp
        self.rank, self.R = rank, R
        self.B = lp.batch_size
        self.b = lp.batch_size // R
        self.stream = DD.IndexStream(lp, seed)
        self._pending = []
        self._async = os.environ.get("TDL_ASYNC_INDICES", "1") == "1"
        self._producer: Optional[_IndexProducer] = None
        self._epochs_used = 0

    def new_iterator(self):
        self.close()
        self.stream = DD.IndexStream(self.lp, self.stream._seed)
        self._pending = []
        self._epochs_used = 0

    def close(self):
        if self._producer is not None:
            self._producer.close()
            self._producer = None
        self.stream.commit(self._epochs_used)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _next_global(self):
        if self._pending:
            return self._pending.pop(0)
        if not self._async:
            g = self.stream.next_batch()
            self._epochs_used = self.stream._epoch
            return g
        if self._producer is None:
            self._producer = _IndexProducer(self.stream)
        g, ep = self._producer.get()
        if ep is not None:
            self._epochs_used = ep
        return g

    def take(self, K: int) -> Optional[np.ndarray]:
        """Up to K full global batches -> this replica's [K'*b] indices.  Stops early in front of
        a partial batch (the epoch's remainder, left pending for ``next_ragged``) or the end of
        finite data; None when the next batch is not a full one."""
        got = []
        for _ in range(K):
            g = self._next_global()
            if g is None or len(g) < self.B:
                if g is not None:
                    self._pending.insert(0, g)
                break
            got.append(g)
        if not got:
            return None
        return np.concatenate([g[self.rank * self.b:(self.rank + 1) * self.b] for g in got])

    def next_ragged(self):
        g = self._next_global()
        if g is None:
            return None
        sizes = input_lib.split_sizes(len(g), self.R)
        lo = sum(sizes[: self.rank])
        n = sizes[self.rank]
        return g[lo:lo + n], n, len(g)

"""The MI355X fast path of ``fit`` for the reference model (tf_dist_example.py:39-59).

``compile()`` + ``fit()`` on the reference's Sequential (Conv2D(32,3,relu) MaxPool Conv2D(64,3,relu)
MaxPool Flatten Dense(128,relu) Dense(10); SparseCategoricalCrossentropy(from_logits) ; SGD ;
SparseCategoricalAccuracy) on a GPU replica is compiled into:

* the model's flat parameter/gradient slabs (the same storage its MirroredVariables view);
* a device-resident dataset (data/device.py) with per-step index vectors;
* :class:`~..models.mnist_cnn.FusedMnistTrainStep` (hand-written gfx950 kernels);
* the cross-replica gradient all-reduce (``world > 1``): on one node the xGMI all-reduce kernel
  with the SGD update fused into it, one 900 KB message per step; RCCL otherwise, followed by the
  SGD kernel;
* ONE hipGraph per execution of ``steps_per_execution`` steps, replayed with a new index vector,
  the all-reduce captured inside it on the step's stream (serial; the side-stream overlap of a
  dense bucket with the conv backward is opt-in, TDL_OVERLAP_ALLREDUCE=1, and measured slower:
  profiles/mnist_side_stream_ab_r2.txt).

Host work per execution: one H2D copy of K*B int32 indices and one graph launch.  Metrics (loss
sum, correct count, sample count) are accumulated by the loss kernel on the device and reduced
across replicas only when logs are read.
"""
from __future__ import annotations

import gc
import os
import time
from typing import Dict, Optional

import numpy as np
import torch

from ..data import device as DD
from ..models import mnist_cnn as M
from ..parallel import input_lib
from . import execution as EX


def _is_reference_cnn(model) -> bool:
    from ..keras import activations as A
    from ..keras import layers as L
    from ..keras.models import Sequential

    if not isinstance(model, Sequential):
        return False
    ls = [l for l in model.layers if not isinstance(l, L.InputLayer)]
    pat = [L.Conv2D, L.MaxPooling2D, L.Conv2D, L.MaxPooling2D, L.Flatten, L.Dense, L.Dense]
    if len(ls) != len(pat) or any(type(l) is not p for l, p in zip(ls, pat)):
        return False
    c1, p1, c2, p2, _, d1, d2 = ls
    for c, f in ((c1, 32), (c2, 64)):
        if not (c.filters == f and c.kernel_size == (3, 3) and c.strides == (1, 1) and c.padding == "valid" and
                c.dilation_rate == (1, 1) and c.groups == 1 and c.use_bias and c.activation is A.relu):
            return False
    for p in (p1, p2):
        if not (p.pool_size == (2, 2) and p.strides == (2, 2) and p.padding == "valid"):
            return False
    if not (d1.units == 128 and d1.use_bias and d1.activation is A.relu):
        return False
    if not (d2.units == 10 and d2.use_bias and d2.activation is A.linear):
        return False
    if tuple(model._built_input_shape[1:]) != (28, 28, 1):
        return False
    if any(getattr(l, "kernel_regularizer", None) or getattr(l, "bias_regularizer", None) for l in ls):
        return False
    return all(l.trainable for l in ls)


def eligible(model, dataset=None) -> Optional[str]:
    """None if the fused path applies, else the reason it does not."""
    from .. import ops
    from ..keras import losses, metrics, optimizers

    if os.environ.get("TDL_DISABLE_FUSED") == "1":
        return "disabled by TDL_DISABLE_FUSED"
    s = model._get_strategy()
    if s.extended.device.type != "cuda":
        return "replica is not on a GPU"
    if not ops.hip_available():
        ops.hip()  # GPU replica without the HIP kernels: fail loudly
    if not _is_reference_cnn(model):
        return "model is not the reference CNN"
    if model._dtype_policy() != "float32":
        return "non-f32 dtype policy"
    lo = model.loss
    if not (isinstance(lo, losses.SparseCategoricalCrossentropy) and lo.from_logits and lo.ignore_class is None and
            lo.reduction in (losses.Reduction.AUTO, losses.Reduction.SUM_OVER_BATCH_SIZE)):
        return "loss is not SparseCategoricalCrossentropy(from_logits=True)"
    if lo.label_smoothing:
        return "label smoothing is not in the fused step's loss head"
    opt = model.optimizer
    if type(opt) not in (optimizers.SGD, optimizers.Adam, optimizers.AdamW, optimizers.RMSprop, optimizers.Adagrad,
                         optimizers.LARS, optimizers.LAMB):
        return f"optimizer {type(opt).__name__} has no fused update"
    if opt._clipped and not hasattr(ops.hip(), "clip_norm"):
        return "the extension has no clip_norm kernel (rebuild: python build_native.py)"
    if opt._accumulating and not hasattr(ops.hip(), "grad_accum"):
        return "the extension has no grad_accum kernel (rebuild: python build_native.py)"
    if getattr(opt, "use_ema", False) and not hasattr(ops.hip(), "weight_ema"):
        return "the extension has no weight_ema kernel (rebuild: python build_native.py)"
    if opt.weight_decay and not isinstance(opt, optimizers.Adam):
        return "decoupled weight decay is fused for Adam/AdamW only"
    kern = {"Adam": "adam", "AdamW": "adam", "RMSprop": "rmsprop", "Adagrad": "adagrad", "LARS": "layer_tables",
            "LAMB": "layer_tables"}.get(type(opt).__name__)
    if kern is not None and not hasattr(ops.hip(), kern):
        return f"the extension has no {kern} kernel (rebuild: python build_native.py)"
    for m in model.compiled_metrics:
        if not isinstance(m, metrics.SparseCategoricalAccuracy):
            return f"metric {m.name} not supported by the fused step"
    return None


def overlap_enabled() -> bool:
    """TDL_OVERLAP_ALLREDUCE=1: R > 1 steps all-reduce the dense bucket on a side stream while the
    conv backward runs (a forked execution graph); default serial."""
    return os.environ.get("TDL_OVERLAP_ALLREDUCE", "0") == "1"



def _source_key(x, y):
    """Identity of a host data source: the tensors themselves (strong references, so a freed
    tensor's id can never be reused for a different dataset) plus their in-place version counters."""
    return (x, y, x._version, None if y is None else y._version)


def _same_source(a, b) -> bool:
    return a is not None and b is not None and a[0] is b[0] and a[1] is b[1] and a[2:] == b[2:]


def _reference_columns(lp, labels: bool = True):
    """(x, y) of a lowered pipeline when they are the reference model's input (y is None without
    ``labels``); None otherwise, or when the pipeline did not lower (``lp`` is None)."""
    if lp is None:
        return None
    cols = lp.columns if isinstance(lp.columns, (tuple, list)) else (lp.columns,)
    x = cols[0]
    y = cols[1] if labels and len(cols) > 1 else None
    if not isinstance(x, torch.Tensor) or tuple(x.shape[1:]) not in ((28, 28, 1), (28, 28)) or \
            x.dtype != torch.float32:
        return None
    if labels and (not isinstance(y, torch.Tensor) or y.dim() != 1):
        return None
    return x, y


class FusedMnistTrainer(EX.Prefetching):
    kind = "fused"

    def __init__(self, model):
        self.model = model
        self.strategy = model._get_strategy()
        self.device = self.strategy.extended.device
        self.comm = self.strategy.extended.communicator
        self.R = self.strategy.num_replicas_in_sync
        self.rank = self.strategy.extended.rank
        model._ensure_slabs()
        self.layout = model._layout
        self.W, self.G = model._W, model._G
        for v in model._trainable_vars:
            v._leaf = None
        self.optimizer = model.optimizer
        self.optimizer.set_layout(model._layout)
        self.optimizer.build(self.W.numel(), self.device)
        self.optimizer.init_ema(self.W)  # (use_ema: E = W once, before any capture; a restored E is kept)
        self.K = max(1, int(model._steps_per_execution))
        self.metrics_dev = torch.zeros(4, dtype=torch.float32, device=self.device)
        self._steps = {}
        self._graphs = {}
        self._data_key = None
        # (no capture for the replica threads of a single-process MirroredStrategy: their
        # collectives are host rendezvous, and concurrent captures in threads of one process are not
        # safe with torch's process-global capture mode)
        self.capture = os.environ.get("TDL_GRAPH", "1") == "1" and not getattr(self.comm, "threaded", False)
        # With R > 1 the cross-replica all-reduce is recorded inside the execution graph (RCCL
        # supports hipGraph capture) unless TDL_CAPTURE_ALLREDUCE=0 or the collective capture probe
        # fails on some rank; then each step's graph is followed by an eager all-reduce + update.
        self._capture_comm = None
        self._comm_stream = None
        self.allreduce_mode = "local" if self.R == 1 else None
        self.fallbacks = []  # why a faster path was not taken (bench.py reports them)
        # R > 1: the dense bucket's all-reduce on a side stream overlapping the conv backward is
        # opt-in; serial is the default: on one MI355X (2 replica processes sharing it) the forked
        # execution graph ran 350 us/step against 68.6 serial (profiles/mnist_side_stream_ab_r2.txt)
        self.overlap = overlap_enabled()
        # index-upload slots (one captured graph each): the host may run this many executions ahead
        # of the GPU, which absorbs host hiccups such as an epoch's shuffle (~ms) without starving it
        self._nslots = max(2, int(os.environ.get("TDL_INDEX_SLOTS", "4")))
        self._ring = EX.IndexRing(self.device, self._nslots)
        self._ragged_bufs = {}
        # diagnostics: host seconds per execution (index take, upload, graph launch)
        self._host_times = [] if os.environ.get("TDL_HOST_TIMING") == "1" else None
        self._last_take = (0.0, 0.0, 0.0)
        self._comm_prepared, self._xchg = False, None  # (_prepare_comm)
        self._eval_cache = None
        self._handlers_b = None

    @property
    def capture_comm(self) -> bool:
        if self._capture_comm is None:
            if self.R == 1:
                self._capture_comm = True
            elif os.environ.get("TDL_CAPTURE_ALLREDUCE", "1") != "1" or not self.capture:
                self._capture_comm = False
            else:
                self._capture_comm = bool(self.comm.capture_probe())
                if not self._capture_comm:
                    self.fallbacks.append("all-reduce not capturable into the execution graph (probe failed)")
        return self._capture_comm

    # ------------------------------------------------------------------ data
    def set_class_weight(self, table):
        """The fused step's loss head is unweighted: Model.fit trains a weighted fit on the generic engine."""
        if table is not None:
            raise RuntimeError("the fused MNIST engine has no class weights (Model.fit uses the generic engine)")

    def prepare(self, dataset):
        lp = DD.lower(dataset)
        cols = _reference_columns(lp)
        if cols is None:
            return None
        if lp.batch_size % self.R:
            raise ValueError(f"global batch {lp.batch_size} is not divisible by {self.R} replicas")
        x, y = cols
        key = _source_key(x, y)
        if not _same_source(self._data_key, key):
            self.X = x.reshape(len(x), 28, 28, 1).to(self.device, torch.float32).contiguous()
            self.Y = y.to(self.device, torch.int32).contiguous()
            self._data_key = key
            self._steps, self._graphs = {}, {}
        policy = input_lib.effective_policy(dataset) if self.R > 1 else None
        seed = input_lib.shared_seed(self.strategy) if policy is not None and policy.name in ("DATA", "FILE") else None
        h = EX.DeviceHandler(lp, seed, self.rank, self.R)
        self._handlers_b = [h.b]
        return h

    # ------------------------------------------------------------------ steps
    def _step(self, b: int, idx_buf: torch.Tensor, global_b: Optional[int] = None):
        key = (b, idx_buf.data_ptr(), global_b)
        st = self._steps.get(key)
        if st is None:
            st = M.FusedMnistTrainStep(self.X, self.Y, idx_buf, self.W, self.G, self.layout, b, self.R,
                                       self.optimizer.lr_dev, self.metrics_dev, global_batch=global_b)
            self._steps[key] = st
        return st

    def _apply(self, st, global_b: int, k: int = 0):
        """finalize + (all-reduce) + optimizer for one step (step ``k`` of its execution).  R > 1
        with plain SGD: one all-reduce of the whole 900 KB slab with the SGD update fused into it
        (xGMI kernel), when the communicator has one.  Other optimizers: finalize leaves the
        gradient in G, their flat-slab kernel (csrc/kernels/optim.hip) applies it.  A clipped
        optimizer is never plain: finalize(False) -> all-reduce -> clip_norm -> update kernel.  Neither is
        an accumulating one (``gradient_accumulation_steps``): finalize(False) -> accumulate, and only the
        cycle's last micro-step goes on to the all-reduce and the update; step k's phase is that of
        ``iterations + k`` (``iterations`` advances once per execution), baked in at capture.  A weight
        EMA (``use_ema``) leaves plain SGD plain: the SGD inside finalize, the exchange in finalize and
        all_reduce_sgd are kept and one ``weight_ema`` launch follows them (``ema_after``), so the R > 1
        exchange stays in the finalize launch; every other optimizer's update kernel keeps the average
        itself.  ``self.update_path`` names the path the last step took."""
        opt = self.optimizer
        if opt._accumulating:
            st.finalize(False)
            if opt.accumulate(self.G, k):
                self._reduce_and_update(k)
            return
        plain = self._plain_sgd
        if self.R == 1 and plain:
            st.finalize(True, keep_grad=False)  # (nothing reads G on this path)
            self.update_path = "sgd-in-finalize"
            opt.ema_after(self.W, k)
            return
        if self.R > 1 and plain and st.has_exchange:
            # fused backward: the finalize launch itself all-reduces over xGMI and applies SGD
            st.finalize(True, exchange=True, keep_grad=False)  # (G is not read on this path)
            self.update_path = "exchange-in-finalize"
            opt.ema_after(self.W, k)
            return
        st.finalize(False)
        if self.R > 1 and plain and self.comm.all_reduce_sgd(self.G, self.W, opt.lr_dev):
            self.update_path = "all-reduce-sgd"
            opt.ema_after(self.W, k)
            return
        self._reduce_and_update(k)

    update_path = None  # how the last step updated W: one of the plain-SGD paths above or "update-kernel"

    def _train_step(self, st, off: int, global_b: int):
        """One whole step on the current stream.  R > 1 default (serial): forward + backward,
        finalize, then ONE all-reduce of the 900 KB gradient slab with the SGD update fused into it
        (_apply).  With TDL_OVERLAP_ALLREDUCE=1 the gradient all-reduce instead runs as two
        buckets: the dense-layer bucket (G[dense_offset:], 91% of the bytes) is final after
        forward_dense() and reduces on a side stream while the conv backward runs; the conv bucket
        follows finalize().  With the xGMI one-shot communicator each bucket's all-reduce also
        applies plain SGD to its own parameter range (W[dense_offset:] is not read again in the
        step), so no separate optimizer kernel runs; otherwise the optimizer waits for both."""
        k = off // max(1, st.b)
        if self.R == 1 or not self.overlap or not self._plain_sgd:
            st.forward_backward(off)
            self._apply(st, global_b, k)
            return
        main = torch.cuda.current_stream(self.device)
        if self._comm_stream is None:
            self._comm_stream = torch.cuda.Stream(self.device)
        cs = self._comm_stream
        d0 = st.dense_offset
        G, W = self.G, self.W
        lr = self.optimizer.lr_dev
        st.forward_dense(off)
        cs.wait_stream(main)
        with torch.cuda.stream(cs):
            dense_fused = self.comm.all_reduce_sgd(G[d0:], W[d0:], lr)
            if not dense_fused:
                self.comm.all_reduce(G[d0:], "sum")
        st.backward_conv()
        st.finalize(False)
        if dense_fused and self.comm.all_reduce_sgd(G[:d0], W[:d0], lr):
            main.wait_stream(cs)
            self.update_path = "overlap-all-reduce-sgd"
            self.optimizer.ema_after(self.W, k)  # (main stream, both buckets have joined)
            return
        cs.wait_stream(main)
        with torch.cuda.stream(cs):
            self.comm.all_reduce(G[:d0], "sum")
        main.wait_stream(cs)
        self._update(0, d0 if dense_fused else None, k)
        if dense_fused:
            # (the conv bucket's k_sgd saw a slice and took no EMA operands: the whole slab now, both joined)
            self.optimizer.ema_after(self.W, k)

    def _prepare_comm(self, st):
        """Collective set-up of the communicator's all-reduce channels for this step's buckets
        (must precede any graph capture; every rank reaches it at the same point).  With the fused
        backward and plain SGD the finalize kernel all-reduces through a dedicated xGMI channel
        (one exchange slot per finalize workgroup)."""
        if self.R == 1:
            return
        if not self._comm_prepared:
            n, d0 = self.W.numel(), st.dense_offset
            self.comm.prepare_all_reduce(n - d0, d0, n)
            self._xchg = None
            # one-shot moves (R-1) slabs per rank over the fabric, two-shot 2 (R-1)/R in two rounds
            self._xchg_twoshot = self.R >= int(os.environ.get("TDL_FX_TWOSHOT_MIN_R", "3"))
            if st.fused_bwd and self._plain_sgd and os.environ.get("TDL_MNIST_FINALIZE_XCHG", "1") == "1":
                self._xchg = self.comm.exchange_channel(n, M.FINALIZE_BLOCKS)
                if self._xchg is not None and not self._selftest_exchange(st.b):
                    self._xchg = None
            self.allreduce_mode = (("xgmi-in-finalize-twoshot" if self._xchg_twoshot else "xgmi-in-finalize")
                                   if self._xchg is not None else getattr(self.comm, "algorithm", self.comm.name))
            self._comm_prepared = True
        if self._xchg is not None and st.fused_bwd and not st.has_exchange:
            st.set_exchange(self._xchg, twoshot=self._xchg_twoshot)

    def _selftest_exchange(self, b: int) -> bool:
        """Collective start-up check of the exchange-in-finalize path on this job's devices: one
        real step (replica-specific samples) through a scratch step object with the exchange, whose
        updated weights must equal W0 - lr * (sum of the replicas' local gradients) taken through
        the communicator's own (self-tested) all-reduce, and be bit-identical on every replica.
        Parameters, gradients and metrics are restored afterwards.  Any failure on any rank: every
        rank keeps the serial all-reduce (TDL_XCHG_SELFTEST=0 skips the check)."""
        if os.environ.get("TDL_XCHG_SELFTEST", "1") != "1":
            return True
        import warnings

        from ..parallel import consistency

        dev = self.device
        n = len(self.X)
        idx = ((torch.arange(b, dtype=torch.int64) * 7919 + self.rank * 104729) % n).to(torch.int32).to(dev)
        saved = (self.W.clone(), self.G.clone())
        # phase 1, local work only: one step through the exchange.  Whatever happens here, every
        # rank then reaches the same agreement collective (a rank that raised must not wander into
        # a different collective than its peers)
        ok, why, timed_out, w_x, g_local = True, "", False, None, None
        try:
            tst = M.FusedMnistTrainStep(self.X, self.Y, idx, self.W, self.G, self.layout, b, self.R,
                                        self.optimizer.lr_dev, torch.zeros(4, dtype=torch.float32, device=dev),
                                        global_batch=b * self.R)
            if not tst.fused_bwd:
                raise RuntimeError("fused backward unavailable")
            tst.set_exchange(self._xchg, twoshot=self._xchg_twoshot)
            torch.cuda.synchronize(dev)
            if os.environ.get("TDL_FAULT_XCHG_SELFTEST_RAISE") == str(self.rank):  # fault injection (tests)
                raise RuntimeError("injected self-test failure before the exchange")
            tst.forward_backward(0)
            tst.finalize(True, exchange=True)
            torch.cuda.synchronize(dev)
            timed_out = bool(self._xchg.error())
            if timed_out:
                raise RuntimeError("exchange timed out")
            tst.check()
            w_x, g_local = self.W.clone(), self.G.clone()
            del tst
        except Exception as e:  # noqa: BLE001 - any failure means the serial path
            ok, why = False, f"{type(e).__name__}: {e}"
            timed_out = timed_out or bool(self._xchg.error())
        # agreement on the control plane (never through the xGMI kernel: its device may now carry a
        # sticky error word): [step ok everywhere, no rank timed out]
        ok_all, no_timeout = self._agree_flags([ok, not timed_out])
        if not no_timeout:
            # a bounded wait expired: the error word disables every xGMI kernel on that device, so
            # the serial all-reduce could not run there either -- fail the job on every rank
            self.W.copy_(saved[0])
            raise RuntimeError("exchange-in-finalize self-test: a peer did not arrive at the xGMI exchange "
                               f"({why or 'on another rank'}); the device fabric or a peer is broken")
        if ok_all:
            # phase 2, every rank: the reference reduction and the cross-replica identity check
            self.comm.all_reduce(g_local, "sum")
            lr = float(self.optimizer.lr_dev.item())
            w_ref = saved[0] - lr * g_local
            if os.environ.get("TDL_FAULT_XCHG_SELFTEST") == str(self.rank):  # fault injection (tests)
                w_ref = w_ref + 1.0
            if not torch.allclose(w_x, w_ref, rtol=1e-5, atol=1e-7):
                ok, why = False, f"max |W - W_ref| = {float((w_x - w_ref).abs().max()):.3g}"
            if not consistency.replicas_identical(self.comm, w_x):
                ok, why = False, "replicas differ"
            ok_all = self._agree_flags([ok])[0]
        self.W.copy_(saved[0])
        self.G.copy_(saved[1])
        if not ok_all:
            self.fallbacks.append(f"exchange-in-finalize self-test failed ({why or 'on another rank'})")
            if self.rank == 0:
                warnings.warn(f"exchange-in-finalize self-test failed ({why or 'on another rank'}); "
                              "using the serial gradient all-reduce")
        return ok_all

    def _agree_flags(self, flags) -> list:
        """MIN over ranks of boolean flags through the process group itself (not the communicator's
        xGMI fast path)."""
        import torch.distributed as dist

        on = self.device if self.comm.name == "rccl" else torch.device("cpu")
        f = torch.tensor([1.0 if x else 0.0 for x in flags], device=on)
        dist.all_reduce(f, op=dist.ReduceOp.MIN)
        return [bool(v > 0.5) for v in f.tolist()]

    @property
    def _plain_sgd(self) -> bool:
        # (gradient clipping needs the whole reduced gradient before any update: never the SGD inside
        # finalize, all_reduce_sgd, the exchange-in-finalize channel or the two-bucket overlap; gradient
        # accumulation folds the local gradient first and updates on the cycle's last micro-step only)
        # A weight EMA (use_ema) leaves plain SGD plain: the stand-alone weight_ema launch follows the plain update
        # (_apply).  ``leave_plain_for_ema`` (scripts/bench_ema.py's measurement switch, never set by the engines)
        # sends such an optimizer through k_sgd with the average inside instead.
        opt = self.optimizer
        if getattr(opt, "use_ema", False) and getattr(self, "leave_plain_for_ema", False):
            return False
        return type(opt).__name__ == "SGD" and opt.momentum == 0 and not opt._clipped and not opt._accumulating

    def _update(self, lo: int = 0, hi: Optional[int] = None, k: int = 0):
        """The optimizer's own flat-slab kernel over [lo, hi) for step ``k`` of its execution (Adam's step
        offset, baked into the captured graph).  The whole slab, except for the two buckets of the overlap
        path, which is plain SGD only (see _plain_sgd: no clip, no momentum slot to slice)."""
        opt = self.optimizer
        W, G = self.W[lo:hi], self.G[lo:hi]
        if not opt.device_update(W, G, k):
            raise RuntimeError(f"fused trainer: {type(opt).__name__} has no device update on {W.device}")
        self.update_path = "update-kernel"

    def _reduce_and_update(self, k: int):
        if self.R > 1:
            self.comm.all_reduce(self.G, "sum")
        self._update(k=k)

    def _run_eager(self, idx_np: np.ndarray, b: int, global_b: int):
        if b == 0:
            # this replica got no samples of a tiny final batch: contribute zero gradients
            self.G.zero_()
            opt = self.optimizer
            if not opt.accumulate(self.G):  # (every rank is in the same phase: none communicates)
                opt.iterations += 1
                return
            if self.R > 1:
                self.comm.all_reduce(self.G, "sum")
            opt.apply_flat(self.W, self.G, accumulated=True)
            return
        # one persistent index buffer per ragged size (the step object is cached by its address),
        # filled through the next slot of the staging ring without a host sync
        key = ("ragged", b)
        idx_buf = self._ragged_bufs.get(key)
        if idx_buf is None:
            idx_buf = torch.zeros(b, dtype=torch.int32, device=self.device)
            self._ragged_bufs[key] = idx_buf
        self._ring.upload(idx_np, idx_buf, self._ring.next_slot())
        st = self._step(b, idx_buf, global_b)
        self._prepare_comm(st)
        self._train_step(st, 0, global_b)
        self.optimizer.iterations += 1

    def _graph_for(self, K: int, b: int, slot: int = 0, t_add: int = 0):
        """Graph of one K-step execution reading its sample ids from its own index buffer; the
        slots rotate so the host uploads execution i+1's indices while execution i runs.  ``t_add``: the
        execution starts that many micro-steps from now (warm_graphs captures ahead)."""
        opt = self.optimizer
        key = EX.accum_key(opt, (K, b, slot), t_add)
        g = self._graphs.get(key)
        if g is not None:
            return g
        idx_buf = torch.zeros(K * b, dtype=torch.int32, device=self.device)
        st = self._step(b, idx_buf)
        self._prepare_comm(st)
        graph = None
        if self.capture:
            saved = (self.W.clone(), self.metrics_dev.clone(), {k: v.clone() for k, v in opt.slots().items()})
            if self.capture_comm:
                # whole execution (K steps incl. all-reduce + optimizer) in one graph
                with EX.capturing(self.device, opt, t_add) as graph:
                    for k in range(K):
                        self._train_step(st, k * b, b * self.R)
            else:
                # one graph per step holding the fused fwd/bwd/finalize; the RCCL all-reduce and
                # the SGD kernel are issued eagerly between replays
                graph = []
                for k in range(K):
                    with EX.capturing(self.device, opt) as gk:
                        st.forward_backward(k * b)
                        st.finalize(False)
                    graph.append(gk)
            torch.cuda.synchronize(self.device)
            # capture does not execute, but be safe: restore state
            self.W.copy_(saved[0])
            self.metrics_dev.copy_(saved[1])
            for k, v in saved[2].items():
                self.optimizer.slots()[k].copy_(v)
        g = (graph, idx_buf, st)
        self._graphs[key] = g
        return g

    def warm_graphs(self, steps: int, b: Optional[int] = None):
        """Capture every graph ``run_train(steps)`` will replay, ahead of a timed region."""
        if b is None and self._handlers_b:
            b = self._handlers_b[0]
        if b is None:
            return
        # (an accumulating optimizer: one graph per starting phase the executions of this run will have)
        starts = EX.execution_starts(steps, self.K, EX.phase_period(self.optimizer, self.K))
        for K, t_add in starts:
            for slot in range(self._nslots):
                self._graph_for(K, b, slot, t_add)
        if starts:
            self._ring.reserve(max(K for K, _ in starts) * b)

    def _take_upload(self, handler: EX.DeviceHandler, K: int):
        """Take the next K full batches' indices and start their upload into the next index slot
        (None at a ragged tail / the end of finite data)."""
        ta = time.perf_counter()
        idx = handler.take(K)
        tb = time.perf_counter()
        if idx is None:
            return None
        slot = self._ring.next_slot()
        graph, idx_buf, st = self._graph_for(K, handler.b, slot)
        tc = time.perf_counter()
        self._ring.upload(idx, idx_buf, slot)
        self._last_take = (tb - ta, tc - tb, time.perf_counter() - tc)
        return (handler, K, idx.size // handler.b, graph, st)

    def run_train(self, handler: EX.DeviceHandler, steps: int) -> int:
        # everything allocated so far (modules, model, graphs) is long-lived: move it out of the
        # cyclic GC's generations so a collection in the launch loop scans only per-step garbage
        # (a full collection of the torch-sized heap stalled the host ~30 ms mid-run)
        gc.freeze()
        done = 0
        b = handler.b
        opt = self.optimizer
        timing = self._host_times is not None
        while done < steps:
            K = min(self.K, steps - done)
            t0 = time.perf_counter() if timing else 0.0
            r = self._next_execution(handler, K)
            t1 = t2 = time.perf_counter() if timing else 0.0
            if r is None:
                # ragged tail (end of finite data) -> eager steps of their own sizes
                one = handler.next_ragged()
                if one is None:
                    break
                opt._sync_lr()
                self._run_eager(*one)
                done += 1
                continue
            opt._sync_lr()
            _, _, Kr, graph, st = r
            if Kr < K:
                # the full batches in front of an epoch's partial batch: same slot buffers and
                # step object, launched eagerly (no per-step host sync, no new graph size)
                for k in range(Kr):
                    self._train_step(st, k * b, b * self.R)
                K = Kr
            elif isinstance(graph, list):
                for k, gk in enumerate(graph):
                    gk.replay()
                    if opt.accumulate(self.G, k):  # (True when accumulation is off)
                        self._reduce_and_update(k)
            elif graph is not None:
                graph.replay()
            else:
                for k in range(K):
                    self._train_step(st, k * b, b * self.R)
            if timing:
                tk = self._last_take if t1 - t0 > 1e-4 else (t1 - t0, 0.0, 0.0)
                self._host_times.append((tk[0], tk[1] + tk[2], time.perf_counter() - t2))
            opt.iterations += K
            done += K
        return done

    # ------------------------------------------------------------------ evaluate / predict
    def _eval_columns(self, lp, labels: bool):
        """Device copies of an evaluation pipeline's columns (the last one is cached), or None
        when they are not the reference model's input."""
        cols = _reference_columns(lp, labels)
        if cols is None:
            return None
        x, y = cols
        key = _source_key(x, y)
        cached = self._eval_cache
        if cached is None or not _same_source(cached[0], key):
            X = x.reshape(len(x), 28, 28, 1).to(self.device, torch.float32).contiguous()
            Y = (y.to(self.device, torch.int32) if labels else torch.zeros(len(x), dtype=torch.int32, device=self.device)).contiguous()
            self._eval_cache = cached = (key, X, Y, {})
        return cached[1], cached[2], cached[3]

    def _eval_step(self, steps: dict, X, Y, b: int, cap: int, metrics):
        st = steps.get(b)
        if st is None or st.idx_buf.numel() < cap * b:
            idx_buf = torch.zeros(max(cap, 1) * b, dtype=torch.int32, device=self.device)
            st = M.FusedMnistTrainStep(X, Y, idx_buf, self.W, self.G, self.layout, b, self.R, self.optimizer.lr_dev,
                                       metrics)
            steps[b] = st
        st.metrics = metrics
        st._impl.set_metrics(metrics)
        return st

    def _forward_batches(self, handler: EX.DeviceHandler, X, Y, cache, steps, metrics, logits_out=None):
        """Forward-only passes over the handler's batches on the hand-written kernels."""
        K = 64
        done = 0
        while steps is None or done < steps:
            n = K if steps is None else min(K, steps - done)
            idx = handler.take(n)
            if idx is None:
                one = handler.next_ragged()
                if one is None:
                    break
                ids, nb, _ = one
                if nb > 0:
                    st = self._eval_step(cache, X, Y, nb, 1, metrics)
                    st.idx_buf[:nb].copy_(torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int32)))
                    lg = None if logits_out is None else torch.empty(nb * 10, device=self.device)
                    st.forward_eval(0, lg)
                    if lg is not None:
                        logits_out.append(lg.view(nb, 10))
                done += 1
                continue
            b = handler.b
            kb = idx.size // b
            st = self._eval_step(cache, X, Y, b, K, metrics)
            st.idx_buf[:idx.size].copy_(torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int32)))
            lg = None if logits_out is None else torch.empty(kb * b * 10, device=self.device)
            for k in range(kb):
                st.forward_eval(k * b, None if lg is None else lg[k * b * 10:])
            if lg is not None:
                logits_out.append(lg.view(kb * b, 10))
            done += kb
        return done

    def evaluate(self, dataset, steps: Optional[int] = None) -> Optional[Dict[str, float]]:
        """``Model.evaluate`` on the gfx950 forward kernel (head mode 2): each replica evaluates its
        slice of every global batch of the device-resident pipeline; loss / accuracy sums are
        all-reduced once at the end.  None when the pipeline does not lower to the device."""
        lp = DD.lower(dataset)
        if lp is None:
            return None
        cols = self._eval_columns(lp, labels=True)
        if cols is None:
            return None
        X, Y, cache = cols
        if lp.batch_size % self.R:
            return None
        h = EX.DeviceHandler(lp, None, self.rank, self.R)
        h._async = False
        metrics = torch.zeros(4, dtype=torch.float32, device=self.device)
        try:
            self._forward_batches(h, X, Y, cache, steps, metrics)
        finally:
            h.close()
        if self.R > 1:
            self.comm.check_health()
            self.comm.all_reduce(metrics, "sum")
        loss_sum, correct, count = (float(v) for v in metrics[:3].cpu())
        out = {"loss": loss_sum / max(count, 1.0)}
        for m in self.model.compiled_metrics:
            out[m.name] = correct / max(count, 1.0)
        return out

    def predict(self, dataset, steps: Optional[int] = None) -> Optional[np.ndarray]:
        """``Model.predict`` on the gfx950 forward kernel: logits of every sample in order.  Every
        replica computes all of them (inference is replica-independent; no collective)."""
        lp = DD.lower(dataset)
        if lp is None:
            return None
        cols = self._eval_columns(lp, labels=False)
        if cols is None:
            return None
        X, Y, cache = cols
        h = EX.DeviceHandler(lp, None, 0, 1)
        h._async = False
        metrics = torch.zeros(4, dtype=torch.float32, device=self.device)
        out = []
        try:
            self._forward_batches(h, X, Y, cache, steps, metrics, logits_out=out)
        finally:
            h.close()
        if not out:
            return np.zeros((0, 10), dtype=np.float32)
        return torch.cat(out).cpu().numpy()

    def reset_metrics(self):
        self.metrics_dev.zero_()
        self.model._loss_tracker.reset_state()
        for m in self.model.compiled_metrics:
            m.reset_state()

    def logs(self) -> Dict[str, float]:
        for st in list(self._steps.values()):
            st.check()
        t = self.metrics_dev.clone()
        if self.R > 1:
            self.comm.check_health()
            self.comm.all_reduce(t, "sum")
        loss_sum, correct, count = (float(v) for v in t[:3].cpu())
        out = {"loss": loss_sum / max(count, 1.0)}
        for m in self.model.compiled_metrics:
            out[m.name] = correct / max(count, 1.0)
        # mirror into the Keras metric objects so model.metrics results agree
        lt = self.model._loss_tracker
        lt._to(self.device)
        lt.total._value.fill_(float(self.metrics_dev[0]))
        lt.count._value.fill_(float(self.metrics_dev[2]))
        for m in self.model.compiled_metrics:
            m._to(self.device)
            m.total._value.fill_(float(self.metrics_dev[1]))
            m.count._value.fill_(float(self.metrics_dev[2]))
        return out

    def finish(self):
        torch.cuda.synchronize(self.device)

    def on_replica_divergence(self):
        """The replicas' parameters differed after the custom xGMI all-reduce path (detected by
        keras/models.py _check_replicas and already repaired from rank 0): drop that path and the
        graphs that captured it; later executions all-reduce over RCCL / the ring."""
        if getattr(self.comm, "xgmi", None) is not None:
            self.comm.xgmi = None
            self.comm.algorithm = "rccl" if self.comm.name == "rccl" else self.comm.name
            self.comm._capture_ok = None  # re-probe: without xGMI a gloo group cannot be captured
        self._graphs = {}
        self._steps = {}
        self._capture_comm = None
        self._comm_prepared = False
        self._xchg = None
        self.allreduce_mode = getattr(self.comm, "algorithm", self.comm.name)


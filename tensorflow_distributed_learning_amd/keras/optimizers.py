"""Keras optimizers over the flat parameter slab.

Every replica applies the optimizer to its whole slab in ONE update after the gradient
all-reduce (TF applies ``ResourceApplyGradientDescent`` once per variable).  On the GPU every
optimizer is one hand-written gfx950 kernel over the slab (``_C.sgd`` / ``_C.sgd_momentum``,
``_C.adam`` (AdamW's decay in the same pass), ``_C.rmsprop``, ``_C.adagrad``; csrc/kernels/optim.hip),
with the learning rate and Adam's step count read from device memory so the update can sit inside
a captured hipGraph.

Gradient clipping (``clipvalue``, ``clipnorm`` / ``global_clipnorm``) runs on the device too: two
launches (``_C.clip_norm``, csrc/kernels/clip.hip) leave the global norm and the clip scale in device
memory -- an f64 sum in an order fixed by the slab size, bit-identical on every run and replica --
and the update kernel applies ``clamp(g, +-clipvalue) * scale`` where it loads ``g``: no extra pass
over the gradient, no torch reduction, capturable.  The torch formulas (``_clip`` + ``_update``)
remain the CPU implementation.  Their f32 sum of squares overflows to inf for a gradient norm above
~1.8e19, where the device path's f64 sum still returns the finite norm.

LARS and LAMB, the optimizers of large-batch data-parallel training, scale every element's step by a
trust ratio of two norms of its own variable, so they read the slab's layout (``set_layout``, which
the engines call before ``build``).  On the GPU a step is three launches whatever the number of
variables (``_C.lars_sums`` / ``lars_ratio`` / ``lars_update`` and the ``lamb_`` three;
csrc/kernels/layerwise.hip): f64 sums of squares per chunk of a variable, the per-variable norms
and ratios from them in a fixed order (bit-identical on every run and replica), the update.  The
chunk tables are built and validated once on the host (``_C.layer_tables``).  ``last_layer_ratios``
/ ``last_layer_norms`` expose the last step's words.  The per-variable torch formulas are the CPU
implementation.  ``clipnorm`` stays one norm over the whole slab for every optimizer.

Gradient accumulation (``gradient_accumulation_steps=k`` on every optimizer): the local gradients of k
micro-steps are folded in f32 into one more slab, the slot ``"gradient_accumulator"`` (``accumulate``: one
launch of ``_C.grad_accum``, csrc/kernels/accum.hip, on the GPU), and only the k-th micro-step all-reduces,
clips and updates, on the cycle's mean gradient.  ``iterations`` counts micro-steps (Keras 3's counting) and
the phase of a micro-step is ``iterations mod k``, known to the host at launch and at capture time: no device
counter.  Keras is not installed where this was written: parity with its implementation is unpinned.

Weight EMA (``use_ema=True``, ``ema_momentum``, ``ema_overwrite_frequency`` on every optimizer): one more f32
slab, the slot ``"ema"`` (``E``), starts as a copy of the weights before the first update (``init_ema``) and
follows every weight update, element for element in f32: ``E = float32(m) * E + float32(1 - m) * W_new``, two
products and a sum, three roundings, no contraction (numpy's ``np.float32(m) * E + np.float32(1 - m) * W`` gives
the bits; the torch form of it is the CPU implementation).  On the GPU every update kernel has an instantiation
that loads ``e`` with its operands and stores the new average where it stores ``w`` (``device_ema`` hands it the
operands, no extra launch); an update done elsewhere -- the SGD inside the fused step's finalize or an xGMI
all-reduce, a torch formula -- is followed by ``ema_after``: one launch of ``_C.weight_ema``
(csrc/kernels/ema.hip).  With ``ema_overwrite_frequency=f`` the update whose 1-based step count
``iterations + 1`` is a multiple of f also stores ``W = E`` (``_ema_mode``: 2 on such a step, else 1): the host
knows it at launch and at capture time, so it is a kernel mode and part of the execution-graph key, never a device
counter.  With gradient accumulation ``E`` moves on apply micro-steps only and f must be a multiple of k.
``finalize_variable_values`` (end of ``fit``, custom loops) stores ``W = E`` once.  Keras / TF are not installed
where this was written: parity with their implementation is unpinned.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional

import torch

from . import schedules as _sched


class Optimizer:
    def __init__(self, learning_rate=0.001, name="Optimizer", clipnorm=None, clipvalue=None, global_clipnorm=None,
                 weight_decay=None, gradient_accumulation_steps=None, use_ema=False, ema_momentum=0.99,
                 ema_overwrite_frequency=None, **kwargs):
        self.name = name
        k = gradient_accumulation_steps
        if k is not None and (isinstance(k, bool) or not isinstance(k, int) or k < 1):
            raise ValueError(f"gradient_accumulation_steps must be None or an integer >= 1, got {k!r}")
        self.gradient_accumulation_steps = k
        # (the momentum and the frequency are validated even when use_ema is off, where nothing reads them)
        m, f = ema_momentum, ema_overwrite_frequency
        if isinstance(m, bool) or not isinstance(m, (int, float)) or not 0.0 <= m <= 1.0:
            raise ValueError(f"ema_momentum must lie in [0, 1], got {m!r}")
        if f is not None and (isinstance(f, bool) or not isinstance(f, int) or f < 1):
            raise ValueError(f"ema_overwrite_frequency must be None or an integer >= 1, got {f!r}")
        if f is not None and (k or 1) > 1 and f % k:
            raise ValueError(f"ema_overwrite_frequency ({f}) must be a multiple of gradient_accumulation_steps ({k}): "
                             "the average moves, and can overwrite, on apply micro-steps only")
        self.use_ema, self.ema_momentum, self.ema_overwrite_frequency = bool(use_ema), float(m), f
        self._ema_fresh = False  # build() allocated E and nothing has filled it yet (init_ema)
        self._lr = learning_rate
        self.clipnorm, self.clipvalue, self.global_clipnorm = clipnorm, clipvalue, global_clipnorm
        self.weight_decay = weight_decay
        self.iterations = 0
        self._slots: Dict[str, torch.Tensor] = {}
        self._n = None
        self._device = None
        self.lr_dev: Optional[torch.Tensor] = None
        self._lr_synced = None  # (value, lr_dev address) last written by _sync_lr
        # device copy of ``iterations`` at the start of the next step / execution (Adam's bias
        # correction on the device: a captured step graph reads it, each step adds its offset)
        self.t_dev: Optional[torch.Tensor] = None
        self._t_synced = None
        # device clipping (build() on a GPU): [scale, norm, -, -] f32 written by _C.clip_norm and its
        # f64 partial sums; allocated before any graph capture
        self._clip_out: Optional[torch.Tensor] = None
        self._clip_partials: Optional[torch.Tensor] = None
        unknown = set(kwargs) - {"decay", "amsgrad_legacy", "jit_compile", "is_legacy_optimizer"}
        if unknown:
            raise TypeError(f"{type(self).__name__}: unexpected arguments {sorted(unknown)}")

    # ------------------------------------------------------------------ learning rate
    @property
    def learning_rate(self):
        return self._lr

    @learning_rate.setter
    def learning_rate(self, v):
        self._lr = v

    lr = learning_rate

    def current_lr(self, step: Optional[int] = None) -> float:
        lr = self._lr
        if isinstance(lr, _sched.LearningRateSchedule):
            return float(lr(self.iterations if step is None else step))
        if callable(lr):
            return float(lr())
        return float(lr)

    def _sync_lr(self, step: Optional[int] = None):
        # one fill kernel only when the value changes: a constant learning rate costs no launch in
        # front of every graph replay (the device copy is written nowhere else)
        if self.lr_dev is not None:
            v = self.current_lr(step)
            if self._lr_synced != (v, self.lr_dev.data_ptr()):
                self.lr_dev.fill_(v)
                self._lr_synced = (v, self.lr_dev.data_ptr())
        if self.t_dev is not None and self._needs_step:
            t = float(self.iterations if step is None else step)
            if self._t_synced != (t, self.t_dev.data_ptr()):
                self.t_dev.fill_(t)
                self._t_synced = (t, self.t_dev.data_ptr())

    _needs_step = False  # the device update reads t_dev (Adam's bias correction)

    _update_zeroes_grad = False  # the device update kernel can zero G once it has read it (``zero_grad``)

    def device_update(self, W: torch.Tensor, G: torch.Tensor, t_add: int = 0, zero_grad: bool = False,
                      phase_add: Optional[int] = None) -> bool:
        """One hand-written flat-slab update kernel (learning rate and step count read from the
        device: capturable) when this optimizer has one and the slab is on the GPU; False
        otherwise (the caller then uses apply_flat).  ``t_add``: the step's offset inside an
        execution whose first step is t_dev (Adam).  ``zero_grad``: the generic trainer's request to
        zero G after its use, so its next step needs no fill launch; only a kernel of an optimizer
        with ``_update_zeroes_grad`` honours it, the others ignore it.  ``phase_add``: the step's offset from
        ``iterations`` (the weight EMA's overwrite phase); ``t_add`` unless given -- ``apply_flat``, whose
        callers advance ``iterations`` every step, passes 0."""
        return False

    def set_layout(self, layout):
        """The slab's ``SlabLayout`` (the engines pass it just before ``build``).  Only the layer-wise
        optimizers (LARS, LAMB) read it: their step depends on per-variable norms."""
        self._layout = layout

    _layout = None

    # ------------------------------------------------------------------ slots
    def build(self, n: int, device: torch.device):
        if self._n == n and self._device == device:
            return
        self._n, self._device = n, device
        self.lr_dev = torch.full((1,), self.current_lr(), dtype=torch.float32, device=device)
        self._lr_synced = (self.current_lr(), self.lr_dev.data_ptr())
        self.t_dev = torch.full((1,), float(self.iterations), dtype=torch.float32, device=device)
        self._t_synced = (float(self.iterations), self.t_dev.data_ptr())
        self._clip_out = self._clip_partials = None
        if self._clipped and device.type == "cuda" and _kernel_present("clip_norm"):
            from .. import ops

            self._clip_out = torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=torch.float32, device=device)
            self._clip_partials = torch.zeros(max(1, ops.hip().clip_partials(n)), dtype=torch.float64, device=device)
        if self.use_ema:
            old = self._slots.get(EMA)
            self._ema_fresh = old is None or old.numel() != n
        for k in self._slot_names() + ([ACCUMULATOR] if self._accumulating else []) + ([EMA] if self.use_ema else []):
            old = self._slots.get(k)
            self._slots[k] = old.to(device) if (old is not None and old.numel() == n) else torch.zeros(
                n, dtype=torch.float32, device=device)

    def _slot_names(self) -> List[str]:
        return []

    def slots(self) -> Dict[str, torch.Tensor]:
        return self._slots

    # ------------------------------------------------------------------ update
    def _clip_norm_value(self):
        # (one norm over the whole slab for both options; Keras clips ``clipnorm`` per variable)
        return self.global_clipnorm or self.clipnorm

    @property
    def _clipped(self) -> bool:
        return self.clipvalue is not None or self._clip_norm_value() is not None

    @property
    def _clip_on_device(self) -> bool:
        """Unclipped, or built on a GPU slab with the clip kernels: the device update applies the clip."""
        return not self._clipped or self._clip_out is not None

    @property
    def last_clip_norm(self) -> Optional[torch.Tensor]:
        """The gradient norm of the last device norm clip (a 1-element device view; None on the CPU)."""
        return None if self._clip_out is None else self._clip_out[1:2]

    def device_clip(self, G: torch.Tensor) -> dict:
        """The clip operands of this optimizer's update kernel for the gradient slab ``G``; with a norm
        clip, first the two ``clip_norm`` launches that write the scale.  Clamp, then the norm of the
        clamped gradient, then the scale: the order of ``_clip``."""
        if not self._clipped:
            return {}
        norm = self._clip_norm_value()
        if norm is not None:
            from .. import ops

            ops.hip().clip_norm(G, self._clip_partials, self._clip_out, float(norm), self.clipvalue)
        return {"gscale": self._clip_out if norm is not None else None, "clipvalue": self.clipvalue}

    def _clip(self, G: torch.Tensor):
        if self.clipvalue is not None:
            G.clamp_(-self.clipvalue, self.clipvalue)
        norm = self._clip_norm_value()
        if norm is not None:
            n = torch.linalg.vector_norm(G)
            G.mul_(torch.clamp(norm / (n + 1e-12), max=1.0))

    # ------------------------------------------------------------------ gradient accumulation
    @property
    def _accumulating(self) -> bool:
        return (self.gradient_accumulation_steps or 1) > 1

    def _accum_phase(self, t_add: int = 0) -> int:
        """The phase of the micro-step ``t_add`` steps from now: ``iterations mod k`` before its increment.  The
        host knows it at launch and at capture time (no device counter)."""
        return (int(self.iterations) + int(t_add)) % self.gradient_accumulation_steps

    def accumulate(self, G: torch.Tensor, t_add: int = 0, zero_grad: bool = False) -> bool:
        """The fold of one micro-step over the gradient slab ``G`` into the slot ``"gradient_accumulator"``
        (``A``), by the phase p of the micro-step (``t_add``: its offset inside an execution whose first step is
        ``iterations``), every operation one f32 rounding:

            p == 0: A = G        0 < p < k-1: A = A + G        p == k-1: G = (A + G) * float32(1 / k)

        Returns whether this is the apply micro-step (p == k-1): ``G`` then holds the mean gradient of the cycle
        and the caller all-reduces, clips and updates as an unaccumulated step would.  On a GPU slab it is one
        ``_C.grad_accum`` launch (csrc/kernels/accum.hip; capturable, the mode is baked in at capture), which
        also zeroes ``G`` on the other micro-steps when the trainer asked for it (``zero_grad``); the
        torch formulas, the CPU implementation, never do.  A no-op returning True when accumulation is off."""
        if not self._accumulating:
            return True
        if self._n != G.numel() or self._device != G.device:
            self.build(G.numel(), G.device)
        k = self.gradient_accumulation_steps
        p = self._accum_phase(t_add)
        A = self._slots[ACCUMULATOR]
        mode = 0 if p == 0 else (2 if p == k - 1 else 1)
        c = _f32(1.0 / k)
        if G.device.type == "cuda":
            from .. import ops

            if G.dtype != torch.float32 or not hasattr(ops.hip(), "grad_accum"):
                raise RuntimeError("gradient accumulation: the extension has no grad_accum kernel for the GPU slab "
                                   "(rebuild: python build_native.py)")
            ops.hip().grad_accum(G, A, mode, c, zero_grad=bool(zero_grad) and mode != 2)
        elif mode == 0:
            A.copy_(G)
        elif mode == 1:
            A.add_(G)
        else:
            torch.add(A, G, out=G)
            G.mul_(c)
        return mode == 2

    # ------------------------------------------------------------------ weight EMA
    def _ema_mode(self, t_add: int = 0) -> int:
        """The EMA mode of the update ``t_add`` steps from now: 2 when its 1-based step count
        ``iterations + t_add + 1`` is a multiple of ``ema_overwrite_frequency`` (update E, store W = E), else 1
        (update E); 0 with ``use_ema`` off.  The host knows it at launch and at capture time."""
        if not self.use_ema:
            return 0
        f = self.ema_overwrite_frequency
        return 2 if f is not None and (int(self.iterations) + int(t_add) + 1) % f == 0 else 1

    def init_ema(self, W: torch.Tensor):
        """E = W once, for an ``E`` that ``build`` has just allocated (TF 2.11+'s ``initial_value=var``): the
        engines call it after ``build`` and before any capture.  An ``E`` that ``load_state_dict`` brought, or
        that has been filled before, is kept."""
        if not self.use_ema:
            return
        if self._n != W.numel() or self._device != W.device:
            self.build(W.numel(), W.device)
        if self._ema_fresh:
            with torch.no_grad():
                self._slots[EMA].copy_(W)
            self._ema_fresh = False

    def device_ema(self, W: torch.Tensor, t_add: int = 0) -> dict:
        """The EMA operands of this optimizer's update kernel over the GPU slab ``W`` for the step ``t_add``
        from ``iterations`` (analogous to ``device_clip``): the kernel keeps ``E`` where it stores ``w``, at no
        extra launch.  Empty with ``use_ema`` off, and for a slice of the slab (the fused engine's two buckets):
        its caller runs ``ema_after`` over the whole slab once every bucket is updated."""
        if not self.use_ema or W.numel() != self._n:
            return {}
        from .. import ops

        if not hasattr(ops.hip(), "weight_ema"):
            raise RuntimeError("use_ema: the extension has no weight_ema kernel for the GPU slab "
                               "(rebuild: python build_native.py)")
        self.init_ema(W)
        return {"ema": self._slots[EMA], "ema_momentum": self.ema_momentum, "ema_mode": self._ema_mode(t_add)}

    def ema_after(self, W: torch.Tensor, t_add: int = 0):
        """``E = float32(m) * E + float32(1 - m) * W`` after an update of the whole slab ``W`` that no update
        kernel of ours made (the step ``t_add`` from ``iterations``; on an overwrite step also ``W = E``): one
        launch of ``_C.weight_ema`` on a GPU slab (capturable, the mode is baked in at capture), the torch form
        of the numpy expression on the CPU.  A no-op with ``use_ema`` off."""
        if not self.use_ema:
            return
        self.init_ema(W)
        E, mode = self._slots[EMA], self._ema_mode(t_add)
        if W.device.type == "cuda":
            from .. import ops

            if W.dtype != torch.float32 or not hasattr(ops.hip(), "weight_ema"):
                raise RuntimeError("use_ema: the extension has no weight_ema kernel for the GPU slab "
                                   "(rebuild: python build_native.py)")
            ops.hip().weight_ema(W, E, self.ema_momentum, mode)
            return
        with torch.no_grad():
            # two products and a sum, each rounded to f32 (no ``alpha=``: that form may fuse)
            E.mul_(_f32(self.ema_momentum)).add_(W * _f32(1.0 - self.ema_momentum))
            if mode == 2:
                W.copy_(E)

    def finalize_slab(self, W: torch.Tensor):
        """``W = E`` over the whole slab (the end of ``fit``); a no-op with ``use_ema`` off."""
        if self.use_ema and EMA in self._slots and self._slots[EMA].numel() == W.numel() and not self._ema_fresh:
            with torch.no_grad():
                W.copy_(self._slots[EMA].to(W.device))

    def finalize_variable_values(self, var_list):
        """Keras' ``finalize_variable_values`` for custom loops: every variable of ``var_list`` (the ones, in
        the order, ``apply_gradients`` updated) is overwritten with its moving average.  A plain copy: not on
        the hot path.  A no-op with ``use_ema`` off or before the first update."""
        if not self.use_ema or EMA not in self._slots or self._ema_fresh:
            return
        E = self._slots[EMA]
        var_list = list(var_list)
        lay = self._layout
        if lay is not None and lay.total == E.numel() and len(lay.layer_spans()[0]) == len(var_list):
            views = list(lay.views(E))
        else:
            sizes = [int(math.prod(v.shape)) for v in var_list]
            if sum(sizes) != E.numel():
                raise ValueError(f"finalize_variable_values: the variables hold {sum(sizes)} elements, the moving "
                                 f"average {E.numel()}")
            views, off = [], 0
            for n in sizes:
                views.append(E[off:off + n])
                off += n
        for v, e in zip(var_list, views):
            v.assign(e.reshape(v.shape))

    def apply_flat(self, W: torch.Tensor, G: torch.Tensor, sync_lr: bool = True, t_add: int = 0,
                   accumulated: bool = False, zero_grad: bool = False) -> bool:
        """w <- update(w, g) over the whole slab (gradients already all-reduced).  ``t_add``: this
        step's offset from ``t_dev`` inside a multi-step execution (only Adam reads a step count).
        With gradient accumulation on, ``G`` is first folded (``accumulate``) unless the caller has done so
        (``accumulated=True``); a micro-step that is not the cycle's last only counts.  Returns whether the
        update kernel zeroed ``G`` after reading it, as ``zero_grad`` asked (see ``device_update``).  With
        ``use_ema`` the moving average follows the update: inside the update kernel, else by ``ema_after``."""
        if self._n != W.numel() or self._device != W.device:
            self.build(W.numel(), W.device)
        self.init_ema(W)
        if self._accumulating and not accumulated and not self.accumulate(G):
            self.iterations += 1
            return False
        if sync_lr:
            self._sync_lr()
        # clip + (decay +) update (+ moving average) in the kernel; (``iterations`` is this step's: phase_add 0)
        if self.device_update(W, G, t_add, zero_grad=zero_grad, phase_add=0):
            self.iterations += 1
            return bool(zero_grad) and self._update_zeroes_grad
        self._clip(G)
        if self.weight_decay:
            W.mul_(1.0 - self.current_lr() * self.weight_decay)
        with torch.no_grad():
            self._update(W, G)
        self.ema_after(W)  # (no update kernel ran: an _update that retries device_update fails as it did above)
        self.iterations += 1
        return False

    def _update(self, W, G):
        raise NotImplementedError

    def apply_gradients(self, grads_and_vars):
        """Eager per-variable path for custom training loops (tf.GradientTape style).

        Called from the replica functions of a single-process multi-device MirroredStrategy
        (``strategy.run``), this is TF's merge call: the replicas' gradients are summed across
        replicas in rank order and the variables are updated ONCE, by the last replica to arrive
        (parallel/local_replicas.py rendezvous)."""
        gv = [(g, v) for g, v in grads_and_vars if g is not None]
        from ..parallel.strategy import get_strategy, has_strategy

        grp = getattr(get_strategy(), "_local_group", None) if has_strategy() else None
        if grp is not None and grp.in_region():
            def merge(per_replica):
                n = len(per_replica[0])
                if any(len(p) != n for p in per_replica):
                    raise ValueError("apply_gradients: replicas passed different variable lists")
                # (custom-loop path, not the fit engine: full device syncs order the replicas'
                # gradient producers on their streams against this thread's update)
                if grp.device_comm().gpu:
                    grp.device_comm().synchronize()
                summed = []
                for i in range(n):
                    v = per_replica[0][i][1]
                    dev = v.read_value().device
                    acc = torch.as_tensor(per_replica[0][i][0]).to(dev, copy=True)
                    for p in per_replica[1:]:
                        acc += torch.as_tensor(p[i][0]).to(dev)
                    summed.append((acc, v))
                self._apply_gradients_now(summed)
                if grp.device_comm().gpu:
                    grp.device_comm().synchronize()

            grp.rendezvous(gv, merge)
            return
        self._apply_gradients_now(gv)

    def _apply_gradients_now(self, gv):
        if not gv:
            return
        flat_g = torch.cat([torch.as_tensor(g).reshape(-1).float() for g, _ in gv])
        flat_w = torch.cat([v.read_value().reshape(-1).float() for _, v in gv])
        key = "_eager"
        if getattr(self, key, None) is None or self._n != flat_w.numel():
            self.build(flat_w.numel(), flat_w.device)
            setattr(self, key, True)
        self.apply_flat(flat_w, flat_g.to(flat_w.device))
        off = 0
        for _, v in gv:
            n = int(math.prod(v.shape))
            v.assign(flat_w[off : off + n].reshape(v.shape))
            off += n

    def variables(self):
        return [self.iterations] + list(self._slots.values())

    def get_config(self):
        lr = self._lr
        if isinstance(lr, _sched.LearningRateSchedule):
            lr = _sched.serialize(lr)
        return {"name": self.name, "learning_rate": lr, "clipnorm": self.clipnorm, "clipvalue": self.clipvalue,
                "global_clipnorm": self.global_clipnorm,
                "gradient_accumulation_steps": self.gradient_accumulation_steps, "use_ema": self.use_ema,
                "ema_momentum": self.ema_momentum, "ema_overwrite_frequency": self.ema_overwrite_frequency}

    @classmethod
    def from_config(cls, cfg):
        cfg = dict(cfg)
        if isinstance(cfg.get("learning_rate"), dict):
            cfg["learning_rate"] = _sched.deserialize(cfg["learning_rate"])
        return cls(**cfg)

    def state_dict(self):
        return {"iterations": self.iterations, "slots": {k: v.detach().cpu() for k, v in self._slots.items()}}

    def load_state_dict(self, st):
        self.iterations = int(st.get("iterations", 0))
        for k, v in st.get("slots", {}).items():
            self._slots[k] = v.to(self._device) if self._device is not None else v.clone()
            if k == EMA:
                self._ema_fresh = False  # (a restored average is kept: init_ema leaves it alone)


ACCUMULATOR = "gradient_accumulator"  # the slot of the f32 accumulator slab
EMA = "ema"  # the slot of the f32 moving average of the weights


def _kernel_present(kernel: str) -> bool:
    from .. import ops

    return ops.hip_available() and hasattr(ops.hip(), kernel)


def _hip_ok(t: torch.Tensor, kernel: str = "sgd", opt: Optional[Optimizer] = None) -> bool:
    """``kernel`` can update the slab ``t`` (and apply ``opt``'s gradient clipping, if it has any)."""
    if t.device.type != "cuda" or t.dtype != torch.float32:
        return False
    from .. import ops

    if not hasattr(ops.hip(), kernel):  # ops.hip() raises loudly if the HIP kernels are missing on a GPU box
        return False
    return opt is None or (opt._clip_on_device and (not opt._clipped or t.numel() == opt._n))


class SGD(Optimizer):
    """tf.keras.optimizers.SGD(learning_rate=0.01, momentum=0.0, nesterov=False) (ex:51)."""

    # the GPU update reads the learning rate from ``lr_dev`` (refreshed before every step), so a
    # captured step graph stays correct under learning-rate schedules
    graph_safe = True
    _update_zeroes_grad = True  # (k_sgd / k_sgd_momentum take zero_grad)

    def __init__(self, learning_rate=0.01, momentum=0.0, nesterov=False, name="SGD", **kw):
        super().__init__(learning_rate, name, **kw)
        if not 0.0 <= momentum <= 1.0:
            raise ValueError("momentum must be in [0, 1]")
        self.momentum, self.nesterov = float(momentum), bool(nesterov)

    def _slot_names(self):
        return ["momentum"] if self.momentum > 0 else []

    def device_update(self, W, G, t_add=0, zero_grad=False, phase_add=None):
        if not _hip_ok(W, "sgd", self) or self.weight_decay:
            return False
        from .. import ops

        C = ops.hip()
        extra = dict(self.device_clip(G), **self.device_ema(W, t_add if phase_add is None else phase_add))
        if self.momentum > 0:
            C.sgd_momentum(W, G, self._slots["momentum"], self.lr_dev, self.momentum, self.nesterov,
                           zero_grad=bool(zero_grad), **extra)
        else:
            C.sgd(W, G, self.lr_dev, zero_grad=bool(zero_grad), **extra)
        return True

    def _update(self, W, G):
        if self.device_update(W, G):
            return
        lr = self.current_lr()
        if self.momentum > 0:
            v = self._slots["momentum"]
            v.mul_(self.momentum).add_(G, alpha=-lr)
            if self.nesterov:
                W.add_(v, alpha=self.momentum).add_(G, alpha=-lr)
            else:
                W.add_(v)
        else:
            W.add_(G, alpha=-lr)

    def get_config(self):
        return dict(super().get_config(), momentum=self.momentum, nesterov=self.nesterov)


class Adam(Optimizer):
    def __init__(self, learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7, amsgrad=False, name="Adam", **kw):
        super().__init__(learning_rate, name, **kw)
        self.beta_1, self.beta_2, self.epsilon, self.amsgrad = beta_1, beta_2, epsilon, amsgrad

    def _slot_names(self):
        return ["m", "v"] + (["vhat"] if self.amsgrad else [])

    @property
    def graph_safe(self) -> bool:
        """Whether a captured step replays this update correctly: only the kernel path reads the
        learning rate and the step count from device memory (t_dev); the torch fallback (_update)
        bakes the capture-time values into the graph.  A clipped optimizer takes the kernel path once
        it is built on a GPU slab (build() allocates the clip buffers there)."""
        return self._clip_on_device and _kernel_present("adam")

    _needs_step = True

    def device_update(self, W, G, t_add=0, zero_grad=False, phase_add=None):
        """csrc/kernels/optim.hip k_adam (AdamW's decoupled decay inside the same pass)."""
        if not _hip_ok(W, "adam", self):
            return False
        from .. import ops

        ops.hip().adam(W, G, self._slots["m"], self._slots["v"], self._slots.get("vhat"), self.lr_dev, self.t_dev,
                       int(t_add), self.beta_1, self.beta_2, self.epsilon, float(self.weight_decay or 0.0),
                       **self.device_clip(G), **self.device_ema(W, t_add if phase_add is None else phase_add))
        return True

    def _update(self, W, G):
        t = self.iterations + 1
        lr = self.current_lr()
        m, v = self._slots["m"], self._slots["v"]
        m.mul_(self.beta_1).add_(G, alpha=1 - self.beta_1)
        v.mul_(self.beta_2).addcmul_(G, G, value=1 - self.beta_2)
        lr_t = lr * math.sqrt(1 - self.beta_2 ** t) / (1 - self.beta_1 ** t)
        vv = v
        if self.amsgrad:
            torch.maximum(self._slots["vhat"], v, out=self._slots["vhat"])
            vv = self._slots["vhat"]
        W.addcdiv_(m, vv.sqrt().add_(self.epsilon), value=-lr_t)

    def get_config(self):
        return dict(super().get_config(), beta_1=self.beta_1, beta_2=self.beta_2, epsilon=self.epsilon,
                    amsgrad=self.amsgrad)


class AdamW(Adam):
    def __init__(self, learning_rate=0.001, weight_decay=0.004, beta_1=0.9, beta_2=0.999, epsilon=1e-7, amsgrad=False,
                 name="AdamW", **kw):
        super().__init__(learning_rate, beta_1, beta_2, epsilon, amsgrad, name, weight_decay=weight_decay, **kw)


class RMSprop(Optimizer):
    def __init__(self, learning_rate=0.001, rho=0.9, momentum=0.0, epsilon=1e-7, centered=False, name="RMSprop", **kw):
        super().__init__(learning_rate, name, **kw)
        self.rho, self.momentum, self.epsilon, self.centered = rho, momentum, epsilon, centered

    def _slot_names(self):
        return ["rms"] + (["mom"] if self.momentum > 0 else []) + (["mg"] if self.centered else [])

    # (the torch fallback bakes lr; clipping: see Adam.graph_safe)
    graph_safe = property(lambda self: self._clip_on_device and _kernel_present("rmsprop"))

    def device_update(self, W, G, t_add=0, zero_grad=False, phase_add=None):
        """csrc/kernels/optim.hip k_rmsprop."""
        if not _hip_ok(W, "rmsprop", self) or self.weight_decay:
            return False
        from .. import ops

        ops.hip().rmsprop(W, G, self._slots["rms"], self._slots.get("mom"), self._slots.get("mg"), self.lr_dev,
                          self.rho, self.momentum, self.epsilon, **self.device_clip(G),
                          **self.device_ema(W, t_add if phase_add is None else phase_add))
        return True

    def _update(self, W, G):
        if self.device_update(W, G):
            return
        lr = self.current_lr()
        rms = self._slots["rms"]
        rms.mul_(self.rho).addcmul_(G, G, value=1 - self.rho)
        denom = rms
        if self.centered:
            mg = self._slots["mg"]
            mg.mul_(self.rho).add_(G, alpha=1 - self.rho)
            denom = rms - mg * mg
        step = G / (denom.sqrt() + self.epsilon)
        if self.momentum > 0:
            mom = self._slots["mom"]
            mom.mul_(self.momentum).add_(step, alpha=lr)
            W.sub_(mom)
        else:
            W.add_(step, alpha=-lr)


class Adagrad(Optimizer):
    def __init__(self, learning_rate=0.001, initial_accumulator_value=0.1, epsilon=1e-7, name="Adagrad", **kw):
        super().__init__(learning_rate, name, **kw)
        self.init_acc, self.epsilon = initial_accumulator_value, epsilon

    def _slot_names(self):
        return ["acc"]

    def build(self, n, device):
        fresh = "acc" not in self._slots
        super().build(n, device)
        if fresh:
            self._slots["acc"].fill_(self.init_acc)

    graph_safe = property(lambda self: self._clip_on_device and _kernel_present("adagrad"))

    def device_update(self, W, G, t_add=0, zero_grad=False, phase_add=None):
        """csrc/kernels/optim.hip k_adagrad."""
        if not _hip_ok(W, "adagrad", self) or self.weight_decay:
            return False
        from .. import ops

        ops.hip().adagrad(W, G, self._slots["acc"], self.lr_dev, self.epsilon, **self.device_clip(G),
                          **self.device_ema(W, t_add if phase_add is None else phase_add))
        return True

    def _update(self, W, G):
        if self.device_update(W, G):
            return
        acc = self._slots["acc"]
        acc.addcmul_(G, G)
        W.addcdiv_(G, acc.sqrt().add_(self.epsilon), value=-self.current_lr())


def _f32(x) -> float:
    """``x`` rounded to f32 (the value a kernel receives), as a Python float."""
    return torch.tensor(float(x), dtype=torch.float32).item()


class _Layerwise(Optimizer):
    """Shared base of LARS and LAMB: the step of every element is scaled by a trust ratio of two norms of
    its own variable, so the optimizer needs the slab's layout (``set_layout``).

    Variable i has a decay ``weight_decay_rate`` (0 if its name matches a pattern of
    ``exclude_from_weight_decay``) and takes part in the layer adaptation unless its name matches a pattern
    of ``exclude_from_layer_adaptation`` (default: the decay list); patterns are ``re.search`` on the
    variable's name.  The decay is part of the update direction, not the base class's decoupled
    ``weight_decay`` (which stays None).

    On a GPU slab the step is ``clip_norm`` (if clipped) + three launches of csrc/kernels/layerwise.hip over
    host-validated layer tables; every buffer is allocated in ``build()``, before any capture.  On the CPU
    ``_update`` applies the torch formulas over per-variable views, with f32 torch norms as in ``_clip``.
    """

    def __init__(self, learning_rate, name, weight_decay_rate=0.0, exclude_from_weight_decay=None,
                 exclude_from_layer_adaptation=None, **kw):
        super().__init__(learning_rate, name, **kw)
        self.weight_decay_rate = float(weight_decay_rate)
        self.exclude_from_weight_decay = None if exclude_from_weight_decay is None else list(exclude_from_weight_decay)
        self.exclude_from_layer_adaptation = None if exclude_from_layer_adaptation is None else list(
            exclude_from_layer_adaptation)
        self._built_layout = None
        self._spans = self._wd = self._adapt = None
        self._tables = self._layer_partials = self._layer_ratio = self._layer_norms = None
        self._cpu_ratios: Optional[List[float]] = None  # the last CPU step's ratios (host floats)

    def layer_operands(self, layout):
        """(decay per variable, adapt flag per variable) of ``layout`` under the exclusion patterns."""
        import re

        names = layout.layer_spans()[2]
        dec = self.exclude_from_weight_decay or []
        ada = dec if self.exclude_from_layer_adaptation is None else self.exclude_from_layer_adaptation
        wd = [0.0 if any(re.search(p, n) for p in dec) else self.weight_decay_rate for n in names]
        adapt = [not any(re.search(p, n) for p in ada) for n in names]
        return wd, adapt

    def build(self, n: int, device: torch.device):
        lay = self._layout
        if lay is None:
            raise ValueError(f"{type(self).__name__} is a layer-wise optimizer and needs the slab layout: call "
                             "set_layout(layout) before build() / apply_flat() (model.fit and apply_gradients do)")
        if lay.total != n:
            raise ValueError(f"{type(self).__name__}: the layout covers {lay.total} elements, the slab has {n}")
        if self._n == n and self._device == device and self._built_layout is lay:
            return
        self._n = None
        super().build(n, device)
        self._built_layout = lay
        self._spans = lay.layer_spans()
        self._wd, self._adapt = self.layer_operands(lay)
        self._tables = self._layer_partials = self._layer_ratio = self._layer_norms = None
        if device.type == "cuda" and _kernel_present("layer_tables"):
            from .. import ops

            V = len(self._wd)
            with torch.cuda.device(device):
                self._tables = ops.hip().layer_tables(self._spans[0], self._spans[1], n, self._wd, self._adapt)
            self._layer_partials = torch.zeros(max(2, 2 * self._tables.C), dtype=torch.float64, device=device)
            self._layer_ratio = torch.ones(max(1, V), dtype=torch.float32, device=device)
            self._layer_norms = torch.zeros(max(1, V), 2, dtype=torch.float32, device=device)

    @property
    def last_layer_ratios(self) -> Optional[torch.Tensor]:
        """The trust ratios of the last device step, one per variable (a device view; None on the CPU)."""
        return None if self._tables is None else self._layer_ratio[:self._tables.V]

    @property
    def last_layer_norms(self) -> Optional[torch.Tensor]:
        """[V, 2] of the last device step: |w_i| and |g'_i| (LARS) or |u_i| (LAMB); None on the CPU."""
        return None if self._tables is None else self._layer_norms[:self._tables.V]

    @property
    def graph_safe(self) -> bool:
        """The kernels are present, the optimizer is built on a GPU slab and any clipping runs on the device
        (see Adam.graph_safe)."""
        return self._tables is not None and self._clip_on_device

    def device_update(self, W, G, t_add=0, zero_grad=False, phase_add=None):
        """csrc/kernels/layerwise.hip: chunk sums, per-variable ratios, update (the moving average in it)."""
        if W.device.type != "cuda" or W.dtype != torch.float32:
            return False
        if self._tables is None or not self._clip_on_device:
            raise RuntimeError(f"{type(self).__name__}: the extension has no layer_tables / clip_norm kernel for "
                               "the GPU slab (rebuild: python build_native.py)")
        if W.numel() != self._n:
            raise RuntimeError(f"{type(self).__name__} updates the whole slab ({self._n} elements), got {W.numel()}")
        from .. import ops

        self._launch(ops.hip(), W, G, int(t_add), self.device_clip(G),
                     self.device_ema(W, t_add if phase_add is None else phase_add))
        return True

    def _launch(self, C, W, G, t_add, clip, ema):
        raise NotImplementedError

    def _views(self, *flats):
        offs, sizes, _ = self._spans
        for i, (o, s) in enumerate(zip(offs, sizes)):
            yield (i,) + tuple(f[o:o + s] for f in flats)

    def _apply_gradients_now(self, gv):
        """Custom loops: the variables passed are packed into an aligned slab of their own layout, so the
        same kernels (and the same formulas on the CPU) serve them."""
        if not gv:
            return
        from ..engine.slab import SlabLayout

        items = tuple((str(getattr(v, "name", f"variable_{i}")), tuple(int(d) for d in v.shape))
                      for i, (_, v) in enumerate(gv))
        if getattr(self, "_eager_items", None) != items:
            self.set_layout(SlabLayout.from_shapes(items))
            self._eager_items = items
        lay = self._layout
        dev = gv[0][1].read_value().device
        W = lay.pack([v.read_value().float() for _, v in gv], device=dev)
        G = lay.pack([torch.as_tensor(g).float() for g, _ in gv], device=dev)
        self.build(W.numel(), W.device)
        self.apply_flat(W, G)
        for (_, v), view in zip(gv, lay.views(W)):
            v.assign(view)

    def get_config(self):
        return dict(super().get_config(), weight_decay_rate=self.weight_decay_rate,
                    exclude_from_weight_decay=self.exclude_from_weight_decay,
                    exclude_from_layer_adaptation=self.exclude_from_layer_adaptation)


class LARS(_Layerwise):
    """Layer-wise Adaptive Rate Scaling (You, Gitman, Ginsburg 2017), with the arguments of
    ``tf.contrib.opt.LARSOptimizer`` / tf-models ``LARS``:

        r_i = eeta |w_i| / (|g_i| + wd_i |w_i| + epsilon)  if variable i adapts and |w_i| > 0 and |g_i| > 0, else 1
        d = g + wd_i w,  s = lr r_i,  v <- momentum v - s d,  w <- w + v   (nesterov: w <- w + momentum v - s d)

    i.e. this package's momentum SGD with ``lr`` replaced by ``s`` and ``g`` by ``d``; ``g`` is the gradient
    after clipping.  Norms in f64 on the device, in f32 on the CPU.  TF-addons and tf-models are not installed
    where this was written: parity with their implementations is unpinned.
    """

    def __init__(self, learning_rate=0.01, momentum=0.9, weight_decay_rate=0.0, eeta=0.001, epsilon=0.0,
                 nesterov=False, exclude_from_weight_decay=None, exclude_from_layer_adaptation=None, name="LARS",
                 **kw):
        super().__init__(learning_rate, name, weight_decay_rate, exclude_from_weight_decay,
                         exclude_from_layer_adaptation, **kw)
        if not 0.0 <= momentum <= 1.0:
            raise ValueError("momentum must be in [0, 1]")
        self.momentum, self.eeta, self.epsilon, self.nesterov = float(momentum), float(eeta), float(epsilon), bool(
            nesterov)

    def _slot_names(self):
        return ["momentum"]

    def _launch(self, C, W, G, t_add, clip, ema):
        T = self._tables
        C.lars_sums(T, W, G, self._layer_partials, **clip)
        C.lars_ratio(T, self._layer_partials, self._layer_ratio, self._layer_norms, self.eeta, self.epsilon)
        C.lars_update(T, W, G, self._slots["momentum"], self._layer_ratio, self.lr_dev, self.momentum, self.nesterov,
                      **clip, **ema)

    def _update(self, W, G):
        lr, mu = _f32(self.current_lr()), self.momentum
        eeta, eps = _f32(self.eeta), _f32(self.epsilon)
        self._cpu_ratios = []
        for i, w, g, v in self._views(W, G, self._slots["momentum"]):
            wd, r = self._wd[i], 1.0
            if self._adapt[i]:
                nw, ng = float(torch.linalg.vector_norm(w)), float(torch.linalg.vector_norm(g))
                if nw > 0 and ng > 0:
                    r = _f32(eeta * nw / (ng + _f32(wd) * nw + eps))
            self._cpu_ratios.append(r)
            s = _f32(lr * r)
            d = g.add(w, alpha=wd) if wd else g
            v.mul_(mu).add_(d, alpha=-s)
            if self.nesterov:
                w.add_(v, alpha=mu).add_(d, alpha=-s)
            else:
                w.add_(v)

    def get_config(self):
        return dict(super().get_config(), momentum=self.momentum, eeta=self.eeta, epsilon=self.epsilon,
                    nesterov=self.nesterov)


class LAMB(_Layerwise):
    """Layer-wise Adaptive Moments for Batch training (You et al. 2019), with the arguments of
    ``tfa.optimizers.LAMB``; t = iterations + 1:

        m <- beta_1 m + (1 - beta_1) g,   v <- beta_2 v + (1 - beta_2) g^2
        u = (m / (1 - beta_1^t)) / (sqrt(v / (1 - beta_2^t)) + epsilon) + wd_i w
        r_i = |w_i| / |u_i|  if variable i adapts and |w_i| > 0 and |u_i| > 0, else 1
        w <- w - lr r_i u

    ``g`` is the gradient after clipping.  Norms in f64 on the device, in f32 on the CPU.  TF-addons is not
    installed where this was written: parity with its implementation is unpinned.
    """

    _needs_step = True

    def __init__(self, learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-6, weight_decay_rate=0.0,
                 exclude_from_weight_decay=None, exclude_from_layer_adaptation=None, name="LAMB", **kw):
        super().__init__(learning_rate, name, weight_decay_rate, exclude_from_weight_decay,
                         exclude_from_layer_adaptation, **kw)
        if not (0.0 < beta_1 < 1.0 and 0.0 < beta_2 < 1.0):
            raise ValueError("beta_1 and beta_2 must lie in (0, 1)")
        self.beta_1, self.beta_2, self.epsilon = float(beta_1), float(beta_2), float(epsilon)

    def _slot_names(self):
        return ["m", "v"]

    def _launch(self, C, W, G, t_add, clip, ema):
        T, m, v = self._tables, self._slots["m"], self._slots["v"]
        hp = (self.t_dev, t_add, self.beta_1, self.beta_2, self.epsilon)
        C.lamb_sums(T, W, G, m, v, self._layer_partials, *hp, **clip)
        C.lamb_ratio(T, self._layer_partials, self._layer_ratio, self._layer_norms)
        C.lamb_update(T, W, m, v, self._layer_ratio, self.lr_dev, *hp, **ema)

    def _update(self, W, G):
        lr = _f32(self.current_lr())
        # the bias corrections 1 - beta^t in f64 from the f32 betas, rounded once (the kernels reach the same
        # f32 values to a few ulp as -expm1f(t log beta); the plain f32 difference cancels)
        t = self.iterations + 1
        c1, c2 = _f32(1.0 - _f32(self.beta_1) ** t), _f32(1.0 - _f32(self.beta_2) ** t)
        self._cpu_ratios = []
        for i, w, g, m, v in self._views(W, G, self._slots["m"], self._slots["v"]):
            m.mul_(self.beta_1).add_(g, alpha=1 - self.beta_1)
            v.mul_(self.beta_2).addcmul_(g, g, value=1 - self.beta_2)
            u = m.div(c1).div_(v.div(c2).sqrt_().add_(self.epsilon))
            if self._wd[i]:
                u.add_(w, alpha=self._wd[i])
            r = 1.0
            if self._adapt[i]:
                nw, nu = float(torch.linalg.vector_norm(w)), float(torch.linalg.vector_norm(u))
                if nw > 0 and nu > 0:
                    r = _f32(nw / nu)
            self._cpu_ratios.append(r)
            w.add_(u, alpha=-_f32(lr * r))

    def get_config(self):
        return dict(super().get_config(), beta_1=self.beta_1, beta_2=self.beta_2, epsilon=self.epsilon)


Lamb = LAMB

_ALIASES = {"sgd": SGD, "adam": Adam, "adamw": AdamW, "rmsprop": RMSprop, "adagrad": Adagrad, "lars": LARS,
            "lamb": LAMB}


def get(identifier) -> Optimizer:
    if isinstance(identifier, Optimizer):
        return identifier
    if isinstance(identifier, str):
        k = identifier.lower()
        if k not in _ALIASES:
            raise ValueError(f"unknown optimizer {identifier!r}")
        return _ALIASES[k]()
    if isinstance(identifier, dict):
        return _ALIASES[identifier["class_name"].lower()].from_config(identifier.get("config", {}))
    raise ValueError(f"could not interpret optimizer {identifier!r}")


def serialize(opt: Optimizer):
    return {"class_name": type(opt).__name__, "config": opt.get_config()}


schedules = _sched


class legacy:  # noqa: N801 - tf.keras.optimizers.legacy
    SGD = SGD
    Adam = Adam
    RMSprop = RMSprop
    Adagrad = Adagrad

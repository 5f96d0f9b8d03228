"""FusedAdam: ``torch.optim.Adam`` semantics (train.py:872,902) as ONE HIP kernel per contiguous run.

Each param group's parameters are re-homed into one flat fp32 buffer (``p.data`` becomes a
16-byte-aligned view), with a matching flat gradient buffer whose views the backward kernels
write into directly (``fusion.grad_buffer``), and flat ``exp_avg`` / ``exp_avg_sq`` state.
The flat gradient buffer is also what the data-parallel all-reduce ships (``dist.py``).

Like torch's Adam, parameters whose ``.grad`` is None are skipped (no moment decay, no weight
decay, no step increment), and the bias correction uses each parameter's OWN step count
(torch keeps ``state[p]['step']`` per parameter): the kernel runs over maximal runs of
adjacent params that have a gradient and share a step count.  With data parallelism the
"has a gradient" set is the union over ranks (``set_used``), as DDP does for parameters unused
on some ranks.

Three options extend the per-step pass over the flat buffers without a host sync (csrc/optim.hip):

* ``max_grad_norm``: ``clip_grad_norm_`` semantics on the device.  ONE global norm over every parameter that has a
  gradient this step, over all groups, of ``grad_scale * g`` (under data parallelism: of the averaged gradient, after
  the all-reduce, so every rank computes the same bits).  Deterministic fp64 sums; the coefficient stays in a small
  device record that the Adam kernel reads, and the record's running statistics are read once per epoch
  (``grad_norm_stats``).
* ``ema_decay``: a flat ``ema`` plane per group, initialised to the parameters at construction and updated inside the
  Adam kernel, ``e += (1 - d) * (p_new - e)``.  A parameter that Adam skips in a step (no gradient) is skipped by the
  EMA too -- unlike ``torch.optim.swa_utils.AveragedModel``, which would keep pulling the average towards the
  unchanged parameter.  ``ema_weights()`` swaps the average in for evaluation.  Buffers (BatchNorm running
  statistics) are not parameters and are not averaged.
* ``state_dict`` / ``load_state_dict`` in ``torch.optim.Adam``'s format, so a run resumes with its moments, step
  counts and EMA, and the state moves between the two optimizers.

With both options ``None`` (the default) ``step`` issues exactly the ``mer_adam_step`` launches it always did.
"""
from __future__ import annotations

import contextlib
from typing import List, Optional, Sequence

import torch

from . import kernels as K


def _align4(n: int) -> int:
    return (n + 3) // 4 * 4


def weight_version(p: torch.Tensor) -> tuple:
    """Identity of a weight's current VALUE for derived-copy caches (bf16 packs, INT8 images): storage
    address, autograd version counter, and the FusedAdam update count -- the Adam kernel writes the flat
    buffer through a raw pointer, which PyTorch's version counter never sees."""
    return (p.data_ptr(), p._version, getattr(p, "_mer_updates", 0))


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 max_grad_norm: Optional[float] = None, ema_decay: Optional[float] = None):
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError("max_grad_norm must be positive (or None: no clipping)")
        if ema_decay is not None and not 0.0 <= float(ema_decay) < 1.0:
            raise ValueError("ema_decay must lie in [0, 1) (or None: no weight averaging)")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self._clip_rec = None       # fp32[K.CLIP_REC_FLOATS] device record (include/mer.h), allocated below
        self._segments = {}         # run layout -> K.NormSegments (device table + partials)
        self._ema_swapped = False   # inside ema_weights(): ``flat`` holds the average, ``ema`` the live weights
        self.grad_scale = 1.0  # set to 1/world_size by the data-parallel wrapper (SUM all-reduce)
        self._used: Optional[List[List[bool]]] = None  # set_used(): per-group per-param override for one step
        self._flat = []
        for group in self.param_groups:
            ps: List[torch.Tensor] = group["params"]
            if not ps:
                self._flat.append(None)
                continue
            dev = ps[0].device
            offs, total = [], 0
            for p in ps:
                if p.dtype != torch.float32:
                    raise TypeError("FusedAdam keeps fp32 master weights")
                offs.append(total)
                total += _align4(p.numel())
            flat = torch.zeros(total, device=dev, dtype=torch.float32)
            gflat = torch.zeros(total, device=dev, dtype=torch.float32)
            with torch.no_grad():
                for p, o in zip(ps, offs):
                    flat[o:o + p.numel()].copy_(p.detach().reshape(-1))
                    p.data = flat[o:o + p.numel()].view_as(p)
                    # (buffer, offset): a FRESH view is built per backward (fusion.grad_buffer) so autograd's
                    # AccumulateGrad can adopt it without a copy (a view we also kept alive would be cloned)
                    p._mer_grad_slot = (gflat, o)
            self._flat.append(dict(flat=flat, gflat=gflat, m=torch.zeros_like(flat), v=torch.zeros_like(flat),
                                   offs=offs, steps=[0] * len(ps)))
            if self.ema_decay is not None:
                self._flat[-1]["ema"] = flat.clone()
            if self.max_grad_norm is not None and self._clip_rec is None:
                self._clip_rec = torch.zeros(K.CLIP_REC_FLOATS, device=dev, dtype=torch.float32)

    def flat_grads(self):
        return [f["gflat"] for f in self._flat if f is not None]

    def flat_params(self):
        return [f["flat"] for f in self._flat if f is not None]

    def param_slices(self):
        """(flat-buffer index as in ``flat_grads()``, param, offset, numel) of every managed parameter, in
        flat-buffer order."""
        out = []
        for gi, (f, group) in enumerate((f, g) for f, g in zip(self._flat, self.param_groups) if f is not None):
            for p, o in zip(group["params"], f["offs"]):
                out.append((gi, p, o, p.numel()))
        return out

    def zero_grad(self, set_to_none: bool = True) -> None:
        self._used = None
        for f, group in zip(self._flat, self.param_groups):
            if f is None:
                continue
            f["gflat"].zero_()
            for p in group["params"]:
                p.grad = None

    @torch.no_grad()
    def gather_grads(self) -> List[List[bool]]:
        """Bring every gradient autograd produced outside the flat buffer home into it (so the data-parallel
        all-reduce sees it) and return the local per-group "has a gradient" flags."""
        used = []
        for f, group in zip(self._flat, self.param_groups):
            if f is None:
                used.append([])
                continue
            gflat = f["gflat"]
            flags = []
            for p, o in zip(group["params"], f["offs"]):
                has = p.grad is not None
                if has and p.grad.data_ptr() != gflat[o:].data_ptr():
                    gflat[o:o + p.numel()].view_as(p).copy_(p.grad)
                    p.grad = gflat[o:o + p.numel()].view_as(p)
                flags.append(has)
            used.append(flags)
        return used

    def set_used(self, used: Sequence[Sequence[bool]]) -> None:
        """Override, for the next ``step``, which parameters count as having a gradient (the union over
        data-parallel ranks); their flat-buffer slots hold the reduced gradient."""
        self._used = [list(u) for u in used]

    def _runs(self, f, group, flags):
        """Advance the step count of every parameter of the group that has a gradient and return the maximal runs
        [start, end, step] of adjacent ones that share a step count."""
        ps, steps = group["params"], f["steps"]
        runs, cur = [], None
        for i, (p, o) in enumerate(zip(ps, f["offs"])):
            if not flags[i]:
                cur = None
                continue
            steps[i] += 1
            end = o + _align4(p.numel())
            if cur is not None and cur[1] == o and cur[2] == steps[i]:
                cur[1] = end
            else:
                cur = [o, end, steps[i]]
                runs.append(cur)
            p._mer_updates = getattr(p, "_mer_updates", 0) + 1
        return runs

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        if self._ema_swapped:
            raise RuntimeError("FusedAdam.step() inside ema_weights(): the parameters hold the average")
        used = self._used if self._used is not None else self.gather_grads()
        self._used = None
        plain = self.max_grad_norm is None and self.ema_decay is None
        todo = []
        for gi, (f, group, flags) in enumerate(zip(self._flat, self.param_groups, used)):
            if f is None:
                continue
            runs = self._runs(f, group, flags)
            if not plain:
                todo.append((gi, f, group, runs))
                continue
            b1, b2 = group["betas"]
            for s, e, t in runs:
                K.adam_step(f["flat"][s:e], f["gflat"][s:e], f["m"][s:e], f["v"][s:e], group["lr"], b1, b2,
                            group["eps"], group["weight_decay"], t, self.grad_scale)
        if plain or not any(runs for _, _, _, runs in todo):
            return loss
        coef = None
        if self.max_grad_norm is not None:  # one norm over every run of every group, then the coefficient
            key = tuple((gi, s, e) for gi, _, _, runs in todo for s, e, _ in runs)
            segs = self._segments.get(key)
            if segs is None:
                if len(self._segments) >= 64:  # LayerDrop / ModalityDropout layouts: bounded, rebuilt on demand
                    self._segments.clear()
                segs = self._segments[key] = K.NormSegments(
                    [f["gflat"][s:e] for _, f, _, runs in todo for s, e, _ in runs])
            K.grad_sqnorm(segs)
            K.clip_finalize(segs, self.grad_scale, self.max_grad_norm, self._clip_rec)
            coef = self._clip_rec[K.CLIP_COEF:K.CLIP_COEF + 1]
        decay = self.ema_decay if self.ema_decay is not None else 0.0
        for _, f, group, runs in todo:
            b1, b2 = group["betas"]
            ema = f.get("ema")
            for s, e, t in runs:
                K.adam_step_ex(f["flat"][s:e], f["gflat"][s:e], f["m"][s:e], f["v"][s:e], group["lr"], b1, b2,
                               group["eps"], group["weight_decay"], t, self.grad_scale, coef=coef,
                               ema=None if ema is None else ema[s:e], ema_decay=decay)
        return loss

    # ---- gradient-norm telemetry -------------------------------------------------------------------------------
    def grad_norm_stats(self, reset: bool = True) -> dict:
        """``{steps, mean, max, last, nonfinite_steps}`` of the clipped steps since the last reset, as Python
        numbers, in ONE device-to-host read (call it once per epoch).  ``mean`` and ``max`` are over the steps whose
        norm was finite; ``last`` is the latest norm, finite or not.  A window in which no step had a finite norm --
        none at all, or every one non-finite -- has no mean and no max: both are NaN, never a zero that would read as
        a window of vanishing gradients."""
        if self._clip_rec is None:
            raise RuntimeError("grad_norm_stats() needs FusedAdam(max_grad_norm=...)")
        r = self._clip_rec.tolist()
        if reset:
            self._clip_rec[K.CLIP_STEPS:K.CLIP_NONFINITE + 1].zero_()
        steps, bad = int(r[K.CLIP_STEPS]), int(r[K.CLIP_NONFINITE])
        finite = steps - bad
        return {"steps": steps, "mean": r[K.CLIP_NORM_SUM] / finite if finite > 0 else float("nan"),
                "max": r[K.CLIP_NORM_MAX] if finite > 0 else float("nan"), "last": r[K.CLIP_TOTAL_NORM],
                "nonfinite_steps": bad}

    # ---- weight averaging ----------------------------------------------------------------------------------------
    def flat_ema(self):
        return [f["ema"] for f in self._flat if f is not None and "ema" in f]

    @torch.no_grad()
    def _swap_ema(self) -> None:
        for f, group in zip(self._flat, self.param_groups):
            if f is None:
                continue
            tmp = f["flat"].clone()
            f["flat"].copy_(f["ema"])
            f["ema"].copy_(tmp)
            for p in group["params"]:  # every weight_version-keyed cache (bf16 / WavLM packs, INT8 images) refreshes
                p._mer_updates = getattr(p, "_mer_updates", 0) + 1
        self._ema_swapped = not self._ema_swapped

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the context the parameters hold the averaged weights (for ``evaluate`` / ``save_checkpoint``).
        The CONTENTS of ``flat`` and ``ema`` are swapped, so every address stays put and captured graphs stay
        valid; ``_mer_updates`` is bumped on entry and on exit, so derived weight copies are rebuilt."""
        if self.ema_decay is None:
            raise RuntimeError("ema_weights() needs FusedAdam(ema_decay=...)")
        if self._ema_swapped:
            raise RuntimeError("ema_weights() does not nest")
        self._swap_ema()
        try:
            yield self
        finally:
            self._swap_ema()

    # ---- resumable state (torch.optim.Adam's format) ---------------------------------------------------------------
    @staticmethod
    def _torch_group_keys() -> dict:
        """The hyper-parameter keys (with their defaults) of a torch.optim.Adam param group of this torch version."""
        return dict(torch.optim.Adam([torch.zeros(1, requires_grad=True)]).defaults)

    @torch.no_grad()
    def state_dict(self) -> dict:
        """``{"state": {i: {"step": fp32 scalar, "exp_avg", "exp_avg_sq"}}, "param_groups": [...]}`` as
        ``torch.optim.Adam.state_dict()`` gives it, tensors copied to the host; parameters that never stepped are
        absent from ``state``.  With weight averaging every group also carries ``"ema"``, one tensor per parameter
        (an unknown group key: ``Optimizer.load_state_dict`` carries it along untouched), and the top-level
        ``"fused_adam"`` entry (which torch's loader never looks at) holds the two options -- and, when called
        inside ``ema_weights()``, the live weights, since the model's own state dict then holds the average."""
        state, groups, live, idx = {}, [], [], 0
        torch_keys = self._torch_group_keys()

        def host(buf, o, p):
            return buf[o:o + p.numel()].detach().to("cpu", copy=True).view(p.shape)

        for f, group in zip(self._flat, self.param_groups):
            out = dict(torch_keys)
            out.update({k: v for k, v in group.items() if k != "params"})
            ps = group["params"]
            out["params"] = list(range(idx, idx + len(ps)))
            if f is not None:
                for i, (p, o) in enumerate(zip(ps, f["offs"])):
                    if f["steps"][i] > 0:
                        state[idx + i] = {"step": torch.tensor(float(f["steps"][i]), dtype=torch.float32),
                                          "exp_avg": host(f["m"], o, p), "exp_avg_sq": host(f["v"], o, p)}
                if "ema" in f:
                    avg, cur = ("flat", "ema") if self._ema_swapped else ("ema", "flat")
                    out["ema"] = [host(f[avg], o, p) for p, o in zip(ps, f["offs"])]
                    if self._ema_swapped:
                        live.append([host(f[cur], o, p) for p, o in zip(ps, f["offs"])])
            idx += len(ps)
            groups.append(out)
        return {"state": state, "param_groups": groups,
                "fused_adam": {"max_grad_norm": self.max_grad_norm, "ema_decay": self.ema_decay,
                               "live_params": live if self._ema_swapped else None}}

    @torch.no_grad()
    def load_state_dict(self, state_dict: dict) -> None:
        """Load a ``FusedAdam`` or a ``torch.optim.Adam`` state dict over the same parameters (same groups, same
        order).  Hyper-parameters of the groups are taken over as torch does; moments and step counts of parameters
        absent from ``state`` are reset.  An ``"ema"`` list is loaded when this optimizer averages (without one the
        average restarts from the current parameters); ``live_params`` (a state saved inside ``ema_weights()``)
        are written to the parameters, so load the model's state dict BEFORE the optimizer's."""
        if self._ema_swapped:
            raise RuntimeError("load_state_dict() inside ema_weights()")
        saved, state = state_dict["param_groups"], state_dict["state"]
        if len(saved) != len(self.param_groups):
            raise ValueError("loaded state dict has a different number of parameter groups")
        if any(len(sg["params"]) != len(g["params"]) for sg, g in zip(saved, self.param_groups)):
            raise ValueError("loaded state dict contains a parameter group that doesn't match the size of "
                             "optimizer's group")
        if any(sg.get("amsgrad") or sg.get("maximize") or sg.get("decoupled_weight_decay") for sg in saved):
            raise ValueError("FusedAdam is plain Adam: no amsgrad, maximize or decoupled weight decay")
        extra = state_dict.get("fused_adam") or {}
        live = extra.get("live_params")

        def put(buf, o, p, t):
            if tuple(t.shape) != tuple(p.shape):
                raise ValueError(f"state of shape {tuple(t.shape)} for a parameter of shape {tuple(p.shape)}")
            buf[o:o + p.numel()].copy_(t.reshape(-1).to(torch.float32))

        li = 0
        for f, group, sg in zip(self._flat, self.param_groups, saved):
            group.update({k: v for k, v in sg.items() if k not in ("params", "ema")})
            if f is None:
                continue
            f["m"].zero_()
            f["v"].zero_()
            for i, (p, o, sid) in enumerate(zip(group["params"], f["offs"], sg["params"])):
                st = state.get(sid)
                f["steps"][i] = int(round(float(st["step"]))) if st is not None else 0
                if st is not None:
                    put(f["m"], o, p, st["exp_avg"])
                    put(f["v"], o, p, st["exp_avg_sq"])
            if live is not None:
                for p, o, t in zip(group["params"], f["offs"], live[li]):
                    put(f["flat"], o, p, t)
                    p._mer_updates = getattr(p, "_mer_updates", 0) + 1
                li += 1
            if "ema" in f:
                if sg.get("ema") is not None:
                    for p, o, t in zip(group["params"], f["offs"], sg["ema"]):
                        put(f["ema"], o, p, t)
                else:
                    f["ema"].copy_(f["flat"])

    def state_steps(self) -> List[List[int]]:
        """Per-group per-parameter Adam step counts (torch's ``state[p]['step']``)."""
        return [list(f["steps"]) if f is not None else [] for f in self._flat]

"""Restatements for the optimizer's clipping / EMA / resume tests (a plain helper module, not a conftest).

Like tests/kernel_parity.py every restatement is plain torch on the CPU evaluated in the dtype ``dt`` it is given:
float64 is the reference, float32 the same text in the kernels' precision, and ``assert_fp64_parity`` judges a kernel by
the distance between the two.  Scalars that cross the C ABI as ``float`` are rounded to float32 first (``f32``).
"""
from __future__ import annotations

import torch

from tests.kernel_parity import F32, F64, f32, gen, randn

CLIP_EPS = 1e-6  # clip_grad_norm_'s and mer_clip_finalize's 1e-6f


def ref_clip(grads, max_norm, grad_scale, dt):
    """(total_norm, coef) of ``clip_grad_norm_`` over ``grad_scale * g`` restated in dtype dt:
    total_norm = grad_scale * sqrt(sum g^2), coef = min(1, max_norm / (total_norm + 1e-6))."""
    sq = sum((g.to(dt) ** 2).sum() for g in grads)
    total = torch.tensor(f32(grad_scale), dtype=dt) * torch.sqrt(sq)
    coef = torch.clamp(torch.tensor(f32(max_norm), dtype=dt) / (total + torch.tensor(f32(CLIP_EPS), dtype=dt)), max=1.0)
    return total, coef


def norm_inputs(n, seed, outliers=3):
    """adam_inputs-style normals bounded away from zero, with a few 1e3 outliers."""
    g = gen(seed)
    r = randn(g, n)
    x = torch.sign(r) * (0.1 + r.abs())
    x[x == 0] = 0.1
    if n >= 8:
        idx = torch.randint(0, n, (outliers,), generator=g)
        x[idx] = x[idx] * 1e3
    return x


def ref_adam_ex(p, g, m, v, e, lr, b1, b2, eps, wd, step, grad_scale, coef, ema_decay, dt):
    """kernel_parity.ref_adam with the two terms of mer_adam_step_ex: the gradient scale is grad_scale * coef, and
    after the parameter update e += (1 - d) * (p_new - e) (``e`` None: no EMA)."""
    p, g, m, v = (t.to(dt) for t in (p, g, m, v))
    lr, b1, b2, eps, wd, gs, cf = (torch.tensor(f32(t), dtype=dt) for t in (lr, b1, b2, eps, wd, grad_scale, coef))
    st = torch.tensor(float(step), dtype=dt)
    bc1, bc2 = 1 - b1 ** st, 1 - b2 ** st
    gr = (gs * cf) * g + wd * p
    m = b1 * m + (1 - b1) * gr
    v = b2 * v + (1 - b2) * gr * gr
    p = p - (lr / bc1) * m / (torch.sqrt(v) / torch.sqrt(bc2) + eps)
    out = {"p": p, "m": m, "v": v}
    if e is not None:
        e = e.to(dt)
        out["e"] = e + (1 - torch.tensor(f32(ema_decay), dtype=dt)) * (p - e)
    return out


def torch_adam_run(params0, group_of, lrs, grads_per_step, dt, wd, max_norm=None, grad_scale=1.0, ema_decay=None,
                   betas=(0.9, 0.999), eps=1e-8):
    """The optimizer's reference: ``torch.optim.Adam`` (+ ``clip_grad_norm_``) on the CPU in dtype dt.

    ``params0``: initial fp32 tensors; ``group_of[i]``: the param group of parameter i, ``lrs`` the groups' learning
    rates; ``grads_per_step``: per step a list with one fp32 gradient (or None: no gradient this step) per parameter.
    The gradient the optimizer sees is ``grad_scale * g`` (the averaged gradient of a data-parallel step), clipped to
    ``max_norm`` as one global norm.  The EMA follows the rule of optim.py: a parameter without a gradient is skipped.
    Returns {"p", "m", "v", "e", "steps", "norms"} (lists per parameter; zeros for moments that never stepped)."""
    ps = [torch.nn.Parameter(t.detach().clone().to(dt)) for t in params0]
    groups = [{"params": [p for p, gi in zip(ps, group_of) if gi == k], "lr": f32(lr)} for k, lr in enumerate(lrs)]
    opt = torch.optim.Adam(groups, betas=(f32(betas[0]), f32(betas[1])), eps=f32(eps), weight_decay=f32(wd))
    ema = [p.detach().clone() for p in ps] if ema_decay is not None else None
    norms = []
    for grads in grads_per_step:
        for p, g in zip(ps, grads):
            p.grad = None if g is None else g.to(dt) * torch.tensor(f32(grad_scale), dtype=dt)
        if max_norm is not None:
            norms.append(torch.nn.utils.clip_grad_norm_(ps, f32(max_norm)).detach().clone())
        opt.step()
        if ema is not None:
            w = 1 - torch.tensor(f32(ema_decay), dtype=dt)
            for e, p, g in zip(ema, ps, grads):
                if g is not None:
                    e += w * (p.detach() - e)
    st = [opt.state.get(p, {}) for p in ps]
    return {"p": [p.detach().clone() for p in ps],
            "m": [s["exp_avg"].clone() if s else torch.zeros_like(p.detach()) for s, p in zip(st, ps)],
            "v": [s["exp_avg_sq"].clone() if s else torch.zeros_like(p.detach()) for s, p in zip(st, ps)],
            "e": ema, "steps": [int(s["step"]) if s else 0 for s in st], "norms": norms}


def both(fn):
    return fn(F64), fn(F32)

"""Direct parity of single kernels against float64 restatements (a plain helper module, not a conftest).

Every restatement below is the operation written in plain torch on the CPU, evaluated in the dtype ``dt`` it is given:
float64 is the reference, float32 the same text in the kernels' precision.  ``assert_fp64_parity`` bounds a kernel's
error by 16 x the error of the float32 restatement: the bar is measured against the reference,
never against the kernel.  A kernel that stores bfloat16 meets ``assert_bf16_parity``: the same bar, with the final
rounding applied to the reference's interval instead of a bf16 tolerance.

Scalars that cross the C ABI as ``float`` (dropout p, LayerNorm eps, the softmax scale, Adam's hyper-parameters) are
rounded to float32 before either restatement uses them: ``0.999f != 0.999`` is not a kernel error.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from tests.helpers import dropout_keep, dropout_keep_pair

EPS32 = float(np.finfo(np.float32).eps)
ERF_FAST_ABS = 1.5e-7  # csrc/common.h erf_fast: documented absolute error
F64, F32 = torch.float64, torch.float32


def f32(x) -> float:
    """The value a Python float has after crossing the ABI as a C float."""
    return float(np.float32(x))


def _max_abs(t) -> float:
    return float(t.abs().max()) if t.numel() else 0.0


def assert_fp64_parity(got, ref64, ref32, extra=0.0, what=""):
    """err = max|got - ref64| <= 16 * max|ref32 - ref64| + eps32 * max|ref64| + extra; returns err / bar."""
    got = torch.as_tensor(got).detach().cpu()
    assert ref64.dtype == F64 and ref32.dtype == F32, what
    assert tuple(got.shape) == tuple(ref64.shape) == tuple(ref32.shape), (what, got.shape, ref64.shape, ref32.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite kernel output"
    err = _max_abs(got.to(F64) - ref64)
    bar = _max_abs(ref32.to(F64) - ref64)
    ratio = err / bar if bar > 0 else (0.0 if err == 0 else math.inf)
    print(f"parity {what}: err={err:.3e} bar={bar:.3e} ratio={ratio:.3f}")
    bound = 16.0 * bar + EPS32 * _max_abs(ref64) + float(extra)
    assert err <= bound, f"{what}: err {err:.3e} > {bound:.3e} (bar {bar:.3e}, ratio {ratio:.2f})"
    return ratio


def assert_parity_all(got: dict, ref64: dict, ref32: dict, keys, extra=None, what=""):
    for k in keys:
        assert_fp64_parity(got[k], ref64[k], ref32[k], extra=(extra or {}).get(k, 0.0), what=f"{what} {k}")


BF16 = torch.bfloat16


def to_bf16(t) -> torch.Tensor:
    """Round to bfloat16 the way the comparison below means it: float64 -> float32 -> bfloat16, both to nearest even
    (torch converts float64 to bfloat16 through float32 anyway: 1 + 2^-8 + 2^-30 becomes 1.0)."""
    return t.to(F32).to(BF16)


def bf16_interval(ref64, ref32, extra=0.0):
    """(lo, hi, tol): the bfloat16 values a kernel that stores bf16 may return, as float64 tensors.
    tol = 16 max|ref32 - ref64| + eps32 max|ref64| (+ extra) is the float32 bar of assert_fp64_parity; lo / hi are the
    bf16 roundings of ref64 -/+ tol."""
    assert ref64.dtype == F64 and ref32.dtype == F32 and tuple(ref64.shape) == tuple(ref32.shape)
    tol = 16.0 * _max_abs(ref32.to(F64) - ref64) + EPS32 * _max_abs(ref64) + float(extra)
    return to_bf16(ref64 - tol).to(F64), to_bf16(ref64 + tol).to(F64), tol


def bf16_determined(lo, hi, tol):
    """Elements at which the interval says as much as the float32 bar does: no bf16 rounding boundary within tol of
    the reference (lo == hi: the kernel's bits are fixed), or bf16 itself finer than the bar there (hi - lo no wider
    than 2 tol rounded outwards: the exact zeros of a ReLU, of a masked gradient, of the pixels no pooling window
    selects).  Elsewhere the interval spans a whole bf16 step, thousands of times tol."""
    return (hi - lo) <= 2 * tol * (1 + 2.0 ** -7)


def assert_bf16_parity(got, ref64, ref32, what="", min_determined=0.9, extra=0.0):
    """A kernel that stores bfloat16: every element must be the bf16 rounding of something within the float32 bar of
    the reference, bf16(ref64 - tol) <= got <= bf16(ref64 + tol) with tol = 16 max|ref32 - ref64| + eps32 max|ref64|.
    ``ref64`` / ``ref32`` are the restatement before its final rounding.  No bf16 tolerance appears: where no rounding
    boundary lies within tol of the reference (lo == hi, "determined") the kernel's bits are fixed; an element where
    bf16 is finer than tol (an exact zero) counts as determined too, see bf16_determined.  The eps32 term
    also covers the float32 step of the float64 -> bfloat16 conversion.  At least ``min_determined`` of the elements
    must be determined, else the check is blind; that is a condition on the inputs, not on the kernel
    (tests/test_kernel_parity_cpu.py shows the restatements meet it).  ``extra`` is added to tol before the interval
    is formed (the documented error of erf_fast under a GELU, as in assert_fp64_parity).  Prints and returns
    err / bar like assert_fp64_parity, with err the largest distance from ref64 at which a value rounds to the
    kernel's bf16 (0 where got == bf16(ref64))."""
    got = torch.as_tensor(got).detach().cpu()
    assert got.dtype == BF16, f"{what}: expected a bfloat16 output, got {got.dtype}"
    assert tuple(got.shape) == tuple(ref64.shape), (what, got.shape, ref64.shape)
    lo, hi, tol = bf16_interval(ref64, ref32, extra)
    det = bf16_determined(lo, hi, tol)
    share = float(det.double().mean()) if det.numel() else 1.0
    assert share >= min_determined, f"{what}: only {share:.1%} of the elements are determined, the check is blind"
    g = got.to(F64)
    assert bool(torch.isfinite(g).all()), f"{what}: non-finite kernel output (or an element never written)"
    # err: how far from ref64 the value the kernel rounded must have been -- 0 where got is bf16(ref64), else the
    # distance from ref64 to the rounding boundary between the two (their midpoint); this is what tol bounds
    r = to_bf16(ref64).to(F64)
    err = _max_abs(torch.where(g != r, (g + r) / 2 - ref64, torch.zeros_like(g)))
    bar = _max_abs(ref32.to(F64) - ref64)
    ratio = err / bar if bar > 0 else (0.0 if err == 0 else math.inf)
    print(f"parity {what}: err={err:.3e} bar={bar:.3e} ratio={ratio:.3f} determined={share:.3f} tol={tol:.3e}")
    bad = (g < lo) | (g > hi)
    if bool(bad.any()):
        i = int(bad.reshape(-1).nonzero()[0])
        at = [float(t.reshape(-1)[i]) for t in (g, lo, hi, ref64)]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bf16 interval; first at "
                             f"flat index {i}: got {at[0]!r}, interval [{at[1]!r}, {at[2]!r}], ref64 {at[3]!r}, "
                             f"tol {tol:.3e}")
    return ratio


# ---- dropout masks restated on the host (tests/helpers.dropout_keep) ----
def keep_mask(base, site, idx, p) -> torch.Tensor:
    """Boolean keep mask of the kernels' dropout_scale at element indices ``idx`` (any shape); all kept at p == 0."""
    idx = np.asarray(idx, dtype=np.uint64)
    if p <= 0:
        return torch.ones(idx.shape, dtype=torch.bool)
    return torch.from_numpy(dropout_keep(int(base), int(site), idx.reshape(-1), f32(p)).reshape(idx.shape))


def drop_scale(keep: torch.Tensor, p, dt) -> torch.Tensor:
    """keep / (1 - p) in dtype dt (the kernels' 1.0f / (1.0f - p))."""
    if p <= 0:
        return keep.to(dt)
    return keep.to(dt) * (torch.ones((), dtype=dt) / (1 - torch.tensor(f32(p), dtype=dt)))


def assert_dropout_parity(got, keep, p, ref64, ref32, extra=0.0, what=""):
    """The kernel's zeros are the mask's, exactly; the kept values meet the parity bar after scaling by 1/(1-p).
    ``ref64`` / ``ref32`` are the dropped-out results (mask and scale applied).  Every dropped element must be an exact
    zero; every kept element must be non-zero unless its reference value is itself indistinguishable from zero under
    the bar's one-ulp floor (gelu(0), gelu(-6) ~ 6e-9), where a zero says nothing about the mask."""
    got = torch.as_tensor(got).detach().cpu()
    live = keep & (ref64.abs() > EPS32 * _max_abs(ref64))
    assert 2 * int(live.sum()) >= int(keep.sum()), f"{what}: too few kept values are non-zero, the mask check is blind"
    assert bool((got[~keep] == 0).all()) and bool((got[live] != 0).all()), \
        f"{what}: the kernel's zeros differ from the restated mask"
    if got.dtype == BF16:  # a bf16 store: a live value is at least eps32 max|ref|, far above the smallest bf16
        return assert_bf16_parity(got, ref64, ref32, extra=extra, what=what)
    return assert_fp64_parity(got, ref64, ref32, extra=extra, what=what)


def keep_mask_pair(base, site, idx, p) -> torch.Tensor:
    """keep_mask for the paired-index dropout of the WavLM encoder's sites (dropout_scale_pair / dropout_pairs: the
    bf16 GEMM epilogues, mer_layernorm_tr, mer_dropout_rows)."""
    idx = np.asarray(idx, dtype=np.uint64)
    if p <= 0:
        return torch.ones(idx.shape, dtype=torch.bool)
    return torch.from_numpy(dropout_keep_pair(int(base), int(site), idx.reshape(-1), f32(p)).reshape(idx.shape))


# ---- sentinels: outputs are views into wider / longer buffers whose every other element must stay untouched ----
MARKER = -12345.6789


class Guarded:
    """A strided fp32 view (shape, element strides, offset) into a flat buffer pre-filled with MARKER."""

    def __init__(self, shape, strides, device, offset=3, tail=5, init=None):
        shape, strides = tuple(int(s) for s in shape), tuple(int(s) for s in strides)
        span = 1 + sum((n - 1) * s for n, s in zip(shape, strides))
        self.buf = torch.full((offset + span + tail,), MARKER, dtype=F32, device=device)
        self.view = self.buf.as_strided(shape, strides, offset)
        idx = torch.zeros(shape, dtype=torch.int64) + offset
        for d, (n, s) in enumerate(zip(shape, strides)):
            sh = [1] * len(shape)
            sh[d] = n
            idx = idx + (torch.arange(n, dtype=torch.int64) * s).reshape(sh)
        self.inside = torch.zeros(self.buf.numel(), dtype=torch.bool)
        self.inside[idx.reshape(-1)] = True
        assert int(self.inside.sum()) == int(np.prod(shape)), "the view overlaps itself"
        assert not bool(self.inside.all()), "no sentinel element: the view covers its whole buffer"
        if init is not None:
            self.view.copy_(init.to(device))

    def check(self, what=""):
        """Every element outside the view is bit-unchanged."""
        bits = self.buf.detach().cpu().view(torch.int32)
        want = torch.full((1,), MARKER, dtype=F32).view(torch.int32)
        bad = (bits != want) & ~self.inside
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements outside the output view were overwritten " \
                                    f"(first at flat index {int(bad.nonzero()[0])})"


def guarded_rows(rows, cols, ld, device, init=None, offset=3):
    """[rows, cols] with row stride ld > cols."""
    assert ld > cols
    return Guarded((rows, cols), (ld, 1), device, offset=offset, init=init)


def guarded_flat(shape, device, init=None, offset=4):
    """A contiguous tensor of ``shape`` with sentinel elements in front of and behind it."""
    strides, s = [], 1
    for n in reversed(shape):
        strides.append(s)
        s *= n
    return Guarded(shape, tuple(reversed(strides)), device, offset=offset, tail=7, init=init)


def padded_input(t, strides, device, offset=0):
    """``t`` as a strided device view whose gaps hold NaN: a kernel that reads with the wrong stride shows it."""
    span = 1 + sum((n - 1) * s for n, s in zip(t.shape, strides))
    buf = torch.full((offset + span + 4,), float("nan"), dtype=F32, device=device)
    view = buf.as_strided(tuple(t.shape), tuple(int(s) for s in strides), offset)
    view.copy_(t.to(device))
    return view


def padded_rows(t, pad, device, offset=0):
    return padded_input(t, (t.shape[1] + pad, 1), device, offset)


class GuardedBf16:
    """A contiguous bfloat16 (or uint8) output of ``shape`` inside a longer flat buffer.  MARKER is not a bf16 value,
    so the buffer is pre-filled with NaN (0xFF bytes for uint8): ``check`` requires every element in front of and
    behind the view to keep its bits and every element of the view to have been written.  The view starts 16 elements
    in, so 16-byte vector stores stay aligned."""

    def __init__(self, shape, device, dtype=BF16, pad=16):
        n = int(np.prod(shape))
        self.fill = 0xFF if dtype == torch.uint8 else float("nan")
        self.buf = torch.full((pad + n + pad,), self.fill, dtype=dtype, device=device)
        self.view = self.buf[pad:pad + n].view(tuple(shape))
        self.pad, self.n = pad, n

    def _untouched(self, t):
        return bool((t == 0xFF).all()) if t.dtype == torch.uint8 else bool(torch.isnan(t).all())

    def check(self, what="", written=True):
        b = self.buf.detach().cpu()
        assert self._untouched(b[:self.pad]) and self._untouched(b[self.pad + self.n:]), \
            f"{what}: elements outside the output view were overwritten"
        v = b[self.pad:self.pad + self.n]
        if written:
            never = (v == 0xFF) if v.dtype == torch.uint8 else torch.isnan(v)
            assert not bool(never.any()), f"{what}: {int(never.sum())} output elements never written"
        if not written:
            assert self._untouched(v), f"{what}: the output was written by a call that must refuse"


class GuardedBf16Rows:
    """A bfloat16 [rows, cols] output with row stride ld > cols inside a NaN-filled buffer, ``offset`` elements in (a
    multiple of 8 keeps 16-byte vector stores aligned; an odd one forces a kernel's scalar path).  ``check`` requires
    every pad element (in front, between the rows, behind) to still be NaN and every view element to have been
    written; ``written=False``: the view too must be untouched (a call that refuses, a skipped layer)."""

    def __init__(self, rows, cols, ld, device, offset=16, tail=16):
        assert ld > cols
        self.rows, self.cols, self.ld, self.offset = int(rows), int(cols), int(ld), int(offset)
        span = (self.rows - 1) * self.ld + self.cols
        self.buf = torch.full((self.offset + span + tail,), float("nan"), dtype=BF16, device=device)
        self.view = self.buf.as_strided((self.rows, self.cols), (self.ld, 1), self.offset)
        self.inside = torch.zeros(self.buf.numel(), dtype=torch.bool)
        idx = self.offset + torch.arange(self.rows)[:, None] * self.ld + torch.arange(self.cols)[None, :]
        self.inside[idx.reshape(-1)] = True

    def check(self, what="", written=True):
        nan = torch.isnan(self.buf.detach().cpu().float())
        bad = ~nan & ~self.inside
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} pad elements outside the output view were overwritten " \
                                    f"(first at flat index {int(bad.nonzero()[0]) if bool(bad.any()) else -1})"
        never = nan & self.inside
        if written:
            assert not bool(never.any()), f"{what}: {int(never.sum())} output elements never written (or NaN)"
        else:
            assert bool(never[self.inside].all()), f"{what}: the output was written by a call that must leave it alone"


def padded_input_bf16(t, ld, device, offset=0):
    """bf16-valued ``t`` [rows, cols] as a bfloat16 device view with row stride ld >= cols whose gaps (and 8 elements
    behind the last row) hold NaN.  ``offset`` elements in front: a multiple of 8 keeps the rows 16-byte aligned."""
    rows, cols = t.shape
    assert ld >= cols
    buf = torch.full((offset + (rows - 1) * ld + cols + 8,), float("nan"), dtype=BF16, device=device)
    view = buf.as_strided((rows, cols), (ld, 1), offset)
    view.copy_(t.to(BF16).to(device))
    assert bool((view.float().cpu() == t.to(F32)).all()), "the input is not bf16-representable"
    return view


def bf16_truncate(t) -> torch.Tensor:
    """float -> bfloat16 by dropping the low 16 bits (the store a kernel must NOT do; the CPU mutation checks)."""
    bits = t.to(F32).contiguous().view(torch.int32) & -65536
    return bits.view(F32).to(BF16)


# ---- seeded CPU inputs ----
def gen(seed):
    return torch.Generator().manual_seed(int(seed))


def randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=F32)


# ======================================================================================================
# Restatements.  Inputs are float32 CPU tensors; each function converts them to ``dt`` and returns a dict.
# ======================================================================================================
def ref_add_ln(x, r, gamma, beta, row_scale, dy, eps, dt):
    """y = LayerNorm(x + s_b r) with its autograd backward.  ``row_scale``: per-row s_b (None with r None)."""
    x = x.to(dt).requires_grad_(True)
    gamma, beta = gamma.to(dt).requires_grad_(True), beta.to(dt).requires_grad_(True)
    if r is not None:
        r = r.to(dt).requires_grad_(True)
        s = x + row_scale.to(dt)[:, None] * r
    else:
        s = x + 0
    mean = s.mean(1)
    var = ((s - mean[:, None]) ** 2).mean(1)
    rstd = 1 / torch.sqrt(var + torch.tensor(f32(eps), dtype=dt))
    y = (s - mean[:, None]) * rstd[:, None] * gamma + beta
    leaves = [x, gamma, beta] + ([r] if r is not None else [])
    grads = torch.autograd.grad(y, leaves, dy.to(dt))
    out = {"y": y, "s": s, "mean": mean, "rstd": rstd, "dx": grads[0], "dgamma": grads[1], "dbeta": grads[2]}
    if r is not None:
        out["dr"] = grads[3]
    return {k: v.detach() for k, v in out.items()}


def ref_mean_pool(x, dy, dx0, dt):
    L = x.shape[1]
    dx = (dy.to(dt) / L)[:, None, :].expand(x.shape)
    return {"y": x.to(dt).sum(1) / L, "dx": dx + (dx0.to(dt) if dx0 is not None else 0)}


def ref_attn_pool(x, scores, dy, dx0, dt):
    x, dy = x.to(dt), dy.to(dt)
    attn = torch.softmax(scores.to(dt), -1)
    y = torch.einsum("bl,bld->bd", attn, x)
    g = torch.einsum("bd,bld->bl", dy, x)
    ds = attn * (g - (attn * g).sum(-1, keepdim=True))
    dx = attn[:, :, None] * dy[:, None, :]
    return {"attn": attn, "y": y, "dscores": ds, "dx": dx + (dx0.to(dt) if dx0 is not None else 0)}


def ref_gelu_dropout(z, dy, keep, p, dt):
    z, sc = z.to(dt), drop_scale(keep, p, dt)
    cdf = 0.5 * (1 + torch.erf(z * (0.5 ** 0.5)))
    pdf = torch.exp(-0.5 * z * z) * (1 / math.sqrt(2 * math.pi))
    return {"y": z * cdf * sc, "dz": dy.to(dt) * sc * (cdf + z * pdf)}


def ref_add_dropout(x, r, r_period, keep, p, dt):
    rows = x.shape[0]
    rr = r.to(dt)[torch.arange(rows) % r_period]
    return {"y": x.to(dt) + rr * drop_scale(keep, p, dt)}


def ref_dropout(x, keep, p, dt):
    return {"y": x.to(dt) * drop_scale(keep, p, dt)}


def ref_relu_dropout_bwd(dy, y, keep, p, dt):
    return {"dz": torch.where(y > 0, dy.to(dt) * drop_scale(keep, p, dt), torch.zeros((), dtype=dt))}


def ref_softmax_dropout(S, scale, dPp, keep, p, dt):
    """P = softmax(scale S); Pd = P m; dS = P (dPp m - sum_j P dPp m) with m the scaled keep mask."""
    m = drop_scale(keep, p, dt)
    P = torch.softmax(S.to(dt) * torch.tensor(f32(scale), dtype=dt), -1)
    t = dPp.to(dt) * m
    return {"P": P, "Pd": P * m, "dS": P * (t - (P * t).sum(-1, keepdim=True))}


def ref_gate_mix(z, v, a, dout, dv0, da0, dt):
    z, v, a, dout = z.to(dt), v.to(dt), a.to(dt), dout.to(dt)
    g = torch.sigmoid(z)[:, None]
    return {"g": g[:, 0], "out": g * v + (1 - g) * a, "dz": ((dout * (v - a)).sum(1, keepdim=True) * g * (1 - g))[:, 0],
            "dv": dv0.to(dt) + g * dout, "da": da0.to(dt) + (1 - g) * dout}


def ref_token_bias(qt, qp, kt, kp, scale, dbias, dt):
    qt, qp, kt, kp, scale, dbias = (t.to(dt) for t in (qt, qp, kt, kp, scale, dbias))
    th = torch.tanh(qt[:, :, None] + kt[:, None, :] + (qp + kp)[:, None, None])
    g = dbias * scale * (1 - th * th)
    tot = g.sum((1, 2))
    return {"out": th * scale, "dqt": g.sum(2), "dkt": g.sum(1), "dqp": tot, "dkp": tot,
            "dscale_part": (dbias * th).sum((1, 2))}


def ref_softmax_avg(za, zv, dout, dt):
    pa, pv, g = torch.softmax(za.to(dt), -1), torch.softmax(zv.to(dt), -1), dout.to(dt)
    return {"pa": pa, "pv": pv, "out": 0.5 * (pa + pv), "da": 0.5 * pa * (g - (pa * g).sum(-1, keepdim=True)),
            "dv": 0.5 * pv * (g - (pv * g).sum(-1, keepdim=True))}


def ref_vec_sum(x, out0, dt):
    return {"out": (x.to(dt).sum() + (out0.to(dt) if out0 is not None else 0)).reshape(1)}


def ref_scale_dev(x, s, dt):
    return {"y": x.to(dt) * s.to(dt)}


def ref_adam(p, g, m, v, lr, b1, b2, eps, wd, step, grad_scale, dt):
    """One step of the recurrence documented above adam_kernel (csrc/head.hip); hyper-parameters as C floats."""
    p, g, m, v = (t.to(dt) for t in (p, g, m, v))
    lr, b1, b2, eps, wd, gs = (torch.tensor(f32(t), dtype=dt) for t in (lr, b1, b2, eps, wd, grad_scale))
    st = torch.tensor(float(step), dtype=dt)
    bc1, bc2 = 1 - b1 ** st, 1 - b2 ** st
    gr = gs * g + wd * p
    m = b1 * m + (1 - b1) * gr
    v = b2 * v + (1 - b2) * gr * gr
    p = p - (lr / bc1) * m / (torch.sqrt(v) / torch.sqrt(bc2) + eps)
    return {"p": p, "m": m, "v": v}


def _gelu(z):
    return 0.5 * z * (1 + torch.erf(z * (0.5 ** 0.5)))


def ref_gemm(a, b, bias, c0, beta, act, dt):
    """out = act(a @ b + bias + beta c0) over the last two dims (the epilogue order of gemm_f32_kernel);
    also the pre-activation z."""
    z = a.to(dt) @ b.to(dt)
    if bias is not None:
        z = z + bias.to(dt)
    if beta:
        z = z + c0.to(dt)
    out = torch.relu(z) if act == "relu" else (_gelu(z) if act == "gelu" else z)
    return {"out": out, "z": z}


def ref_clip_align(a, v, log_scale, dloss, dls0, dt):
    """The formula of the header comment of csrc/align.hip, with autograd."""
    a, v = a.to(dt).requires_grad_(True), v.to(dt).requires_grad_(True)
    ls = log_scale.to(dt).reshape(()).requires_grad_(True)
    B = a.shape[0]
    na = a.norm(dim=-1).clamp_min(1e-12)
    nv = v.norm(dim=-1).clamp_min(1e-12)
    an, vn = a / na[:, None], v / nv[:, None]
    s = torch.exp(ls).clamp(max=100.0)
    logits = s * (an @ vn.t())
    tgt = torch.arange(B)
    loss = 0.5 * (torch.nn.functional.cross_entropy(logits, tgt) + torch.nn.functional.cross_entropy(logits.t(), tgt))
    da, dv, dls = torch.autograd.grad(loss, [a, v, ls], dloss.to(dt).reshape(()), allow_unused=True)
    dls = torch.zeros((), dtype=dt) if dls is None else dls
    out = {"an": an, "vn": vn, "norms": torch.cat([na, nv]), "logits": logits, "loss": loss.reshape(1), "da": da,
           "dv": dv, "dlog_scale": (dls0.to(dt).reshape(()) + dls).reshape(1)}
    return {k: t.detach() for k, t in out.items()}


# ---- csrc/bn_pool.hip: BatchNorm and pooling of the video trunk (channel-last, bf16 activations) ----
def bf16_values(g, *shape, scale=1.0, shift=0.0):
    """Seeded float32 values that are exactly representable in bfloat16 (the kernels' inputs, widened)."""
    return to_bf16(randn(g, *shape) * scale + shift).to(F32)


def tile_stats(x):
    """Conv-epilogue statistics rows of a bf16-valued x[M, C]: per 64-row tile (sum, sum of squares), accumulated in
    float64 and rounded to float32 -> [ceil(M / 64), C, 2]."""
    M, C = x.shape
    rows = (M + 63) // 64
    xp = torch.zeros(rows * 64, C, dtype=F64)
    xp[:M] = x.to(F64)
    xp = xp.view(rows, 64, C)
    return torch.stack([xp.sum(1), (xp * xp).sum(1)], -1).to(F32)


def ref_bn_finalize(stats, M, eps, momentum, rmean, rvar, dt):
    """Train form: ``stats`` [rows, C, 2] partial (sum, sumsq) rows -> mean, rstd = 1 / sqrt(max(var, 0) + eps), and
    the running statistics with the unbiased variance M / (M - 1) (factor 1 at M = 1).  Eval form (``stats`` None):
    the running statistics copied / inverted, nothing updated.  num_batches_tracked (+1 in the train form) is an
    integer and is asserted by the caller."""
    eps_t, mom = torch.tensor(f32(eps), dtype=dt), torch.tensor(f32(momentum), dtype=dt)
    if stats is None:
        return {"mean": rmean.to(dt).clone(), "rstd": 1 / torch.sqrt(rvar.to(dt) + eps_t)}
    tot = stats.to(dt).sum(0)
    Mt = torch.tensor(float(M), dtype=dt)
    mean = tot[:, 0] / Mt
    var = torch.clamp(tot[:, 1] / Mt - mean * mean, min=0)
    out = {"mean": mean, "rstd": 1 / torch.sqrt(var + eps_t)}
    if rmean is not None:
        out["rmean"] = (1 - mom) * rmean.to(dt) + mom * mean
    if rvar is not None:
        unbias = Mt / torch.tensor(float(M - 1 if M > 1 else 1), dtype=dt)
        out["rvar"] = (1 - mom) * rvar.to(dt) + mom * var * unbias
    return out


def _bn_fold(ms, gamma, beta, dt):
    """BatchNorm as one (scale, shift) per channel, the form the kernels document: scale = rstd gamma,
    shift = beta - mean scale."""
    ms = ms.to(dt)
    scale = ms[:, 1] * gamma.to(dt)
    return scale, beta.to(dt) - ms[:, 0] * scale


def ref_bn_apply(x, ms, gamma, beta, relu, dt, res=None, ms2=None, gamma2=None, beta2=None):
    """y = [relu](bn(x) + r) before its bf16 rounding; r: nothing, the raw residual, or bn2(res)."""
    scale, shift = _bn_fold(ms, gamma, beta, dt)
    y = x.to(dt) * scale + shift
    if res is not None:
        if ms2 is not None:
            scale2, shift2 = _bn_fold(ms2, gamma2, beta2, dt)
            y = y + (res.to(dt) * scale2 + shift2)
        else:
            y = y + res.to(dt)
    return {"y": torch.relu(y) if relu else y}


def ref_bn_bwd(dy, mask, x, ms, gamma, batch_stats, dt, red=None, dgamma0=None, dbeta0=None):
    """g = dy (mask > 0); red = (sum g, sum g xhat); dx = gamma rstd (g - sum g / M - xhat sum g xhat / M) with batch
    statistics, gamma rstd g without; dgamma / dbeta accumulate onto their start values.  ``red`` given: dx, dgamma
    and dbeta use it instead of the sums (the apply kernel judged alone)."""
    C, shape = x.shape[-1], x.shape
    dy, x, ms = dy.to(dt).reshape(-1, C), x.to(dt).reshape(-1, C), ms.to(dt)
    M = x.shape[0]
    g = dy if mask is None else torch.where(mask.reshape(-1, C) > 0, dy, torch.zeros((), dtype=dt))
    mean, rstd = ms[:, 0], ms[:, 1]
    xhat = (x - mean) * rstd
    sums = torch.stack([g.sum(0), (g * xhat).sum(0)], -1)
    use = sums if red is None else red.to(dt)
    k = gamma.to(dt) * rstd
    dx = k * (g - use[:, 0] / M - xhat * (use[:, 1] / M)) if batch_stats else k * g
    zero = torch.zeros(C, dtype=dt)
    return {"red": sums, "dx": dx.reshape(shape), "dgamma": (zero if dgamma0 is None else dgamma0.to(dt)) + use[:, 1],
            "dbeta": (zero if dbeta0 is None else dbeta0.to(dt)) + use[:, 0]}


def maxpool_out(n):
    return (n + 2 - 3) // 2 + 1


def maxpool_taps(xp, Ho, Wo):
    """3x3 / stride-2 max over an already padded [N, >= 2 Ho + 1, >= 2 Wo + 1, C] tensor (-inf outside the frame):
    nine shifted comparisons in tap order t = 3 r + s, a later tap wins only when strictly greater -- the argmax is
    the FIRST maximum (0 when every tap is -inf)."""
    best = torch.full((xp.shape[0], Ho, Wo, xp.shape[3]), -math.inf, dtype=xp.dtype)
    arg = torch.zeros(best.shape, dtype=torch.uint8)
    for t in range(9):
        r, s = divmod(t, 3)
        v = xp[:, r:r + 2 * Ho - 1:2, s:s + 2 * Wo - 1:2]
        up = v > best
        best = torch.where(up, v, best)
        arg = torch.where(up, torch.full((), t, dtype=torch.uint8), arg)
    return best, arg


def ref_maxpool(x, dy, dt, arg=None):
    """MaxPool2d(3, 2, 1) on [N, H, W, C]: y, the argmax tap, and dx = dy gathered through the argmax (``arg`` given:
    through that one; a tap that points outside the frame receives nothing)."""
    N, H, W, C = x.shape
    Ho, Wo = maxpool_out(H), maxpool_out(W)
    xp = torch.full((N, H + 2, W + 2, C), -math.inf, dtype=dt)
    xp[:, 1:H + 1, 1:W + 1] = x.to(dt)
    y, amax = maxpool_taps(xp, Ho, Wo)
    out = {"y": y, "arg": amax.to(dt)}
    if dy is not None:
        out["dx"] = maxpool_gather(dy, amax if arg is None else arg, H, W, dt)
    return out


def maxpool_gather(dy, arg, H, W, dt):
    N, Ho, Wo, C = dy.shape
    dxp = torch.zeros(N, H + 2, W + 2, C, dtype=dt)
    dy = dy.to(dt)
    for t in range(9):
        r, s = divmod(t, 3)
        dxp[:, r:r + 2 * Ho - 1:2, s:s + 2 * Wo - 1:2] += torch.where(arg == t, dy, torch.zeros((), dtype=dt))
    return dxp[:, 1:H + 1, 1:W + 1].contiguous()


def ref_avgpool(x, dy, dt):
    """Global average pool [N, H, W, C] -> [N, C] and its backward dx = dy / HW (before the bf16 rounding)."""
    N, H, W, C = x.shape
    HW = H * W
    return {"y": x.to(dt).sum((1, 2)) / HW, "dx": (dy.to(dt) / HW)[:, None, None, :].expand(N, H, W, C).contiguous()}


def ref_rows_sum(rows, out0, dt):
    """out = out0 + sum over the leading dimension (the partial-row folds)."""
    tot = rows.to(dt).sum(0)
    return {"out": tot if out0 is None else out0.to(dt) + tot}


# ---- csrc/gemm_bf16.hip: the bf16 MFMA GEMM, its Conv1d 'rows' mode and the grouped positional conv ----
def _act(z, act):
    return torch.relu(z) if act == "relu" else (_gelu(z) if act == "gelu" else z)


def gather_rows(buf, M, K, rpg, rstride, gstride):
    """The A operand of rows mode: row m = buf[(m // rpg) * gstride + (m % rpg) * rstride : + K] of the flat buffer."""
    m = torch.arange(M)
    start = (m // rpg) * gstride + (m % rpg) * rstride
    return buf.reshape(-1)[start[:, None] + torch.arange(K)[None, :]]


def ref_gemm_bf16(a, w, bias, res, act, keep, p, dt):
    """z = a w^T (+ bias); y = act(z); y *= keep / (1 - p) when p > 0; y += res -- the epilogue order of
    csrc/gemm_bf16.hip (dropout after the activation, before the residual), before any final rounding."""
    z = a.to(dt) @ w.to(dt).t()
    if bias is not None:
        z = z + bias.to(dt)
    y = _act(z, act)
    if p > 0:
        y = y * drop_scale(keep, p, dt)
    if res is not None:
        y = y + res.to(dt)
    return {"out": y, "z": z}


def ref_posconv(x, wp, bias, res, act, B, L, C, G, taps, pad, dt):
    """Grouped positional conv as the direct sum out[b, t, g cg + n] = act(sum_{tap, c} x[b, t + tap - pad, g cg + c]
    wp[g, n, tap, c] + bias) + res with x zero outside [0, L); x [B, L, C], wp [G, cg, taps, cg]."""
    cg = C // G
    xp = torch.zeros(B, L + taps, G, cg, dtype=dt)
    xp[:, pad:pad + L] = x.to(dt).reshape(B, L, G, cg)
    wp = wp.to(dt).reshape(G, cg, taps, cg)
    z = torch.zeros(B, L, G, cg, dtype=dt)
    for tap in range(taps):
        z = z + torch.einsum("blgc,gnc->blgn", xp[:, tap:tap + L], wp[:, :, tap, :])
    z = z.reshape(B, L, C)
    if bias is not None:
        z = z + bias.to(dt)
    y = _act(z, act)
    if res is not None:
        y = y + res.to(dt)
    return {"out": y, "z": z}


# ---- row kernels of the WavLM encoder and its stage-2 backward (csrc/wavlm.hip, csrc/wavlm_train.hip) ----
def ref_layernorm(x, gamma, beta, eps, keep, p, dt):
    """Row LayerNorm with optional dropout on its output."""
    x = x.to(dt)
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    y = (x - mean) / torch.sqrt(var + torch.tensor(f32(eps), dtype=dt)) * gamma.to(dt) + beta.to(dt)
    return {"y": y * drop_scale(keep, p, dt) if p > 0 else y}


LN_BWD_ROWS = 16  # csrc/wavlm_train.hip LN_ROWS: rows per block = rows per partial row


def ref_ln_bwd(dys, x, gamma, eps, dt, block0=0):
    """LayerNorm backward of g = sum(dys) on the saved input x: dx = rstd (g gamma - mean(g gamma) - xhat mean(g gamma
    xhat)), and per block of 16 rows the partial rows part[blk] = (sum g xhat, sum g, sum dx) -> [nblk, 3, d].
    ``block0`` shifts the blocks' first row (the CPU mutation check only)."""
    x, gamma = x.to(dt), gamma.to(dt)
    g = sum(t.to(dt) for t in dys)
    mean = x.mean(1, keepdim=True)
    rstd = 1 / torch.sqrt(((x - mean) ** 2).mean(1, keepdim=True) + torch.tensor(f32(eps), dtype=dt))
    xh = (x - mean) * rstd
    gg = g * gamma
    dx = rstd * (gg - gg.mean(1, keepdim=True) - xh * (gg * xh).mean(1, keepdim=True))
    rows = x.shape[0]
    parts = []
    for r0 in range(0, rows, LN_BWD_ROWS):
        sl = slice(max(r0 + block0, 0), max(min(r0 + LN_BWD_ROWS, rows) + block0, 0))
        parts.append(torch.stack([(g[sl] * xh[sl]).sum(0), g[sl].sum(0), dx[sl].sum(0)]))
    return {"dx": dx, "part": torch.stack(parts)}


def ref_fold_rows(part, out0, dt):
    """out0 + sum_p part[p]."""
    return {"out": out0.to(dt) + part.to(dt).sum(0)}


def ref_colsum(x, out0, dt):
    return {"out": out0.to(dt) + x.to(dt).sum(0)}


def _gelu_grad(z):
    return 0.5 * (1 + torch.erf(z * (0.5 ** 0.5))) + z * torch.exp(-0.5 * z * z) * (1 / math.sqrt(2 * math.pi))


def ref_gelu(z, dt):
    return {"f": _gelu(z.to(dt))}


def ref_gelu_bwd(df, z, dbias0, dt):
    """dz = df gelu'(z) before its bf16 rounding; dbias = dbias0 + column sums of the unrounded dz."""
    dz = df.to(dt) * _gelu_grad(z.to(dt))
    return {"dz": dz, "dbias": dbias0.to(dt) + dz.sum(0)}


def ref_dropout_rows(x, keep, p, dt):
    return {"y": x.to(dt) * drop_scale(keep, p, dt)}


def ref_linear_wgrad(x, dy, dw0, col0, N, dt):
    """dw0 + dy[:, col0:col0 + N]^T x."""
    return {"dw": dw0.to(dt) + dy.to(dt)[:, col0:col0 + N].t() @ x.to(dt)}


def ref_weightnorm_scale(v, g, dt):
    """g[k] / ||v[:, :, k]||_2."""
    v = v.to(dt)
    return {"scale": g.to(dt) / torch.sqrt((v * v).sum((0, 1)))}


# ---- csrc/conv.hip, csrc/conv_wgrad.hip, csrc/conv_pack.hip: the trunk convolutions (NHWC bf16, fp32 accumulate) ----
def conv_out(n, R, stride, pad):
    return (n + 2 * pad - R) // stride + 1


def ref_conv_fwd(x, w, stride, pad, dt, tap_scale=None, shift=0):
    """y[n, oh, ow, k] = sum_{r, s, c} x[n, oh st - pad + r, ow st - pad + s, c] w[k, c, r, s] (include/mer.h) as a
    direct sum over taps on an explicitly zero-padded x: one shifted strided slice and one matmul per tap, taps in
    (r, s) order.  x [N, H, W, C], w [K, C, R, S] (the bf16 rounding of the fp32 weight: what the pack stores).
    ``tap_scale(r, s)`` (None, or a tensor broadcastable to [N, Ho, Wo, 1] the tap's term is multiplied by) and
    ``shift`` (the frame placed ``shift`` pixels off its place inside the padding) exist for the CPU mutation
    checks only."""
    N, H, W, C = x.shape
    Kc, _, R, S = w.shape
    Ho, Wo = conv_out(H, R, stride, pad), conv_out(W, S, stride, pad)
    xp = torch.zeros(N, H + 2 * pad + 2, W + 2 * pad + 2, C, dtype=dt)  # one spare pixel around the padding
    xp[:, pad + 1 + shift:pad + 1 + shift + H, pad + 1 + shift:pad + 1 + shift + W] = x.to(dt)
    w = w.to(dt)
    y = torch.zeros(N, Ho, Wo, Kc, dtype=dt)
    for r in range(R):
        for s in range(S):
            v = xp[:, r + 1:r + 1 + stride * (Ho - 1) + 1:stride, s + 1:s + 1 + stride * (Wo - 1) + 1:stride]
            term = v @ w[:, :, r, s].t()
            sc = tap_scale(r, s) if tap_scale is not None else None
            y = y + (term if sc is None else term * sc.to(dt))
    return {"y": y}


def ref_conv_dgrad(dy, w, H, W, stride, pad, dt, residual=None, mask=None, ds=None, mask_ge=False):
    """dx[n, h, w, c] = sum_{r, s, k} dy[n, (h + pad - r) / st, (w + pad - s) / st, k] w[k, c, r, s]: a scatter per tap
    into a zero-padded dx, then the crop.  ``ds`` = (ds_dy [N, Ho, Wo, Kd], wd [Kd, C, 1, 1]): the input gradient of a
    1x1 / stride-2 / pad-0 downsample of the same input, into pixels (2i, 2j) of the same accumulator before any
    rounding.  Then + residual: everywhere when ``mask`` is None, else only where mask > 0 (+0.0, -0.0 and negative
    values add nothing).  ``mask_ge``: mask >= 0 instead (the CPU mutation check only)."""
    N, Ho, Wo, Kc = dy.shape
    _, C, R, S = w.shape
    assert (Ho, Wo) == (conv_out(H, R, stride, pad), conv_out(W, S, stride, pad))
    dxp = torch.zeros(N, H + 2 * pad, W + 2 * pad, C, dtype=dt)
    dy, w = dy.to(dt), w.to(dt)
    for r in range(R):
        for s in range(S):
            dxp[:, r:r + stride * (Ho - 1) + 1:stride, s:s + stride * (Wo - 1) + 1:stride] += dy @ w[:, :, r, s]
    if ds is not None:
        ds_dy, wd = ds
        assert tuple(ds_dy.shape[:3]) == (N, Ho, Wo) and stride == 2
        dxp[:, pad:pad + 2 * (Ho - 1) + 1:2, pad:pad + 2 * (Wo - 1) + 1:2] += ds_dy.to(dt) @ wd.to(dt)[:, :, 0, 0]
    dx = dxp[:, pad:pad + H, pad:pad + W].contiguous()
    if residual is not None:
        res = residual.to(dt)
        if mask is not None:
            res = torch.where((mask >= 0) if mask_ge else (mask > 0), res, torch.zeros((), dtype=dt))
        dx = dx + res
    return {"dx": dx}


def wgrad_split_pixels(P, splits):
    """Pixels per split of conv_wgrad.hip's plan: ceil(P / splits) rounded up to whole 64-pixel granules."""
    return ((P + splits - 1) // splits + 63) // 64 * 64


def ref_conv_wgrad(x, dy, R, S, stride, pad, creal, dw0, dt, splits=1, chunk=32, c0=0, drop_tail=False):
    """dw0 + dw[k, c, r, s], dw = sum_p dy[p, k] x(p; r, s, c) for c < creal, in the order conv_wgrad.hip documents:
    every split (whole 64-pixel granules, wgrad_split_pixels) accumulated sequentially in ``chunk``-pixel pieces (one
    MFMA covers 32 pixels), the splits added in order, the total added to dw0.  In float64 the grouping changes
    nothing; in float32 it makes the bar grow with the chain length the way any fp32 chain does.  ``c0`` (the creal
    channels read from channel c0 on) and ``drop_tail`` (the last, partial granule of every split dropped) exist for
    the CPU mutation checks only."""
    N, H, W, C = x.shape
    _, Ho, Wo, Kc = dy.shape
    assert (Ho, Wo) == (conv_out(H, R, stride, pad), conv_out(W, S, stride, pad))
    xp = torch.zeros(N, H + 2 * pad, W + 2 * pad, C, dtype=dt)
    xp[:, pad:pad + H, pad:pad + W] = x.to(dt)
    P = N * Ho * Wo
    cols = [xp[:, r:r + stride * (Ho - 1) + 1:stride, s:s + stride * (Wo - 1) + 1:stride, c0:c0 + creal]
            .reshape(P, creal) for r in range(R) for s in range(S)]
    a = torch.stack(cols, 1).reshape(P, R * S * creal)  # [P][(r, s)][c]
    dyt = dy.to(dt).reshape(P, Kc).t().contiguous()
    per = wgrad_split_pixels(P, splits)
    total = None
    for beg in range(0, P, per):
        end = min(P, beg + per)
        if drop_tail and (end - beg) % 64:
            end -= (end - beg) % 64
        acc = torch.zeros(Kc, R * S * creal, dtype=dt)
        for p0 in range(beg, end, chunk):
            p1 = min(end, p0 + chunk)
            acc = acc + dyt[:, p0:p1] @ a[p0:p1]
        total = acc if total is None else total + acc
    dw = total.reshape(Kc, R, S, creal).permute(0, 3, 1, 2)
    return {"dw": dw0.to(dt) + dw}


def ref_conv_sums(y_stored, dt):
    """Forward BatchNorm statistics as include/mer.h defines them: per channel (sum, sum of squares) of the STORED
    bf16 outputs (the kernel's own y, widened) -> [C, 2]."""
    y = y_stored.to(dt).reshape(-1, y_stored.shape[-1])
    return {"stats": torch.stack([y.sum(0), (y * y).sum(0)], -1)}


def ref_bnr_sums(dx_stored, mask, x, ms, dt):
    """The dgrad's fused BN-backward sums (mer_conv_dgrad_bnr): g = the STORED bf16 dx where mask > 0, else 0;
    (sum g, sum g (x - mean) rstd) per channel with (mean, rstd) = ms[c] -> [C, 2]."""
    C = dx_stored.shape[-1]
    dx, x, ms = dx_stored.to(dt).reshape(-1, C), x.to(dt).reshape(-1, C), ms.to(dt)
    g = torch.where(mask.reshape(-1, C) > 0, dx, torch.zeros((), dtype=dt))
    return {"red": torch.stack([g.sum(0), (g * (x - ms[:, 0]) * ms[:, 1]).sum(0)], -1)}


def ref_pack_conv_weight(w, cp, mode):
    """The exact bf16 tensor of each weight layout of csrc/conv_pack.hip from the fp32 weight [K, C, R, S]:
    mode 0 [K][R][S][Cp]; mode 1 (and 3, the same values) [Cp][R][S][K]; mode 2 the space-to-depth stem layout
    [K][(R+2)/2][(S+2)/2][Cp] with out[k, ry, rx, (dy 2 + dx) C + c] = w[k, c, 2 ry + dy - 1, 2 rx + dx - 1] (zero
    where that tap is outside the filter).  Channels >= C (mode 2: >= 4 C) are zero."""
    Kc, C, R, S = w.shape
    wb = to_bf16(w)
    if mode == 0:
        out = torch.zeros(Kc, R, S, cp, dtype=BF16)
        out[..., :C] = wb.permute(0, 2, 3, 1)
    elif mode in (1, 3):
        out = torch.zeros(cp, R, S, Kc, dtype=BF16)
        out[:C] = wb.permute(1, 2, 3, 0)
    else:
        Ro, So = (R + 2) // 2, (S + 2) // 2
        out = torch.zeros(Kc, Ro, So, cp, dtype=BF16)
        for ry in range(Ro):
            for rx in range(So):
                for d in range(4):
                    r, s = 2 * ry + (d >> 1) - 1, 2 * rx + (d & 1) - 1
                    if 0 <= r < R and 0 <= s < S:
                        out[:, ry, rx, d * C:(d + 1) * C] = wb[:, :, r, s]
    return out


def ref_pack_input_s2d(x):
    """fp32 NCHW frames [N, C <= 4, H, W] (H, W even) -> the exact bf16 [N][H/2+3][W/2+3][16] of mer_pack_input_s2d:
    pixel (j, i) holds the 2x2 block (j - 2, i - 2) of the frame, channel (dy 2 + dx) C + c; two leading and one
    trailing border rows / columns and the channels >= 4 C are zero."""
    N, C, H, W = x.shape
    out = torch.zeros(N, H // 2 + 3, W // 2 + 3, 16, dtype=BF16)
    xb = to_bf16(x)
    for d in range(4):
        out[:, 2:2 + H // 2, 2:2 + W // 2, d * C:(d + 1) * C] = xb[:, :, (d >> 1)::2, (d & 1)::2].permute(0, 2, 3, 1)
    return out


SUBNORMAL_BF16 = float(torch.tensor([1], dtype=torch.int16).view(BF16)[0])  # 2^-133: the smallest positive bf16


def conv_inputs(N, H, W, C, Kc, R, stride, pad, seed=None, ds_k=0):
    """Seeded inputs of one convolution shape, all bf16-valued float32 CPU tensors but the fp32 weight ``w32`` (the
    packs round it; ``w`` is that rounding): unit-normal x / dy / residual / BN inputs, weights scaled by
    1 / sqrt(R S C), a unit-normal mask whose first elements are +0.0, -0.0, a negative value and the smallest
    positive bf16, BatchNorm (mean, rstd) pairs, and with ``ds_k`` the fused downsample's dy and weight."""
    if seed is None:  # a polynomial of the shape: the same inputs under every interpreter
        seed = 0
        for v in (N, H, W, C, Kc, R, stride, pad):
            seed = (seed * 1009 + v) % 2147483647
    g = gen(seed)
    Ho, Wo = conv_out(H, R, stride, pad), conv_out(W, R, stride, pad)
    w32 = randn(g, Kc, C, R, R) / math.sqrt(R * R * C)
    i = {"x": bf16_values(g, N, H, W, C), "w32": w32, "w": to_bf16(w32).to(F32), "dy": bf16_values(g, N, Ho, Wo, Kc),
         "res": bf16_values(g, N, H, W, C), "mask": bf16_values(g, N, H, W, C), "xb": bf16_values(g, N, H, W, C),
         "xb2": bf16_values(g, N, H, W, C),
         "ms": torch.stack([randn(g, C), torch.rand(C, generator=g) + 0.5], 1).contiguous(),
         "ms2": torch.stack([randn(g, C), torch.rand(C, generator=g) + 0.5], 1).contiguous()}
    flat = i["mask"].reshape(-1)
    for j, v in enumerate((0.0, -0.0, -1.0, SUBNORMAL_BF16)):
        flat[j * 3 % flat.numel()] = v
    if ds_k:
        wd32 = randn(g, ds_k, C, 1, 1) / math.sqrt(C)
        i.update(ds_dy=bf16_values(g, N, Ho, Wo, ds_k), wd32=wd32, wd=to_bf16(wd32).to(F32))
    return i


# Every (N, H, W, C, Kc, R, stride, pad) tests/test_conv_kernels_gpu.py runs forward and as an input gradient
# (dx [N, H, W, C] from dy [N, Ho, Wo, Kc]); tests/test_kernel_parity_cpu.py shows the restatements leave at least 90 %
# of every one of their bf16 outputs determined.  What each shape is there for is said at the GPU test's case lists.
CONV_SHAPES = [
    (2, 7, 7, 64, 64, 3, 1, 1), (3, 9, 9, 128, 192, 3, 1, 1), (2, 9, 9, 64, 128, 3, 2, 1), (2, 8, 8, 64, 128, 1, 2, 0),
    (2, 12, 12, 64, 64, 3, 1, 1), (3, 17, 17, 16, 24, 3, 1, 1), (2, 30, 30, 8, 64, 7, 2, 3),
    (2, 6, 9, 64, 64, 3, 1, 1), (2, 9, 6, 64, 128, 3, 2, 1), (1, 5, 13, 64, 64, 3, 1, 1), (2, 7, 7, 64, 136, 3, 1, 1),
    (2, 7, 7, 136, 64, 3, 1, 1), (5, 3, 28, 64, 64, 3, 1, 1), (300, 3, 28, 64, 64, 3, 1, 1),
    (800, 3, 28, 64, 64, 3, 1, 1), (2, 8, 8, 256, 64, 1, 1, 0), (2, 8, 8, 128, 256, 3, 2, 1),
    (1, 7, 7, 64, 64, 3, 3, 1)]
CONV_FWD_ONLY = [(2, 7, 7, 64, 20, 3, 1, 1), (4, 56, 56, 64, 512, 3, 1, 1)]
CONV_DGRAD_ONLY = [(4, 56, 56, 512, 64, 3, 1, 1), (4, 56, 56, 512, 64, 3, 2, 1), (1, 12, 12, 8, 64, 11, 2, 5)]
CONV_FORMS = ("plain", "res", "res_mask", "ds")


class ConvCase:
    """The seeded inputs of one shape and its restated outputs (float64, float32), each computed once on demand and
    then shared: "fwd", and the input-gradient forms "plain", "res" (+ residual), "res_mask" (+ residual where
    mask > 0) and "ds" ("res_mask" with the fused 1x1 / stride-2 downsample gradient; 3x3 / stride-2 / pad-1 shapes
    with Kc a multiple of 64 only)."""

    def __init__(self, shape):
        self.shape = tuple(shape)
        N, H, W, C, Kc, R, stride, pad = self.shape
        self.has_ds = R == 3 and stride == 2 and pad == 1 and Kc % 64 == 0
        self.i = conv_inputs(*self.shape, ds_k=64 if self.has_ds else 0)
        self._refs = {}

    def ref(self, form):
        if form not in self._refs:
            N, H, W, C, Kc, R, stride, pad = self.shape
            i = self.i

            def run(dt):
                if form == "fwd":
                    return ref_conv_fwd(i["x"], i["w"], stride, pad, dt)["y"]
                res = None if form == "plain" else i["res"]
                mask = i["mask"] if form in ("res_mask", "ds") else None
                ds = (i["ds_dy"], i["wd"]) if form == "ds" else None
                return ref_conv_dgrad(i["dy"], i["w"], H, W, stride, pad, dt, res, mask, ds)["dx"]
            self._refs[form] = (run(F64), run(F32))
        return self._refs[form]


_CONV_CASES = {}


def conv_case(shape) -> ConvCase:
    shape = tuple(shape)
    if shape not in _CONV_CASES:
        _CONV_CASES[shape] = ConvCase(shape)
    return _CONV_CASES[shape]


def stem_case(N=3, Hf=112, Kc=64, seed=20261206):
    """The stem off its benchmark batch: fp32 frames [N, 3, Hf, Hf], the 7x7 weight, and the restated output of the
    original 7x7 / stride-2 / pad-3 convolution of the bf16-rounded frames -- what mer_pack_input_s2d, the mode-2
    weight pack and the 4x4 / stride-1 / pad-0 convolution of their outputs must reproduce."""
    key = ("stem", N, Hf, Kc, seed)
    if key not in _CONV_CASES:
        g = gen(seed)
        frames = randn(g, N, 3, Hf, Hf)
        w32 = randn(g, Kc, 3, 7, 7) / math.sqrt(147.0)
        x = to_bf16(frames).to(F32).permute(0, 2, 3, 1).contiguous()
        w = to_bf16(w32).to(F32)
        _CONV_CASES[key] = {"frames": frames, "w32": w32, "x": x, "w": w, "dy": bf16_values(g, N, Hf // 2, Hf // 2, Kc),
                            "ref": tuple(ref_conv_fwd(x, w, 2, 3, dt)["y"] for dt in (F64, F32))}
    return _CONV_CASES[key]


# ======================================================================================================
# One small seeded instance of every restatement (tests/test_kernel_parity_cpu.py checks that its float32
# evaluation is a non-degenerate bar).  name -> fn(dt) -> dict of outputs.
# ======================================================================================================
BASE, SITE = 0x1234_5678_9ABC, 7


def gelu_z(rows, cols, seed):
    """z over [-6, 6] with 0 and +-1e-6 among its first elements."""
    z = (torch.rand(rows, cols, generator=gen(seed), dtype=F32) * 12 - 6).reshape(-1)
    for i, val in enumerate((0.0, 1e-6, -1e-6, 6.0, -6.0)[:z.numel()]):
        z[i] = val
    return z.reshape(rows, cols)


def adam_inputs(n, seed):
    """Gradients bounded away from zero: the update lr * g / (|g| + eps) has slope lr / eps at g = 0, where a
    rounding of g is amplified without bound in any float32 evaluation, the kernel's and the restatement's alike."""
    g = gen(seed)
    p, r = randn(g, n), randn(g, n)
    grad = torch.sign(r) * (0.1 + r.abs())
    grad[grad == 0] = 0.1
    return p, grad, torch.zeros(n), torch.zeros(n)


def _instances():
    g = gen(20261020)
    inst = {}
    rows, d, rps = 18, 128, 9
    x, r, dy = randn(g, rows, d) * 3 + 1, randn(g, rows, d) * 3 + 1, randn(g, rows, d)
    gamma, beta = randn(g, d), randn(g, d)
    sc = drop_scale(keep_mask(BASE, SITE, np.arange(rows) // rps, 0.5), 0.5, F32)
    inst["add_ln"] = lambda dt: ref_add_ln(x, r, gamma, beta, sc, dy, 1e-5, dt)
    inst["add_ln_no_r"] = lambda dt: ref_add_ln(x, None, gamma, beta, None, dy, 1e-5, dt)
    xm, dym, dx0 = randn(g, 3, 13, 70), randn(g, 3, 70), randn(g, 3, 13, 70)
    inst["mean_pool"] = lambda dt: ref_mean_pool(xm, dym, dx0, dt)
    scores = randn(g, 3, 13) * 3 + 50
    inst["attn_pool"] = lambda dt: ref_attn_pool(xm, scores, dym, dx0, dt)
    z, dz = gelu_z(7, 130, 1), randn(g, 7, 130)
    kz = keep_mask(BASE, SITE, np.arange(7 * 130).reshape(7, 130), 0.3)
    inst["gelu_dropout"] = lambda dt: ref_gelu_dropout(z, dz, kz, 0.3, dt)
    xa, ra = randn(g, 12, 70), randn(g, 4, 70)
    ka = keep_mask(BASE, SITE, np.arange(12 * 70).reshape(12, 70), 0.25)
    inst["add_dropout"] = lambda dt: ref_add_dropout(xa, ra, 4, ka, 0.25, dt)
    xd, yd = randn(g, 7, 33), torch.relu(randn(g, 7, 33))
    kd = keep_mask(BASE, SITE, np.arange(7 * 33).reshape(7, 33), 0.3)
    inst["dropout"] = lambda dt: ref_dropout(xd, kd, 0.3, dt)
    inst["relu_dropout_bwd"] = lambda dt: ref_relu_dropout_bwd(xd, yd, kd, 0.3, dt)
    S, dPp = randn(g, 2, 5, 70) * 4, randn(g, 2, 5, 70)
    ks = keep_mask(BASE, SITE, np.arange(2 * 5 * 70).reshape(2, 5, 70), 0.2)
    inst["softmax_dropout"] = lambda dt: ref_softmax_dropout(S, 0.25, dPp, ks, 0.2, dt)
    zg, vg, ag, dg = randn(g, 5), randn(g, 5, 300), randn(g, 5, 300), randn(g, 5, 300)
    zg[0], zg[1] = 20.0, -20.0
    inst["gate_mix"] = lambda dt: ref_gate_mix(zg, vg, ag, dg, vg * 0.5, ag * 0.5, dt)
    qt, qp, kt, kp, db = randn(g, 2, 17), randn(g, 2), randn(g, 2, 241), randn(g, 2), randn(g, 2, 17, 241)
    tscale = torch.tensor([0.7])
    inst["token_bias"] = lambda dt: ref_token_bias(qt, qp, kt, kp, tscale, db, dt)
    za, zv, dso = randn(g, 6, 70) * 3, randn(g, 6, 70) * 3, randn(g, 6, 70)
    inst["softmax_avg"] = lambda dt: ref_softmax_avg(za, zv, dso, dt)
    xs = randn(g, 1000)
    inst["vec_sum"] = lambda dt: ref_vec_sum(xs, torch.tensor(0.3), dt)
    inst["scale_dev"] = lambda dt: ref_scale_dev(xs, torch.tensor([0.37]), dt)
    pa_, ga_, ma_, va_ = adam_inputs(1027, 3)
    inst["adam"] = lambda dt: ref_adam(pa_, ga_, ma_, va_, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1, 0.5, dt)
    A, Bm, bias, c0 = randn(g, 65, 33), randn(g, 33, 70), randn(g, 70), randn(g, 65, 70)
    for act in ("none", "relu", "gelu"):
        inst[f"gemm_{act}"] = lambda dt, act=act: ref_gemm(A, Bm, bias, c0, 1, act, dt)
    Ab, Bb, cb = randn(g, 3, 17, 37), randn(g, 3, 37, 19), randn(g, 3, 17, 19)
    inst["gemm_batched"] = lambda dt: ref_gemm(Ab, Bb, None, cb, 1, "none", dt)
    ca, cv = randn(g, 5, 70), randn(g, 5, 70)
    ls, dl, dls0 = torch.tensor([math.log(1 / 0.07)]), torch.tensor([0.7]), torch.tensor([0.25])
    inst["clip_align"] = lambda dt: ref_clip_align(ca, cv, ls, dl, dls0, dt)
    # csrc/bn_pool.hip
    gb = gen(20261021)
    C, M = 24, 200
    xb = bf16_values(gb, M, C, shift=0.5)
    st = tile_stats(xb)
    rm0, rv0 = randn(gb, C) * 0.1, torch.rand(C, generator=gb) + 0.5
    inst["bn_finalize"] = lambda dt: ref_bn_finalize(st, M, 1e-5, 0.1, rm0, rv0, dt)
    inst["bn_finalize_eval"] = lambda dt: ref_bn_finalize(None, M, 1e-5, 0.1, rm0, rv0, dt)
    ms_b = torch.stack([xb.mean(0), 1 / torch.sqrt(xb.var(0, unbiased=False) + 1e-5)], 1)
    ms_r = torch.stack([randn(gb, C) * 0.2, torch.rand(C, generator=gb) + 0.5], 1)
    ga, be, ga2, be2 = torch.rand(C, generator=gb) + 0.5, randn(gb, C) * 0.2, torch.rand(C, generator=gb) + 0.5, \
        randn(gb, C) * 0.2
    rb = bf16_values(gb, M, C)
    inst["bn_apply"] = lambda dt: ref_bn_apply(xb, ms_b, ga, be, False, dt)
    inst["bn_apply_res_relu"] = lambda dt: ref_bn_apply(xb, ms_b, ga, be, True, dt, res=rb)
    inst["bn_apply_resbn_relu"] = lambda dt: ref_bn_apply(xb, ms_b, ga, be, True, dt, res=rb, ms2=ms_r, gamma2=ga2,
                                                          beta2=be2)
    dyb, mk = bf16_values(gb, M, C), torch.relu(bf16_values(gb, M, C))
    dg0, db0 = randn(gb, C), randn(gb, C)
    inst["bn_bwd"] = lambda dt: ref_bn_bwd(dyb, mk, xb, ms_b, ga, True, dt, dgamma0=dg0, dbeta0=db0)
    inst["bn_bwd_running"] = lambda dt: ref_bn_bwd(dyb, None, xb, ms_b, ga, False, dt, dgamma0=dg0, dbeta0=db0)
    xp_, dyp = bf16_values(gb, 2, 9, 7, 8), bf16_values(gb, 2, 5, 4, 8)
    inst["maxpool"] = lambda dt: ref_maxpool(xp_, dyp, dt)
    dya = randn(gb, 2, 8)
    inst["avgpool"] = lambda dt: ref_avgpool(xp_, dya, dt)
    pr, o0 = randn(gb, 65, 40), randn(gb, 40)
    inst["rows_sum"] = lambda dt: ref_rows_sum(pr, o0, dt)
    inst.update(_audio_instances())
    inst.update(_conv_instances())
    return inst


def gemm_bf16_inputs(M, N, K, seed, zsigma=0.8):
    """bf16-valued A [M, K] (unit normal), W [N, K] scaled so that z = A W^T has sigma ``zsigma`` (a GELU output is
    then determined at 90 % and more of its elements: DESIGN.md section 2), an fp32 bias and a bf16-valued residual."""
    g = gen(seed)
    return {"a": bf16_values(g, M, K), "w": bf16_values(g, N, K, scale=zsigma / math.sqrt(K)),
            "bias": randn(g, N) * 0.5, "res": bf16_values(g, M, N)}


def posconv_inputs(B, L, C, G, taps, seed, zsigma=0.8):
    """x [B, L, C], wp [G, cg, taps, cg] (K-contiguous (tap, c) rows per output channel), bias, residual."""
    g = gen(seed)
    cg = C // G
    return {"x": bf16_values(g, B, L, C), "wp": bf16_values(g, G, cg, taps, cg, scale=zsigma / math.sqrt(taps * cg)),
            "bias": randn(g, C) * 0.5, "res": bf16_values(g, B, L, C)}


def grid_index(*shape):
    return np.arange(int(np.prod(shape)), dtype=np.uint64).reshape(shape)


def _audio_instances():
    """csrc/gemm_bf16.hip and the WavLM row kernels: one small instance per restatement."""
    inst = {}
    M, N, K = 37, 24, 64
    gi = gemm_bf16_inputs(M, N, K, 20261101)
    for act in ("none", "relu", "gelu"):
        inst[f"gemm_bf16_{act}"] = lambda dt, act=act: ref_gemm_bf16(gi["a"], gi["w"], gi["bias"], gi["res"], act, None,
                                                                     0.0, dt)
    inst["gemm_bf16_gelu_plain"] = lambda dt: ref_gemm_bf16(gi["a"], gi["w"], None, None, "gelu", None, 0.0, dt)
    kg = keep_mask_pair(BASE, SITE, grid_index(M, N), 0.1)
    inst["gemm_bf16_gelu_drop"] = lambda dt: ref_gemm_bf16(gi["a"], gi["w"], gi["bias"], None, "gelu", kg, 0.1, dt)
    # rows mode: Conv1d(k = 3, s = 2) over 2 clips of 9 frames of 64 channels
    g = gen(20261102)
    Lin, Cc = 9, 64
    Lo = (Lin - 3) // 2 + 1
    xr = bf16_values(g, 2 * Lin * Cc)
    wr = bf16_values(g, N, 3 * Cc, scale=0.8 / math.sqrt(3 * Cc))
    ar = gather_rows(xr, 2 * Lo, 3 * Cc, Lo, 2 * Cc, Lin * Cc)
    inst["gemm_bf16_rows"] = lambda dt: ref_gemm_bf16(ar, wr, gi["bias"], None, "none", None, 0.0, dt)
    pc = posconv_inputs(2, 17, 96, 2, 5, 20261103)
    inst["posconv_gelu"] = lambda dt: ref_posconv(pc["x"], pc["wp"], pc["bias"], pc["res"], "gelu", 2, 17, 96, 2, 5, 2,
                                                  dt)
    inst["posconv_none"] = lambda dt: ref_posconv(pc["x"], pc["wp"], pc["bias"], None, "none", 2, 17, 96, 2, 5, 2, dt)
    rows, d = 37, 256
    xl, gam, bet = randn(g, rows, d) * 2 + 0.5, randn(g, d) * 0.3 + 1, randn(g, d) * 0.3
    kl = keep_mask_pair(BASE, SITE, grid_index(rows, d), 0.1)
    inst["layernorm"] = lambda dt: ref_layernorm(xl, gam, bet, 1e-5, None, 0.0, dt)
    inst["layernorm_drop"] = lambda dt: ref_layernorm(xl, gam, bet, 1e-5, kl, 0.1, dt)
    dya, dyb = randn(g, rows, d), randn(g, rows, d)
    inst["ln_bwd"] = lambda dt: ref_ln_bwd([dya, dyb], xl, gam, 1e-5, dt)
    parts, o0 = randn(g, 65, 33), randn(g, 33)
    inst["fold_rows"] = lambda dt: ref_fold_rows(parts, o0, dt)
    inst["colsum"] = lambda dt: ref_colsum(parts, o0, dt)
    zb = to_bf16(gelu_z(8, 33, 5)).to(F32)
    df, db0 = randn(g, 8, 33), randn(g, 33)
    inst["gelu"] = lambda dt: ref_gelu(zb, dt)
    inst["gelu_bwd"] = lambda dt: ref_gelu_bwd(df, zb, db0, dt)
    xd = bf16_values(g, 9, 40)
    kd = keep_mask_pair(BASE, SITE, grid_index(9, 40), 0.1)
    inst["dropout_rows"] = lambda dt: ref_dropout_rows(xd, kd, 0.1, dt)
    xw, dyw, dw0 = bf16_values(g, 37, 24), bf16_values(g, 37, 32), randn(g, 16, 24)
    inst["linear_wgrad"] = lambda dt: ref_linear_wgrad(xw, dyw, dw0, 8, 16, dt)
    vw, gw = randn(g, 5, 7, 5), randn(g, 5)
    inst["weightnorm_scale"] = lambda dt: ref_weightnorm_scale(vw, gw, dt)
    return inst


def _conv_instances():
    """csrc/conv.hip, conv_wgrad.hip, conv_pack.hip: one small instance per restatement."""
    inst = {}
    N, H, W, C, Kc = 2, 6, 9, 64, 64
    i = conv_inputs(N, H, W, C, Kc, 3, 1, 1, seed=20261201)
    inst["conv_fwd"] = lambda dt: ref_conv_fwd(i["x"], i["w"], 1, 1, dt)
    inst["conv_dgrad"] = lambda dt: ref_conv_dgrad(i["dy"], i["w"], H, W, 1, 1, dt)
    inst["conv_dgrad_res_mask"] = lambda dt: ref_conv_dgrad(i["dy"], i["w"], H, W, 1, 1, dt, i["res"], i["mask"])
    s = conv_inputs(N, 9, 6, C, 128, 3, 2, 1, seed=20261202, ds_k=64)
    inst["conv_fwd_s2"] = lambda dt: ref_conv_fwd(s["x"], s["w"], 2, 1, dt)
    inst["conv_dgrad_s2_ds"] = lambda dt: ref_conv_dgrad(s["dy"], s["w"], 9, 6, 2, 1, dt, s["res"], s["mask"],
                                                         ds=(s["ds_dy"], s["wd"]))
    dw0 = randn(gen(20261203), Kc, C, 3, 3)
    inst["conv_wgrad"] = lambda dt: ref_conv_wgrad(i["x"], i["dy"], 3, 3, 1, 1, C, dw0, dt, splits=2)
    stored = to_bf16(ref_conv_fwd(i["x"], i["w"], 1, 1, F64)["y"]).to(F32)
    inst["conv_sums"] = lambda dt: ref_conv_sums(stored, dt)
    inst["conv_bnr_sums"] = lambda dt: ref_bnr_sums(stored, i["mask"], i["xb"], i["ms"], dt)
    w7 = randn(gen(20261204), 8, 3, 7, 7)
    for mode in (0, 1, 2):
        inst[f"conv_pack_w{mode}"] = lambda dt, mode=mode: {"out": ref_pack_conv_weight(w7, 16 if mode == 2 else 8,
                                                                                     mode).to(dt)}
    frames = randn(gen(20261205), 2, 3, 6, 10)
    inst["conv_pack_s2d"] = lambda dt: {"out": ref_pack_input_s2d(frames).to(dt)}
    return inst


INSTANCES = _instances()
# Outputs that are copies of an input in any precision (no arithmetic): their bar is zero by construction and only
# the one-ulp floor of assert_fp64_parity applies.  Without a residual the saved pre-norm sum is x itself; the max
# pool's y and argmax and the eval-mode BatchNorm mean are copies; the max pool's dx adds at most four bf16 values of
# one scale, which float32 does exactly.
EXACT_OUTPUTS = {"add_ln_no_r": {"s"}, "maxpool": {"y", "arg", "dx"}, "bn_finalize_eval": {"mean"},
                 "conv_pack_w0": {"out"}, "conv_pack_w1": {"out"}, "conv_pack_w2": {"out"}, "conv_pack_s2d": {"out"}}
# Outputs the kernels store as bfloat16: judged by assert_bf16_parity.
BF16_OUTPUTS = {"bn_apply": {"y"}, "bn_apply_res_relu": {"y"}, "bn_apply_resbn_relu": {"y"}, "bn_bwd": {"dx"},
                "bn_bwd_running": {"dx"}, "maxpool": {"y", "dx"}, "avgpool": {"dx"},
                "gemm_bf16_none": {"out"}, "gemm_bf16_relu": {"out"}, "gemm_bf16_gelu": {"out"},
                "gemm_bf16_gelu_plain": {"out"}, "gemm_bf16_gelu_drop": {"out"}, "gemm_bf16_rows": {"out"},
                "posconv_gelu": {"out"}, "posconv_none": {"out"}, "layernorm": {"y"}, "layernorm_drop": {"y"},
                "ln_bwd": {"dx"}, "gelu": {"f"}, "gelu_bwd": {"dz"}, "dropout_rows": {"y"},
                "conv_fwd": {"y"}, "conv_fwd_s2": {"y"}, "conv_dgrad": {"dx"}, "conv_dgrad_res_mask": {"dx"},
                "conv_dgrad_s2_ds": {"dx"}}

"""Each fp32 kernel of csrc/head.hip, csrc/temporal.hip and csrc/align.hip against its float64 restatement
(tests/kernel_parity.py), at the shapes where its code takes another path: tails, partial blocks, the thresholds
between two kernels, every leading dimension wider than its row, every accumulate flag.

Outputs are views into marker-filled buffers (every element outside the view must stay bit-unchanged), strided inputs
carry NaN in their gaps, dropout masks are restated on the host from (base, site, index, p) and must match exactly.
Where a backward kernel reads what its forward saved, it is given the forward kernel's own output and compared with
the float64 chain from the original inputs.
"""
import functools
import math

import numpy as np
import pytest
import torch

from multimodalemotionrecognition_amd import kernels as K
from multimodalemotionrecognition_amd._lib import MerKernelError
from tests import kernel_parity as kp
from tests.kernel_parity import (BASE, F32, F64, SITE, assert_dropout_parity, assert_fp64_parity, drop_scale, gen,
                                 guarded_flat, guarded_rows, keep_mask, padded_input, padded_rows, randn)

pytestmark = pytest.mark.gpu
DEV = "cuda"


def rng_base():
    return torch.tensor([BASE], dtype=torch.int64, device=DEV)


def both(fn):
    """(float64, float32) evaluations of one restatement."""
    return fn(F64), fn(F32)


def check(name, case, got, refs, keys, extra=None):
    for k in keys:
        assert_fp64_parity(got[k], refs[0][k], refs[1][k], extra=(extra or {}).get(k, 0.0), what=f"{name}[{case}] {k}")


def grid_idx(*shape):
    return np.arange(int(np.prod(shape)), dtype=np.uint64).reshape(shape)


# ---------------------------------------------------------------------------------------------------------
# add_ln_fwd / add_ln_bwd
# ---------------------------------------------------------------------------------------------------------
LN_SHAPES = [(1, 8, 1), (5, 70, 5), (18, 128, 9), (33, 200, 11)]
LN_EPS = 1e-5


@functools.lru_cache(maxsize=None)
def ln_case(rows, d, rps, variant):
    g = gen(1000 + rows * 7 + d)
    x, r, dy = randn(g, rows, d) * 3 + 1, randn(g, rows, d) * 3 + 1, randn(g, rows, d) * 3 + 1
    gamma, beta, pre = randn(g, d), randn(g, d), randn(g, 2, d)
    p = 0.5 if variant == "r_drop" else 0.0
    keep = keep_mask(BASE, SITE, np.arange(rows) // rps, p)
    if variant == "no_r":
        r = None
    refs = both(lambda dt: kp.ref_add_ln(x, r, gamma, beta, None if r is None else drop_scale(keep, p, dt), dy,
                                         LN_EPS, dt))
    return dict(x=x, r=r, dy=dy, gamma=gamma, beta=beta, pre=pre, p=p, keep=keep, refs=refs)


def ln_forward(c, rows, d, rps, saved=True):
    o = {k: guarded_flat(s, DEV) for k, s in (("y", (rows, d)), ("s", (rows, d)), ("mean", (rows,)), ("rstd", (rows,)))}
    K.add_ln_fwd(c["x"].to(DEV), None if c["r"] is None else c["r"].to(DEV), c["gamma"].to(DEV), c["beta"].to(DEV),
                 o["y"].view, o["s"].view if saved else None, o["mean"].view if saved else None,
                 o["rstd"].view if saved else None, rps, dp_p=c["p"], rng=rng_base() if c["p"] > 0 else None, site=SITE,
                 eps=LN_EPS)
    for k, t in o.items():
        t.check(f"add_ln_fwd {k}")
    return o


def ln_backward(c, fwd, rows, d, rps, want=("dr", "dgamma", "dbeta")):
    o = {"dx": guarded_flat((rows, d), DEV), "dr": guarded_flat((rows, d), DEV),
         "dgamma": guarded_flat((d,), DEV, init=c["pre"][0]), "dbeta": guarded_flat((d,), DEV, init=c["pre"][1])}
    arg = {k: (o[k].view if k in want and (k != "dr" or c["r"] is not None) else None) for k in ("dr", "dgamma", "dbeta")}
    K.add_ln_bwd(c["dy"].to(DEV), fwd["s"].view, fwd["mean"].view, fwd["rstd"].view, c["gamma"].to(DEV), o["dx"].view,
                 arg["dr"], arg["dgamma"], arg["dbeta"], rps, dp_p=c["p"], rng=rng_base() if c["p"] > 0 else None,
                 site=SITE)
    for k, t in o.items():
        t.check(f"add_ln_bwd {k}")
    return o, arg


def ln_check_backward(c, o, arg, case, rows, d):
    r64, r32 = c["refs"]
    assert_fp64_parity(o["dx"].view, r64["dx"], r32["dx"], what=f"add_ln_bwd[{case}] dx")
    if arg["dr"] is not None:
        keep = c["keep"][:, None].expand(rows, d)
        assert_dropout_parity(o["dr"].view, keep, c["p"], r64["dr"], r32["dr"], what=f"add_ln_bwd[{case}] dr")
    for i, k in enumerate(("dgamma", "dbeta")):  # += into the pre-filled buffers
        if arg[k] is not None:
            assert_fp64_parity(o[k].view, c["pre"][i].double() + r64[k], c["pre"][i] + r32[k],
                               what=f"add_ln_bwd[{case}] {k}")
        else:
            assert torch.equal(o[k].view.cpu(), c["pre"][i]), f"{k} was not passed and must stay as it was"


@pytest.mark.parametrize("variant", ["no_r", "r_keep", "r_drop"])
@pytest.mark.parametrize("rows,d,rps", LN_SHAPES)
def test_add_ln(rows, d, rps, variant):
    c = ln_case(rows, d, rps, variant)
    case = f"{rows}x{d}/{rps} {variant}"
    fwd = ln_forward(c, rows, d, rps)
    check("add_ln_fwd", case, {k: t.view for k, t in fwd.items()}, c["refs"], ("y", "s", "mean", "rstd"))
    if variant == "r_drop":  # a dropped sample's rows are x itself
        dropped = ~c["keep"]
        assert torch.equal(fwd["s"].view.cpu()[dropped], c["x"][dropped])
    o, arg = ln_backward(c, fwd, rows, d, rps)
    ln_check_backward(c, o, arg, case, rows, d)
    o2, _ = ln_backward(c, fwd, rows, d, rps)
    for k in o:
        assert torch.equal(o[k].buf, o2[k].buf), f"add_ln_bwd {k}: two launches differ"


@pytest.mark.parametrize("leave_out", ["saved", "dr", "dgamma", "dbeta"])
def test_add_ln_optional_outputs(leave_out):
    rows, d, rps = 18, 128, 9
    c = ln_case(rows, d, rps, "r_drop")
    case = f"{rows}x{d}/{rps} without {leave_out}"
    if leave_out == "saved":
        fwd = ln_forward(c, rows, d, rps, saved=False)
        check("add_ln_fwd", case, {"y": fwd["y"].view}, c["refs"], ("y",))
        for k in ("s", "mean", "rstd"):
            assert bool((fwd[k].buf.cpu() == torch.tensor(kp.MARKER)).all())
        return
    fwd = ln_forward(c, rows, d, rps)
    o, arg = ln_backward(c, fwd, rows, d, rps, want=tuple(k for k in ("dr", "dgamma", "dbeta") if k != leave_out))
    assert arg[leave_out] is None
    if leave_out == "dr":
        assert bool((o["dr"].buf.cpu() == torch.tensor(kp.MARKER)).all())
    ln_check_backward(c, o, arg, case, rows, d)


@pytest.mark.parametrize("rows,d,rps", [(3, 2112, 3), (2, 5120, 2)])
def test_add_ln_bwd_large_lds(rows, d, rps):
    """8*d*4 bytes of dynamic LDS: 66 KB (just over the default limit of a launch) and 160 KB (the guard's limit)."""
    c = ln_case(rows, d, rps, "r_keep")
    case = f"{rows}x{d}/{rps} r_keep"
    fwd = ln_forward(c, rows, d, rps)
    check("add_ln_fwd", case, {k: t.view for k, t in fwd.items()}, c["refs"], ("y", "s", "mean", "rstd"))
    o, arg = ln_backward(c, fwd, rows, d, rps)
    ln_check_backward(c, o, arg, case, rows, d)


def test_add_ln_bwd_rejects_d_past_the_lds_limit():
    rows, d = 2, 5121
    z = torch.zeros(rows, d, device=DEV)
    v, one = torch.zeros(rows, device=DEV), torch.ones(d, device=DEV)
    with pytest.raises(MerKernelError):
        K.add_ln_bwd(z, z, v, v + 1, one, torch.empty_like(z), None, torch.zeros_like(one), torch.zeros_like(one), rows)


# ---------------------------------------------------------------------------------------------------------
# mean_pool_fwd / mean_pool_bwd
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L,D", [(2, L, 65) for L in (1, 2, 4, 5, 8, 9, 13)] + [(3, 149, 70)])
def test_mean_pool(B, L, D):
    g = gen(2000 + L)
    x, dy, dx0 = randn(g, B, L, D), randn(g, B, D), randn(g, B, L, D)
    case = f"{B}x{L}x{D}"
    y = guarded_rows(B, D, D + 7, DEV, offset=5)  # a column offset into a wider buffer
    K.mean_pool_fwd(x.to(DEV), y.view)
    y.check("mean_pool_fwd y")
    refs = both(lambda dt: kp.ref_mean_pool(x, dy, None, dt))
    check("mean_pool_fwd", case, {"y": y.view}, refs, ("y",))
    y2 = guarded_rows(B, D, D + 7, DEV, offset=5)
    K.mean_pool_fwd(x.to(DEV), y2.view, ldy=D + 7)
    assert torch.equal(y.buf, y2.buf)
    for acc in (0, 1):
        refs = both(lambda dt: kp.ref_mean_pool(x, dy, dx0 if acc else None, dt))
        dx = guarded_flat((B, L, D), DEV, init=dx0 if acc else None)
        K.mean_pool_bwd(padded_rows(dy, 5, DEV, offset=2), dx.view, accumulate=bool(acc))
        dx.check("mean_pool_bwd dx")
        check("mean_pool_bwd", f"{case} acc{acc}", {"dx": dx.view}, refs, ("dx",))


# ---------------------------------------------------------------------------------------------------------
# attn_pool_fwd / attn_pool_bwd
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L,D", [(1, 1, 1), (2, 5, 70), (2, 257, 33), (1, 4096, 8)])
def test_attn_pool(B, L, D):
    g = gen(3000 + L)
    x, scores, dy, dx0 = randn(g, B, L, D), randn(g, B, L) * 3 + 50, randn(g, B, D), randn(g, B, L, D)
    case = f"{B}x{L}x{D}"
    attn, y = guarded_flat((B, L), DEV), guarded_rows(B, D, D + 3, DEV)
    K.attn_pool_fwd(x.to(DEV), scores.to(DEV), attn.view, y.view)
    attn.check("attn_pool_fwd attn")
    y.check("attn_pool_fwd y")
    refs = both(lambda dt: kp.ref_attn_pool(x, scores, dy, None, dt))
    check("attn_pool_fwd", case, {"attn": attn.view, "y": y.view}, refs, ("attn", "y"))
    for acc in (0, 1):
        refs = both(lambda dt: kp.ref_attn_pool(x, scores, dy, dx0 if acc else None, dt))
        dx, ds = guarded_flat((B, L, D), DEV, init=dx0 if acc else None), guarded_flat((B, L), DEV)
        K.attn_pool_bwd(x.to(DEV), attn.view, padded_rows(dy, 5, DEV, offset=1), dx.view, ds.view, accumulate=bool(acc))
        dx.check("attn_pool_bwd dx")
        ds.check("attn_pool_bwd dscores")
        check("attn_pool_bwd", f"{case} acc{acc}", {"dx": dx.view, "dscores": ds.view}, refs, ("dx", "dscores"))


def test_attn_pool_rejects_L_past_4096():
    B, L, D = 1, 4097, 2
    x, s = torch.zeros(B, L, D, device=DEV), torch.zeros(B, L, device=DEV)
    with pytest.raises(MerKernelError):
        K.attn_pool_fwd(x, s, torch.empty_like(s), torch.empty(B, D, device=DEV))
    with pytest.raises(MerKernelError):
        K.attn_pool_bwd(x, s, torch.zeros(B, D, device=DEV), torch.empty_like(x), torch.empty_like(s))


# ---------------------------------------------------------------------------------------------------------
# gelu_dropout_fwd / gelu_dropout_bwd
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("rows,cols,strided", [(3, 5, True), (7, 130, True), (1100, 1000, False)])
def test_gelu_dropout(rows, cols, strided, p):
    """The contiguous case has more than 4096*256 elements, so the grid-stride loop wraps.  |dy| <= 1, so that the
    documented erf error enters the derivative as 0.5 * 1.5e-7."""
    z = kp.gelu_z(rows, cols, 4000 + rows)
    dy = torch.rand(rows, cols, generator=gen(4100 + rows), dtype=F32) * 2 - 1
    keep = keep_mask(BASE, SITE, grid_idx(rows, cols), p)
    refs = both(lambda dt: kp.ref_gelu_dropout(z, dy, keep, p, dt))
    case = f"{rows}x{cols} p{p}"
    rng = rng_base() if p > 0 else None
    if strided:
        zd, dyd = padded_rows(z, 3, DEV, offset=1), padded_rows(dy, 6, DEV, offset=2)
        y, dz = guarded_rows(rows, cols, cols + 2, DEV), guarded_rows(rows, cols, cols + 4, DEV)
    else:
        zd, dyd = z.to(DEV), dy.to(DEV)
        y, dz = guarded_flat((rows, cols), DEV), guarded_flat((rows, cols), DEV)
    K.gelu_dropout_fwd(zd, y.view, p=p, rng=rng, site=SITE)
    K.gelu_dropout_bwd(dyd, zd, dz.view, p=p, rng=rng, site=SITE)
    y.check("gelu_dropout_fwd y")
    dz.check("gelu_dropout_bwd dz")
    assert_dropout_parity(y.view, keep, p, refs[0]["y"], refs[1]["y"], extra=0.5 * float(z.abs().max()) * kp.ERF_FAST_ABS,
                          what=f"gelu_dropout_fwd[{case}] y")
    assert_dropout_parity(dz.view, keep, p, refs[0]["dz"], refs[1]["dz"], extra=0.5 * kp.ERF_FAST_ABS,
                          what=f"gelu_dropout_bwd[{case}] dz")


# ---------------------------------------------------------------------------------------------------------
# add_dropout, dropout_, relu_dropout_bwd_
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("rows,cols,period", [(12, 70, 4), (5, 33, None)])
def test_add_dropout(rows, cols, period, p):
    g = gen(5000 + rows)
    x, r = randn(g, rows, cols), randn(g, period or rows, cols)
    keep = keep_mask(BASE, SITE, grid_idx(rows, cols), p)
    refs = both(lambda dt: kp.ref_add_dropout(x, r, period or rows, keep, p, dt))
    rng = rng_base() if p > 0 else None
    if period is None:  # in place: y is x
        y = guarded_flat((rows, cols), DEV, init=x)
        out = K.add_dropout(y.view, r.to(DEV), y.view, r_period=None, p=p, rng=rng, site=SITE)
        assert out.data_ptr() == y.view.data_ptr()
    else:
        y = guarded_flat((rows, cols), DEV)
        K.add_dropout(x.to(DEV), r.to(DEV), y.view, r_period=period, p=p, rng=rng, site=SITE)
    y.check("add_dropout y")
    check("add_dropout", f"{rows}x{cols}/{period} p{p}", {"y": y.view}, refs, ("y",))
    # the mask, exactly: y - x is zero where dropped and r / (1 - p) where kept
    delta = y.view.cpu().double() - x.double()
    assert bool(((delta != 0) == keep).all())


def test_dropout_inplace_strided():
    rows, cols, ld, p = 7, 33, 40, 0.3
    x = randn(gen(5100), rows, cols)
    keep = keep_mask(BASE, SITE, grid_idx(rows, cols), p)
    assert 0 < int(keep.sum()) < rows * cols
    refs = both(lambda dt: kp.ref_dropout(x, keep, p, dt))
    buf = guarded_rows(rows, cols, ld, DEV, init=x)
    K.dropout_(buf.view, p, rng=rng_base(), site=SITE)
    buf.check("dropout_ x")
    assert_dropout_parity(buf.view, keep, p, refs[0]["y"], refs[1]["y"], what=f"dropout_[{rows}x{cols}/{ld} p{p}] x")
    same = guarded_rows(rows, cols, ld, DEV, init=x)
    K.dropout_(same.view, 0.0)  # p == 0: nothing is launched
    assert torch.equal(same.view.cpu(), x)


@pytest.mark.parametrize("p", [0.0, 0.3])
def test_relu_dropout_bwd_strided(p):
    rows, cols, ld = 7, 33, 40
    g = gen(5200)
    dy, y = randn(g, rows, cols), torch.relu(randn(g, rows, cols))
    assert bool((y == 0).any()) and bool((y > 0).any())  # exact zeros in the gate
    keep = keep_mask(BASE, SITE, grid_idx(rows, cols), p)
    refs = both(lambda dt: kp.ref_relu_dropout_bwd(dy, y, keep, p, dt))
    buf = guarded_rows(rows, cols, ld, DEV, init=dy)
    K.relu_dropout_bwd_(buf.view, padded_rows(y, 4, DEV, offset=3), p, rng=rng_base() if p > 0 else None, site=SITE)
    buf.check("relu_dropout_bwd_ dy")
    assert_dropout_parity(buf.view, keep & (y > 0), p, refs[0]["dz"], refs[1]["dz"],
                          what=f"relu_dropout_bwd_[{rows}x{cols}/{ld} p{p}] dz")


# ---------------------------------------------------------------------------------------------------------
# softmax_dropout_fwd / softmax_dropout_bwd
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("B,H,Lq,Lk,h", [(1, 1, 1, 1, 0), (2, 3, 5, 70, 1), (2, 4, 3, 149, 3)])
def test_softmax_dropout(B, H, Lq, Lk, h, p):
    g = gen(6000 + Lk)
    S, dPp, scale = randn(g, B, Lq, Lk) * 4, randn(g, B, Lq, Lk), 0.3
    b, i, j = np.meshgrid(np.arange(B), np.arange(Lq), np.arange(Lk), indexing="ij")
    keep = keep_mask(BASE, SITE, ((b * H + h) * Lq + i) * Lk + j, p)
    refs = both(lambda dt: kp.ref_softmax_dropout(S, scale, dPp, keep, p, dt))
    case = f"{B}x{H}x{Lq}x{Lk} h{h} p{p}"
    rng = rng_base() if p > 0 else None
    plane = Lq * Lk
    # head h of P[B, H, Lq, Lk] as a view of the whole tensor: every other head is sentinel
    P = kp.Guarded((B, Lq, Lk), (H * plane, Lk, 1), DEV, offset=h * plane, tail=(H - 1 - h) * plane + 5)
    P4 = P.buf[:B * H * plane].view(B, H, Lq, Lk)
    Pd = guarded_flat((B, Lq, Lk), DEV)
    K.softmax_dropout_fwd(S.to(DEV), scale, P4, Pd.view, h, p=p, rng=rng, site=SITE)
    P.check("softmax_dropout_fwd P")
    Pd.check("softmax_dropout_fwd Pd")
    assert_fp64_parity(P.view, refs[0]["P"], refs[1]["P"], what=f"softmax_dropout_fwd[{case}] P")
    assert_dropout_parity(Pd.view, keep, p, refs[0]["Pd"], refs[1]["Pd"], what=f"softmax_dropout_fwd[{case}] Pd")
    dS, Pd2 = guarded_flat((B, Lq, Lk), DEV), guarded_flat((B, Lq, Lk), DEV)
    K.softmax_dropout_bwd(P4, dPp.to(DEV), dS.view, Pd2.view, h, p=p, rng=rng, site=SITE)
    P.check("softmax_dropout_bwd P")
    dS.check("softmax_dropout_bwd dS")
    Pd2.check("softmax_dropout_bwd Pd")
    assert_fp64_parity(dS.view, refs[0]["dS"], refs[1]["dS"], what=f"softmax_dropout_bwd[{case}] dS")
    assert_dropout_parity(Pd2.view, keep, p, refs[0]["Pd"], refs[1]["Pd"], what=f"softmax_dropout_bwd[{case}] Pd")


# ---------------------------------------------------------------------------------------------------------
# gate_mix_fwd / gate_mix_bwd
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,D", [(1, 1), (3, 70), (5, 300)])
def test_gate_mix(B, D):
    g = gen(7000 + D)
    z, v, a, dout, dv0, da0 = randn(g, B), randn(g, B, D), randn(g, B, D), randn(g, B, D), randn(g, B, D), randn(g, B, D)
    z[0] = 20.0
    if B > 1:
        z[1] = -20.0
    refs = both(lambda dt: kp.ref_gate_mix(z, v, a, dout, dv0, da0, dt))
    case = f"{B}x{D}"
    vd, ad = padded_rows(v, 3, DEV, offset=1), padded_rows(a, 5, DEV, offset=2)
    out, gate = guarded_flat((B, D), DEV), guarded_flat((B,), DEV)
    K.gate_mix_fwd(z.to(DEV), vd, ad, out.view, gate.view)
    out.check("gate_mix_fwd out")
    gate.check("gate_mix_fwd g")
    check("gate_mix_fwd", case, {"g": gate.view, "out": out.view}, refs, ("g", "out"))
    dz = guarded_flat((B,), DEV)
    dv, da = guarded_rows(B, D, D + 2, DEV, init=dv0), guarded_rows(B, D, D + 6, DEV, init=da0)
    K.gate_mix_bwd(gate.view, vd, ad, dout.to(DEV), dz.view, dv.view, da.view)
    for t, k in ((dz, "dz"), (dv, "dv"), (da, "da")):
        t.check(f"gate_mix_bwd {k}")
    check("gate_mix_bwd", case, {"dz": dz.view, "dv": dv.view, "da": da.view}, refs, ("dz", "dv", "da"))


# ---------------------------------------------------------------------------------------------------------
# token_bias_fwd / token_bias_bwd: Lq*Lk <= 4096 stages g in LDS, above it the global-memory kernel runs
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Lq,Lk", [(1, 1, 1), (2, 8, 149), (2, 149, 8), (3, 64, 64), (2, 17, 241), (1, 5, 1000)])
def test_token_bias(B, Lq, Lk):
    g = gen(8000 + Lq * 3 + Lk)
    qt, qp, kt, kp_, db = randn(g, B, Lq), randn(g, B), randn(g, B, Lk), randn(g, B), randn(g, B, Lq, Lk)
    scale = torch.tensor([0.7])
    refs = both(lambda dt: kp.ref_token_bias(qt, qp, kt, kp_, scale, db, dt))
    case = f"{B}x{Lq}x{Lk}"
    ins = [t.to(DEV) for t in (qt, qp, kt, kp_, scale)]
    out = guarded_flat((B, Lq, Lk), DEV)
    K.token_bias_fwd(*ins, out.view)
    out.check("token_bias_fwd out")
    check("token_bias_fwd", case, {"out": out.view}, refs, ("out",))
    o = {k: guarded_flat(s, DEV) for k, s in (("dqt", (B, Lq)), ("dkt", (B, Lk)), ("dqp", (B,)), ("dkp", (B,)),
                                              ("dscale_part", (B,)))}
    K.token_bias_bwd(*ins, db.to(DEV), *(o[k].view for k in ("dqt", "dkt", "dqp", "dkp", "dscale_part")))
    for k, t in o.items():
        t.check(f"token_bias_bwd {k}")
    check("token_bias_bwd", case, {k: t.view for k, t in o.items()}, refs, tuple(o))
    assert torch.equal(o["dqp"].view, o["dkp"].view)


# ---------------------------------------------------------------------------------------------------------
# softmax_avg_fwd / softmax_avg_bwd
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C", [(1, 1), (5, 8), (9, 3), (6, 70)])
def test_softmax_avg(B, C):
    g = gen(9000 + C)
    za, zv, dout = randn(g, B, C) * 3, randn(g, B, C) * 3, randn(g, B, C)
    refs = both(lambda dt: kp.ref_softmax_avg(za, zv, dout, dt))
    o = {k: guarded_flat((B, C), DEV) for k in ("out", "pa", "pv", "da", "dv")}
    K.softmax_avg_fwd(za.to(DEV), zv.to(DEV), o["out"].view, o["pa"].view, o["pv"].view)
    K.softmax_avg_bwd(o["pa"].view, o["pv"].view, dout.to(DEV), o["da"].view, o["dv"].view)
    for k, t in o.items():
        t.check(f"softmax_avg {k}")
    check("softmax_avg_fwd", f"{B}x{C}", {k: t.view for k, t in o.items()}, refs, ("out", "pa", "pv"))
    check("softmax_avg_bwd", f"{B}x{C}", {k: t.view for k, t in o.items()}, refs, ("da", "dv"))


# ---------------------------------------------------------------------------------------------------------
# vec_sum, scale_dev
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("n", [1, 63, 257, 1000])
def test_vec_sum(n, acc):
    x, out0 = randn(gen(10000 + n), n), torch.tensor([0.3])
    refs = both(lambda dt: kp.ref_vec_sum(x, out0[0] if acc else None, dt))
    out = guarded_flat((1,), DEV, init=out0 if acc else None)
    K.vec_sum(padded_input(x, (1,), DEV, offset=3), out.view, accumulate=bool(acc))
    out.check("vec_sum out")
    check("vec_sum", f"n{n} acc{acc}", {"out": out.view}, refs, ("out",))


@pytest.mark.parametrize("n", [1, 1_100_000])
def test_scale_dev(n):
    x, s = randn(gen(10100 + n), n), torch.tensor([0.37])
    refs = both(lambda dt: kp.ref_scale_dev(x, s, dt))
    y = guarded_flat((n,), DEV)
    K.scale_dev(x.to(DEV), s.to(DEV), y.view)
    y.check("scale_dev y")
    check("scale_dev", f"n{n}", {"y": y.view}, refs, ("y",))


# ---------------------------------------------------------------------------------------------------------
# adam_step: the 4-wide body, the scalar tail (n % 4) and the grid-stride wrap (n > 2048*256*4)
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wd,grad_scale", [(0.0, 1.0), (0.01, 0.5)])
@pytest.mark.parametrize("n", [1, 3, 4, 7, 1027, 2_097_159])
def test_adam_step(n, wd, grad_scale):
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    p0, _, m0, v0 = kp.adam_inputs(n, 11000 + n)
    state = {dt: {"p": p0.to(dt), "m": m0.to(dt), "v": v0.to(dt)} for dt in (F64, F32)}
    dev = {k: guarded_flat((n,), DEV, init=t, offset=4) for k, t in (("p", p0), ("m", m0), ("v", v0))}
    for step in (1, 2, 3, 1000):  # the references carry their own state, as the kernel does
        grad = kp.adam_inputs(n, 11500 + n + step)[1]
        for dt in (F64, F32):
            s = state[dt]
            state[dt] = kp.ref_adam(s["p"], grad, s["m"], s["v"], lr, b1, b2, eps, wd, step, grad_scale, dt)
        K.adam_step(dev["p"].view, grad.to(DEV), dev["m"].view, dev["v"].view, lr, b1, b2, eps, wd, step,
                    grad_scale=grad_scale)
        for k, t in dev.items():
            t.check(f"adam_step {k}")
        check("adam_step", f"n{n} wd{wd} gs{grad_scale} step{step}", {k: t.view for k, t in dev.items()},
              (state[F64], state[F32]), ("p", "m", "v"))


def test_adam_step_rejects_a_misaligned_view():
    n = 8
    buf = [torch.zeros(n + 1, device=DEV) for _ in range(4)]
    with pytest.raises(MerKernelError):
        K.adam_step(buf[0][1:], buf[1][:n], buf[2][:n], buf[3][:n], 1e-3, 0.9, 0.999, 1e-8, 0.0, 1)
    with pytest.raises(MerKernelError):
        K.adam_step(buf[0][:n], buf[1][1:], buf[2][:n], buf[3][:n], 1e-3, 0.9, 0.999, 1e-8, 0.0, 1)


# ---------------------------------------------------------------------------------------------------------
# gemm epilogue (bias, activation, beta) and layout (ldc, batch strides, split-K)
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gemm_inputs():
    g = gen(12000)
    M, N, Kd = 65, 70, 33
    return randn(g, M, Kd), randn(g, Kd, N), randn(g, N), randn(g, M, N)


@pytest.mark.parametrize("beta", [0, 1])
@pytest.mark.parametrize("act", ["none", "relu", "gelu"])
@pytest.mark.parametrize("with_bias", [False, True])
def test_gemm_epilogue(with_bias, act, beta):
    a, b, bias, c0 = gemm_inputs()
    M, N = c0.shape
    bias = bias if with_bias else None
    refs = both(lambda dt: kp.ref_gemm(a, b, bias, c0, beta, act, dt))
    out = guarded_rows(M, N, N + 3, DEV, init=c0)
    K.gemm(a.to(DEV), b.to(DEV), out.view, bias=None if bias is None else bias.to(DEV), beta=beta, act=act)
    out.check("gemm out")
    extra = 0.5 * float(refs[0]["z"].abs().max()) * kp.ERF_FAST_ABS if act == "gelu" else 0.0
    check("gemm", f"65x70x33 bias{int(with_bias)} {act} beta{beta}", {"out": out.view}, refs, ("out",), {"out": extra})


@pytest.mark.parametrize("with_bias", [False, True])
def test_gemm_splitk_last_slice_of_one_k(with_bias):
    """K = 7937 in 32 slices of 256: the last slice holds a single k; the bias is added by slice 0 alone."""
    M, N, Kd = 8, 8, 7937
    g = gen(12100)
    at, b, bias, c0 = randn(g, Kd, M), randn(g, Kd, N), randn(g, N), randn(g, M, N)
    bias = bias if with_bias else None
    refs = both(lambda dt: kp.ref_gemm(at.t(), b, bias, c0, 1, "none", dt))
    out = guarded_rows(M, N, N + 3, DEV, init=c0)
    K.gemm(at.to(DEV), b.to(DEV), out.view, trans_a=True, bias=None if bias is None else bias.to(DEV), beta=1, splitk=32)
    out.check("gemm split-K out")
    check("gemm", f"8x8x7937 splitk32 bias{int(with_bias)} beta1", {"out": out.view}, refs, ("out",))


@pytest.mark.parametrize("beta", [0, 1])
@pytest.mark.parametrize("odd", [False, True])
def test_gemm_batched_strides(odd, beta):
    """Aligned: row strides 40 / 20 and batch strides that are multiples of 4 floats (the 16-byte loads run).
    Odd: dense rows (37 / 19) and batch strides M*K + 1, K*N + 1 (the scalar-load path)."""
    batch, M, N, Kd = 3, 17, 19, 37
    g = gen(12200)
    a, b, c0 = randn(g, batch, M, Kd), randn(g, batch, Kd, N), randn(g, batch, M, N)
    sam, sbk = (Kd, N) if odd else (40, 20)
    bsa, bsb = (M * Kd + 1, Kd * N + 1) if odd else (M * sam, Kd * sbk)
    ldc = N + 2
    bsc = M * ldc + 5
    refs = both(lambda dt: kp.ref_gemm(a, b, None, c0, beta, "none", dt))
    out = kp.Guarded((batch, M, N), (bsc, ldc, 1), DEV, init=c0)
    ad, bd = padded_input(a, (bsa, sam, 1), DEV), padded_input(b, (bsb, sbk, 1), DEV)
    assert odd or (ad.data_ptr() % 16 == 0 and bd.data_ptr() % 16 == 0)
    K.gemm_batched(ad, bd, out.view, M=M, N=N, K=Kd, sam=sam, sak=1, bsa=bsa, sbk=sbk, sbn=1, bsb=bsb, ldc=ldc,
                   bsc=bsc, batch=batch, beta=beta)
    out.check("gemm_batched out")
    check("gemm_batched", f"3x17x19x37 {'odd' if odd else 'aligned'} beta{beta}", {"out": out.view}, refs, ("out",))


# ---------------------------------------------------------------------------------------------------------
# clip_align_fwd / clip_align_bwd
# ---------------------------------------------------------------------------------------------------------
def run_clip_align(a, v, log_scale, dloss, dls0):
    B, D = a.shape
    o = {k: guarded_flat(s, DEV) for k, s in (("an", (B, D)), ("vn", (B, D)), ("norms", (2 * B,)), ("logits", (B, B)),
                                              ("loss", (1,)), ("da", (B, D)), ("dv", (B, D)))}
    o["dlog_scale"] = guarded_flat((1,), DEV, init=dls0)
    ls = log_scale.to(DEV)
    K.clip_align_fwd(a.to(DEV), v.to(DEV), ls, o["an"].view, o["vn"].view, o["norms"].view, o["logits"].view,
                     o["loss"].view)
    K.clip_align_bwd(o["an"].view, o["vn"].view, o["norms"].view, o["logits"].view, ls, dloss.to(DEV), o["da"].view,
                     o["dv"].view, o["dlog_scale"].view)
    for k, t in o.items():
        t.check(f"clip_align {k}")
    return {k: t.view for k, t in o.items()}


CLIP_FWD, CLIP_BWD = ("an", "vn", "norms", "logits", "loss"), ("da", "dv", "dlog_scale")


@pytest.mark.parametrize("log_scale", [math.log(1 / 0.07), 5.0])
@pytest.mark.parametrize("B,D", [(1, 4), (2, 1), (5, 70), (65, 33)])
def test_clip_align(B, D, log_scale):
    g = gen(13000 + B)
    a, v = randn(g, B, D), randn(g, B, D)
    ls, dloss, dls0 = torch.tensor([log_scale]), torch.tensor([0.7]), torch.tensor([0.25])
    refs = both(lambda dt: kp.ref_clip_align(a, v, ls, dloss, dls0, dt))
    got = run_clip_align(a, v, ls, dloss, dls0)
    case = f"{B}x{D} ls{log_scale:.2f}"
    check("clip_align_fwd", case, got, refs, CLIP_FWD)
    check("clip_align_bwd", case, got, refs, CLIP_BWD)
    if log_scale == 5.0:  # exp(5) > 100: the scale is clamped and no gradient reaches it
        assert float(refs[0]["dlog_scale"]) == 0.25
        assert torch.equal(got["dlog_scale"].cpu(), dls0)
    else:
        assert B == 1 or float(refs[0]["dlog_scale"]) != 0.25


def test_clip_align_zero_row():
    """An all-zero row of a: its norm is clamped at 1e-12, its gradient is d a_n / 1e-12 (huge), so that row is
    compared relative to its own maximum."""
    B, D, zr = 5, 70, 2
    g = gen(13100)
    a, v = randn(g, B, D), randn(g, B, D)
    a[zr] = 0.0
    ls, dloss, dls0 = torch.tensor([math.log(1 / 0.07)]), torch.tensor([0.7]), torch.tensor([0.25])
    r64, r32 = both(lambda dt: kp.ref_clip_align(a, v, ls, dloss, dls0, dt))
    got = {k: t.cpu().clone() for k, t in run_clip_align(a, v, ls, dloss, dls0).items()}
    top = float(r64["da"][zr].abs().max())
    assert top > 1e6 and float(r64["norms"][zr]) == 1e-12
    row = {"got": got["da"][zr].double() / top, "r64": r64["da"][zr] / top, "r32": (r32["da"][zr].double() / top).float()}
    assert_fp64_parity(row["got"].float(), row["r64"], row["r32"], what="clip_align_bwd[5x70 zero row] da[zero row]/max")
    for t in (got["da"], r64["da"], r32["da"]):
        t[zr] = 0.0
    case = "5x70 zero row"
    check("clip_align_fwd", case, got, (r64, r32), CLIP_FWD)
    check("clip_align_bwd", case, got, (r64, r32), CLIP_BWD)


def test_clip_align_rejects_B_past_4096():
    B, D = 4097, 1
    a, n = torch.ones(B, D, device=DEV), torch.ones(2 * B, device=DEV)
    ls, one = torch.zeros(1, device=DEV), torch.ones(1, device=DEV)
    logits = torch.empty(B, B, device=DEV)
    with pytest.raises(MerKernelError):
        K.clip_align_fwd(a, a, ls, torch.empty_like(a), torch.empty_like(a), n, logits, torch.empty(1, device=DEV))
    with pytest.raises(MerKernelError):
        K.clip_align_bwd(a, a, n, logits, ls, one, torch.empty_like(a), torch.empty_like(a), torch.zeros(1, device=DEV))

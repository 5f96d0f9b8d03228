"""The kernels of csrc/optim.hip against float64: the deterministic gradient norm (mer_grad_sqnorm + mer_clip_finalize),
its telemetry record, and mer_adam_step_ex (clip coefficient from the device, EMA plane) against the extended Adam
restatement of tests/optim_ref.py -- at the sizes where the code takes another path: a segment shorter than, equal to
and just longer than a chunk, several segments in one launch, more chunks than the finalize kernel has threads, the
4-wide body, the scalar tail and the grid-stride wrap of the Adam kernel."""
import functools
import math

import numpy as np
import pytest
import torch

from multimodalemotionrecognition_amd import kernels as K
from multimodalemotionrecognition_amd._lib import MerKernelError
from tests import kernel_parity as kp
from tests import optim_ref as R
from tests.kernel_parity import F32, F64, assert_fp64_parity, f32, gen, guarded_flat, randn

pytestmark = pytest.mark.gpu
DEV = "cuda"
C, T = K.NORM_CHUNK, K.CLIP_THREADS
REL = 4 * 2.0 ** -24  # the record is fp32: its rounding plus the multiply, add and divide (fp64 sums: n 2^-53)

NORM_CASES = {"one4": (4,), "C-4": (C - 4,), "C": (C,), "C+4": (C + 4,), "three": (8, 3 * C + 4, 132),
              "chunks>T": ((T + 1) * C + 4,)}


def _place(host_segments):
    """The segments as 16-byte aligned views of ONE device buffer whose gaps (4 floats in front of, between and behind
    them) hold NaN: a chunk that reads past its segment's end shows it."""
    total = 4 + sum(s.numel() + 4 for s in host_segments)
    buf = torch.full((total,), float("nan"), dtype=F32, device=DEV)
    views, o = [], 4
    for s in host_segments:
        v = buf[o:o + s.numel()]
        v.copy_(s)
        views.append(v)
        o += s.numel() + 4
    return buf, views


@functools.lru_cache(maxsize=None)
def norm_case(name):
    host = [R.norm_inputs(n, 30000 + 17 * i + n % 1000) for i, n in enumerate(NORM_CASES[name])]
    ref = math.sqrt(sum(float((h.numpy().astype(np.float64) ** 2).sum()) for h in host))
    return host, ref


def _record():
    return torch.zeros(K.CLIP_REC_FLOATS, dtype=F32, device=DEV)


def _rel(got, want):
    return abs(float(got) - want) / abs(want)


@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
@pytest.mark.parametrize("name", list(NORM_CASES))
def test_grad_norm_and_clip_coefficient(name, grad_scale):
    host, ref = norm_case(name)
    buf, views = _place(host)
    segs = K.NormSegments(views)
    assert segs.nchunks == sum((n + C - 1) // C for n in NORM_CASES[name])
    want_total = grad_scale * ref
    max_norm = f32(0.5 * want_total)  # clips: coef ~ 0.5
    want_coef = min(1.0, max_norm / (want_total + f32(R.CLIP_EPS)))
    assert 0.2 <= want_coef <= 0.8
    runs = []
    for _ in range(2):  # the same launch twice: equal bits
        rec = _record()
        segs.partials.fill_(float("nan"))
        K.grad_sqnorm(segs)
        K.clip_finalize(segs, grad_scale, max_norm, rec)
        runs.append((segs.partials.cpu().clone(), rec.cpu().clone()))
    (pa, ra), (pb, rb) = runs
    assert torch.equal(pa.view(torch.int64), pb.view(torch.int64)) and torch.equal(ra.view(torch.int32), rb.view(torch.int32))
    assert bool(torch.isfinite(pa).all())
    e_t, e_c = _rel(ra[K.CLIP_TOTAL_NORM], want_total), _rel(ra[K.CLIP_COEF], want_coef)
    print(f"norm[{name} gs{grad_scale}] total {float(ra[0]):.6e} rel {e_t:.2e}; coef {float(ra[1]):.6f} rel {e_c:.2e}")
    assert e_t <= REL and e_c <= REL
    # one partial per chunk, each the sum of squares of its own chunk (cut from the SEGMENT's start)
    c = 0
    for h in host:
        for o in range(0, h.numel(), C):
            w = float((h[o:o + C].numpy().astype(np.float64) ** 2).sum())
            assert abs(float(pa[c]) - w) <= 1e-12 * w, (name, c)
            c += 1
    assert ra[2:].tolist() == [1.0, float(ra[0]), float(ra[0]), 0.0, 0.0, 0.0]
    # far above the norm nothing is clipped: the coefficient is exactly 1
    K.clip_finalize(segs, grad_scale, 1e30, rec)
    assert float(rec[K.CLIP_COEF]) == 1.0


def test_norm_does_not_depend_on_where_the_segments_lie():
    """The same values as one segment and as the middle segment of three give that segment's partials bit for bit
    (chunks are cut relative to the segment's start, whatever precedes it)."""
    host, _ = norm_case("three")
    _, alone = _place([host[1]])
    _, views = _place(host)
    a, b = K.NormSegments(alone), K.NormSegments(views)
    K.grad_sqnorm(a)
    K.grad_sqnorm(b)
    assert torch.equal(a.partials.cpu().view(torch.int64), b.partials.cpu()[1:1 + a.nchunks].view(torch.int64))


def test_telemetry_counts_nonfinite_norms_apart():
    """mer.h: a non-finite norm counts in STEPS and NONFINITE and enters neither NORM_SUM nor NORM_MAX."""
    rec = _record()
    seen = []
    for i, plant in enumerate((None, float("inf"), None)):
        h = R.norm_inputs(C + 132, 31000 + i) * (1.0 + i)
        if plant is not None:
            h[C + 5] = plant
        _, views = _place([h])
        segs = K.NormSegments(views)
        K.grad_sqnorm(segs)
        K.clip_finalize(segs, 1.0, 1.0, rec)
        seen.append(rec.cpu().clone())
    t0, t1, t2 = (float(r[K.CLIP_TOTAL_NORM]) for r in seen)
    assert math.isfinite(t0) and math.isinf(t1) and math.isfinite(t2) and t2 > t0
    assert float(seen[1][K.CLIP_COEF]) == 0.0  # max_norm / inf, as torch
    last = seen[2]
    assert float(last[K.CLIP_STEPS]) == 3.0 and float(last[K.CLIP_NONFINITE]) == 1.0
    assert float(last[K.CLIP_NORM_SUM]) == float(np.float32(np.float32(t0) + np.float32(t2)))
    assert float(last[K.CLIP_NORM_MAX]) == max(t0, t2) and float(last[K.CLIP_TOTAL_NORM]) == t2
    assert seen[1][K.CLIP_NORM_SUM:K.CLIP_NORM_MAX + 1].tolist() == [t0, t0]  # untouched by the infinite step
    assert last[6:].tolist() == [0.0, 0.0]
    # a NaN norm gives a NaN coefficient (clip_grad_norm_ with error_if_nonfinite=False)
    h = R.norm_inputs(8, 31009)
    h[3] = float("nan")
    _, views = _place([h])
    segs = K.NormSegments(views)
    K.grad_sqnorm(segs)
    K.clip_finalize(segs, 1.0, 1.0, rec)
    assert math.isnan(float(rec[K.CLIP_TOTAL_NORM])) and math.isnan(float(rec[K.CLIP_COEF]))
    assert float(rec[K.CLIP_STEPS]) == 4.0 and float(rec[K.CLIP_NONFINITE]) == 2.0


# ---------------------------------------------------------------------------------------------------------
# adam_step_ex
# ---------------------------------------------------------------------------------------------------------
HP = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)
ADAM_N = [1, 3, 4, 7, 1027, 2_097_159]


@pytest.mark.parametrize("with_ema", [False, True])
@pytest.mark.parametrize("n", ADAM_N)
def test_adam_step_ex(n, with_ema):
    wd, grad_scale, coef, d = 0.01, 0.5, 0.37, 0.999
    p0, _, m0, v0 = kp.adam_inputs(n, 41000 + n)
    e0 = p0 + 0.1 * randn(gen(41500 + n), n)
    keys = ("p", "m", "v") + (("e",) if with_ema else ())
    init = {"p": p0, "m": m0, "v": v0, "e": e0}
    state = {dt: {k: init[k].to(dt) for k in keys} for dt in (F64, F32)}
    dev = {k: guarded_flat((n,), DEV, init=init[k], offset=4) for k in keys}
    coef_dev = torch.tensor([coef], dtype=F32, device=DEV)
    for step in (1, 2, 3, 1000):  # the references carry their own state, as the kernel does
        grad = kp.adam_inputs(n, 41700 + n + step)[1]
        for dt in (F64, F32):
            s = state[dt]
            state[dt] = R.ref_adam_ex(s["p"], grad, s["m"], s["v"], s.get("e"), HP["lr"], HP["b1"], HP["b2"], HP["eps"],
                                      wd, step, grad_scale, coef, d, dt)
        K.adam_step_ex(dev["p"].view, grad.to(DEV), dev["m"].view, dev["v"].view, HP["lr"], HP["b1"], HP["b2"],
                       HP["eps"], wd, step, grad_scale=grad_scale, coef=coef_dev,
                       ema=dev["e"].view if with_ema else None, ema_decay=d)
        for k, t in dev.items():
            t.check(f"adam_step_ex {k}")
        for k in keys:
            assert_fp64_parity(dev[k].view, state[F64][k], state[F32][k],
                               what=f"adam_step_ex[n{n} ema{int(with_ema)} step{step}] {k}")
    assert float(coef_dev) == f32(coef)  # read, never written


@pytest.mark.parametrize("n", ADAM_N)
def test_adam_step_ex_with_unit_coefficient_is_adam_step_bit_for_bit(n):
    wd, grad_scale = 0.01, 0.5
    p0, _, m0, v0 = kp.adam_inputs(n, 42000 + n)
    a = {k: guarded_flat((n,), DEV, init=t, offset=4) for k, t in (("p", p0), ("m", m0), ("v", v0))}
    b = {k: guarded_flat((n,), DEV, init=t, offset=4) for k, t in (("p", p0), ("m", m0), ("v", v0))}
    c = {k: guarded_flat((n,), DEV, init=t, offset=4) for k, t in (("p", p0), ("m", m0), ("v", v0))}
    one = torch.ones(1, dtype=F32, device=DEV)
    for step in (1, 2, 1000):
        grad = kp.adam_inputs(n, 42500 + n + step)[1].to(DEV)
        args = (HP["lr"], HP["b1"], HP["b2"], HP["eps"], wd, step)
        K.adam_step(a["p"].view, grad, a["m"].view, a["v"].view, *args, grad_scale=grad_scale)
        K.adam_step_ex(b["p"].view, grad, b["m"].view, b["v"].view, *args, grad_scale=grad_scale, coef=one)
        K.adam_step_ex(c["p"].view, grad, c["m"].view, c["v"].view, *args, grad_scale=grad_scale, coef=None)
        for k in ("p", "m", "v"):
            want = a[k].buf.cpu().view(torch.int32)
            assert torch.equal(b[k].buf.cpu().view(torch.int32), want), (n, step, k)
            assert torch.equal(c[k].buf.cpu().view(torch.int32), want), (n, step, k)


def test_adam_step_ex_rejects_a_misaligned_view():
    n = 8
    buf = [torch.zeros(n + 1, device=DEV) for _ in range(5)]
    hp = (1e-3, 0.9, 0.999, 1e-8, 0.0, 1)
    with pytest.raises(MerKernelError):
        K.adam_step_ex(buf[0][:n], buf[1][:n], buf[2][:n], buf[3][:n], *hp, ema=buf[4][1:], ema_decay=0.9)
    with pytest.raises(MerKernelError):
        K.adam_step_ex(buf[0][1:], buf[1][:n], buf[2][:n], buf[3][:n], *hp, ema=buf[4][:n], ema_decay=0.9)
    with pytest.raises(ValueError):
        K.adam_step_ex(buf[0][:n], buf[1][:n], buf[2][:n], buf[3][:n], *hp, ema=buf[4][:4], ema_decay=0.9)
    assert all(float(b.abs().max()) == 0.0 for b in buf)  # refused before any launch

"""The row, fold and weight-preparation kernels of the WavLM encoder and of its stage-2 backward (csrc/wavlm.hip,
csrc/wavlm_train.hip, mer_linear_wgrad of csrc/conv_wgrad.hip), each alone against a float64 restatement
(tests/kernel_parity.py) under the bars of DESIGN.md section 2, at the sizes where their 16-row blocks, 64-row tiles,
256-column tiles, vector / scalar paths and grid caps begin or end.  fp32 outputs: ``assert_fp64_parity``; bf16 outputs:
``assert_bf16_parity``; dropout: the exact mask; copies, casts and the transpose: equal bits.  Outputs live in guarded
buffers, strided inputs have NaN in their gaps.

Left to their own tests (tests/test_wavlm_gpu.py, tests/test_wavlm_train_gpu.py): the WavLM attention forward and
backward (P is rounded to bf16 inside the kernel, which an fp32 restatement does not describe), wavlm_conv0_gn_gelu
and wavlm_time_mask."""
import functools

import pytest
import torch

from multimodalemotionrecognition_amd import kernels as K
from tests import kernel_parity as kp
from tests.kernel_parity import (BASE, BF16, F32, F64, SITE, GuardedBf16, GuardedBf16Rows, assert_bf16_parity,
                                 assert_dropout_parity, assert_fp64_parity, gen, guarded_flat, guarded_rows,
                                 padded_input, padded_input_bf16, randn)

pytestmark = pytest.mark.gpu
DEV = "cuda"
LN_EPS = 1e-5


def rng_base():
    return torch.tensor([BASE], dtype=torch.int64, device=DEV)


def both(fn):
    return fn(F64), fn(F32)


def name(dt):
    return "bf16" if dt == BF16 else "fp32"


def cpu(t):
    return t.detach().cpu()


def parity(got, r64, r32, what, extra=0.0):
    got = cpu(got)
    if got.dtype == BF16:
        return assert_bf16_parity(got, r64, r32, extra=extra, what=what)
    return assert_fp64_parity(got, r64, r32, extra=extra, what=what)


def rows_in(t, dt, pad, offset=0):
    """``t`` [rows, cols] on the device as dtype ``dt`` with row stride cols + pad and NaN in the gaps."""
    if dt == BF16:
        return padded_input_bf16(t, t.shape[1] + pad, DEV, offset=offset)
    return padded_input(t, (t.shape[1] + pad, 1), DEV, offset=offset)


def rows_out(rows, cols, dt, pad, offset=None):
    if dt == BF16:
        return GuardedBf16Rows(rows, cols, cols + pad, DEV, offset=16 if offset is None else offset)
    return guarded_rows(rows, cols, cols + pad, DEV, offset=4 if offset is None else offset)


# ---------------------------------------------------------------------------------------------------------
# layernorm / layernorm_tr
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ln_inputs(rows, d, idt):
    g = gen(8000 + 13 * rows + d + (1 if idt == BF16 else 0))
    x = kp.bf16_values(g, rows, d, scale=2.0, shift=0.5) if idt == BF16 else randn(g, rows, d) * 2 + 0.5
    return x, randn(g, d) * 0.3 + 1, randn(g, d) * 0.3


@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("d", [70, 256, 768, 1024])  # 70: the scalar path
def test_layernorm(d, rows):
    for idt in (F32, BF16):
        x, gamma, beta = ln_inputs(rows, d, idt)
        r64, r32 = both(lambda dt: kp.ref_layernorm(x, gamma, beta, LN_EPS, None, 0.0, dt))
        for odt in (F32, BF16):
            y = rows_out(rows, d, odt, 8)
            K.layernorm(rows_in(x, idt, 8), gamma.to(DEV), beta.to(DEV), y.view, eps=LN_EPS)
            y.check(f"layernorm[{rows}x{d} {name(idt)}->{name(odt)}]")
            parity(y.view, r64["y"], r32["y"], f"layernorm[{rows}x{d} {name(idt)}->{name(odt)}] y")


@pytest.mark.parametrize("idt,odt", [(F32, F32), (BF16, BF16), (F32, BF16)])
def test_layernorm_unaligned_pointer_takes_the_scalar_path(idt, odt):
    """d = 256 with x or y one element off its vector alignment: the scalar path, held to the same bar."""
    rows, d = 5, 256
    x, gamma, beta = ln_inputs(rows, d, idt)
    r64, r32 = both(lambda dt: kp.ref_layernorm(x, gamma, beta, LN_EPS, None, 0.0, dt))
    for xoff, yoff in ((1, None), (0, 17 if odt == BF16 else 5)):
        y = rows_out(rows, d, odt, 8, offset=yoff)
        K.layernorm(rows_in(x, idt, 8, offset=xoff), gamma.to(DEV), beta.to(DEV), y.view, eps=LN_EPS)
        what = f"layernorm[{rows}x{d} {name(idt)}->{name(odt)} x+{xoff} y+{yoff}]"
        y.check(what)
        parity(y.view, r64["y"], r32["y"], what + " y")


@pytest.mark.parametrize("d", [70, 256])
def test_layernorm_row_with_a_large_mean(d):
    """One row with mean 100 and spread 0.01: a one-pass variance would lose it."""
    g = gen(8100 + d)
    x = randn(g, 5, d)
    x[2] = 100 + 0.01 * randn(g, d)
    gamma, beta = randn(g, d) * 0.3 + 1, randn(g, d) * 0.3
    r64, r32 = both(lambda dt: kp.ref_layernorm(x, gamma, beta, LN_EPS, None, 0.0, dt))
    y = rows_out(5, d, F32, 4)
    K.layernorm(rows_in(x, F32, 4), gamma.to(DEV), beta.to(DEV), y.view, eps=LN_EPS)
    y.check(f"layernorm[mean 100, d {d}]")
    parity(y.view, r64["y"], r32["y"], f"layernorm[mean 100, d {d}] y")
    parity(y.view[2:3], r64["y"][2:3], r32["y"][2:3], f"layernorm[mean 100, d {d}] that row")


@pytest.mark.parametrize("d", [70, 256, 768])
def test_layernorm_output_dropout_and_skip(d):
    rows, p = 5, 0.1
    keep = kp.keep_mask_pair(BASE, SITE, kp.grid_index(rows, d), p)
    for idt, odt in ((F32, F32), (BF16, BF16)):
        x, gamma, beta = ln_inputs(rows, d, idt)
        r64, r32 = both(lambda dt: kp.ref_layernorm(x, gamma, beta, LN_EPS, keep, p, dt))
        y = rows_out(rows, d, odt, 8)
        K.layernorm(rows_in(x, idt, 8), gamma.to(DEV), beta.to(DEV), y.view, eps=LN_EPS, drop_p=p, rng=rng_base(),
                    site=SITE)
        what = f"layernorm_tr[{rows}x{d} {name(idt)}->{name(odt)} p{p}]"
        y.check(what)
        assert_dropout_parity(cpu(y.view), keep, p, r64["y"], r32["y"], what=what + " y")
        # LayerDrop: bit 3 of the mask set -> nothing written; bit 2 clear -> the bits of a call without a mask
        mask = torch.tensor([1 << 3], dtype=torch.int64, device=DEV)
        s = GuardedBf16Rows(rows, d, d + 8, DEV)
        K.layernorm(rows_in(x, idt, 8), gamma.to(DEV), beta.to(DEV), s.view, eps=LN_EPS, skip=mask, skip_bit=3)
        s.check(what + " skipped", written=False)
        K.layernorm(rows_in(x, idt, 8), gamma.to(DEV), beta.to(DEV), s.view, eps=LN_EPS, skip=mask, skip_bit=2)
        s.check(what + " not skipped")
        plain = GuardedBf16Rows(rows, d, d + 8, DEV)
        K.layernorm(rows_in(x, idt, 8), gamma.to(DEV), beta.to(DEV), plain.view, eps=LN_EPS)
        assert torch.equal(cpu(s.view), cpu(plain.view))


# ---------------------------------------------------------------------------------------------------------
# ln_bwd and ln_bwd_fold
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 16, 17, 37])
@pytest.mark.parametrize("d", [256, 768, 1024])
def test_ln_bwd(d, rows):
    g = gen(8200 + 7 * rows + d)
    x, gamma = randn(g, rows, d) * 2 + 0.5, randn(g, d) * 0.3 + 1
    dys = [randn(g, rows, d) for _ in range(3)]
    acc0 = [randn(g, d) for _ in range(3)]
    nblk = (rows + 15) // 16
    for n_dy, outs in ((1, "both"), (3, "dx32"), (2, "dx16"), (3, "both")):
        use = dys[:n_dy]
        r64, r32 = both(lambda dt: kp.ref_ln_bwd(use, x, gamma, LN_EPS, dt))
        dx32 = guarded_flat((rows, d), DEV, offset=4) if outs in ("both", "dx32") else None
        dx16 = GuardedBf16((rows, d), DEV) if outs in ("both", "dx16") else None
        dev = [t.to(DEV) for t in use] + [None] * (3 - n_dy)
        part = K.ln_bwd(dev[0], x.to(DEV), gamma.to(DEV), LN_EPS, dy_b=dev[1], dy_c=dev[2],
                        dx32=dx32.view if dx32 else None, dx16=dx16.view if dx16 else None)
        what = f"ln_bwd[{rows}x{d} dy{n_dy} {outs}]"
        if dx32:
            dx32.check(what)
            parity(dx32.view, r64["dx"], r32["dx"], what + " dx32")
        if dx16:
            dx16.check(what)
            parity(dx16.view, r64["dx"], r32["dx"], what + " dx16")
        # every partial row against the restatement over its own 16 rows
        got = cpu(part[:nblk * 3 * d]).reshape(nblk, 3, d)
        for q, key in enumerate(("dgamma", "dbeta", "sum dx")):
            parity(got[:, q], r64["part"][:, q], r32["part"][:, q], f"{what} part {key}")
        # then the fold into accumulators that start non-zero
        accs = [guarded_flat((d,), DEV, init=a, offset=4) for a in acc0]
        K.ln_bwd_fold(part, rows, d, dgamma=accs[0].view, dbeta=accs[1].view, dbias=accs[2].view)
        for q, key in enumerate(("dgamma", "dbeta", "dbias")):
            accs[q].check(f"{what} fold {key}")
            f64 = kp.ref_fold_rows(r64["part"][:, q], acc0[q], F64)["out"]
            parity(accs[q].view, f64, kp.ref_fold_rows(r32["part"][:, q], acc0[q], F32)["out"], f"{what} fold {key}")


# ---------------------------------------------------------------------------------------------------------
# fold_rows (two stages past 64 parts), colsum_into
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parts", [1, 3, 4, 5, 64, 65, 130, 4100])  # 65: S = 2; 4100: S = 64, chunk 65
def test_fold_rows(parts):
    for n in (1, 63, 64, 65, 257):
        g = gen(8300 + parts + n)
        part, out0 = randn(g, parts, n), randn(g, n)
        ldp, offset = n + 3, 5
        buf = torch.full((offset + parts * ldp + 4,), float("nan"), dtype=F32, device=DEV)
        buf.as_strided((parts, n), (ldp, 1), offset).copy_(part.to(DEV))
        out = guarded_flat((n,), DEV, init=out0, offset=4)
        K.fold_rows(buf, parts, n, ldp, out.view, offset=offset)
        out.check(f"fold_rows[{parts}x{n}]")
        r64, r32 = both(lambda dt: kp.ref_fold_rows(part, out0, dt))
        parity(out.view, r64["out"], r32["out"], f"fold_rows[{parts}x{n}] out")


def sixteenths(g, rows, cols):
    """bf16 values that are multiples of 1/16 below 8: any fp32 summation order of a few hundred of them is exact, so a
    kernel that sums them must return the exact sum (the bar is then the one-ulp floor alone)."""
    return (torch.round(randn(g, rows, cols) * 16).clamp(-127, 127) / 16).to(F32)


@pytest.mark.parametrize("rows", [1, 63, 64, 65, 129])
@pytest.mark.parametrize("idt", [F32, BF16], ids=name)
def test_colsum_into(idt, rows):
    for cols in (1, 255, 256, 257):
        g = gen(8400 + rows + cols)
        x = sixteenths(g, rows, cols) if idt == BF16 else randn(g, rows, cols)
        xd = rows_in(x, idt, 8 if idt == BF16 else 3)
        windows = [(0, cols)] + ([(cols // 3, cols - cols // 3 - 1)] if cols > 2 else [])
        for col0, ncols in windows:
            out0 = randn(g, ncols)
            out = guarded_flat((ncols,), DEV, init=out0, offset=4)
            K.colsum_into(xd, out.view, col0=col0, ncols=ncols)
            what = f"colsum_into[{rows}x{cols} {name(idt)} cols {col0}+{ncols}]"
            out.check(what)
            r64, r32 = both(lambda dt: kp.ref_colsum(x[:, col0:col0 + ncols], out0, dt))
            parity(out.view, r64["out"], r32["out"], what + " out")


# ---------------------------------------------------------------------------------------------------------
# gelu_bf16, gelu_bwd
# ---------------------------------------------------------------------------------------------------------
def gelu_input(rows, cols, seed):
    return kp.to_bf16(kp.gelu_z(rows, cols, seed)).to(F32)


@pytest.mark.parametrize("n", [8, 8 * 257])
def test_gelu_bf16(n):
    z = gelu_input(1, n, 8500 + n).reshape(n)
    f = GuardedBf16((n,), DEV)
    K.gelu_bf16(z.to(BF16).to(DEV), f.view)
    f.check(f"gelu_bf16[{n}]")
    r64, r32 = both(lambda dt: kp.ref_gelu(z, dt))
    parity(f.view, r64["f"], r32["f"], f"gelu_bf16[{n}] f", extra=0.5 * float(z.abs().max()) * kp.ERF_FAST_ABS)


@pytest.mark.parametrize("rows,cols", [(1, 8), (64, 256), (65, 264)])
def test_gelu_bwd(rows, cols):
    """erf_fast enters gelu'(z) through the cdf, 0.5 * 1.5e-7, times |df|; a column sum adds it once per row."""
    g = gen(8600 + rows + cols)
    z, db0 = gelu_input(rows, cols, 8600 + rows), randn(g, cols)
    df = torch.rand(rows, cols, generator=g, dtype=F32) * 2 - 1  # |df| <= 1 keeps the bar, and with it tol, small
    dz, dbias = GuardedBf16((rows, cols), DEV), guarded_flat((cols,), DEV, init=db0, offset=4)
    K.gelu_bwd(df.to(DEV), z.to(BF16).to(DEV), dz.view, dbias.view)
    dz.check(f"gelu_bwd[{rows}x{cols}]")
    dbias.check(f"gelu_bwd[{rows}x{cols}]")
    r64, r32 = both(lambda dt: kp.ref_gelu_bwd(df, z, db0, dt))
    extra = 0.5 * kp.ERF_FAST_ABS * float(df.abs().max())
    parity(dz.view, r64["dz"], r32["dz"], f"gelu_bwd[{rows}x{cols}] dz", extra=extra)
    parity(dbias.view, r64["dbias"], r32["dbias"], f"gelu_bwd[{rows}x{cols}] dbias", extra=rows * extra)


# ---------------------------------------------------------------------------------------------------------
# dropout_rows
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("idt", [F32, BF16], ids=name)
def test_dropout_rows(idt, p):
    rows, cols = 37, 264
    g = gen(8700 + (1 if idt == BF16 else 0))
    x = kp.bf16_values(g, rows, cols) if idt == BF16 else randn(g, rows, cols)
    keep = kp.keep_mask_pair(BASE, SITE, kp.grid_index(rows, cols), p)
    r64, r32 = both(lambda dt: kp.ref_dropout_rows(x, keep, p, dt))
    rng = rng_base() if p > 0 else None
    for outs in ("y32", "y16", "both", "in place"):
        what = f"dropout_rows[{rows}x{cols} {name(idt)} p{p} {outs}]"
        xd = rows_in(x, idt, 8)
        if outs == "in place":
            y = rows_out(rows, cols, idt, 8)
            y.view.copy_(xd)
            K.dropout_rows(y.view, p, rng, SITE, **{"y32" if idt == F32 else "y16": y.view})
            got = [y]
        else:
            y32 = rows_out(rows, cols, F32, 4) if outs in ("y32", "both") else None
            y16 = rows_out(rows, cols, BF16, 8) if outs in ("y16", "both") else None
            K.dropout_rows(xd, p, rng, SITE, y32=y32.view if y32 else None, y16=y16.view if y16 else None)
            got = [o for o in (y32, y16) if o is not None]
        for o in got:
            o.check(what)
            assert_dropout_parity(cpu(o.view), keep, p, r64["y"], r32["y"], what=f"{what} {name(o.view.dtype)}")


def test_dropout_rows_grid_stride_second_pass():
    """rows * cols / 8 > 4096 * 256 threads: the grid-stride loop takes a second pass."""
    rows, cols, p = 1032, 8136, 0.1
    assert rows * cols // 8 > 4096 * 256
    x = kp.bf16_values(gen(8800), rows, cols)
    keep = kp.keep_mask_pair(BASE, SITE, kp.grid_index(rows, cols), p)
    y = GuardedBf16((rows, cols), DEV)
    K.dropout_rows(x.to(BF16).to(DEV), p, rng_base(), SITE, y16=y.view)
    y.check("dropout_rows[second pass]")
    r64, r32 = both(lambda dt: kp.ref_dropout_rows(x, keep, p, dt))
    assert_dropout_parity(cpu(y.view), keep, p, r64["y"], r32["y"], what="dropout_rows[second pass] y16")


# ---------------------------------------------------------------------------------------------------------
# transpose_bf16
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 130])
def test_transpose_bf16(rows):
    for cols in (1, 63, 64, 65, 130):
        x = kp.bf16_values(gen(8900 + rows + cols), rows, cols)
        dst = GuardedBf16Rows(cols, rows, rows + 3, DEV, offset=5)
        K.transpose_bf16(padded_input_bf16(x, cols + 5, DEV, offset=3), dst.view)
        dst.check(f"transpose_bf16[{rows}x{cols}]")
        assert torch.equal(cpu(dst.view).to(F32), x.t()), f"transpose_bf16[{rows}x{cols}]"


# ---------------------------------------------------------------------------------------------------------
# linear_wgrad
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 37, 1027, 2051])  # splits 1, 1, 2, 4
@pytest.mark.parametrize("N,Kin", [(8, 8), (72, 136), (136, 264)])
def test_linear_wgrad(N, Kin, M):
    for col0 in (0, 8):
        g = gen(9000 + M + N + col0)
        ldy = col0 + N + 8
        x, dy, dw0 = kp.bf16_values(g, M, Kin), kp.bf16_values(g, M, col0 + N), randn(g, N, Kin)
        dw = guarded_flat((N, Kin), DEV, init=dw0, offset=4)
        dyd = padded_input_bf16(dy, ldy, DEV)
        K.linear_wgrad(x.to(BF16).to(DEV), dyd, dw.view, col0=col0)
        what = f"linear_wgrad[M{M} N{N} K{Kin} col0 {col0}]"
        dw.check(what)
        r64, r32 = both(lambda dt: kp.ref_linear_wgrad(x, dy, dw0, col0, N, dt))
        parity(dw.view, r64["dw"], r32["dw"], what + " dw")


# ---------------------------------------------------------------------------------------------------------
# weight preparation: permute3_bf16, cast_bf16, bf16_convert (equal bits), weightnorm_scale
# ---------------------------------------------------------------------------------------------------------
SPECIALS = [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 2.0 ** -8 + 2.0 ** -23, 1 + 2.0 ** -8 - 2.0 ** -24,
            3.3895313892515355e38, 3.4e38, -3.4e38, float("inf"), float("-inf"), float("nan"), 0.0, -0.0, 2.0 ** -120]


def with_specials(t):
    """Ties (to even, both ways), the top binade (overflow to inf), inf, NaN and signed zeros among the values."""
    flat = t.reshape(-1)
    k = min(len(SPECIALS), flat.numel())
    flat[:k] = torch.tensor(SPECIALS[:k], dtype=F32)
    return t


def same_bf16(got, want):
    """Equal values with NaN where NaN is wanted (a NaN's payload is not part of the contract) and equal zero signs."""
    got, want = cpu(got).to(F32).reshape(-1), want.to(F32).reshape(-1)
    nan = torch.isnan(want)
    return bool((torch.isnan(got) == nan).all()) and torch.equal(got[~nan], want[~nan]) and \
        torch.equal(torch.signbit(got[~nan]), torch.signbit(want[~nan]))


def pads_untouched(g):
    """GuardedBf16.check would take a NaN the kernel must produce for an element never written: the pads alone."""
    b = cpu(g.buf)
    return bool(torch.isnan(b[:g.pad]).all()) and bool(torch.isnan(b[g.pad + g.n:]).all())


@pytest.mark.parametrize("n", [1, 1027, 8192 * 256 + 1027])  # the last: past the 8192-block grid cap
def test_cast_bf16(n):
    x = with_specials(randn(gen(9100 + n), n))
    y = GuardedBf16((n,), DEV)
    K.cast_bf16(x.to(DEV), y.view)
    assert pads_untouched(y), "cast_bf16 wrote outside its output"
    assert same_bf16(y.view, x.to(BF16)), f"cast_bf16[{n}]"


@pytest.mark.parametrize("shape", [(5, 3, 7), (129, 125, 131)], ids=str)  # the second: past the 8192-block grid cap
@pytest.mark.parametrize("scaled", [False, True])
def test_permute3_bf16(scaled, shape):
    """Conv1d weight [Cout][Cin][k] -> [Cout][k][Cin], optionally times the weight-norm scale of tap k."""
    Cout, k, Cin = shape
    g = gen(9200 + Cout)
    src = with_specials(randn(g, Cout, Cin, k))
    scale = (randn(g, k) * 0.5 + 1) if scaled else None
    n = Cout * k * Cin
    assert (n > 8192 * 256) == (Cout == 129)
    dst = GuardedBf16((Cout, k, Cin), DEV)
    K.permute3_bf16(src.to(DEV), (Cout, k, Cin), (Cin * k, 1, k), dst.view, scale=scale.to(DEV) if scaled else None)
    assert pads_untouched(dst), "permute3_bf16 wrote outside its output"
    want = src.permute(0, 2, 1)
    want = (want * scale[None, :, None]) if scaled else want
    assert same_bf16(dst.view, want.contiguous().to(BF16)), f"permute3_bf16[{shape} scaled {scaled}]"


@pytest.mark.parametrize("odt", [F32, BF16], ids=name)
@pytest.mark.parametrize("n", [1, 1027, 4096 * 256 + 777])  # the last: past the 4096-block grid cap
def test_bf16_convert(n, odt):
    x = with_specials(randn(gen(9300 + n), n)).to(BF16)
    y = GuardedBf16((n,), DEV) if odt == BF16 else guarded_flat((n,), DEV, offset=4)
    K.bf16_convert(x.to(DEV), y.view)
    if odt == BF16:
        assert pads_untouched(y), "bf16_convert wrote outside its output"
    else:
        y.check(f"bf16_convert[{n}]")
    assert same_bf16(y.view, x), f"bf16_convert[{n} -> {name(odt)}]"


@pytest.mark.parametrize("taps", [1, 5])
@pytest.mark.parametrize("n01", [1, 255, 256, 257, 768])
def test_weightnorm_scale(n01, taps):
    g = gen(9400 + n01 + taps)
    v, gain = randn(g, 1, n01, taps), randn(g, taps)
    scale = guarded_flat((taps,), DEV, offset=4)
    K.weightnorm_scale(v.to(DEV), gain.to(DEV), scale.view)
    scale.check(f"weightnorm_scale[{n01}x{taps}]")
    r64, r32 = both(lambda dt: kp.ref_weightnorm_scale(v, gain, dt))
    parity(scale.view, r64["scale"], r32["scale"], f"weightnorm_scale[{n01}x{taps}] scale")

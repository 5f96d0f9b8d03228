"""csrc/gemm_bf16.hip against float64: every variant and every epilogue form of the bf16 MFMA GEMM, its Conv1d rows
mode, its train-mode dropout / LayerDrop and the grouped positional conv, each compared with a plain restatement
(tests/kernel_parity.py) under the bars of DESIGN.md section 2: fp32 outputs by ``assert_fp64_parity``, bf16 outputs by
``assert_bf16_parity`` (no bf16 tolerance: the reference's interval is rounded), dropout by the exact mask.  Outputs
live in guarded buffers, strided operands have NaN in their gaps.  A GELU epilogue adds the documented error of erf_fast,
0.5 max|z| 1.5e-7 (scaled by 1 / (1 - p) under dropout), as tests/test_head_kernels_gpu.py does.

The six epilogue forms and how a call reaches them:
  register-staged direct        variant 0 (and every variant when K % 64 != 0)
  pipelined direct              variant 9 with the 16-byte epilogue off (N % 8 != 0, or ldc / the C pointer unaligned)
  pipelined 16-byte through LDS variant 9 / 13 / 18 / 22 with N, ldc, ldr multiples of 8
  operand-swapped direct        variant 23 with the 16-byte epilogue off
  operand-swapped fp32-staged   variant 23, 16-byte epilogue, an fp32 output or a residual or dropout
  operand-swapped bf16-staged   variant 23, 16-byte epilogue, a bf16 output without residual and dropout
"""
import functools
import math

import pytest
import torch

from multimodalemotionrecognition_amd import kernels as K
from multimodalemotionrecognition_amd._lib import LIB, MerKernelError
from tests import kernel_parity as kp
from tests.kernel_parity import (BASE, BF16, F32, F64, SITE, GuardedBf16, GuardedBf16Rows, Guarded, assert_bf16_parity,
                                 assert_dropout_parity, assert_fp64_parity, gen, guarded_flat, padded_input_bf16)

pytestmark = pytest.mark.gpu
DEV = "cuda"

VARIANTS = (-2, -1, 0, 7, 9, 13, 18, 22, 23)
PIPELINED = (7, 9, 13, 18, 22, 23, -1, -2)
# (M, N, K): the smallest shapes that reach each edge
SHAPES = [(1, 8, 64),          # single row, single K-tile, ring prologue only
          (257, 136, 192),     # one row past a 256 tile (clamped rows), N % 8 == 0, 3 K-tiles = the A ring's depth
          (300, 130, 320),     # N % 8 != 0: direct epilogues; 5 K-tiles: the rings wrap
          (261, 1040, 128),    # N > 1024: tgroup 8 with a partial last band, tiles % 8 != 0; 2 K-tiles < ring depth
          (130, 72, 2048),     # deep K; -1 picks v7
          (100, 130, 72)]      # K % 64 != 0: every variant falls back to the register-staged kernel
VEC, NOVEC = (257, 136, 192), (300, 130, 320)
# every pair of (act, bias, residual, output dtype) values occurs in one of these six
PAIRWISE = [("none", True, True, F32), ("none", False, False, BF16), ("relu", True, False, F32),
            ("relu", False, True, BF16), ("gelu", True, False, BF16), ("gelu", False, True, F32)]
FULL = [(a, b, r, o) for a in ("none", "relu", "gelu") for b in (False, True) for r in (False, True)
        for o in (F32, BF16)]


def rng_base():
    return torch.tensor([BASE], dtype=torch.int64, device=DEV)


@functools.lru_cache(maxsize=None)
def inputs(M, N, Kd):
    return kp.gemm_bf16_inputs(M, N, Kd, 7000 + M + 3 * N + 5 * Kd)


@functools.lru_cache(maxsize=None)
def refs(M, N, Kd, act, bias, res, p=0.0):
    """(float64, float32) restatements and the keep mask of one call; computed once, shared, never modified."""
    i = inputs(M, N, Kd)
    keep = kp.keep_mask_pair(BASE, SITE, kp.grid_index(M, N), p) if p > 0 else None
    both = tuple(kp.ref_gemm_bf16(i["a"], i["w"], i["bias"] if bias else None, i["res"] if res else None, act, keep, p,
                                  dt) for dt in (F64, F32))
    return both[0], both[1], keep


def gelu_extra(act, z64, p=0.0):
    return 0.5 * float(z64.abs().max()) * kp.ERF_FAST_ABS / (1.0 - kp.f32(p)) if act == "gelu" else 0.0


def out_buffer(M, N, odt, ldc=None, offset=None):
    """A guarded output: contiguous (ldc None) or with row stride ldc > N; ``offset`` elements into its buffer (default:
    16-byte aligned)."""
    if odt == BF16:
        if ldc is None and offset is None:
            return GuardedBf16((M, N), DEV)
        return GuardedBf16Rows(M, N, ldc if ldc is not None else N + 8, DEV, offset=16 if offset is None else offset)
    if ldc is None and offset is None:
        return guarded_flat((M, N), DEV, offset=4)
    return Guarded((M, N), (ldc if ldc is not None else N + 8, 1), DEV, offset=4 if offset is None else offset)


def run_gemm(i, variant, act, bias, res, odt, *, M=None, Kd=None, rows=None, lda=None, ldw=None, ldr=None, ldc=None,
             c_offset=None, p=0.0, skip=None, skip_bit=0, out=None):
    """One launch on NaN-gapped device operands into a guarded output, which is returned."""
    w = padded_input_bf16(i["w"], ldw or i["w"].shape[1], DEV)
    N = w.shape[0]
    if rows is None:
        a = padded_input_bf16(i["a"], lda or i["a"].shape[1], DEV)
        M = a.shape[0]
    else:
        a = padded_input_bf16(i["buf"].reshape(1, -1), i["buf"].numel(), DEV).reshape(-1)
    r = padded_input_bf16(i["res"], ldr or N, DEV) if res else None
    o = out_buffer(M, N, odt, ldc, c_offset) if out is None else out
    K.gemm_bf16(a, w, o.view, M=M, K=Kd, rows=rows, bias=i["bias"].to(DEV) if bias else None, residual=r, act=act,
                variant=variant, drop_p=p, rng=rng_base() if p > 0 else None, site=SITE, skip=skip, skip_bit=skip_bit)
    return o


def check(o, i, r64, r32, keep, act, res, p, what):
    """The guard, then the parity assertion that fits the output's dtype and the call's dropout."""
    o.check(what)
    got = o.view.detach().cpu()
    extra = gelu_extra(act, r64["z"], p)
    if p > 0 and not res:
        return assert_dropout_parity(got, keep, p, r64["out"], r32["out"], extra=extra, what=what)
    if p > 0:  # a dropped element is act(z) * 0 + residual: the residual's bits in either output dtype
        assert 0 < int((~keep).sum()) < keep.numel() // 4, what
        assert bool((got.to(F32)[~keep] == i["res"][~keep]).all()), f"{what}: a dropped element is not the residual"
    if got.dtype == BF16:
        return assert_bf16_parity(got, r64["out"], r32["out"], extra=extra, what=what)
    return assert_fp64_parity(got, r64["out"], r32["out"], extra=extra, what=what)


def name(odt):
    return "bf16" if odt == BF16 else "fp32"


def assert_same_bits(outs, base, others, what):
    want = outs[base].view.detach().cpu()
    for v in others:
        assert torch.equal(want, outs[v].view.detach().cpu()), f"{what}: variant {v} differs in bits from variant {base}"


# ---------------------------------------------------------------------------------------------------------
# every variant on every shape; all pipelined variants (and the register-staged one) give the same bits
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,Kd", SHAPES)
def test_every_variant_on_every_shape(M, N, Kd):
    i = inputs(M, N, Kd)
    for act, bias, res, odt in PAIRWISE:
        r64, r32, _ = refs(M, N, Kd, act, bias, res)
        outs = {}
        for v in VARIANTS:
            what = f"gemm_bf16[{M}x{N}x{Kd} v{v} {act} bias{int(bias)} res{int(res)} {name(odt)}]"
            outs[v] = run_gemm(i, v, act, bias, res, odt)
            check(outs[v], i, r64, r32, None, act, res, 0.0, what)
        # "All variants are bit-identical (same fragments, same k order)": plain rows have no K-tile permutation, so
        # the register-staged kernel is held to it too; with K % 64 != 0 every variant IS that kernel
        assert_same_bits(outs, 0, PIPELINED, f"gemm_bf16[{M}x{N}x{Kd} {act} res{int(res)} {name(odt)}]")


# ---------------------------------------------------------------------------------------------------------
# the six epilogue forms: act x bias x residual x output dtype
# ---------------------------------------------------------------------------------------------------------
FORMS = {"register-direct": (0, VEC), "pipelined-direct": (9, NOVEC), "pipelined-lds": (9, VEC),
         "swapped-direct": (23, NOVEC), "swapped-staged": (23, VEC)}  # the last: fp32- and bf16-staged


@pytest.mark.parametrize("form", sorted(FORMS))
def test_epilogue_forms(form):
    v, (M, N, Kd) = FORMS[form]
    i = inputs(M, N, Kd)
    for act, bias, res, odt in FULL:
        r64, r32, _ = refs(M, N, Kd, act, bias, res)
        what = f"gemm_bf16[{form} v{v} {act} bias{int(bias)} res{int(res)} {name(odt)}]"
        check(run_gemm(i, v, act, bias, res, odt), i, r64, r32, None, act, res, 0.0, what)


# ---------------------------------------------------------------------------------------------------------
# leading dimensions and alignment
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,Kd", [VEC, NOVEC])
def test_leading_dimensions_and_alignment(M, N, Kd):
    """lda / ldw / ldr / ldc wider than the logical width (16-byte epilogue still on where N allows); then an odd ldc
    and a C pointer one element off, which turn it off: the same bits as the aligned call."""
    i = inputs(M, N, Kd)
    for act, bias, res, odt in [("gelu", True, True, BF16), ("none", True, True, F32), ("relu", True, False, BF16),
                                ("gelu", False, True, F32)]:
        r64, r32, _ = refs(M, N, Kd, act, bias, res)
        for v in (0, 9, 13, 23, -1, -2):
            what = f"gemm_bf16[{M}x{N}x{Kd} v{v} {act} res{int(res)} {name(odt)}"
            plain = run_gemm(i, v, act, bias, res, odt)
            wide = run_gemm(i, v, act, bias, res, odt, lda=Kd + 8, ldw=Kd + 16, ldr=N + 8, ldc=N + 8)
            check(wide, i, r64, r32, None, act, res, 0.0, what + " wide ld]")
            odd = run_gemm(i, v, act, bias, res, odt, lda=Kd + 8, ldw=Kd + 16, ldr=N + 8, ldc=N + 3)
            check(odd, i, r64, r32, None, act, res, 0.0, what + " ldc N+3]")
            off = run_gemm(i, v, act, bias, res, odt, ldc=N + 8, c_offset=17 if odt == BF16 else 5)
            check(off, i, r64, r32, None, act, res, 0.0, what + " C off by one]")
            want = plain.view.detach().cpu()
            for o, how in ((wide, "wide ld"), (odd, "ldc N+3"), (off, "C off by one")):
                assert torch.equal(want, o.view.detach().cpu()), f"{what} {how}]: bits differ from the contiguous call"


# ---------------------------------------------------------------------------------------------------------
# rows mode: channel-last Conv1d as a GEMM over overlapping windows of a flat buffer
# ---------------------------------------------------------------------------------------------------------
# name -> (C, k, s, Lin, N): K = k C, rstride = s C, 3 clips, gstride = Lin C, Lin odd
ROWS = {"k3s2c64": (64, 3, 2, 201, 136),     # K = 192, rstride = 128: kp_taps = 3, kp_c = 64
        "k3s2c128": (128, 3, 2, 201, 130),   # two channel blocks per tap
        "k2s2c64": (64, 2, 2, 201, 136),     # rstride == K: no permutation
        "k16s5c8": (8, 16, 5, 301, 72)}      # K = 128, rstride = 40: gcd 8, natural order


@functools.lru_cache(maxsize=None)
def rows_case(case):
    C, k, s, Lin, N = ROWS[case]
    Kd, Lout = k * C, (Lin - k) // s + 1
    g = gen(7100 + C + k)
    i = {"buf": kp.bf16_values(g, 3 * Lin * C), "w": kp.bf16_values(g, N, Kd, scale=0.8 / math.sqrt(Kd)),
         "bias": kp.randn(g, N) * 0.5, "res": kp.bf16_values(g, 3 * Lout, N)}
    rows = (Lout, s * C, Lin * C)
    i["a"] = kp.gather_rows(i["buf"], 3 * Lout, Kd, *rows)
    permuted = s * C < Kd and math.gcd(s * C, Kd) % 64 == 0 and Kd // math.gcd(s * C, Kd) > 1
    return i, 3 * Lout, N, Kd, rows, permuted


@pytest.mark.parametrize("case", sorted(ROWS))
def test_rows_mode(case):
    i, M, N, Kd, rows, permuted = rows_case(case)
    assert permuted == (case in ("k3s2c64", "k3s2c128"))
    for act, bias, res, odt in [("gelu", True, False, BF16), ("none", True, True, F32), ("none", False, False, BF16)]:
        r64, r32 = (kp.ref_gemm_bf16(i["a"], i["w"], i["bias"] if bias else None, i["res"] if res else None, act, None,
                                     0.0, dt) for dt in (F64, F32))
        outs = {}
        for v in VARIANTS:
            what = f"gemm_bf16 rows[{case} v{v} {act} res{int(res)} {name(odt)}]"
            outs[v] = run_gemm(i, v, act, bias, res, odt, M=M, Kd=Kd, rows=rows)
            check(outs[v], i, r64, r32, None, act, res, 0.0, what)
        # with the K-tile permutation the register-staged kernel walks K in another order: parity only
        assert_same_bits(outs, 9, [v for v in PIPELINED if v != 9] + ([] if permuted else [0]), f"rows[{case} {act}]")


# ---------------------------------------------------------------------------------------------------------
# dropout (exact mask) through every epilogue form that has a dropout line; LayerDrop
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", sorted(FORMS))
def test_dropout_through_every_epilogue_form(form):
    """With dropout variant 23 stages fp32 (its bf16-staged form is for calls without residual and dropout)."""
    v, (M, N, Kd) = FORMS[form]
    i, p = inputs(M, N, Kd), 0.1
    for act, bias, res, odt in [("gelu", True, False, F32), ("gelu", True, True, BF16), ("none", False, False, BF16),
                                ("relu", True, True, F32)]:
        r64, r32, keep = refs(M, N, Kd, act, bias, res, p)
        what = f"gemm_bf16 dropout[{form} v{v} {act} res{int(res)} {name(odt)}]"
        check(run_gemm(i, v, act, bias, res, odt, p=p), i, r64, r32, keep, act, res, p, what)


@pytest.mark.parametrize("v", [-2, -1, 7, 13, 18, 22])
def test_dropout_other_variants(v):
    M, N, Kd = VEC
    i, p = inputs(M, N, Kd), 0.1
    for act, bias, res, odt in [("gelu", True, True, BF16), ("none", True, False, F32)]:
        r64, r32, keep = refs(M, N, Kd, act, bias, res, p)
        check(run_gemm(i, v, act, bias, res, odt, p=p), i, r64, r32, keep, act, res, p,
              f"gemm_bf16 dropout[v{v} {act} res{int(res)} {name(odt)}]")


@pytest.mark.parametrize("v", [0, 9, 23])
def test_layerdrop_skip_bit(v):
    M, N, Kd = VEC
    i = inputs(M, N, Kd)
    mask = torch.tensor([1 << 5], dtype=torch.int64, device=DEV)
    for odt in (BF16, F32):
        o = run_gemm(i, v, "gelu", True, True, odt, ldc=N + 8, skip=mask, skip_bit=5)
        if odt == BF16:
            o.check(f"gemm_bf16 skip[v{v}]", written=False)
        else:
            o.check(f"gemm_bf16 skip[v{v}]")
            assert bool((o.view.detach().cpu() == kp.MARKER).all()), "a skipped launch wrote its fp32 output"
        # the bit beside it is clear: the launch runs and gives the bits of a call without a mask
        ran = run_gemm(i, v, "gelu", True, True, odt, skip=mask, skip_bit=4)
        ran.check(f"gemm_bf16 skip bit clear[v{v}]")
        assert torch.equal(ran.view.detach().cpu(), run_gemm(i, v, "gelu", True, True, odt).view.detach().cpu())


# ---------------------------------------------------------------------------------------------------------
# refusals: an error, and the guarded output unwritten
# ---------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_output_unwritten():
    M, N, Kd = 37, 24, 64
    i = kp.gemm_bf16_inputs(M, N, Kd, 7200)
    a, w = padded_input_bf16(i["a"], Kd + 8, DEV), padded_input_bf16(i["w"], Kd, DEV)
    o = GuardedBf16Rows(M, N, N + 8, DEV)
    raw = dict(W=w.data_ptr(), ldw=Kd, C=o.view.data_ptr(), ldc=N + 8)

    def ex(Kq, A, lda, variant):
        LIB("mer_gemm_bf16_ex", M, N, Kq, A, 0, lda, M, raw["W"], raw["ldw"], raw["C"], K.BF16, raw["ldc"], 0, 0, 0, 0,
            variant, K.stream_ptr())

    with pytest.raises(MerKernelError):  # K % 8 != 0
        ex(60, a.data_ptr(), Kd + 8, -1)
    with pytest.raises(MerKernelError):  # A two bytes off a 16-byte boundary
        ex(Kd, a.data_ptr() + 2, Kd + 8, -1)
    with pytest.raises((MerKernelError, ValueError)):  # the same through the wrapper
        K.gemm_bf16(a.as_strided((M, Kd - 8), (Kd + 8, 1), a.storage_offset() + 1), w[:, :Kd - 8], o.view)
    for variant in (1, 8, 21, 24, -3):  # unknown variants
        with pytest.raises(MerKernelError):
            ex(Kd, a.data_ptr(), Kd + 8, variant)
    for p in (1.0, 1.5, -0.1):  # drop_p outside [0, 1)
        with pytest.raises(MerKernelError):
            K.gemm_bf16(a, w, o.view, drop_p=p, rng=rng_base(), site=SITE, skip=None if p > 0 else
                        torch.zeros(1, dtype=torch.int64, device=DEV))
    torch.cuda.synchronize()
    o.check("gemm_bf16 refusals", written=False)
    K.gemm_bf16(a, w, o.view)  # and the same operands are accepted once the call is valid
    o.check("gemm_bf16 after the refusals")


# ---------------------------------------------------------------------------------------------------------
# grouped positional conv: strip kernel, gather GEMM, and the register-staged kernel in positional mode
# ---------------------------------------------------------------------------------------------------------
POSCONV = {"strip": (96, 2, 8, 4),        # K = 384: the Toeplitz strip kernel, two 192-wide weight chunks
           "register": (96, 2, 5, 2),     # K = 240, not a multiple of 64: the register-staged mode-1 kernel
           "production": (768, 16, 128, 64)}
POS_L = (1, 15, 16, 17, 37, 160, 161)     # 161 is past PS_MAXL: -1 must take the gather kernel
POS_CASES = [(c, L) for c in ("strip", "register") for L in POS_L] + [("production", 37)]
POS_B = 2


@functools.lru_cache(maxsize=None)
def posconv_case(case, L):
    C, G, taps, pad = POSCONV[case]
    return kp.posconv_inputs(POS_B, L, C, G, taps, 7300 + C + taps + L)


@functools.lru_cache(maxsize=None)
def posconv_refs(case, L, act, res):
    C, G, taps, pad = POSCONV[case]
    i = posconv_case(case, L)
    return tuple(kp.ref_posconv(i["x"], i["wp"], i["bias"], i["res"] if res else None, act, POS_B, L, C, G, taps, pad,
                                dt) for dt in (F64, F32))


@pytest.mark.parametrize("case,L", POS_CASES)
def test_posconv(case, L):
    C, G, taps, pad = POSCONV[case]
    i, M = posconv_case(case, L), POS_B * L
    wp = i["wp"].reshape(C, -1).to(BF16).to(DEV)
    for act, res, odt, padded in [("gelu", True, BF16, False), ("gelu", False, BF16, True), ("none", True, F32, True),
                                  ("relu", False, F32, False), ("none", False, BF16, False)]:
        r64, r32 = posconv_refs(case, L, act, res)
        r64 = {k: t.reshape(M, C) for k, t in r64.items()}
        r32 = {k: t.reshape(M, C) for k, t in r32.items()}
        x = padded_input_bf16(i["x"].reshape(M, C), C + 8 if padded else C, DEV)
        r = padded_input_bf16(i["res"].reshape(M, C), C + 16 if padded else C, DEV) if res else None
        outs = {}
        for v in (0, -1):
            what = f"posconv[{case} L{L} v{v} {act} res{int(res)} {name(odt)} {'padded' if padded else 'contiguous'}]"
            outs[v] = out_buffer(M, C, odt, ldc=C + 8 if padded else None)
            K.posconv_gemm_bf16(x, wp, outs[v].view, POS_B, L, C, G, taps, pad, i["bias"].to(DEV), r, act=act,
                                variant=v)
            check(outs[v], i, r64, r32, None, act, res, 0.0, what)
        assert_same_bits(outs, 0, [-1], f"posconv[{case} L{L} {act} res{int(res)} {name(odt)}]")


def test_posconv_refusals():
    C, G, taps, pad, L = 96, 2, 8, 4, 17
    i = posconv_case("strip", L)
    x, wp = i["x"].reshape(POS_B * L, C).to(BF16).to(DEV), i["wp"].reshape(C, -1).to(BF16).to(DEV)
    o = GuardedBf16((POS_B * L, C), DEV)
    for variant in (1, -2):
        with pytest.raises(MerKernelError):
            K.posconv_gemm_bf16(x, wp, o.view, POS_B, L, C, G, taps, pad, None, None, variant=variant)
    with pytest.raises(MerKernelError):  # 96 channels do not split into 5 groups
        K.posconv_gemm_bf16(x, wp, o.view, POS_B, L, C, 5, taps, pad, None, None)
    torch.cuda.synchronize()
    o.check("posconv refusals", written=False)

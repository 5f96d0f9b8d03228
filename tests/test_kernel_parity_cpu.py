"""The bars of tests/test_head_kernels_gpu.py and tests/test_bn_pool_kernels_gpu.py are sound: every float32
restatement is close to, and distinct from, its float64 reference, and ``assert_fp64_parity`` accepts the former and
rejects a 1e-4 perturbation of it.  ``assert_bf16_parity`` accepts bf16(ref32), rejects one bf16 step of a determined
element and anything outside the interval, and finds at least 90 % of every bf16 output determined.  The max pool's
restatement takes the first maximum; csrc/common.h ``fdiv``, emulated in float32, is exact below 2^22 and first wrong
at 2^23 + 7 for a divisor of 8.  For the bf16 GEMM and the WavLM row kernels (tests/test_gemm_bf16_parity_gpu.py,
tests/test_wavlm_rows_kernels_gpu.py) the faults a loose bar would let through are applied to the float32 restatement
and must be rejected: a dropped K chunk, swapped bias columns, the residual before the activation, dropout after the
residual, a truncating bf16 store, a shifted tap, an ``ln_bwd`` partial row over the wrong rows.  For the trunk
convolutions (tests/test_conv_kernels_gpu.py): the tap-sum restatements are torch's convolutions in float64, leave at
least 90 % of every bf16 output determined at every shape and form the GPU file runs, and the faults a relative-RMS bar
lets through are rejected -- a tap dropped at the border only, padding off by one pixel, ``mask >= 0`` at planted signed
zeros, the downsample gradient rounded before the add, a dropped K chunk of one tile, a truncating store, sums over
unrounded values, wgrad channels from the wrong offset, a dropped partial granule."""
import numpy as np
import pytest
import torch

from tests import kernel_parity as kp

NAMES = sorted(kp.INSTANCES)


@pytest.fixture(scope="module")
def evaluated():
    return {n: (kp.INSTANCES[n](kp.F64), kp.INSTANCES[n](kp.F32)) for n in NAMES}


@pytest.mark.parametrize("name", NAMES)
def test_restatement_bar_is_not_degenerate(name, evaluated):
    ref64, ref32 = evaluated[name]
    assert set(ref64) == set(ref32) and ref64
    for k in ref64:
        a, b = ref64[k], ref32[k]
        assert a.dtype == torch.float64 and b.dtype == torch.float32 and a.shape == b.shape, (name, k)
        top = float(a.abs().max())
        assert top > 0, (name, k)
        diff = float((b.double() - a).abs().max())
        assert diff <= 1e-5 * top, (name, k, diff, top)
        if k in kp.EXACT_OUTPUTS.get(name, ()):
            assert diff == 0, (name, k)
            continue
        assert diff > 0, f"{name}.{k}: the float32 restatement equals the float64 one, its bar would be zero"


@pytest.mark.parametrize("name", NAMES)
def test_assert_fp64_parity_accepts_ref32_and_rejects_a_perturbed_element(name, evaluated, capsys):
    ref64, ref32 = evaluated[name]
    for k in ref64:
        ratio = kp.assert_fp64_parity(ref32[k], ref64[k], ref32[k], what=f"{name}.{k}")
        assert ratio == (0.0 if k in kp.EXACT_OUTPUTS.get(name, ()) else pytest.approx(1.0))
        line = capsys.readouterr().out.strip().splitlines()[-1]
        assert f"{name}.{k}" in line and "err=" in line and "bar=" in line and "ratio=" in line
        bad = ref32[k].clone().reshape(-1)
        i = int(np.random.default_rng(len(k)).integers(bad.numel()))
        bad[i] += 1e-4 * float(ref64[k].abs().max())
        with pytest.raises(AssertionError):
            kp.assert_fp64_parity(bad.reshape(ref32[k].shape), ref64[k], ref32[k], what=f"{name}.{k} perturbed")


def test_extra_is_added_to_the_bound():
    ref64 = torch.tensor([1.0, 2.0], dtype=torch.float64)
    ref32 = ref64.float()
    got = ref32 + 1e-5
    with pytest.raises(AssertionError):
        kp.assert_fp64_parity(got, ref64, ref32)
    kp.assert_fp64_parity(got, ref64, ref32, extra=2e-5)


def test_dropout_parity_requires_the_exact_mask():
    keep = kp.keep_mask(kp.BASE, kp.SITE, np.arange(64), 0.3)
    assert 0 < int(keep.sum()) < 64
    x = torch.arange(1, 65, dtype=torch.float32)
    ref64, ref32 = kp.ref_dropout(x, keep, 0.3, kp.F64)["y"], kp.ref_dropout(x, keep, 0.3, kp.F32)["y"]
    kp.assert_dropout_parity(ref32, keep, 0.3, ref64, ref32)
    wrong = ref32.clone()
    wrong[int(keep.nonzero()[0])] = 0.0  # one kept element dropped
    with pytest.raises(AssertionError, match="zeros differ"):
        kp.assert_dropout_parity(wrong, keep, 0.3, ref64, ref32)
    assert bool(kp.keep_mask(kp.BASE, kp.SITE, np.arange(5), 0.0).all())


def test_guarded_view_detects_a_write_outside_it():
    g = kp.guarded_rows(3, 5, 8, "cpu", init=torch.zeros(3, 5))
    assert tuple(g.view.shape) == (3, 5) and g.view.stride() == (8, 1)
    g.view += 1.0
    g.check("inside writes")
    g.buf[3 + 5] = 0.0  # the first pad element of row 0
    with pytest.raises(AssertionError, match="outside the output view"):
        g.check("pad write")
    f = kp.guarded_flat((2, 3), "cpu")
    f.view.fill_(2.0)
    f.check()
    f.buf[-1] = kp.MARKER + 1
    with pytest.raises(AssertionError):
        f.check()


# ---- bfloat16 outputs: the interval rule of assert_bf16_parity ----
BF16_CASES = sorted((n, k) for n, ks in kp.BF16_OUTPUTS.items() for k in ks)


def _bf16_step(t, i, ulps):
    """t (bfloat16) with element i moved by ``ulps`` representable values away from zero (towards it if negative)."""
    bits = t.clone().reshape(-1).view(torch.int16)
    bits[i] += ulps
    return bits.view(torch.bfloat16).reshape(t.shape)


@pytest.mark.parametrize("name,key", BF16_CASES)
def test_assert_bf16_parity_on_every_bf16_output(name, key, evaluated, capsys):
    ref64, ref32 = evaluated[name][0][key], evaluated[name][1][key]
    got = kp.to_bf16(ref32)
    kp.assert_bf16_parity(got, ref64, ref32, what=f"{name}.{key}")  # includes the 90 % determined-share condition
    line = capsys.readouterr().out.strip().splitlines()[-1]
    assert f"{name}.{key}" in line and "err=" in line and "bar=" in line and "ratio=" in line
    lo, hi, tol = kp.bf16_interval(ref64, ref32)
    assert tol <= 1e-4 * float(ref64.abs().max())
    assert bool(((lo == hi) <= kp.bf16_determined(lo, hi, tol)).all())
    det = (lo == hi).reshape(-1).nonzero().reshape(-1)
    i = int(det[int(np.random.default_rng(len(name)).integers(det.numel()))])
    for ulps in (1, -1):  # one bf16 step of one determined element, either way
        with pytest.raises(AssertionError, match="outside the bf16 interval"):
            kp.assert_bf16_parity(_bf16_step(got, i, ulps), ref64, ref32, what=f"{name}.{key} one ulp")
    zeros = (ref64 == 0).reshape(-1).nonzero().reshape(-1)
    if zeros.numel():  # an exact zero is determined although lo < hi: it admits nothing beyond tol
        assert bool(kp.bf16_determined(lo, hi, tol).reshape(-1)[zeros].all())
        assert float(hi.reshape(-1)[zeros[0]]) <= 1.01 * tol
        bad = got.clone().reshape(-1)
        bad[int(zeros[0])] = 1.05 * tol
        with pytest.raises(AssertionError, match="outside the bf16 interval"):
            kp.assert_bf16_parity(bad.reshape(got.shape), ref64, ref32, what=f"{name}.{key} non-zero")
    for v in (float("nan"), float("inf")):
        bad = got.clone().reshape(-1)
        bad[i] = v
        with pytest.raises(AssertionError):
            kp.assert_bf16_parity(bad.reshape(got.shape), ref64, ref32, what=f"{name}.{key} {v}")


def test_assert_bf16_parity_at_a_rounding_boundary():
    """An element whose reference sits on a bf16 rounding boundary admits both neighbours and nothing beyond them; a
    tensor with too many such elements is refused as blind."""
    ref64 = torch.tensor([1.0 + 2.0 ** -8] + [1.001 + 2.0 ** -7 * k for k in range(19)], dtype=torch.float64)
    ref32 = (ref64 + 1e-7).float()  # bar ~ 1e-7: tol ~ 1.7e-6, far below the bf16 step 2^-7
    lo, hi, tol = kp.bf16_interval(ref64, ref32)
    assert 1e-6 < tol < 3e-6
    assert float(lo[0]) == 1.0 and float(hi[0]) == 1.0 + 2.0 ** -7 and bool((lo[1:] == hi[1:]).all())
    ok = kp.to_bf16(ref64)
    for v in (1.0, 1.0 + 2.0 ** -7):
        ok[0] = v
        kp.assert_bf16_parity(ok, ref64, ref32, what="boundary")
    for v in (1.0 - 2.0 ** -8, 1.0 + 2.0 ** -6):  # just outside: the next bf16 value on either side
        bad = ok.clone()
        bad[0] = v
        with pytest.raises(AssertionError, match="outside the bf16 interval"):
            kp.assert_bf16_parity(bad, ref64, ref32, what="boundary")
    with pytest.raises(AssertionError, match="blind"):
        kp.assert_bf16_parity(ok[:5], ref64[:5], ref32[:5], what="one in five undetermined")
    with pytest.raises(AssertionError, match="bfloat16"):
        kp.assert_bf16_parity(ok.float(), ref64, ref32, what="float32 output")
    # float64 -> bfloat16 goes through float32: the eps32 term of tol covers that step
    assert float(torch.tensor(1 + 2.0 ** -8 + 2.0 ** -30, dtype=torch.float64).to(torch.bfloat16)) == 1.0
    assert float(kp.to_bf16(torch.tensor(1 + 2.0 ** -8 + 2.0 ** -30, dtype=torch.float64))) == 1.0


def test_guarded_bf16_detects_unwritten_and_outside_writes():
    for dtype in (torch.bfloat16, torch.uint8):
        g = kp.GuardedBf16((2, 3), "cpu", dtype=dtype)
        g.check("refused call", written=False)
        g.view.fill_(1)
        g.check("written")
        with pytest.raises(AssertionError, match="must refuse"):
            g.check("refused call", written=False)
        g.buf[-1] = 0
        with pytest.raises(AssertionError, match="outside the output view"):
            g.check("tail write")
    g = kp.GuardedBf16((2, 3), "cpu")
    g.view[0].fill_(1.0)
    with pytest.raises(AssertionError, match="never written"):
        g.check("half written")


def test_guarded_bf16_rows_detects_pad_writes_and_unwritten_elements():
    g = kp.GuardedBf16Rows(3, 5, 8, "cpu")
    assert tuple(g.view.shape) == (3, 5) and g.view.stride() == (8, 1) and g.view.storage_offset() == 16
    g.check("refused call", written=False)
    with pytest.raises(AssertionError, match="never written"):
        g.check("nothing written")
    g.view[:2].fill_(1.0)
    with pytest.raises(AssertionError, match="never written"):
        g.check("last row missing")
    with pytest.raises(AssertionError, match="must leave it alone"):
        g.check("refused call", written=False)
    g.view.fill_(1.0)
    g.check("written")
    g.buf[16 + 5] = 0.0  # the first pad element of row 0
    with pytest.raises(AssertionError, match="outside the output view"):
        g.check("pad write")
    odd = kp.GuardedBf16Rows(2, 4, 7, "cpu", offset=17)
    assert odd.view.storage_offset() == 17
    odd.view.fill_(2.0)
    odd.check("odd offset")
    odd.buf[16] = 1.0
    with pytest.raises(AssertionError, match="outside the output view"):
        odd.check("write in front")


def test_padded_input_bf16_has_nan_gaps():
    t = kp.bf16_values(kp.gen(1), 3, 5)
    v = kp.padded_input_bf16(t, 8, "cpu", offset=8)
    assert v.dtype == torch.bfloat16 and v.stride() == (8, 1) and bool((v.float() == t).all())
    whole = v.as_strided((8 + 2 * 8 + 5 + 8,), (1,), 0).float()
    inside = torch.zeros(whole.numel(), dtype=torch.bool)
    inside[(8 + torch.arange(3)[:, None] * 8 + torch.arange(5)[None, :]).reshape(-1)] = True
    assert bool(torch.isnan(whole[~inside]).all()) and not bool(torch.isnan(whole[inside]).any())
    with pytest.raises(AssertionError, match="bf16-representable"):
        kp.padded_input_bf16(t + 2.0 ** -12, 8, "cpu")


def test_bf16_parity_extra_widens_tol_before_the_interval():
    ref64 = torch.tensor([1.0 + 2.0 ** -8 - 1e-5] + [1.001 + 2.0 ** -7 * k for k in range(19)], dtype=torch.float64)
    ref32 = (ref64 + 1e-7).float()
    up = kp.to_bf16(ref64)
    up[0] = 1.0 + 2.0 ** -7  # the boundary is 1e-5 above the reference: out of reach of tol ~ 1.7e-6 ...
    with pytest.raises(AssertionError, match="outside the bf16 interval"):
        kp.assert_bf16_parity(up, ref64, ref32, what="no extra")
    kp.assert_bf16_parity(up, ref64, ref32, what="extra", extra=2e-5)  # ... and within reach of tol + extra
    assert kp.bf16_interval(ref64, ref32, 2e-5)[2] == pytest.approx(kp.bf16_interval(ref64, ref32)[2] + 2e-5)


# ---- mutations of the float32 restatements that the GPU tests' assertions must reject ----
def _rejected_both_ways(bad32, ref64, ref32, what):
    """As an fp32 output (assert_fp64_parity) and as a correctly rounded bf16 output (assert_bf16_parity)."""
    with pytest.raises(AssertionError):
        kp.assert_fp64_parity(bad32, ref64, ref32, what=f"{what} fp32")
    with pytest.raises(AssertionError, match="outside the bf16 interval"):
        kp.assert_bf16_parity(kp.to_bf16(bad32), ref64, ref32, what=f"{what} bf16")


GEMM_MUT = [(37, 24, 64, 0.8, 11), (130, 72, 2048, 0.8, 12), (45, 40, 1536, 0.05 * 1536 ** 0.5, 13)]


@pytest.mark.parametrize("M,N,K,zsigma,seed", GEMM_MUT)
@pytest.mark.parametrize("act", ["none", "relu", "gelu"])
def test_gemm_bf16_mutations_are_rejected(M, N, K, zsigma, seed, act):
    """The last shape has W scaled by 0.05 as the Conv1d case of tests/test_wavlm_gpu.py: a dropped chunk is small."""
    i = kp.gemm_bf16_inputs(M, N, K, seed, zsigma=zsigma)
    a, w, bias, res = i["a"], i["w"], i["bias"], i["res"]
    ref64 = kp.ref_gemm_bf16(a, w, bias, res, act, None, 0.0, kp.F64)["out"]
    ref32 = kp.ref_gemm_bf16(a, w, bias, res, act, None, 0.0, kp.F32)["out"]
    kp.assert_fp64_parity(ref32, ref64, ref32, what="unmutated")
    kp.assert_bf16_parity(kp.to_bf16(ref32), ref64, ref32, what="unmutated bf16")
    # one 8-wide K chunk of one row dropped
    rng = np.random.default_rng(seed)
    r, c = int(rng.integers(M)), int(rng.integers(K // 8))
    a2 = a.clone()
    a2[r, 8 * c:8 * c + 8] = 0
    _rejected_both_ways(kp.ref_gemm_bf16(a2, w, bias, res, act, None, 0.0, kp.F32)["out"], ref64, ref32, "K chunk")
    # two bias columns swapped
    b2 = bias.clone()
    b2[[3, 4]] = bias[[4, 3]]
    _rejected_both_ways(kp.ref_gemm_bf16(a, w, b2, res, act, None, 0.0, kp.F32)["out"], ref64, ref32, "bias swap")
    # the residual added before the activation (the same thing for act none)
    if act != "none":
        z32 = kp.ref_gemm_bf16(a, w, bias, None, "none", None, 0.0, kp.F32)["out"]
        _rejected_both_ways(kp._act(z32 + res, act), ref64, ref32, "residual before act")
    # the final store truncated instead of rounded to nearest even
    with pytest.raises(AssertionError, match="outside the bf16 interval"):
        kp.assert_bf16_parity(kp.bf16_truncate(ref32), ref64, ref32, what="truncating store")


def test_dropout_before_the_activation_or_after_the_residual_is_rejected():
    M, N, K, p = 37, 24, 64, 0.1
    i = kp.gemm_bf16_inputs(M, N, K, 14)
    keep = kp.keep_mask_pair(kp.BASE, kp.SITE, kp.grid_index(M, N), p)
    assert 0 < int((~keep).sum()) < M * N // 4
    ref64 = kp.ref_gemm_bf16(i["a"], i["w"], i["bias"], i["res"], "gelu", keep, p, kp.F64)["out"]
    ref32 = kp.ref_gemm_bf16(i["a"], i["w"], i["bias"], i["res"], "gelu", keep, p, kp.F32)["out"]
    assert bool((ref32[~keep] == i["res"][~keep]).all())  # a dropped element is its residual, exactly
    after = kp.ref_gemm_bf16(i["a"], i["w"], i["bias"], i["res"], "gelu", None, 0.0, kp.F32)["out"] * \
        kp.drop_scale(keep, p, kp.F32)
    _rejected_both_ways(after, ref64, ref32, "dropout after the residual")
    # the single-index mask (the xattn head's) instead of the paired one
    other = kp.keep_mask(kp.BASE, kp.SITE, kp.grid_index(M, N), p)
    assert not bool((other == keep).all())


def test_posconv_restatement_is_the_grouped_conv1d_and_rejects_a_shifted_tap():
    B, L, C, G, taps, pad = 2, 17, 96, 2, 5, 2
    cg = C // G
    i = kp.posconv_inputs(B, L, C, G, taps, 15)
    ref64 = kp.ref_posconv(i["x"], i["wp"], i["bias"], i["res"], "gelu", B, L, C, G, taps, pad, kp.F64)
    ref32 = kp.ref_posconv(i["x"], i["wp"], i["bias"], i["res"], "gelu", B, L, C, G, taps, pad, kp.F32)
    w = i["wp"].reshape(C, taps, cg).permute(0, 2, 1).double()  # Conv1d's [Cout][Cin / G][k]
    z = torch.nn.functional.conv1d(i["x"].double().transpose(1, 2), w, i["bias"].double(), padding=pad, groups=G)
    assert float((z.transpose(1, 2)[:, :L] - ref64["z"]).abs().max()) < 1e-12
    shifted = kp.ref_posconv(i["x"], i["wp"], i["bias"], i["res"], "gelu", B, L, C, G, taps, pad + 1, kp.F32)["out"]
    _rejected_both_ways(shifted, ref64["out"], ref32["out"], "pad + 1")


def test_ln_bwd_partial_row_over_the_wrong_rows_is_rejected():
    g = kp.gen(16)
    rows, d = 37, 256
    x, gamma, dy = kp.randn(g, rows, d) * 2 + 0.5, kp.randn(g, d) * 0.3 + 1, kp.randn(g, rows, d)
    ref64, ref32 = (kp.ref_ln_bwd([dy], x, gamma, 1e-5, dt) for dt in (kp.F64, kp.F32))
    assert tuple(ref64["part"].shape) == (3, 3, d)
    assert float((ref64["part"][:, 1].sum(0) - dy.double().sum(0)).abs().max()) < 1e-12  # dbeta = sum dy
    shifted = kp.ref_ln_bwd([dy], x, gamma, 1e-5, kp.F32, block0=-1)["part"]
    for q in range(3):  # partial row 1 (dgamma, dbeta or sum dx) over rows 15..30 instead of 16..31
        bad = ref32["part"].clone()
        bad[1, q] = shifted[1, q]
        with pytest.raises(AssertionError):
            kp.assert_fp64_parity(bad[1, q], ref64["part"][1, q], ref32["part"][1, q], what=f"ln_bwd part 1 / {q}")
    kp.assert_fp64_parity(ref32["part"][1], ref64["part"][1], ref32["part"][1], what="ln_bwd part 1")


def test_gather_rows_is_the_conv1d_window():
    x = torch.arange(2 * 9 * 4, dtype=torch.float32)
    a = kp.gather_rows(x, 2 * 4, 12, 4, 8, 36)  # k = 3, s = 2, C = 4, Lin = 9 -> Lout = 4
    assert a[0].tolist() == list(range(12)) and a[1].tolist() == list(range(8, 20))
    assert a[4].tolist() == list(range(36, 48)) and a[7].tolist() == list(range(60, 72))


def test_ref_maxpool_takes_the_first_maximum_in_tap_order():
    x = torch.tensor([[1., 5., 5.], [5., 2., 5.], [0., 5., 1.]]).reshape(1, 3, 3, 1)
    dy = torch.tensor([[1., 2.], [4., 8.]]).reshape(1, 2, 2, 1)
    for dt in (kp.F64, kp.F32):
        o = kp.ref_maxpool(x, dy, dt)
        assert o["y"].reshape(2, 2).tolist() == [[5., 5.], [5., 5.]]
        # window (0,0) sees taps 4, 5, 7, 8 = 1, 5, 5, 2; (0,1) taps 3, 4, 6, 7 = 5, 5, 2, 5; (1,0) taps 1, 2, 4, 5 =
        # 5, 2, 0, 5; (1,1) taps 0, 1, 3, 4 = 2, 5, 5, 1: the first 5 of each
        assert o["arg"].reshape(2, 2).tolist() == [[5., 3.], [1., 1.]]
        assert o["dx"].reshape(3, 3).tolist() == [[0., 3., 0.], [4., 0., 8.], [0., 0., 0.]]
    lone = kp.ref_maxpool(torch.full((1, 1, 1, 1), -np.inf), torch.ones(1, 1, 1, 1), kp.F64)
    assert float(lone["y"]) == -np.inf and float(lone["arg"]) == 0 and float(lone["dx"]) == 0  # tap 0 is off the frame
    # a given argmax replaces the computed one; a tap outside the frame receives nothing
    arg = torch.tensor([[0, 7], [4, 4]], dtype=torch.uint8).reshape(1, 2, 2, 1)
    o = kp.ref_maxpool(x, dy, kp.F64, arg=arg)
    assert o["dx"].reshape(3, 3).tolist() == [[0., 0., 0.], [0., 0., 2.], [4., 0., 8.]]
    arg[0, 0, 1, 0] = 8  # (row 1, column 3) of a 3-wide frame
    assert kp.ref_maxpool(x, dy, kp.F64, arg=arg)["dx"].reshape(3, 3).tolist() == [[0.] * 3, [0.] * 3, [4., 0., 8.]]


# ---- csrc/common.h fdiv, emulated in float32: why the pooling kernels may not split their chunk index with it ----
def fdiv_emulated(a, d):
    inv = np.float32(1.0) / np.float32(d)
    return ((a.astype(np.float32) + np.float32(0.5)) * inv).astype(np.int64)


FDIV_DIVISORS = sorted(set(range(1, 65)) | {72, 112, 224, 515, 592, 600, 1030, 3136, 12544})


def test_fdiv_is_exact_below_2_22_and_first_wrong_at_2_23_plus_7_for_8():
    a = np.arange(1 << 22, dtype=np.int64)
    for d in FDIV_DIVISORS:  # C / 8 up to 64, and the widths / heights / plane sizes the kernels divide by
        assert np.array_equal(fdiv_emulated(a, d), a // d), d
    a = np.arange(1 << 24, dtype=np.int64)  # float32 still holds every such a exactly
    first = {}
    for d in (8, 64, 3, 7, 28, 56, 112):
        wrong = np.nonzero(fdiv_emulated(a, d) != a // d)[0]
        first[d] = int(wrong[0])
        assert first[d] >= 1 << 22, (d, first[d])
    assert first[8] == (1 << 23) + 7 and first[64] == (1 << 23) + 63, first
    wrong8 = np.nonzero(fdiv_emulated(a, 8) != a // 8)[0]
    tail = a[(1 << 23):]
    assert np.array_equal(wrong8, tail[tail % 8 == 7])  # every a = 7 (mod 8) from there on ...
    assert np.array_equal(fdiv_emulated(wrong8, 8), wrong8 // 8 + 1)  # ... gives q + 1
    for d in (3, 7, 28, 56, 112):
        assert 1.4 * (1 << 22) < first[d] < 1.6 * (1 << 22), (d, first[d])


# ---- csrc/conv.hip / conv_wgrad.hip / conv_pack.hip: the restatements of tests/test_conv_kernels_gpu.py ----
def _conv_forms(shape):
    c = kp.conv_case(shape)
    forms = [] if shape in kp.CONV_DGRAD_ONLY else ["fwd"]
    if shape not in kp.CONV_FWD_ONLY:
        forms += [f for f in kp.CONV_FORMS if f != "ds" or c.has_ds]
    return c, forms


@pytest.mark.parametrize("shape", kp.CONV_SHAPES + kp.CONV_FWD_ONLY + kp.CONV_DGRAD_ONLY, ids=str)
def test_conv_restatements_leave_every_gpu_shape_determined(shape):
    """min_determined = 0.9 is a condition on the inputs: the restatement alone meets it for every shape and form the
    GPU test runs (assert_bf16_parity asserts the share), with a bar far below one bf16 step."""
    c, forms = _conv_forms(shape)
    for f in forms:
        ref64, ref32 = c.ref(f)
        kp.assert_bf16_parity(kp.to_bf16(ref32), ref64, ref32, what=f"{shape} {f}")
        assert kp.bf16_interval(ref64, ref32)[2] <= 1e-5 * float(ref64.abs().max())


def test_stem_restatement_is_determined_and_the_s2d_form_is_the_7x7_conv():
    """The 4x4 / stride-1 / pad-0 convolution of the restated space-to-depth packs IS the 7x7 / stride-2 / pad-3 one
    (float64, a small frame), so the GPU test may judge the stem kernel against the latter."""
    s = kp.stem_case()
    kp.assert_bf16_parity(kp.to_bf16(s["ref"][1]), s["ref"][0], s["ref"][1], what="stem")
    g = kp.gen(31)
    frames, w32 = kp.randn(g, 2, 3, 10, 14), kp.randn(g, 8, 3, 7, 7)
    xs, ws = kp.ref_pack_input_s2d(frames).float(), kp.ref_pack_conv_weight(w32, 16, 2).float()
    assert tuple(xs.shape) == (2, 8, 10, 16) and tuple(ws.shape) == (8, 4, 4, 16)
    a = kp.ref_conv_fwd(xs, ws.permute(0, 3, 1, 2), 1, 0, kp.F64)["y"]
    b = kp.ref_conv_fwd(kp.to_bf16(frames).float().permute(0, 2, 3, 1), kp.to_bf16(w32).float(), 2, 3, kp.F64)["y"]
    assert tuple(a.shape) == tuple(b.shape) == (2, 5, 7, 8) and float((a - b).abs().max()) < 1e-12
    # every border slot and pad channel of both packs is zero
    assert float(xs[:, :2].abs().max()) == 0 and float(xs[:, -1].abs().max()) == 0
    assert float(xs[..., 12:].abs().max()) == 0
    assert float(xs[:, :, :2].abs().max()) == 0 and float(xs[:, :, -1].abs().max()) == 0
    assert float(ws[..., 12:].abs().max()) == 0 and float(ws[:, 0, :, :6].abs().max()) == 0  # tap r = -1: dy = 0 rows


def test_conv_restatements_are_the_library_convolutions():
    """The tap sums against torch's own convolutions in float64 (a check of the restatement's text, not a bar)."""
    F = torch.nn.functional
    for shape in [(2, 6, 9, 64, 64, 3, 1, 1), (2, 9, 6, 64, 128, 3, 2, 1), (2, 30, 30, 8, 64, 7, 2, 3),
                  (1, 7, 7, 64, 64, 3, 3, 1), (2, 8, 8, 64, 128, 1, 2, 0)]:
        N, H, W, C, Kc, R, stride, pad = shape
        c = kp.conv_case(shape)
        i = c.i
        x, w, dy = (i[k].double() for k in ("x", "w", "dy"))
        xn = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
        wn = w.clone().requires_grad_(True)
        y = F.conv2d(xn, wn, stride=stride, padding=pad)
        assert float((y.detach().permute(0, 2, 3, 1) - c.ref("fwd")[0]).abs().max()) < 1e-12
        gx, gw = torch.autograd.grad(y, [xn, wn], dy.permute(0, 3, 1, 2))
        assert float((gx.permute(0, 2, 3, 1) - c.ref("plain")[0]).abs().max()) < 1e-12
        dw0 = kp.randn(kp.gen(5), Kc, C, R, R)
        for splits in (1, 3):
            dw = kp.ref_conv_wgrad(i["x"], i["dy"], R, R, stride, pad, C, dw0, kp.F64, splits=splits)["dw"]
            assert float((dw - dw0.double() - gw).abs().max()) < 1e-11
        if c.has_ds:
            yd = F.conv2d(xn, i["wd"].double(), stride=2)
            gd, = torch.autograd.grad(yd, [xn], i["ds_dy"].double().permute(0, 3, 1, 2))
            keep = (i["mask"] > 0).double()
            want = (gx + gd).permute(0, 2, 3, 1) + i["res"].double() * keep
            assert float((want - c.ref("ds")[0]).abs().max()) < 1e-12


def test_conv_mask_restatement_at_signed_zeros_and_the_smallest_bf16():
    i = kp.conv_case((2, 7, 7, 64, 64, 3, 1, 1)).i
    m = i["mask"].reshape(-1)
    assert m[0] == 0 and not bool(torch.signbit(m[0])) and m[3] == 0 and bool(torch.signbit(m[3]))
    assert m[6] == -1 and 0 < float(m[9]) == kp.SUBNORMAL_BF16 == 2.0 ** -133
    assert float(kp.to_bf16(m[9:10]).float()) == kp.SUBNORMAL_BF16  # bf16-representable
    plain, masked = (kp.conv_case((2, 7, 7, 64, 64, 3, 1, 1)).ref(f)[0].reshape(-1) for f in ("plain", "res_mask"))
    r = i["res"].double().reshape(-1)
    assert bool((masked[[0, 3, 6]] == plain[[0, 3, 6]]).all()) and float(masked[9]) == float(plain[9] + r[9])


CONV_MUT = (2, 6, 9, 64, 64, 3, 1, 1)


def test_conv_fwd_mutations_are_rejected():
    N, H, W, C, Kc, R, stride, pad = CONV_MUT
    c = kp.conv_case(CONV_MUT)
    i = c.i
    ref64, ref32 = c.ref("fwd")
    kp.assert_bf16_parity(kp.to_bf16(ref32), ref64, ref32, what="unmutated")
    # one tap dropped at the image border only: the centre tap of the first output row (it reads real pixels there)
    border = torch.ones(1, H, W, 1)
    border[:, 0] = 0
    bad = kp.ref_conv_fwd(i["x"], i["w"], stride, pad, kp.F32,
                          tap_scale=lambda r, s: border if (r, s) == (1, 1) else None)
    assert bool((bad["y"][:, 1:] == ref32[:, 1:]).all())
    _rejected_both_ways(bad["y"], ref64, ref32, "border tap")
    # ... and a corner tap at the one pixel column where it is inside the frame's last column
    col = torch.ones(1, H, W, 1)
    col[:, :, W - 2] = 0
    bad = kp.ref_conv_fwd(i["x"], i["w"], stride, pad, kp.F32, tap_scale=lambda r, s: col if (r, s) == (2, 2) else None)
    _rejected_both_ways(bad["y"], ref64, ref32, "last-column tap")
    # padding off by one pixel
    for shift in (1, -1):
        _rejected_both_ways(kp.ref_conv_fwd(i["x"], i["w"], stride, pad, kp.F32, shift=shift)["y"], ref64, ref32, "pad")
    # the last 64-deep K chunk (tap (2, 2), channels C - 64 ...) of the second 64-row tile dropped
    xp = torch.zeros(N, H + 2, W + 2, C)
    xp[:, 1:H + 1, 1:W + 1] = i["x"]
    last = (xp[:, 2:2 + H, 2:2 + W, C - 64:] @ i["w"][:, C - 64:, 2, 2].t()).reshape(-1, Kc)
    bad = ref32.clone().reshape(-1, Kc)
    bad[64:128] -= last[64:128]
    _rejected_both_ways(bad.reshape(ref32.shape), ref64, ref32, "K chunk of one tile")
    # a truncating bf16 store
    with pytest.raises(AssertionError, match="outside the bf16 interval"):
        kp.assert_bf16_parity(kp.bf16_truncate(ref32), ref64, ref32, what="truncating store")
    # the statistics taken over the unrounded values instead of the stored ones
    stored = kp.to_bf16(ref32).float()
    s64, s32 = (kp.ref_conv_sums(stored, dt)["stats"] for dt in (kp.F64, kp.F32))
    kp.assert_fp64_parity(s32, s64, s32, what="stats of the stored values")
    with pytest.raises(AssertionError):
        kp.assert_fp64_parity(kp.ref_conv_sums(ref32, kp.F32)["stats"], s64, s32, what="stats of the accumulators")
    for q in range(2):  # either column alone
        with pytest.raises(AssertionError):
            kp.assert_fp64_parity(kp.ref_conv_sums(ref32, kp.F32)["stats"][:, q], s64[:, q], s32[:, q], what="stats")


@pytest.mark.parametrize("shape", [CONV_MUT, (2, 9, 6, 64, 128, 3, 2, 1)], ids=str)
def test_conv_dgrad_mutations_are_rejected(shape):
    N, H, W, C, Kc, R, stride, pad = shape
    c = kp.conv_case(shape)
    i = c.i
    form = "ds" if c.has_ds else "res_mask"
    ds = (i["ds_dy"], i["wd"]) if c.has_ds else None
    ref64, ref32 = c.ref(form)
    kp.assert_bf16_parity(kp.to_bf16(ref32), ref64, ref32, what="unmutated")
    # mask >= 0 instead of mask > 0: the planted +0.0 and -0.0 then receive the residual
    bad = kp.ref_conv_dgrad(i["dy"], i["w"], H, W, stride, pad, kp.F32, i["res"], i["mask"], ds, mask_ge=True)["dx"]
    diff = (bad != ref32).reshape(-1).nonzero().reshape(-1).tolist()
    assert diff == [0, 3], diff  # exactly the two zeros (the mask has no other)
    _rejected_both_ways(bad, ref64, ref32, "mask >= 0")
    # the mask ignored / the masked elements given the residual's negative
    _rejected_both_ways(c.ref("res")[1] if not c.has_ds else kp.ref_conv_dgrad(
        i["dy"], i["w"], H, W, stride, pad, kp.F32, i["res"], None, ds)["dx"], ref64, ref32, "no mask")
    # a truncating store
    with pytest.raises(AssertionError, match="outside the bf16 interval"):
        kp.assert_bf16_parity(kp.bf16_truncate(ref32), ref64, ref32, what="truncating store")
    # one tap of one border row dropped: tap (1, 1) at input row 0 (stride 1: it reads dy row 0; stride 2 likewise)
    w2 = i["w"].clone()
    w2[:, :, 1, 1] = 0
    drop = kp.ref_conv_dgrad(i["dy"], w2, H, W, stride, pad, kp.F32, i["res"], i["mask"], ds)["dx"]
    bad = ref32.clone()
    bad[:, 0] = drop[:, 0]
    _rejected_both_ways(bad, ref64, ref32, "border tap")
    # the BN-backward sums over the unrounded gradient, and under mask >= 0
    stored = kp.to_bf16(ref32).float()
    r64, r32 = (kp.ref_bnr_sums(stored, i["mask"], i["xb"], i["ms"], dt)["red"] for dt in (kp.F64, kp.F32))
    kp.assert_fp64_parity(r32, r64, r32, what="sums of the stored gradient")
    with pytest.raises(AssertionError):
        kp.assert_fp64_parity(kp.ref_bnr_sums(ref32, i["mask"], i["xb"], i["ms"], kp.F32)["red"], r64, r32,
                              what="unrounded")
    ge = torch.where(i["mask"] == 0, torch.ones(()), i["mask"])
    with pytest.raises(AssertionError):
        kp.assert_fp64_parity(kp.ref_bnr_sums(stored, ge, i["xb"], i["ms"], kp.F32)["red"], r64, r32, what="mask >= 0")
    if c.has_ds:
        # the two-launch form: the downsample's gradient rounded to bf16 before the 3x3 gradient is added to it
        dsg = kp.ref_conv_dgrad(i["ds_dy"], i["wd"], H, W, 2, 0, kp.F32)["dx"]
        keep = i["mask"] > 0
        two = kp.ref_conv_dgrad(i["dy"], i["w"], H, W, stride, pad, kp.F32)["dx"] + kp.to_bf16(dsg).float() + \
            torch.where(keep, i["res"], torch.zeros(()))
        _rejected_both_ways(two, ref64, ref32, "downsample gradient rounded before the add")


def test_conv_wgrad_mutations_are_rejected():
    shape = (2, 30, 30, 8, 64, 7, 2, 3)  # P = 450 pixels: 7 granules and a partial one
    N, H, W, C, Kc, R, stride, pad = shape
    i = kp.conv_case(shape).i
    dw0 = kp.randn(kp.gen(8), Kc, 3, R, R)
    args = (i["x"], i["dy"], R, R, stride, pad, 3, dw0)
    ref64, ref32 = (kp.ref_conv_wgrad(*args, dt, splits=2)["dw"] for dt in (kp.F64, kp.F32))
    assert kp.wgrad_split_pixels(450, 2) == 256 and kp.wgrad_split_pixels(450, 3) == 192
    kp.assert_fp64_parity(ref32, ref64, ref32, what="unmutated")
    # the plain one-chain float32 sum and another split count stay inside the bar: it is not slack, nor razor thin
    kp.assert_fp64_parity(kp.ref_conv_wgrad(*args, kp.F32, splits=1, chunk=450)["dw"], ref64, ref32, what="plain")
    kp.assert_fp64_parity(kp.ref_conv_wgrad(*args, kp.F32, splits=3)["dw"], ref64, ref32, what="three splits")
    with pytest.raises(AssertionError):  # creal channels read from channel 1 on
        kp.assert_fp64_parity(kp.ref_conv_wgrad(*args, kp.F32, splits=2, c0=1)["dw"], ref64, ref32,
                              what="channel offset")
    with pytest.raises(AssertionError):  # the last, partial granule (pixels 448, 449) dropped
        kp.assert_fp64_parity(kp.ref_conv_wgrad(*args, kp.F32, splits=2, drop_tail=True)["dw"], ref64, ref32,
                              what="partial granule")
    with pytest.raises(AssertionError):  # dw = instead of dw +=
        kp.assert_fp64_parity(ref32 - dw0, ref64, ref32, what="dw0 dropped")
    with pytest.raises(AssertionError):  # one split's slab left out of the fold
        one = kp.ref_conv_wgrad(i["x"][:1], i["dy"][:1], R, R, stride, pad, 3, dw0, kp.F32, splits=1)["dw"]
        kp.assert_fp64_parity(one, ref64, ref32, what="a slab dropped")


def test_conv_pack_restatements():
    w = torch.arange(2 * 3 * 2 * 2, dtype=torch.float32).reshape(2, 3, 2, 2) + 1
    p0, p1 = kp.ref_pack_conv_weight(w, 8, 0), kp.ref_pack_conv_weight(w, 8, 1)
    assert tuple(p0.shape) == (2, 2, 2, 8) and tuple(p1.shape) == (8, 2, 2, 2)
    assert float(p0[1, 0, 1, 2]) == float(w[1, 2, 0, 1]) == float(p1[2, 0, 1, 1])
    assert float(p0[..., 3:].abs().max()) == 0 and float(p1[3:].abs().max()) == 0
    assert bool((kp.ref_pack_conv_weight(w, 8, 3) == p1).all())
    x = torch.arange(1 * 3 * 4 * 6, dtype=torch.float32).reshape(1, 3, 4, 6)
    xs = kp.ref_pack_input_s2d(x)
    assert tuple(xs.shape) == (1, 5, 6, 16)
    assert float(xs[0, 2, 2, 0]) == 0.0 and float(xs[0, 3, 4, (1 * 2 + 0) * 3 + 2]) == float(x[0, 2, 3, 4])
    assert float(xs[..., 12:].abs().max()) == 0
    rounds = torch.tensor([1 + 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -16, 1 + 3 * 2.0 ** -8]).reshape(3, 1, 1, 1)
    assert kp.ref_pack_conv_weight(rounds, 8, 0)[:, 0, 0, 0].float().tolist() == [1.0, 1 + 2.0 ** -7, 1 + 2.0 ** -6]

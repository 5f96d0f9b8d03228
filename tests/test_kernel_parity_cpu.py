"""The bars of tests/test_head_kernels_gpu.py are sound: every float32 restatement is close to, and distinct from,
its float64 reference, and ``assert_fp64_parity`` accepts the former and rejects a 1e-4 perturbation of it."""
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

"""FusedAdam's host side without a GPU: the torch.optim.Adam-format state dict (both directions, two groups, a
parameter that never stepped, the EMA), the checkpoint that carries it, the clip coefficient's restatement against
``clip_grad_norm_``, and which kernels ``step`` launches with the options off and on (the launches are recorded, not
run)."""
import re

import pytest
import torch

from tests.kernel_parity import F32, F64, gen, randn
from tests.optim_ref import ref_clip

SHAPES = [(5,), (3, 7), (130,), (4, 4)]
GROUP_OF = [0, 0, 1, 1]
LRS = [1e-3, 1e-5]
STEPS = [3, 0, 7, 3]  # parameter 1 never stepped


def _params(seed=1):
    g = gen(seed)
    return [torch.nn.Parameter(randn(g, *s)) for s in SHAPES]


def _groups(ps):
    return [{"params": [p for p, gi in zip(ps, GROUP_OF) if gi == k], "lr": lr} for k, lr in enumerate(LRS)]


def _fused(seed=1, **kw):
    from multimodalemotionrecognition_amd.optim import FusedAdam

    ps = _params(seed)
    return ps, FusedAdam(_groups(ps), weight_decay=1e-4, **kw)


def _fill(opt, seed=2):
    """Moments, step counts (and the EMA) by hand; returns what was written, per parameter in group order."""
    g = gen(seed)
    want = {"m": [], "v": [], "e": [], "steps": []}
    it = iter(STEPS)
    for f, group in zip(opt._flat, opt.param_groups):
        for i, (p, o) in enumerate(zip(group["params"], f["offs"])):
            st = next(it)
            f["steps"][i] = st
            m, v = (randn(g, *p.shape), randn(g, *p.shape).abs()) if st else (torch.zeros_like(p), torch.zeros_like(p))
            f["m"][o:o + p.numel()].copy_(m.reshape(-1))
            f["v"][o:o + p.numel()].copy_(v.reshape(-1))
            want["m"].append(m), want["v"].append(v), want["steps"].append(st)
            if "ema" in f:
                e = randn(g, *p.shape)
                f["ema"][o:o + p.numel()].copy_(e.reshape(-1))
                want["e"].append(e)
    return want


def _read(opt):
    got = {"m": [], "v": [], "e": [], "steps": []}
    for f, group in zip(opt._flat, opt.param_groups):
        for i, (p, o) in enumerate(zip(group["params"], f["offs"])):
            got["m"].append(f["m"][o:o + p.numel()].view(p.shape).clone())
            got["v"].append(f["v"][o:o + p.numel()].view(p.shape).clone())
            got["steps"].append(f["steps"][i])
            if "ema" in f:
                got["e"].append(f["ema"][o:o + p.numel()].view(p.shape).clone())
    return got


def _same(a, b):
    assert a["steps"] == b["steps"]
    for k in ("m", "v", "e"):
        assert len(a[k]) == len(b[k])
        for x, y in zip(a[k], b[k]):
            assert torch.equal(x, y), k


def test_state_dict_is_torch_adams_format():
    ps, opt = _fused()
    want = _fill(opt)
    sd = opt.state_dict()
    assert sorted(sd["state"]) == [0, 2, 3]  # the parameter with steps == 0 is absent
    ref_keys = set(torch.optim.Adam([torch.zeros(1, requires_grad=True)]).state_dict()["param_groups"][0])
    for k, g in enumerate(sd["param_groups"]):
        assert set(g) == ref_keys and g["lr"] == LRS[k] and g["weight_decay"] == 1e-4
    assert [g["params"] for g in sd["param_groups"]] == [[0, 1], [2, 3]]
    for i, st in sd["state"].items():
        assert set(st) == {"step", "exp_avg", "exp_avg_sq"}
        assert st["step"].dtype == F32 and st["step"].shape == () and float(st["step"]) == STEPS[i]
        assert st["exp_avg"].device.type == "cpu" and torch.equal(st["exp_avg"], want["m"][i])
        assert torch.equal(st["exp_avg_sq"], want["v"][i])
    # copies, not views of the flat buffers
    opt._flat[0]["m"].add_(1.0)
    assert torch.equal(sd["state"][0]["exp_avg"], want["m"][0])


def test_round_trip_through_torch_adam_and_back():
    ps, opt = _fused()
    want = _fill(opt)
    tps = _params()
    tadam = torch.optim.Adam(_groups(tps), weight_decay=1e-4)
    tadam.load_state_dict(opt.state_dict())  # extra keys must not break torch's loader
    assert [g["lr"] for g in tadam.param_groups] == LRS
    for i, p in enumerate(tps):
        if STEPS[i] == 0:
            assert p not in tadam.state
            continue
        assert float(tadam.state[p]["step"]) == STEPS[i]
        assert torch.equal(tadam.state[p]["exp_avg"], want["m"][i])
        assert torch.equal(tadam.state[p]["exp_avg_sq"], want["v"][i])
    for p in tps:  # torch can go on from the loaded state
        p.grad = torch.ones_like(p)
    tadam.step()
    assert float(tadam.state[tps[0]]["step"]) == STEPS[0] + 1 and float(tadam.state[tps[1]]["step"]) == 1

    # a torch.optim.Adam state dict loads into FusedAdam
    tadam2 = torch.optim.Adam(_groups(_params()), weight_decay=1e-4)
    tadam2.load_state_dict(opt.state_dict())
    for g in tadam2.param_groups:
        g["lr"] *= 0.5  # a scheduler moved it: hyper-parameters travel with the state
    _, back = _fused(seed=5)
    back.load_state_dict(tadam2.state_dict())
    _same(_read(back), want)
    assert [g["lr"] for g in back.param_groups] == [lr * 0.5 for lr in LRS]
    assert back.state_steps() == [[3, 0], [7, 3]]


def test_load_resets_parameters_absent_from_the_state():
    _, a = _fused()
    _fill(a)
    _, b = _fused()
    want = _fill(b, seed=9)
    b._flat[0]["steps"][1] = 4  # parameter 1 has state in b, none in a's dict
    b._flat[0]["m"][8:29].fill_(3.0)
    b.load_state_dict(a.state_dict())
    got = _read(b)
    assert got["steps"] == STEPS and float(got["m"][1].abs().max()) == 0.0 and float(got["v"][1].abs().max()) == 0.0
    del want


def test_ema_round_trips_and_torch_ignores_it():
    _, opt = _fused(ema_decay=0.999, max_grad_norm=2.0)
    want = _fill(opt)
    sd = opt.state_dict()
    assert sd["fused_adam"] == {"max_grad_norm": 2.0, "ema_decay": 0.999, "live_params": None}
    assert all(len(g["ema"]) == 2 for g in sd["param_groups"])
    _, back = _fused(seed=5, ema_decay=0.999)
    back.load_state_dict(sd)
    _same(_read(back), want)
    # torch's loader carries the unknown group key along and never looks at the top-level entry
    tps = _params()
    tadam = torch.optim.Adam(_groups(tps), weight_decay=1e-4)
    tadam.load_state_dict(sd)
    for p in tps:
        p.grad = torch.ones_like(p)
    tadam.step()
    assert torch.equal(tadam.state_dict()["param_groups"][1]["ema"][0], want["e"][2])
    # a state without an EMA (torch's own) restarts the average from the parameters
    _, fresh = _fused(seed=5, ema_decay=0.9)
    plain = torch.optim.Adam(_groups(_params()), weight_decay=1e-4).state_dict()
    fresh.load_state_dict(plain)
    for f in fresh._flat:
        assert torch.equal(f["ema"], f["flat"])


def test_mismatched_groups_are_refused():
    from multimodalemotionrecognition_amd.optim import FusedAdam

    _, opt = _fused()
    other = FusedAdam([torch.nn.Parameter(torch.zeros(3))])
    with pytest.raises(ValueError):
        other.load_state_dict(opt.state_dict())
    sd = opt.state_dict()
    sd["param_groups"][0]["amsgrad"] = True
    with pytest.raises(ValueError):
        _fused()[1].load_state_dict(sd)
    with pytest.raises(ValueError):
        _fused(max_grad_norm=0.0)
    with pytest.raises(ValueError):
        _fused(ema_decay=1.0)


def test_ema_weights_swaps_contents_in_place():
    from multimodalemotionrecognition_amd.optim import weight_version

    ps, opt = _fused(ema_decay=0.99)
    want = _fill(opt)
    live = [p.detach().clone() for p in ps]
    ptrs = [p.data_ptr() for p in ps]
    v0 = [weight_version(p) for p in ps]
    with opt.ema_weights():
        v1 = [weight_version(p) for p in ps]
        assert all(a != b for a, b in zip(v0, v1)) and [p.data_ptr() for p in ps] == ptrs
        for p, e in zip(ps, want["e"]):
            assert torch.equal(p.detach(), e)
        with pytest.raises(RuntimeError):
            opt.step()
        inside = opt.state_dict()  # the average stays "ema"; the live weights travel along
        assert torch.equal(inside["param_groups"][0]["ema"][1], want["e"][1])
        assert torch.equal(inside["fused_adam"]["live_params"][1][0], live[2])
    assert all(a != b for a, b in zip(v1, [weight_version(p) for p in ps]))
    for p, w in zip(ps, live):
        assert torch.equal(p.detach(), w)
    _same(_read(opt), want)
    with pytest.raises(RuntimeError):
        with _fused()[1].ema_weights():
            pass


class _Tiny(torch.nn.Module):
    def __init__(self, seed):
        super().__init__()
        torch.manual_seed(seed)
        self.a = torch.nn.Linear(5, 3)
        self.bn = torch.nn.BatchNorm1d(3)


def test_checkpoint_keeps_the_legacy_keys_and_resumes(tmp_path):
    from multimodalemotionrecognition_amd.optim import FusedAdam
    from multimodalemotionrecognition_amd.train import load_training_state, save_checkpoint

    m = _Tiny(1)
    opt = FusedAdam(m.parameters(), ema_decay=0.9)
    f = opt._flat[0]
    f["steps"][:] = [2] * len(f["steps"])
    f["m"].copy_(randn(gen(3), f["m"].numel()))
    f["v"].copy_(randn(gen(4), f["v"].numel()).abs())
    f["ema"].copy_(randn(gen(5), f["ema"].numel()))
    m.bn.running_mean.fill_(0.25)
    plain, full, avg = tmp_path / "plain.pt", tmp_path / "full.pt", tmp_path / "avg.pt"
    cfg = {"fusion": "xattn"}
    save_checkpoint(m, plain, 0.5, cfg)
    save_checkpoint(m, full, 0.5, cfg, optimizer=opt, epoch=3)
    with opt.ema_weights():
        save_checkpoint(m, avg, 0.5, cfg, optimizer=opt, epoch=3)
    a, b, c = (torch.load(p, weights_only=True) for p in (plain, full, avg))
    assert set(a) == {"model", "val_f1", "config"}
    assert set(b) == set(c) == {"model", "val_f1", "config", "optimizer", "epoch", "best_f1"}
    for k in ("val_f1", "config"):
        assert a[k] == b[k] == c[k]
    assert list(a["model"]) == list(b["model"]) and all(torch.equal(a["model"][k], b["model"][k]) for k in a["model"])
    assert b["epoch"] == 3 and b["best_f1"] == 0.5
    assert torch.equal(c["model"]["a.weight"].reshape(-1), f["ema"][:15])  # the averaged weights are the model

    with pytest.raises(KeyError):
        load_training_state(plain, _Tiny(2), FusedAdam(_Tiny(2).parameters()))
    for path in (full, avg):  # either file resumes the LIVE weights, moments, step counts, EMA and buffers
        m2 = _Tiny(2)
        opt2 = FusedAdam(m2.parameters(), ema_decay=0.9)
        assert load_training_state(path, m2, opt2) == {"epoch": 3, "best_f1": 0.5}
        f2 = opt2._flat[0]
        for k in ("flat", "m", "v", "ema"):
            for p, o in zip(opt.param_groups[0]["params"], f["offs"]):  # (the alignment gaps belong to nobody)
                assert torch.equal(f2[k][o:o + p.numel()], f[k][o:o + p.numel()]), (path.name, k)
        assert f2["steps"] == f["steps"] and float(m2.bn.running_mean[0]) == 0.25
        assert m2.a.weight.data_ptr() == f2["flat"].data_ptr()  # still a view of the flat buffer


@pytest.mark.parametrize("scale,clipped", [(1.0, True), (0.01, False)])
@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
def test_clip_restatement_equals_clip_grad_norm(scale, clipped, grad_scale):
    """The fp64 restatement of (total_norm, coef) is torch's clip_grad_norm_ in fp64, above and below max_norm."""
    g = gen(7)
    shapes = [(5,), (3, 7), (130,)]
    grads = [randn(g, *s) * (0.3 * scale) for s in shapes]
    max_norm = 1.0
    total, coef = ref_clip(grads, max_norm, grad_scale, F64)
    ps = [torch.nn.Parameter(torch.zeros(s, dtype=F64)) for s in shapes]
    for p, x in zip(ps, grads):
        p.grad = x.to(F64) * grad_scale
    tn = torch.nn.utils.clip_grad_norm_(ps, max_norm)
    assert abs(float(tn) - float(total)) <= 4 * 2.0 ** -53 * float(total)
    # the restatement adds the kernel's 1e-6f where torch adds 1e-6: they differ by at most 2^-24 * 1e-6, relative to
    # total_norm + 1e-6; beyond that only a few fp64 roundings (sum order, the divide, the multiply) separate the two
    rel = 2.0 ** -24 * 1e-6 / float(total) + 8 * 2.0 ** -53
    for p, x in zip(ps, grads):
        want = x.to(F64) * grad_scale * coef
        assert float((p.grad - want).abs().max()) <= rel * float(want.abs().max())
    print(f"total_norm {float(total):.4f} coef {float(coef):.4f}")
    if clipped:
        assert 0.2 <= float(coef) <= 0.8
    else:
        assert float(coef) == 1.0 and float(total) < max_norm


def test_constants_match_the_header():
    from multimodalemotionrecognition_amd import kernels as K
    from multimodalemotionrecognition_amd._lib import _HEADER

    text = _HEADER.read_text()
    for name, val in (("MER_NORM_CHUNK", K.NORM_CHUNK), ("MER_CLIP_THREADS", K.CLIP_THREADS),
                      ("MER_CLIP_REC_FLOATS", K.CLIP_REC_FLOATS), ("MER_CLIP_TOTAL_NORM", K.CLIP_TOTAL_NORM),
                      ("MER_CLIP_COEF", K.CLIP_COEF), ("MER_CLIP_STEPS", K.CLIP_STEPS),
                      ("MER_CLIP_NORM_SUM", K.CLIP_NORM_SUM), ("MER_CLIP_NORM_MAX", K.CLIP_NORM_MAX),
                      ("MER_CLIP_NONFINITE", K.CLIP_NONFINITE)):
        m = re.search(rf"#define\s+{name}\s+(\d+)", text)
        assert m and int(m.group(1)) == val, name


class _Launches:
    """Record the optimizer's kernel launches instead of running them."""

    def __init__(self, monkeypatch):
        from multimodalemotionrecognition_amd import kernels as K

        self.log = []
        monkeypatch.setattr(K, "adam_step", lambda p, *a, **k: self.log.append(("adam_step", p.numel())))
        monkeypatch.setattr(K, "adam_step_ex", lambda p, *a, **k: self.log.append(
            ("adam_step_ex", p.numel(), k["coef"] is not None, k["ema"] is not None)))
        monkeypatch.setattr(K, "grad_sqnorm", lambda segs: self.log.append(("grad_sqnorm", segs.nseg, segs.nchunks)))
        monkeypatch.setattr(K, "clip_finalize", lambda segs, gs, mx, rec: self.log.append(("clip_finalize", gs, mx)))


def _give_grads(ps, skip=()):
    for i, p in enumerate(ps):
        p.grad = None if i in skip else torch.ones_like(p)


def test_step_launches_with_the_options_off_and_on(monkeypatch):
    rec = _Launches(monkeypatch)
    ps, opt = _fused()
    _give_grads(ps)
    opt.step()
    assert rec.log == [("adam_step", 32), ("adam_step", 148)]  # today's path: one launch per run, nothing else
    assert opt._clip_rec is None and not opt._segments and "ema" not in opt._flat[0]

    rec.log.clear()
    ps, opt = _fused(max_grad_norm=1.0)
    opt.grad_scale = 0.5
    _give_grads(ps)
    opt.step()
    assert rec.log == [("grad_sqnorm", 2, 2), ("clip_finalize", 0.5, 1.0), ("adam_step_ex", 32, True, False),
                       ("adam_step_ex", 148, True, False)]
    (segs,) = opt._segments.values()
    assert segs.table.tolist() == [[opt._flat[0]["gflat"].data_ptr(), 32, 0], [opt._flat[1]["gflat"].data_ptr(), 148, 1]]
    _give_grads(ps)
    opt.step()
    assert list(opt._segments.values()) == [segs]  # the same layout: the cached table, no new copy
    rec.log.clear()
    _give_grads(ps, skip={1})  # parameter 1 has no gradient: another layout, its own table
    opt.step()
    assert rec.log[0] == ("grad_sqnorm", 2, 2) and rec.log[2:] == [("adam_step_ex", 8, True, False),
                                                                    ("adam_step_ex", 148, True, False)]
    assert len(opt._segments) == 2 and opt.state_steps() == [[3, 2], [3, 3]]
    rec.log.clear()
    _give_grads(ps)  # parameters 0 and 1 now differ in step count: two runs in group 0
    opt.step()
    assert rec.log[0] == ("grad_sqnorm", 3, 3) and [r[1] for r in rec.log[2:]] == [8, 24, 148]
    rec.log.clear()
    _give_grads(ps, skip={0, 1, 2, 3})
    opt.step()
    assert rec.log == []  # nothing has a gradient: no norm, no step

    rec.log.clear()
    ps, opt = _fused(ema_decay=0.99)
    _give_grads(ps)
    opt.step()
    assert rec.log == [("adam_step_ex", 32, False, True), ("adam_step_ex", 148, False, True)]


def test_new_entry_points_check_their_arguments_before_any_launch():
    """hipErrorInvalidValue (1) before any HIP call, so this runs without a GPU."""
    from multimodalemotionrecognition_amd._lib import LIB

    LIB.load()
    f = LIB._fns
    fake = 1 << 20  # never dereferenced
    hp = (1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1.0)
    assert f["mer_adam_step_ex"](8, fake, fake, fake, fake, *hp, None, fake + 4, 0.9, None) == 1  # misaligned ema
    assert f["mer_adam_step_ex"](8, fake + 4, fake, fake, fake, *hp, None, None, 0.0, None) == 1
    assert f["mer_adam_step_ex"](8, fake, fake, fake, fake, *hp, fake + 2, None, 0.0, None) == 1
    assert f["mer_adam_step_ex"](0, fake, fake, fake, fake, *hp, None, None, 0.0, None) == 0  # n == 0: nothing to do
    assert f["mer_grad_sqnorm"](0, fake, 1, fake, None) == 1
    assert f["mer_grad_sqnorm"](1, fake, 0, fake, None) == 1
    assert f["mer_grad_sqnorm"](1, fake + 4, 1, fake, None) == 1
    assert f["mer_clip_finalize"](0, fake, 1.0, 1.0, fake, None) == 1
    assert f["mer_clip_finalize"](1, fake, 1.0, 1.0, None, None) == 1


def test_norm_segments_refuse_bad_runs():
    from multimodalemotionrecognition_amd import kernels as K

    buf = torch.zeros(64)
    for bad in (buf[1:9], buf[:6], buf[:0], buf[:8].double(), buf[:16:2]):
        with pytest.raises(ValueError):
            K.NormSegments([bad])
    with pytest.raises(ValueError):
        K.NormSegments([])
    C = K.NORM_CHUNK
    big = torch.zeros(3 * C + 4 + 8)
    segs = K.NormSegments([big[:8], big[8:]])
    assert segs.nchunks == 5 and segs.table[:, 2].tolist() == [0, 1] and segs.partials.dtype == F64


def test_grad_norm_stats_of_a_window_without_a_finite_norm():
    import math

    from multimodalemotionrecognition_amd import kernels as K

    _, opt = _fused(max_grad_norm=1.0)
    rec = opt._clip_rec
    rec[K.CLIP_TOTAL_NORM], rec[K.CLIP_STEPS], rec[K.CLIP_NORM_SUM], rec[K.CLIP_NORM_MAX], rec[K.CLIP_NONFINITE] = \
        2.0, 3.0, 5.0, 3.0, 1.0
    assert opt.grad_norm_stats(reset=False) == {"steps": 3, "mean": 2.5, "max": 3.0, "last": 2.0, "nonfinite_steps": 1}
    rec[K.CLIP_TOTAL_NORM], rec[K.CLIP_STEPS], rec[K.CLIP_NORM_SUM], rec[K.CLIP_NORM_MAX], rec[K.CLIP_NONFINITE] = \
        float("inf"), 2.0, 0.0, 0.0, 2.0
    st = opt.grad_norm_stats(reset=True)  # every norm non-finite: no mean, no max -- not a zero
    assert st["steps"] == 2 and st["nonfinite_steps"] == 2 and math.isnan(st["mean"]) and math.isnan(st["max"])
    assert math.isinf(st["last"])
    st = opt.grad_norm_stats()  # after the reset: an empty window
    assert st["steps"] == 0 and math.isnan(st["mean"]) and math.isnan(st["max"]) and math.isinf(st["last"])
    with pytest.raises(RuntimeError):
        _fused()[1].grad_norm_stats()


def test_fit_swaps_the_average_in_once_per_epoch(monkeypatch):
    """ema_eval: evaluate and save_checkpoint run inside ONE ema_weights() per epoch (one swap in, one out), the
    training epoch outside it; without ema_eval nothing is swapped."""
    from multimodalemotionrecognition_amd import train

    _, opt = _fused(ema_decay=0.9)
    swaps, seen = [], []
    real = opt._swap_ema
    monkeypatch.setattr(opt, "_swap_ema", lambda: (swaps.append(1), real())[1])
    f1s = iter([0.2, 0.1, 0.3] * 2)
    monkeypatch.setattr(train, "train_one_epoch", lambda *a, **k: seen.append(("train", opt._ema_swapped)) or {"f1": 0.0})
    monkeypatch.setattr(train, "evaluate", lambda *a, **k: seen.append(("eval", opt._ema_swapped)) or {"f1": next(f1s)})
    monkeypatch.setattr(train, "save_checkpoint", lambda *a, **k: seen.append(("save", opt._ema_swapped, sorted(k))))
    out = train.fit(torch.nn.Identity(), None, None, opt, "cpu", None, "xattn", 3, checkpoint_path="best.pt",
                    ema_eval=True, save_optimizer=True, early_stopping_patience=0)
    assert out["best_epoch"] == 3 and len(swaps) == 6 and not opt._ema_swapped
    assert seen == [("train", False), ("eval", True), ("save", True, ["epoch", "optimizer"]),
                    ("train", False), ("eval", True),
                    ("train", False), ("eval", True), ("save", True, ["epoch", "optimizer"])]
    swaps.clear(), seen.clear()
    out = train.fit(torch.nn.Identity(), None, None, opt, "cpu", None, "xattn", 3, checkpoint_path="best.pt",
                    early_stopping_patience=1, start_epoch=1)
    assert swaps == [] and out["epochs_run"] == 2 and out["stopped_early"] and out["best_epoch"] == 2
    assert seen == [("train", False), ("eval", False), ("save", False, []), ("train", False), ("eval", False)]

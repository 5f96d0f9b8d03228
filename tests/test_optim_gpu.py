"""FusedAdam with device-side clipping, weight EMA and resumable state, on the GPU.

* Three steps on synthetic gradients (two groups, four shapes, one parameter without a gradient in step 2) against
  ``torch.optim.Adam`` + ``clip_grad_norm_`` on the CPU in float64, with the same run in float32 as the bar
  (tests/optim_ref.torch_adam_run); the same with ``grad_scale = 0.5`` through ``set_used``.
* Clipping far above the norm changes no bit; two fresh optimizers agree bit for bit, ``total_norm`` included.
* The EMA plane, ``ema_weights()`` (in-place swap, version bumps, the eval forward really uses the average).
* Resume: save after two steps, two more; a fresh model + optimizer resumed from the file repeat them bit for bit.
* ``fit`` with clipping and ``ema_eval``; one world-2 data-parallel run with clipping on.
"""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp
from torch import nn

from tests import optim_ref as R
from tests.kernel_parity import F32, F64, assert_fp64_parity, gen, randn

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = [(5,), (3, 7), (130,), (64, 64)]
GROUP_OF = [0, 0, 1, 1]
LRS = [1e-3, 1e-5]
WD = 1e-4
NSTEPS = 3
GRAD_STD = 0.035  # 4252 elements of sign(r) (0.1 + |r|): a norm of ~2.5, so max_norm 1 clips at ~0.4 (asserted)


def _host_params():
    g = gen(50)
    return [randn(g, *s) for s in SHAPES]


def _host_grads():
    """Per step one gradient per parameter (bounded away from zero, kernel_parity.adam_inputs); parameter 1 has none
    in step 2."""
    out = []
    for s in range(NSTEPS):
        g = gen(60 + s)
        row = []
        for i, sh in enumerate(SHAPES):
            r = randn(g, *sh)
            row.append(None if (s == 1 and i == 1) else torch.sign(r) * (0.1 + r.abs()) * GRAD_STD)
        out.append(row)
    return out


def _fused(**kw):
    from multimodalemotionrecognition_amd.optim import FusedAdam

    ps = [nn.Parameter(t.to(DEV)) for t in _host_params()]
    groups = [{"params": [p for p, gi in zip(ps, GROUP_OF) if gi == k], "lr": lr} for k, lr in enumerate(LRS)]
    return ps, FusedAdam(groups, weight_decay=WD, **kw)


def _feed(opt, ps, grads, through_set_used=False):
    """Write the gradients into the parameters' slots of the flat gradient buffers, as the backward kernels do."""
    opt.zero_grad()
    for p, g in zip(ps, grads):
        if g is None:
            continue
        flat, o = p._mer_grad_slot
        view = flat[o:o + p.numel()].view_as(p)
        view.copy_(g)
        if not through_set_used:
            p.grad = view
    if through_set_used:  # the data-parallel path: the slots hold the SUM, the flags come from the all-reduce
        flags = [g is not None for g in grads]
        opt.set_used([[f for f, gi in zip(flags, GROUP_OF) if gi == k] for k in range(len(LRS))])


def _run(grad_scale=1.0, through_set_used=False, **kw):
    ps, opt = _fused(**kw)
    opt.grad_scale = grad_scale
    for grads in _host_grads():
        _feed(opt, ps, grads, through_set_used)
        opt.step()
    torch.cuda.synchronize()
    return ps, opt


def _planes(opt, ps):
    """{"p", "m", "v", "e"}: per parameter, from the flat buffers."""
    out = {"p": [], "m": [], "v": [], "e": []}
    for f, group in zip(opt._flat, opt.param_groups):
        for p, o in zip(group["params"], f["offs"]):
            for k, name in (("p", "flat"), ("m", "m"), ("v", "v"), ("e", "ema")):
                if name in f:
                    out[k].append(f[name][o:o + p.numel()].view(p.shape).cpu())
    return out


def _bits_equal(a, b, what):
    for k in a:
        assert len(a[k]) == len(b[k]), (what, k)
        for i, (x, y) in enumerate(zip(a[k], b[k])):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (what, k, i)


_REFS = {}


def _refs(grad_scale, ema_decay=None):
    key = (grad_scale, ema_decay)
    if key not in _REFS:
        _REFS[key] = R.both(lambda dt: R.torch_adam_run(_host_params(), GROUP_OF, LRS, _host_grads(), dt, WD,
                                                         max_norm=1.0, grad_scale=grad_scale, ema_decay=ema_decay))
    return _REFS[key]


@pytest.mark.parametrize("grad_scale,through_set_used", [(1.0, False), (0.5, True)])
def test_three_clipped_steps_match_torch_adam(grad_scale, through_set_used):
    r64, r32 = _refs(grad_scale)
    assert all(float(n) > 1.0 for n in r64["norms"]), "the inputs must really clip"
    ps, opt = _run(grad_scale, through_set_used, max_grad_norm=1.0)
    got = _planes(opt, ps)
    assert [s for g in opt.state_steps() for s in g] == r64["steps"] == [3, 2, 3, 3]
    for k in ("p", "m", "v"):
        for i in range(len(SHAPES)):
            assert_fp64_parity(got[k][i], r64[k][i], r32[k][i], what=f"clipped adam gs{grad_scale} {k}[{i}]")
    st = opt.grad_norm_stats(reset=True)
    norms = [float(n) for n in r64["norms"]]
    print("grad_norm_stats", st, "reference norms", norms)
    assert st["steps"] == NSTEPS and st["nonfinite_steps"] == 0
    # each norm is within 4 * 2^-24 of the reference (tests/test_optim_kernels_gpu.py); the record's fp32 sum of the
    # three adds two more roundings of 2^-24 each
    for got_v, want, ulps in ((st["last"], norms[-1], 4), (st["max"], max(norms), 4),
                              (st["mean"], sum(norms) / NSTEPS, 6)):
        assert abs(got_v - want) <= ulps * 2.0 ** -24 * want
    assert opt.grad_norm_stats(reset=False)["steps"] == 0 and opt.grad_norm_stats()["last"] == st["last"]


def test_clipping_far_above_the_norm_changes_no_bit():
    a_ps, a = _run(max_grad_norm=None)
    b_ps, b = _run(max_grad_norm=1e30)
    _bits_equal(_planes(a, a_ps), _planes(b, b_ps), "max_grad_norm=1e30 vs None")
    assert a.state_steps() == b.state_steps()


def test_two_fresh_optimizers_agree_bit_for_bit():
    a_ps, a = _run(max_grad_norm=1.0, ema_decay=0.999)
    b_ps, b = _run(max_grad_norm=1.0, ema_decay=0.999)
    _bits_equal(_planes(a, a_ps), _planes(b, b_ps), "run to run")
    assert torch.equal(a._clip_rec.cpu().view(torch.int32), b._clip_rec.cpu().view(torch.int32))


def test_ema_plane_and_the_swap():
    from multimodalemotionrecognition_amd.optim import weight_version

    d = 0.999
    r64, r32 = _refs(1.0, d)
    ps, opt = _run(max_grad_norm=1.0, ema_decay=d)
    got = _planes(opt, ps)
    for i in range(len(SHAPES)):
        assert_fp64_parity(got["e"][i], r64["e"][i], r32["e"][i], what=f"ema[{i}]")
        assert not torch.equal(got["e"][i], got["p"][i])
    live = [p.detach().clone() for p in ps]
    ptrs, v0 = [p.data_ptr() for p in ps], [weight_version(p) for p in ps]
    with opt.ema_weights():
        v1 = [weight_version(p) for p in ps]
        assert all(a != b for a, b in zip(v0, v1)) and [p.data_ptr() for p in ps] == ptrs
        for p, e in zip(ps, got["e"]):
            assert torch.equal(p.detach().cpu(), e)
    assert all(a != b for a, b in zip(v1, [weight_version(p) for p in ps]))
    for p, w in zip(ps, live):
        assert torch.equal(p.detach().view(torch.int32), w.view(torch.int32))
    _bits_equal(_planes(opt, ps), got, "after the swap back")


# ---------------------------------------------------------------------------------------------------------
# a small trunk-free model: AudioCNN over log-mel + a feature-level video stub + the xattn head
# ---------------------------------------------------------------------------------------------------------
class _StubVideo(nn.Module):
    """Feature-level stand-in for VideoNet (the pattern of tests/test_audionet_gpu.py)."""

    def __init__(self, dim=512, num_classes=8):
        super().__init__()
        from tests.gpu_helpers import IdentityBackbone

        self.embedding_dim = dim
        self.backbone = IdentityBackbone()
        self.classifier = nn.Linear(dim, num_classes)

    def encode(self, x):
        return x


def _model(seed=7, deterministic=False):
    from multimodalemotionrecognition_amd.audio import AudioNet
    from multimodalemotionrecognition_amd.fusion import FusionModel

    torch.manual_seed(seed)
    m = FusionModel(AudioNet(num_classes=8, use_resnet=False, spec_augment=not deterministic), _StubVideo(),
                    num_classes=8, mode="xattn", audio_n_mels=64).to(DEV)
    if deterministic:  # no dropout anywhere: the data-parallel comparison is bitwise across processes
        m.attn_dropout = 0.0
        m.v_drop_path.drop_prob = m.a_drop_path.drop_prob = 0.0
        m.xattn_mlp[2].p = 0.0
    return m


def _batch(seed, B=4, T=301):
    g = torch.Generator().manual_seed(seed)
    video = torch.randn(B, 8, 512, 1, 1, generator=g)
    audio = torch.randn(B, 1, 64, T, generator=g) * 15.0 - 40.0
    labels = torch.randint(0, 8, (B,), generator=g)
    return video.to(DEV), audio.to(DEV), labels.to(DEV)


def _train_steps(m, opt, seeds):
    from multimodalemotionrecognition_amd.train import TrainStep, make_loss

    step = TrainStep(m, opt, make_loss("xattn"), "xattn")
    for s in seeds:
        torch.manual_seed(1000 + s)  # SpecAugment and the dropout seeds are host-drawn
        step(*_batch(s))
    torch.cuda.synchronize()


def _opt_state(opt):
    out = {k: [f[k].cpu().clone() for f in opt._flat] for k in ("flat", "m", "v", "ema")}
    out["steps"] = opt.state_steps()
    return out


def test_eval_forward_uses_the_average_inside_the_context():
    from multimodalemotionrecognition_amd.train import build_optimizer

    m = _model()
    opt = build_optimizer(m, max_grad_norm=1.0, ema_decay=0.5)
    _train_steps(m, opt, (1, 2, 3))
    video, audio, _ = _batch(9)
    m.eval()
    with torch.no_grad():
        live = m(video, audio).clone()
        with opt.ema_weights():
            avg = m(video, audio).clone()
        again = m(video, audio).clone()
    assert bool(torch.isfinite(avg).all()) and not torch.equal(avg, live)
    assert torch.equal(again, live)  # every derived weight copy was refreshed on the way back


def test_resume_is_bit_identical(tmp_path):
    from multimodalemotionrecognition_amd.train import build_optimizer, load_training_state, save_checkpoint

    kw = dict(max_grad_norm=1.0, ema_decay=0.99)
    ma = _model(7)
    oa = build_optimizer(ma, **kw)
    _train_steps(ma, oa, (1, 2))
    save_checkpoint(ma, tmp_path / "state.pt", 0.25, {"fusion": "xattn"}, optimizer=oa, epoch=1)
    at_save = oa.state_steps()
    _train_steps(ma, oa, (3, 4))
    mb = _model(8)  # other initial weights: everything must come from the file
    ob = build_optimizer(mb, **kw)
    assert load_training_state(tmp_path / "state.pt", mb, ob) == {"epoch": 1, "best_f1": 0.25}
    assert ob.state_steps() == at_save and max(s for g in at_save for s in g) == 2
    _train_steps(mb, ob, (3, 4))
    a, b = _opt_state(oa), _opt_state(ob)
    assert a["steps"] == b["steps"] and max(s for g in a["steps"] for s in g) == 4
    for k in ("flat", "m", "v", "ema"):
        for x, y in zip(a[k], b[k]):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), k
    sa, sb = ma.state_dict(), mb.state_dict()
    for k in sa:  # BatchNorm running statistics travel in the model's state dict
        assert torch.equal(sa[k], sb[k]), k
    print("resume: grad norms", oa.grad_norm_stats(), ob.grad_norm_stats())


def test_fit_reports_grad_norm_and_checkpoints_the_average(tmp_path, monkeypatch):
    from multimodalemotionrecognition_amd import train

    m = _model()
    opt = train.build_optimizer(m, max_grad_norm=1.0, ema_decay=0.9)
    loader = [_batch(20 + i) for i in range(4)]
    val = [_batch(30), _batch(31)]
    saved = {}
    real_save = train.save_checkpoint

    def save(model, path, f1, config=None, **kw):  # fit looks save_checkpoint up at call time
        saved.update(swapped=opt._ema_swapped, avg=[f.clone() for f in opt.flat_params()],
                     live=[f.clone() for f in opt.flat_ema()])
        real_save(model, path, f1, config, **kw)

    monkeypatch.setattr(train, "save_checkpoint", save)
    torch.manual_seed(5)
    out = train.fit(m, loader, val, opt, DEV, train.make_loss("xattn"), "xattn", 2, checkpoint_path=tmp_path / "best.pt",
                    config={"fusion": "xattn"}, early_stopping_patience=0, ema_eval=True, save_optimizer=True)
    assert out["epochs_run"] == 2 and not opt._ema_swapped
    for h in out["history"]:
        t = h["train"]
        print("fit epoch", {k: t[k] for k in ("loss", "grad_norm", "grad_norm_max", "nonfinite_steps")})
        assert 0.0 < t["grad_norm"] <= t["grad_norm_max"] and t["nonfinite_steps"] == 0
    assert opt.grad_norm_stats()["steps"] == 0  # read and reset once per epoch
    ckpt = torch.load(tmp_path / "best.pt", weights_only=True)
    assert {"model", "val_f1", "config", "optimizer", "epoch", "best_f1"} == set(ckpt)
    assert ckpt["epoch"] == out["best_epoch"] and ckpt["best_f1"] == out["best_f1"]
    assert saved["swapped"]
    names = {id(p): n for n, p in m.named_parameters()}
    checked = 0
    for gi, p, o, n in opt.param_slices():
        got = ckpt["model"][names[id(p)]].reshape(-1)
        assert torch.equal(got, saved["avg"][gi][o:o + n].cpu()), names[id(p)]
        checked += int(not torch.equal(got, saved["live"][gi][o:o + n].cpu()))
    assert checked > len(opt.param_slices()) // 2, "the average must differ from the live weights"
    if out["best_epoch"] == 2:  # saved after the last epoch: the file holds the EMA plane as it stands now
        for gi, p, o, n in opt.param_slices():
            assert torch.equal(ckpt["model"][names[id(p)]].reshape(-1), opt.flat_ema()[gi][o:o + n].cpu())
    # without clipping the metrics keep their old keys
    m3 = _model(3)
    plain = train.train_one_epoch(m3, loader[:1], train.build_optimizer(m3), DEV, train.make_loss("xattn"), "xattn")
    assert "grad_norm" not in plain


# ---------------------------------------------------------------------------------------------------------
# data parallel, world 2 on one device (gloo over device tensors), modelled on tests/test_dp_gpu.py
# ---------------------------------------------------------------------------------------------------------
DP_STEPS, DP_MAX_NORM = 2, 0.5


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_build():
    from multimodalemotionrecognition_amd.train import build_optimizer

    m = _model(1234, deterministic=True).train()
    return m, build_optimizer(m, lr=1e-3, weight_decay=1e-4, max_grad_norm=DP_MAX_NORM, ema_decay=0.99)


def _dp_record(opt):
    return {"flat": [f.cpu() for f in opt.flat_params()], "ema": [f.cpu() for f in opt.flat_ema()],
            "m": [f["m"].cpu() for f in opt._flat], "rec": opt._clip_rec.cpu()}


def _dp_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist

    from multimodalemotionrecognition_amd.dist import GradAllReduce, init_distributed
    from multimodalemotionrecognition_amd.train import TrainStep, make_loss

    try:
        init_distributed(backend="gloo")
        m, opt = _dp_build()
        step = TrainStep(m, opt, make_loss("xattn"), "xattn", GradAllReduce(opt, model=m))
        for s in range(DP_STEPS):
            step(*_batch(100 + 10 * rank + s))
        torch.cuda.synchronize()
        torch.save(_dp_record(opt), os.path.join(out_dir, f"rank{rank}.pt"))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_dp_world2_clipped_replicas_are_bit_identical(tmp_path):
    port = _free_port()
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=300)
        assert p.exitcode == 0
    r0 = torch.load(tmp_path / "rank0.pt", weights_only=True)
    r1 = torch.load(tmp_path / "rank1.pt", weights_only=True)

    def same(a, b, what):
        for k in ("flat", "ema", "m"):
            for x, y in zip(a[k], b[k]):
                assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (what, k)
        assert torch.equal(a["rec"].view(torch.int32), b["rec"].view(torch.int32)), (what, a["rec"], b["rec"])

    same(r0, r1, "replicas diverged")
    # single process: every step applies the mean of the two ranks' gradients, clipped as ONE averaged gradient
    from multimodalemotionrecognition_amd.losses import CrossEntropyLoss

    m, opt = _dp_build()
    loss_fn = CrossEntropyLoss()
    opt.grad_scale = 0.5
    for s in range(DP_STEPS):
        opt.zero_grad()
        v, a, y = _batch(100 + s)
        loss_fn(m(v, a), y).backward()
        g0 = [f.clone() for f in opt.flat_grads()]
        opt.zero_grad()
        v, a, y = _batch(110 + s)
        loss_fn(m(v, a), y).backward()
        for f, g in zip(opt.flat_grads(), g0):
            f.add_(g)
        opt.step()
    torch.cuda.synchronize()
    single = _dp_record(opt)
    print("dp clip record", single["rec"].tolist())
    same(single, r0, "DP step != mean-gradient step")
    assert float(single["rec"][2]) == DP_STEPS and float(single["rec"][1]) < 1.0, "the run must really clip"

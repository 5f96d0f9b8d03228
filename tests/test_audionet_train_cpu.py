"""Training of the mel audio path, host side: SpecAugment's draws against goldens of the imported reference
(tools/gen_golden_mel_train.py), the argument checks of csrc/audionet_train.hip's entry points (they return before any
HIP call, so they run here), and the optimizer's parameter order over a mel model."""
from pathlib import Path

import numpy as np
import pytest
import torch

from multimodalemotionrecognition_amd.audio import SpecAugment

GOLD = Path(__file__).resolve().parent / "golden"


def _keep_mask(bands, n_mels, T):
    keep = np.ones((n_mels, T), dtype=bool)
    if bands is not None:
        for s, n in bands[0]:
            keep[s:s + n, :] = False
        for s, n in bands[1]:
            keep[:, s:s + n] = False
    return keep


def test_draws_match_the_reference():
    """Under each seed ``draw`` zeroes the reference's bands and leaves the generator where the reference left it."""
    g = np.load(GOLD / "spec_augment_draws.npz")
    aug = SpecAugment(20, 40, p=0.5).train()
    applied = 0
    for seed in range(g["keep"].shape[0]):
        torch.manual_seed(seed)
        bands = aug.draw(64, 301)
        assert float(torch.rand(1)) == float(g["next_rand"][seed]), seed
        assert np.array_equal(_keep_mask(bands, 64, 301), g["keep"][seed]), seed
        if bands is not None:
            assert len(bands[0]) <= 2 and len(bands[1]) <= 2
            applied += 1
    assert 4 <= applied <= g["keep"].shape[0] - 4  # neither branch alone passes this test


def test_draws_fail_where_the_reference_fails():
    """T = 37 with time_mask_param = 40: a drawn length >= 37 leaves randint an empty range; torch's own error."""
    g = np.load(GOLD / "spec_augment_draws.npz")
    aug = SpecAugment(20, 40, p=0.5).train()
    raised = []
    for seed in range(40):
        torch.manual_seed(seed)
        try:
            aug.draw(64, 37)
        except RuntimeError:
            raised.append(seed)
    assert raised == g["raises_37"].tolist() and len(raised) >= 1


def test_draw_limits_and_eval_identity():
    with pytest.raises(ValueError, match="num_masks"):
        SpecAugment(num_masks=9).train().draw(64, 301)
    state = torch.get_rng_state()
    x = torch.zeros(2, 1, 64, 37)
    assert SpecAugment().eval()(x) is x and torch.equal(torch.get_rng_state(), state)
    with pytest.raises(NotImplementedError, match="training"):  # a host tensor: refused before any draw
        SpecAugment().train()(x)
    assert torch.equal(torch.get_rng_state(), state)
    aug = SpecAugment(0, 0, p=1.0).train()  # no parameter > 0: one rand, no bands
    assert aug.draw(64, 37) == ([], [])


def test_argument_checks_reject_before_any_launch():
    """Every new entry point returns hipErrorInvalidValue (1) on a bad argument before any HIP call."""
    import ctypes

    from multimodalemotionrecognition_amd._lib import LIB

    LIB.load()
    f = LIB._fns
    fake = 1 << 20  # never dereferenced
    # mer_audiocnn_train_conv(B,H,W,Cin,Cout,transposed, x,w,bias,wpack,z, stream)
    conv = f["mer_audiocnn_train_conv"]
    assert conv(2, 8, 8, 1, 16, 0, None, fake, fake, None, fake, None) == 1
    assert conv(2, 8, 8, 1, 16, 0, fake, fake, fake, None, None, None) == 1
    assert conv(2, 8, 8, 16, 32, 0, fake, fake, fake, None, fake, None) == 1  # MFMA layers need wpack
    assert conv(2, 8, 8, 16, 64, 0, fake, fake, fake, fake, fake, None) == 1  # not a layer of AudioCNN
    assert conv(2, 8, 8, 16, 32, 1, fake, fake, None, fake, fake, None) == 1  # no such data gradient
    assert conv(2, 8, 8, 1, 16, 1, fake, fake, None, fake, fake, None) == 1
    assert conv(0, 8, 8, 1, 16, 0, fake, fake, fake, None, fake, None) == 1
    assert conv(2, 0, 8, 1, 16, 0, fake, fake, fake, None, fake, None) == 1
    assert conv(1 << 30, 64, 64, 32, 64, 0, fake, fake, fake, fake, fake, None) == 1  # grid overflow
    # mer_bn_train_stats(B,C,HW, z,gamma,beta, eps,momentum, part,ss, rmean,rvar,nbt, stream)
    st = f["mer_bn_train_stats"]
    assert st(1, 16, 1, fake, fake, fake, 1e-5, 0.1, fake, fake, fake, fake, fake, None) == 1  # one value per channel
    assert st(2, 16, 4, None, fake, fake, 1e-5, 0.1, fake, fake, fake, fake, fake, None) == 1
    assert st(2, 16, 4, fake, None, fake, 1e-5, 0.1, fake, fake, fake, fake, fake, None) == 1
    assert st(2, 16, 4, fake, fake, fake, 1e-5, 0.1, None, fake, fake, fake, fake, None) == 1
    assert st(2, 16, 4, fake, fake, fake, 1e-5, 0.1, fake, None, fake, fake, fake, None) == 1
    assert st(2, 16, 4, fake, fake, fake, 1e-5, 1.5, fake, fake, fake, fake, fake, None) == 1
    assert st(1 << 20, 1 << 12, 4, fake, fake, fake, 1e-5, 0.1, fake, fake, fake, fake, fake, None) == 1
    # mer_bn_relu_pool_fwd(B,C,H,W,pool, z,ss,y, stream)
    fw = f["mer_bn_relu_pool_fwd"]
    assert fw(2, 16, 8, 8, 1, None, fake, fake, None) == 1
    assert fw(2, 16, 8, 8, 1, fake, None, fake, None) == 1
    assert fw(2, 16, 8, 8, 1, fake, fake, None, None) == 1
    assert fw(2, 16, 1, 8, 1, fake, fake, fake, None) == 1  # nothing to pool
    assert fw(0, 16, 8, 8, 0, fake, fake, fake, None) == 1
    # mer_bn_relu_pool_bwd(B,C,H,W,pool, z,ss,g, part, dgamma,dbeta,dbias, dz, x,dw1, stream)
    bw = f["mer_bn_relu_pool_bwd"]
    assert bw(2, 16, 8, 8, 1, None, fake, fake, fake, fake, fake, fake, fake, None, None, None) == 1
    assert bw(2, 16, 8, 8, 1, fake, fake, fake, None, fake, fake, fake, fake, None, None, None) == 1
    assert bw(2, 16, 8, 8, 1, fake, fake, fake, fake, fake, fake, fake, None, None, None, None) == 1  # no dz, no x
    assert bw(2, 16, 8, 8, 1, fake, fake, fake, fake, fake, fake, fake, None, fake, None, None) == 1  # x without dw1
    assert bw(2, 16, 8, 8, 1, fake, fake, fake, fake, fake, fake, fake, fake, fake, fake, None) == 1  # dz and x
    assert bw(1, 16, 1, 1, 0, fake, fake, fake, fake, fake, fake, fake, fake, None, None, None) == 1  # one value
    assert bw(2, 16, 1, 8, 1, fake, fake, fake, fake, fake, fake, fake, fake, None, None, None) == 1
    # mer_audiocnn_wgrad(B,H,W,Cin,Cout, x,dz,part,dw, stream)
    wg = f["mer_audiocnn_wgrad"]
    assert wg(2, 8, 8, 16, 32, None, fake, fake, fake, None) == 1
    assert wg(2, 8, 8, 16, 32, fake, fake, None, fake, None) == 1
    assert wg(2, 8, 8, 16, 32, fake, fake, fake, None, None) == 1
    assert wg(2, 8, 8, 1, 16, fake, fake, fake, fake, None) == 1  # layer 1 goes through mer_bn_relu_pool_bwd
    assert wg(2, 8, 8, 32, 32, fake, fake, fake, fake, None) == 1
    assert wg(1 << 30, 64, 64, 32, 64, fake, fake, fake, fake, None) == 1
    # mer_adaptive_avgpool_seq_bwd(B,C,H,W,bins, g,dx, stream)
    ap = f["mer_adaptive_avgpool_seq_bwd"]
    assert ap(2, 64, 5, 9, 16, None, fake, None) == 1
    assert ap(2, 64, 5, 9, 16, fake, None, None) == 1
    assert ap(2, 64, 5, 9, 0, fake, fake, None) == 1
    assert ap(2, 64, 0, 9, 16, fake, fake, None) == 1
    # mer_spec_augment_mask(planes,n_mels,T, x,y, n_freq,freq_bands, n_time,time_bands, stream)
    sa = f["mer_spec_augment_mask"]
    ok = (ctypes.c_int * 4)(3, 5, 10, 2)
    ptr = ctypes.cast(ok, ctypes.c_void_p)
    assert sa(2, 64, 37, None, fake, 1, ptr, 1, ptr, None) == 1
    assert sa(2, 64, 37, fake, fake, 1, ptr, 1, ptr, None) == 1  # in place
    assert sa(2, 64, 37, fake, fake + 4096, 9, ptr, 0, None, None) == 1  # more than 8 bands
    assert sa(2, 64, 37, fake, fake + 4096, 1, None, 0, None, None) == 1
    out = (ctypes.c_int * 2)(30, 8)  # 30 + 8 > 37
    assert sa(2, 64, 37, fake, fake + 4096, 0, None, 1, ctypes.cast(out, ctypes.c_void_p), None) == 1
    neg = (ctypes.c_int * 2)(-1, 4)
    assert sa(2, 64, 37, fake, fake + 4096, 1, ctypes.cast(neg, ctypes.c_void_p), 0, None, None) == 1
    assert sa(0, 64, 37, fake, fake + 4096, 0, None, 0, None, None) == 1


def test_wrapper_constants_match_the_header():
    import re

    from multimodalemotionrecognition_amd import kernels as K
    from multimodalemotionrecognition_amd._lib import _HEADER

    text = _HEADER.read_text()
    assert int(re.search(r"#define\s+MER_AUDIOCNN_WGRAD_WGS\s+(\d+)", text).group(1)) == K.AUDIOCNN_WGRAD_WGS
    assert int(re.search(r"#define\s+MER_SPEC_AUGMENT_MAX_BANDS\s+(\d+)", text).group(1)) == K.SPEC_AUGMENT_MAX_BANDS
    assert int(re.search(r"#define\s+MER_BN_PLANE_CHUNK\s+(\d+)", text).group(1)) == K.BN_PLANE_CHUNK
    assert K.audiocnn_wgrad_rows(32, 32, 150, 32) == 512 and K.audiocnn_wgrad_rows(2, 5, 9, 64) == 4


def test_optimizer_order_holds_the_encoder():
    from multimodalemotionrecognition_amd.train import build_model, build_optimizer_param_order

    m = build_model(8, "xattn", use_wavlm=False, use_resnet_audio=False, pretrained_video=False)
    order = build_optimizer_param_order(m)
    ids = [id(p) for p in order]
    enc = [id(p) for p in m.audio_model.encoder.parameters()]
    assert len(enc) == 14 and all(i in ids for i in enc)
    first_enc = min(ids.index(i) for i in enc)
    named = {n: p for n, p in m.named_parameters() if id(p) in ids}  # the mode's unused parameters are left out
    head = [ids.index(id(p)) for n, p in named.items() if not n.startswith(("audio_model.", "video_model."))]
    video = [ids.index(id(p)) for n, p in named.items() if n.startswith("video_model.")]
    assert head and video and max(head) < first_enc and max(video) < first_enc

"""Incremental im2col addressing of the pipelined convolutions: conv_pipe_kernel's scalar tap walk (csrc/conv.hip:
forward, stride-1 and parity-class input gradients, the fused downsample segment) and wgrad_pipe_kernel's pixel
walk (csrc/conv_wgrad.hip), at the smallest shapes where a hoisted address can go wrong.  The register-staged kernels
(conv variant 0, wgrad variant 1) compute every address from scratch and are the bit-exact reference; torch is
checked with the bars of tests/test_resnet_gpu.py."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

RING = (1, 2, 3, 4, 5)  # pipelined conv variants with the reference's K order; 7 = two K-groups (fp32 sum splits)


def rel_rms(y, ref):
    y, ref = y.detach().float().cpu(), ref.detach().float().cpu()
    return float((y - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt().clamp_min(1e-12))


def nchw(t):
    return t.float().permute(0, 3, 1, 2)


@pytest.mark.parametrize("N,H,C,Kc,R,stride,pad", [
    (2, 7, 64, 64, 3, 1, 1),     # IC == K-step: every step a new tap; M = 98 < one tile
    (3, 9, 128, 192, 3, 1, 1),   # two steps per tap, column tail, odd width
    (2, 9, 64, 128, 3, 2, 1),    # strided forward; parity classes of unequal size (5x5, 5x4, 4x5, 4x4)
    (2, 8, 64, 128, 1, 2, 0),    # 1x1 stride-2: empty parity classes
    (2, 12, 64, 64, 3, 1, 1),    # variant 5: the 32-wide K-step, two steps per tap
    (3, 17, 16, 24, 3, 1, 1),    # IC = 16: the generic staging
    (2, 30, 8, 64, 7, 2, 3)])    # fwd: 49 taps, IC = 8 -> generic staging; dgrad: IC = 64, 16 taps per class -> walks
def test_conv_fwd_dgrad_addressing(N, H, C, Kc, R, stride, pad):
    from multimodalemotionrecognition_amd import kernels as K

    torch.manual_seed(21)
    Ho = (H + 2 * pad - R) // stride + 1
    x = torch.randn(N, H, H, C, device="cuda").bfloat16()
    w = torch.randn(Kc, C, R, R, device="cuda") / (C * R * R) ** 0.5
    wp = torch.empty(Kc, R * R * C, device="cuda", dtype=torch.bfloat16)
    K.pack_conv_weight(w, wp, C, False)
    wt = torch.empty(C, R * R * Kc, device="cuda", dtype=torch.bfloat16)
    K.pack_conv_weight(w, wt, C, True)
    wr = w.bfloat16().float()

    def fwd(v):
        y = torch.full((N, Ho, Ho, Kc), float("nan"), device="cuda", dtype=torch.bfloat16)
        st = K.bn_stats_buffer(Kc, "cuda", N * Ho * Ho)
        K.conv_fwd(x, wp, y, st, R, R, stride, pad, variant=v)
        return y, st.sum(0)

    y0, s0 = fwd(0)
    assert rel_rms(y0, F.conv2d(nchw(x), wr, stride=stride, padding=pad).permute(0, 2, 3, 1)) < 1e-2
    for v in RING:
        y, s = fwd(v)
        assert torch.equal(y0, y), f"fwd variant {v}"
        assert torch.allclose(s0, s, rtol=1e-5, atol=1e-3), f"fwd stats variant {v}"
    (yk, sk), (yk2, sk2) = fwd(7), fwd(7)
    assert torch.equal(yk, yk2) and torch.equal(sk, sk2)
    assert rel_rms(yk, y0) < 4e-3
    assert (yk.float() - y0.float()).abs().max() <= 2 ** -6 * y0.float().abs().max()
    assert torch.allclose(sk, s0, rtol=1e-3, atol=0.5)

    dy = torch.randn(N, Ho, Ho, Kc, device="cuda").bfloat16()
    res = torch.randn(N, H, H, C, device="cuda").bfloat16()
    mask = torch.randn(N, H, H, C, device="cuda").bfloat16()
    xb = torch.randn(N, H, H, C, device="cuda").bfloat16()
    xb2 = torch.randn(N, H, H, C, device="cuda").bfloat16()
    ms = torch.stack([torch.randn(C), torch.rand(C) + 0.5], 1).cuda().contiguous()
    ms2 = torch.stack([torch.randn(C), torch.rand(C) + 0.5], 1).cuda().contiguous()

    def dgrad(v, fused=False, **kw):
        dx = torch.full((N, H, H, C), float("nan"), device="cuda", dtype=torch.bfloat16)
        if not fused:
            K.conv_dgrad(dy, wt, dx, R, R, stride, pad, variant=v, **kw)
            return dx
        rows = K.bn_red_rows(N * H * H)
        red, red2 = torch.zeros(rows, C, 2, device="cuda"), torch.zeros(rows, C, 2, device="cuda")
        K.conv_dgrad(dy, wt, dx, R, R, stride, pad, variant=v, bnr=(mask, xb, ms, red, xb2, ms2, red2), **kw)
        return dx, red, red2

    plain = dgrad(0)
    gx = torch.nn.grad.conv2d_input((N, C, H, H), wr, nchw(dy), stride=stride, padding=pad).permute(0, 2, 3, 1)
    assert rel_rms(plain, gx) < 1e-2
    d0 = dgrad(0, residual=res, mask=mask)
    # the standalone BN-backward sums over the stored gradient: what the fused epilogue must reproduce
    ref1, ref2 = torch.zeros(C, 2, device="cuda"), torch.zeros(C, 2, device="cuda")
    K.bn_bwd_reduce(d0, mask, xb, ms, ref1)
    K.bn_bwd_reduce(d0, mask, xb2, ms2, ref2)
    for v in RING:
        assert torch.equal(plain, dgrad(v)), f"dgrad variant {v}"
        assert torch.equal(d0, dgrad(v, residual=res, mask=mask)), f"dgrad + residual variant {v}"
        dx, red, red2 = dgrad(v, True, residual=res, mask=mask)
        assert torch.equal(d0, dx), f"dgrad + bnr variant {v}"
        assert torch.allclose(K.partials_sum(red, torch.empty(C, 2, device="cuda")), ref1, rtol=1e-4, atol=1e-3), v
        assert torch.allclose(K.partials_sum(red2, torch.empty(C, 2, device="cuda")), ref2, rtol=1e-4, atol=1e-3), v
    a, b = dgrad(7, True, residual=res, mask=mask), dgrad(7, True, residual=res, mask=mask)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    assert rel_rms(a[0], d0) < 4e-3
    assert torch.allclose(a[1].sum(0), ref1, rtol=1e-3, atol=0.5) and torch.allclose(a[2].sum(0), ref2, rtol=1e-3, atol=0.5)


def test_stride2_dgrad_more_than_32_class_taps():
    """An 11x11 stride-2 input gradient: parity class (1, 1) has 6 x 6 = 36 taps, more than the scalar walk's one
    validity bit per tap holds, so the launcher must keep it on the generic staging (IC = 64 alone would allow the
    walk).  Against the register-staged kernel bit for bit, and torch."""
    from multimodalemotionrecognition_amd import kernels as K

    torch.manual_seed(23)
    N, H, C, Kc, R, stride, pad = 1, 12, 8, 64, 11, 2, 5
    Ho = (H + 2 * pad - R) // stride + 1
    w = torch.randn(Kc, C, R, R, device="cuda") / (C * R * R) ** 0.5
    wt = torch.empty(C, R * R * Kc, device="cuda", dtype=torch.bfloat16)
    K.pack_conv_weight(w, wt, C, True)
    dy = torch.randn(N, Ho, Ho, Kc, device="cuda").bfloat16()

    def dgrad(v):
        dx = torch.full((N, H, H, C), float("nan"), device="cuda", dtype=torch.bfloat16)
        K.conv_dgrad(dy, wt, dx, R, R, stride, pad, variant=v)
        return dx

    d0 = dgrad(0)
    gx = torch.nn.grad.conv2d_input((N, C, H, H), w.bfloat16().float(), nchw(dy), stride=stride, padding=pad)
    assert rel_rms(d0, gx.permute(0, 2, 3, 1)) < 1e-2
    for v in RING:
        assert torch.equal(d0, dgrad(v)), f"variant {v}"
    assert rel_rms(dgrad(7), d0) < 4e-3


@pytest.mark.parametrize("C,Kc,H", [(64, 128, 9), (128, 256, 8)])  # odd / even input size
def test_dgrad_fused_downsample_addressing(C, Kc, H):
    """mer_conv_dgrad_ds on every pipelined variant: the switch from the 3x3 taps to the downsample segment inside
    parity class (0, 0), against torch's sum of the two branches and the two-launch form."""
    from multimodalemotionrecognition_amd import kernels as K

    torch.manual_seed(C)
    N = 2
    Ho = (H + 2 - 3) // 2 + 1
    dy = torch.randn(N, Kc, Ho, Ho).bfloat16().float()
    dyd = torch.randn(N, Kc, Ho, Ho).bfloat16().float()
    w = (torch.randn(Kc, C, 3, 3) / (9 * C) ** 0.5).bfloat16().float()
    wd = (torch.randn(Kc, C, 1, 1) / C ** 0.5).bfloat16().float()
    ref = F.conv_transpose2d(dy, w, stride=2, padding=1, output_padding=1) + \
        F.conv_transpose2d(dyd, wd, stride=2, output_padding=1)
    ref = ref[:, :, :H, :H]
    wt = w.permute(1, 2, 3, 0).reshape(C, 9 * Kc).contiguous().cuda().bfloat16()  # [C][r][s][k]
    wdt = wd.reshape(Kc, C).t().contiguous().cuda().bfloat16()                   # [C][k]
    dyh = dy.permute(0, 2, 3, 1).contiguous().cuda().bfloat16()
    dydh = dyd.permute(0, 2, 3, 1).contiguous().cuda().bfloat16()
    dxd = torch.empty(N, H, H, C, device="cuda", dtype=torch.bfloat16)
    K.conv_dgrad(dydh, wdt, dxd, 1, 1, 2, 0, variant=0)
    two = torch.empty_like(dxd)
    K.conv_dgrad(dyh, wt, two, 3, 3, 2, 1, residual=dxd, variant=0)
    two = two.float().permute(0, 3, 1, 2).cpu()
    outs = {}
    for v in RING + (7, 7):
        dx = torch.full((N, H, H, C), float("nan"), device="cuda", dtype=torch.bfloat16)
        K.conv_dgrad(dyh, wt, dx, 3, 3, 2, 1, ds=(dydh, wdt), variant=v)
        if v in outs:
            assert torch.equal(outs[v], dx)  # repeatable
        outs[v] = dx
        got = dx.float().permute(0, 3, 1, 2).cpu()
        assert rel_rms(got, ref) < 4e-3, (v, rel_rms(got, ref))
        assert rel_rms(got, two) < 6e-3, v
    for v in RING[1:]:  # one K order on every one-group tile
        assert torch.equal(outs[RING[0]], outs[v]), f"variant {v}"


@pytest.mark.parametrize("N,H,C,Kc,R,stride,pad,splits", [
    (5, 7, 256, 256, 3, 1, 1, 3),  # Ho*Wo = 49 < 64: a K-step spans two images; P = 245: pixel tail, mid-image splits
    (3, 9, 64, 64, 3, 1, 1, 2),    # a 128-column tile spans two taps
    (2, 9, 64, 128, 3, 2, 1, 2),   # strided, odd input
    (2, 8, 64, 128, 1, 2, 0, 2)])  # 1x1 stride-2; one K-step: the second K-group idles
def test_wgrad_addressing(N, H, C, Kc, R, stride, pad, splits):
    from multimodalemotionrecognition_amd import kernels as K

    torch.manual_seed(22)
    Ho = (H + 2 * pad - R) // stride + 1
    x = torch.randn(N, H, H, C, device="cuda").bfloat16()
    dy = torch.randn(N, Ho, Ho, Kc, device="cuda").bfloat16()

    def wgrad(v):
        dw = torch.zeros(Kc, C, R, R, device="cuda")
        K.conv_wgrad(x, dy, dw, R, R, stride, pad, variant=v, splits=splits)
        return dw

    d1 = wgrad(1)
    dw_ref = torch.nn.grad.conv2d_weight(nchw(x), (Kc, C, R, R), nchw(dy), stride=stride, padding=pad)
    scale = float(dw_ref.abs().max())
    assert (d1 - dw_ref).abs().max() <= 5e-3 * scale + 1e-3
    for v in (4, 5, 6, 7):
        assert torch.equal(d1, wgrad(v)), f"variant {v} differs"
    a, b = wgrad(8), wgrad(8)
    assert torch.equal(a, b)
    assert (a - dw_ref).abs().max() <= 5e-3 * scale + 1e-3
    assert (a - d1).abs().max() <= 2e-5 * scale + 1e-6  # same splits: only the in-workgroup split point differs

"""Each kernel of csrc/bn_pool.hip -- BatchNorm finalize / apply / backward reduce / backward apply, the partial-row
folds, the max and average pools, the fused stem tail -- against its float64 restatement (tests/kernel_parity.py), at
the shapes where its code takes another path: the row counts at which the finalize changes launch, C / 8 that does and
does not divide the block, the dead rows of the four-rows-in-flight loop, tails, more than one block, ties in the pool.

fp32 outputs meet ``assert_fp64_parity``; bf16 outputs meet ``assert_bf16_parity`` (the bf16 rounding of something
within the float32 bar of the reference -- no bf16 tolerance).  Outputs live in marker- or NaN-filled buffers, so an
element never written, or written outside the view, shows.  The last three tests run the pooling kernels past 2^23
16-byte chunks, where a float-reciprocal split of the chunk index is no longer exact.
"""
import functools

import pytest
import torch

from multimodalemotionrecognition_amd import kernels as K
from multimodalemotionrecognition_amd._lib import MerKernelError
from tests import kernel_parity as kp
from tests.kernel_parity import (BF16, F32, F64, GuardedBf16, assert_bf16_parity, assert_fp64_parity, bf16_values, gen,
                                 guarded_flat, randn, to_bf16)

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS, MOM = 1e-5, 0.1
NAN = float("nan")


def both(fn):
    """(float64, float32) evaluations of one restatement."""
    return fn(F64), fn(F32)


def dbf(t):
    """A bf16-valued float32 CPU tensor as a bf16 device tensor."""
    return t.to(BF16).to(DEV).contiguous()


def d32(t):
    return t.to(F32).to(DEV).contiguous()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def rand_pos(g, *shape):
    return torch.rand(*shape, generator=g, dtype=F32) + 0.5


def bn_params(g, C, mean_shift=0.5):
    """(ms, gamma, beta): mean near the data's, rstd and gamma in [0.5, 1.5)."""
    ms = torch.stack([mean_shift + randn(g, C) * 0.2, rand_pos(g, C)], 1).contiguous()
    return ms, rand_pos(g, C), randn(g, C) * 0.2


# ---------------------------------------------------------------------------------------------------------
# bn_finalize / bn_finalize_pair
# ---------------------------------------------------------------------------------------------------------
# data-row counts on both sides of every launch change: <= 64 one kernel; the wide kernel with 16 / 32 / 64 loads per
# thread up to 256 / 512 / 1024 rows (wide_pick); the two-stage fold above 1024
FIN_ROWS = [1, 3, 64, 65, 256, 257, 512, 513, 1024, 1025]
FIN_C = [8, 24, 72, 512]  # 2 C below, straddling and a multiple of the 64 columns of a block


@functools.lru_cache(maxsize=2)
def fin_tensor_stats(rows, shift=0.5):
    """(M, statistics rows [rows, 512, 2]) of one bf16 x[M = 64 rows - 63, 512]; a narrower C takes its first channels,
    so the reference mean and variance are those of an actual tensor."""
    M = 64 * rows - 63
    return M, kp.tile_stats(bf16_values(gen(5000 + rows), M, 512, shift=shift))


def finalize_check(what, data, M, C, rows_arg, seed):
    """``data`` [n, C, 2]: the leading statistics rows.  The rows behind them hold NaN when ``rows_arg`` says how many
    were written and zeros otherwise (the contract); the scratch rows hold NaN either way."""
    g = gen(seed)
    all_rows = K.bn_stat_rows(M) - 64
    n = data.shape[0]
    assert n <= all_rows and (rows_arg is None or rows_arg == n)
    buf = torch.full((all_rows + 64, C, 2), NAN, dtype=F32)
    buf[:n] = data
    if rows_arg is None:
        buf[n:all_rows] = 0
    buf = buf.to(DEV)
    before = bits(buf[:all_rows])
    rm0, rv0 = randn(g, C) * 0.1, rand_pos(g, C)
    ms, rmean, rvar = guarded_flat((C, 2), DEV), guarded_flat((C,), DEV, init=rm0), guarded_flat((C,), DEV, init=rv0)
    nbt = torch.tensor([-7, 41, -7], dtype=torch.int64, device=DEV)
    K.bn_finalize(buf, M, EPS, MOM, ms.view, rmean.view, rvar.view, nbt[1:2], rows=rows_arg)
    r64, r32 = both(lambda dt: kp.ref_bn_finalize(data, M, EPS, MOM, rm0, rv0, dt))
    for t, name in ((ms, "ms"), (rmean, "rmean"), (rvar, "rvar")):
        t.check(f"{what} {name}")
    assert_fp64_parity(ms.view[:, 0], r64["mean"], r32["mean"], what=f"{what} mean")
    assert_fp64_parity(ms.view[:, 1], r64["rstd"], r32["rstd"], what=f"{what} rstd")
    assert_fp64_parity(rmean.view, r64["rmean"], r32["rmean"], what=f"{what} running mean")
    assert_fp64_parity(rvar.view, r64["rvar"], r32["rvar"], what=f"{what} running var")
    assert nbt.tolist() == [-7, 42, -7], f"{what}: num_batches_tracked must grow by exactly one"
    assert torch.equal(bits(buf[:all_rows]), before), f"{what}: the statistics rows were modified"


@pytest.mark.parametrize("C", FIN_C)
@pytest.mark.parametrize("rows", FIN_ROWS)
def test_bn_finalize(rows, C):
    M, st = fin_tensor_stats(rows)
    finalize_check(f"bn_finalize[{rows} rows, M={M}, C={C}]", st[:, :C].contiguous(), M, C, None, rows * 1000 + C)


@pytest.mark.parametrize("rows,C", [(3, 24), (257, 72), (1025, 8)])
def test_bn_finalize_mean_30_sigma(rows, C):
    """mean = 30 standard deviations: sumsq / M - mean^2 cancels five digits, and the float32 restatement, which loses
    them too, sets the bar."""
    M, st = fin_tensor_stats(rows, shift=30.0)
    data = st[:, :C].contiguous()
    mean, var = data[:, :, 0].double().sum(0) / M, data[:, :, 1].double().sum(0) / M
    assert float((mean / torch.sqrt(var - mean * mean)).min()) > 25
    finalize_check(f"bn_finalize[{rows} rows, C={C}, mean 30 sigma]", data, M, C, None, rows + C)


@pytest.mark.parametrize("all_rows,n,C", [(70, 40, 24), (300, 70, 72), (1100, 1030, 8)])
@pytest.mark.parametrize("passed", [True, False])
def test_bn_finalize_fewer_rows_than_the_buffer(all_rows, n, C, passed):
    M = 64 * all_rows
    data = kp.tile_stats(bf16_values(gen(all_rows + n), 64 * n, C, shift=0.5))
    finalize_check(f"bn_finalize[{n} of {all_rows} rows, C={C}, rows {'passed' if passed else 'not passed'}]", data, M,
                   C, n if passed else None, all_rows)


@pytest.mark.parametrize("C", FIN_C)
def test_bn_finalize_eval_form(C):
    g = gen(77 + C)
    rm0, rv0 = randn(g, C), rand_pos(g, C)
    ms, rmean, rvar = guarded_flat((C, 2), DEV), guarded_flat((C,), DEV, init=rm0), guarded_flat((C,), DEV, init=rv0)
    nbt = torch.tensor([41], dtype=torch.int64, device=DEV)
    K.bn_finalize(None, 4097, EPS, MOM, ms.view, rmean.view, rvar.view, nbt)
    r64, r32 = both(lambda dt: kp.ref_bn_finalize(None, 4097, EPS, MOM, rm0, rv0, dt))
    for t in (ms, rmean, rvar):
        t.check("bn_finalize eval")
    assert torch.equal(ms.view[:, 0].cpu(), rm0), "eval: the mean is the running mean, copied"
    assert_fp64_parity(ms.view[:, 1], r64["rstd"], r32["rstd"], what=f"bn_finalize[eval, C={C}] rstd")
    assert torch.equal(rmean.view.cpu(), rm0) and torch.equal(rvar.view.cpu(), rv0) and nbt.tolist() == [41], \
        "eval: nothing is updated"


@pytest.mark.parametrize("a,b", [((3, 24), (64, 72)), ((65, 24), (300, 72)), ((600, 8), (40, 512)),
                                 ((1025, 8), (3, 24))])
def test_bn_finalize_pair(a, b):
    """Two BatchNorms of different C and M in one launch, each against its own reference (the last pair takes the
    two-stage folds one after the other)."""
    recs, args = [], []
    for i, (rows, C) in enumerate((a, b)):
        g = gen(900 + rows + C)
        M, st = fin_tensor_stats(rows)
        data = st[:, :C].contiguous()
        buf = torch.full((rows + 64, C, 2), NAN, dtype=F32)
        buf[:rows] = data
        rm0, rv0 = randn(g, C) * 0.1, rand_pos(g, C)
        o = dict(ms=guarded_flat((C, 2), DEV), rmean=guarded_flat((C,), DEV, init=rm0),
                 rvar=guarded_flat((C,), DEV, init=rv0), nbt=torch.tensor([5 + i], dtype=torch.int64, device=DEV))
        recs.append((rows, C, M, data, rm0, rv0, o, buf.to(DEV)))
        args.append((recs[-1][7], M, o["ms"].view, o["rmean"].view, o["rvar"].view, o["nbt"], rows if i else None))
    K.bn_finalize_pair(args[0], args[1], EPS, MOM)
    for i, (rows, C, M, data, rm0, rv0, o, _) in enumerate(recs):
        what = f"bn_finalize_pair[{a},{b}] record {i}"
        r64, r32 = both(lambda dt: kp.ref_bn_finalize(data, M, EPS, MOM, rm0, rv0, dt))
        for k in ("ms", "rmean", "rvar"):
            o[k].check(what)
        assert_fp64_parity(o["ms"].view[:, 0], r64["mean"], r32["mean"], what=f"{what} mean")
        assert_fp64_parity(o["ms"].view[:, 1], r64["rstd"], r32["rstd"], what=f"{what} rstd")
        assert_fp64_parity(o["rmean"].view, r64["rmean"], r32["rmean"], what=f"{what} running mean")
        assert_fp64_parity(o["rvar"].view, r64["rvar"], r32["rvar"], what=f"{what} running var")
        assert o["nbt"].tolist() == [6 + i]


# ---------------------------------------------------------------------------------------------------------
# partials_sum / partials_sum_pair / fold_rows
# ---------------------------------------------------------------------------------------------------------
FOLD_PARTS = [1, 63, 64, 65, 1024, 1025]
FOLD_C = [3, 32, 200]


def parts_buffer(parts, C, seed):
    """A [parts + 64, C, 2] reduction buffer inside a marker-filled one: seeded data rows, NaN in the scratch rows."""
    data = randn(gen(seed), parts, C, 2) + 0.3
    buf = guarded_flat((parts + 64, C, 2), DEV, init=torch.cat([data, torch.full((64, C, 2), NAN)]))
    return data, buf


def parts_check(what, data, buf, out, parts):
    r64, r32 = both(lambda dt: kp.ref_rows_sum(data, None, dt))
    out.check(what)
    buf.check(what)  # everything past the scratch rows
    assert_fp64_parity(out.view, r64["out"], r32["out"], what=what)
    assert torch.equal(bits(buf.view[:parts]), bits(data)), f"{what}: the data rows were modified"
    if parts <= 1024:  # one launch reads the rows directly: the scratch rows are not used
        assert bool(torch.isnan(buf.view[parts:]).all()), f"{what}: scratch rows written by a one-launch fold"


@pytest.mark.parametrize("C", FOLD_C)
@pytest.mark.parametrize("parts", FOLD_PARTS)
def test_partials_sum(parts, C):
    data, buf = parts_buffer(parts, C, 7000 + parts + C)
    out = guarded_flat((C, 2), DEV)
    K.partials_sum(buf.view, out.view)
    parts_check(f"partials_sum[{parts} parts, C={C}]", data, buf, out, parts)


@pytest.mark.parametrize("parts,C", [(40, 32), (300, 3)])
def test_partials_sum_leading_rows_only(parts, C):
    """``rows`` passed: the rows behind them are not read (NaN here)."""
    data, buf = parts_buffer(parts, C, 7100 + parts)
    out = guarded_flat((C, 2), DEV)
    K.partials_sum(buf.view, out.view, rows=parts - 7)
    r64, r32 = both(lambda dt: kp.ref_rows_sum(data[:parts - 7], None, dt))
    out.check("partials_sum rows")
    assert_fp64_parity(out.view, r64["out"], r32["out"], what=f"partials_sum[{parts - 7} of {parts} parts, C={C}]")
    buf.view[parts - 7:parts].fill_(NAN)
    K.partials_sum(buf.view, out.view, rows=parts - 7)
    assert_fp64_parity(out.view, r64["out"], r32["out"], what=f"partials_sum[{parts - 7} of {parts} parts, C={C}, NaN]")


@pytest.mark.parametrize("C", FOLD_C)
@pytest.mark.parametrize("parts", FOLD_PARTS)
def test_partials_sum_pair(parts, C):
    da, ba = parts_buffer(parts, C, 7200 + parts + C)
    db, bb = parts_buffer(parts, C, 7300 + parts + C)
    oa, ob = guarded_flat((C, 2), DEV), guarded_flat((C, 2), DEV)
    K.partials_sum_pair(ba.view, oa.view, bb.view, ob.view)
    parts_check(f"partials_sum_pair[{parts} parts, C={C}] first", da, ba, oa, parts)
    parts_check(f"partials_sum_pair[{parts} parts, C={C}] second", db, bb, ob, parts)


@pytest.mark.parametrize("n", FOLD_C)
@pytest.mark.parametrize("parts", FOLD_PARTS)
def test_fold_rows(parts, n):
    """out[k] += sum_p part[offset + p ldp + k], rows wider than n with NaN in the gaps."""
    g = gen(7400 + parts + n)
    data, out0 = randn(g, parts, n) + 0.3, randn(g, n)
    ldp, off = n + 5, 3
    flat = torch.full((off + parts * ldp + 4,), NAN, dtype=F32)
    flat[off:off + parts * ldp].view(parts, ldp)[:, :n] = data
    flat = flat.to(DEV)
    before = bits(flat)
    out = guarded_flat((n,), DEV, init=out0)
    K.fold_rows(flat, parts, n, ldp, out.view, offset=off)
    out.check("fold_rows")
    r64, r32 = both(lambda dt: kp.ref_rows_sum(data, out0, dt))
    assert_fp64_parity(out.view, r64["out"], r32["out"], what=f"fold_rows[{parts} parts, n={n}]")
    assert torch.equal(bits(flat), before), "fold_rows: the partial rows were modified"


# ---------------------------------------------------------------------------------------------------------
# bn_apply
# ---------------------------------------------------------------------------------------------------------
APPLY_C = [8, 64, 128, 512]  # every C / 8 divides 256
APPLY_M = [1, 33, 257, 4100]  # the tail alone, the two-vector loop with and without a tail, more than one block


@functools.lru_cache(maxsize=2)
def apply_case(M, C):
    g = gen(11011 + 31 * M + C)
    c = dict(x=bf16_values(g, M, C, shift=0.5), res=bf16_values(g, M, C), x2=bf16_values(g, M, C, shift=-0.3),
             mask=torch.relu(bf16_values(g, M, C)))
    if M == 1:  # a single row: dx = -gamma rstd xhat^2 g, which vanishes with xhat -- keep x a deviation off the mean
        for k, m in (("x", 0.5), ("x2", -0.3)):
            r = c[k] - m
            c[k] = to_bf16(m + torch.sign(r) * (1 + r.abs())).to(F32)
    # a gradient with a mean and a slope along both inputs: sum g / M and sum g xhat / M are then O(1), and the
    # elements the mask zeroes get a dx of ordinary size instead of one lost among the bf16 steps near zero
    c["dy"] = to_bf16(randn(g, M, C) + 0.5 + 0.5 * (c["x"] - 0.5) - 0.4 * (c["x2"] + 0.3)).to(F32)
    if M == 1:  # (and g off zero)
        c["dy"] = to_bf16(torch.sign(c["dy"]) * (0.5 + c["dy"].abs())).to(F32)
    c["ms"], c["gamma"], c["beta"] = bn_params(g, C)
    c["ms2"], c["gamma2"], c["beta2"] = bn_params(g, C, mean_shift=-0.3)
    c["start"] = randn(g, 4, C)
    return c


def apply_refs(c, form, relu):
    kw = {} if form == "none" else dict(res=c["res"])
    if form == "bn":
        kw.update(ms2=c["ms2"], gamma2=c["gamma2"], beta2=c["beta2"])
    return both(lambda dt: kp.ref_bn_apply(c["x"], c["ms"], c["gamma"], c["beta"], relu, dt, **kw))


@pytest.mark.parametrize("C", APPLY_C)
@pytest.mark.parametrize("M", APPLY_M)
def test_bn_apply(M, C):
    c = apply_case(M, C)
    x, res = dbf(c["x"]), dbf(c["res"])
    p = {k: d32(c[k]) for k in ("ms", "gamma", "beta", "ms2", "gamma2", "beta2")}
    for form in ("none", "raw", "bn"):
        for relu in (False, True):
            what = f"bn_apply[M={M}, C={C}, residual {form}, relu {relu}]"
            y = GuardedBf16((M, C), DEV)
            kw = {} if form == "none" else dict(res=res)
            if form == "bn":
                kw.update(ms2=p["ms2"], gamma2=p["gamma2"], beta2=p["beta2"])
            K.bn_apply(x, p["ms"], p["gamma"], p["beta"], y.view, relu, **kw)
            y.check(what)
            r64, r32 = apply_refs(c, form, relu)
            assert_bf16_parity(y.view, r64["y"], r32["y"], what=what)


@pytest.mark.parametrize("C", [24, 520])
def test_bn_apply_refuses_unsupported_channel_counts(C):
    g = gen(C)
    x, (ms, gamma, beta) = dbf(bf16_values(g, 33, C)), bn_params(g, C)
    y = GuardedBf16((33, C), DEV)
    with pytest.raises(MerKernelError):
        K.bn_apply(x, d32(ms), d32(gamma), d32(beta), y.view, True)
    torch.cuda.synchronize()
    y.check(f"bn_apply C={C}", written=False)


# ---------------------------------------------------------------------------------------------------------
# bn_bwd_reduce
# ---------------------------------------------------------------------------------------------------------
RED_C = [8, 24, 64, 512]  # 24: 256 / (C / 8) is not an integer, 10 threads idle; 8: 256 rows per iteration
RED_M = [1, 31, 85 * 4 + 1, 1000, 16385]  # 16385: the first M with more than 32 rows per block
TINY_BF16 = torch.tensor([1], dtype=torch.int16).view(BF16)  # the smallest positive bfloat16, 2^-133


@functools.lru_cache(maxsize=2)
def reduce_case(M, C):
    g = gen(13000 + 31 * M + C)
    c = dict(x=bf16_values(g, M, C, shift=0.5), dy=bf16_values(g, M, C), mask=torch.relu(bf16_values(g, M, C)))
    c["ms"], c["gamma"], _ = bn_params(g, C)
    # +0.0, -0.0, a negative and the smallest positive bf16 in the mask, under gradients too large to go unnoticed
    planted = torch.cat([torch.tensor([0.0, -0.0, -1.0], dtype=BF16), TINY_BF16]).to(F32)
    c["mask"].reshape(-1)[:4] = planted
    c["dy"].reshape(-1)[:4] = torch.tensor([3.0, 5.0, 7.0, 9.0])
    assert (c["mask"].reshape(-1)[:4] > 0).tolist() == [False, False, False, True]
    stored = c["mask"].to(BF16).reshape(-1)[:4].view(torch.int16).tolist()
    assert stored[0] == 0 and stored[1] == -32768 and stored[3] == 1  # the signed zero and the subnormal survive
    return c


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("C", RED_C)
@pytest.mark.parametrize("M", RED_M)
def test_bn_bwd_reduce(M, C, masked):
    c = reduce_case(M, C)
    what = f"bn_bwd_reduce[M={M}, C={C}, {'mask' if masked else 'no mask'}]"
    red = guarded_flat((C, 2), DEV)
    K.bn_bwd_reduce(dbf(c["dy"]), dbf(c["mask"]) if masked else None, dbf(c["x"]), d32(c["ms"]), red.view)
    red.check(what)
    r64, r32 = both(lambda dt: kp.ref_bn_bwd(c["dy"], c["mask"] if masked else None, c["x"], c["ms"], c["gamma"], True,
                                             dt))
    assert_fp64_parity(red.view, r64["red"], r32["red"], what=what)


# ---------------------------------------------------------------------------------------------------------
# bn_bwd_apply / bn_bwd_apply2
# ---------------------------------------------------------------------------------------------------------
def bwd_refs(c, masked, batch_stats, second=False, chained=False):
    """The apply judged alone: ``red`` is the float64 sums rounded to float32, given to the kernel and to both
    restatements.  ``chained``: the restatements use their own sums (the kernel is given its own too)."""
    x, ms, gamma = (c["x2"], c["ms2"], c["gamma2"]) if second else (c["x"], c["ms"], c["gamma"])
    s0 = c["start"][2:4] if second else c["start"][0:2]
    mask = c["mask"] if masked else None
    red = None if chained else kp.ref_bn_bwd(c["dy"], mask, x, ms, gamma, batch_stats, F64)["red"].to(F32)
    refs = both(lambda dt: kp.ref_bn_bwd(c["dy"], mask, x, ms, gamma, batch_stats, dt, red=red, dgamma0=s0[0],
                                         dbeta0=s0[1]))
    return red, s0, refs


def check_param_grads(what, dg, db, s0, refs, want):
    for buf, k, i in ((dg, "dgamma", 0), (db, "dbeta", 1)):
        buf.check(f"{what} {k}")
        if k in want:
            assert_fp64_parity(buf.view, refs[0][k], refs[1][k], what=f"{what} {k}")
        else:
            assert torch.equal(buf.view.cpu(), s0[i]), f"{what}: {k} was not passed and must stay as it was"


@pytest.mark.parametrize("batch_stats", [True, False])
@pytest.mark.parametrize("C", APPLY_C)
@pytest.mark.parametrize("M", APPLY_M)
def test_bn_bwd_apply(M, C, batch_stats):
    c = apply_case(M, C)
    x, ms, gamma = dbf(c["x"]), d32(c["ms"]), d32(c["gamma"])
    for masked, want, in_place in ((True, ("dgamma", "dbeta"), False), (False, (), False), (True, ("dgamma",), True),
                                   (False, ("dbeta",), False)):
        what = f"bn_bwd_apply[M={M}, C={C}, batch_stats {batch_stats}, {'mask' if masked else 'no mask'}, " \
               f"{'+'.join(want) or 'no parameter gradients'}{', in place' if in_place else ''}]"
        red, s0, refs = bwd_refs(c, masked, batch_stats)
        dg, db = guarded_flat((C,), DEV, init=s0[0]), guarded_flat((C,), DEV, init=s0[1])
        dx = GuardedBf16((M, C), DEV)
        if in_place:
            dx.view.copy_(dbf(c["dy"]))
        dy = dx.view if in_place else dbf(c["dy"])
        K.bn_bwd_apply(dy, dbf(c["mask"]) if masked else None, x, ms, gamma, d32(red), dx.view,
                       dg.view if "dgamma" in want else None, db.view if "dbeta" in want else None, batch_stats)
        dx.check(what)
        assert_bf16_parity(dx.view, refs[0]["dx"], refs[1]["dx"], what=f"{what} dx")
        check_param_grads(what, dg, db, s0, refs, want)


@pytest.mark.parametrize("M,C", [(257, 64), (4100, 8)])
def test_bn_bwd_reduce_then_apply(M, C):
    """The apply fed the reduce kernel's own sums, against the float64 chain from the inputs."""
    c = apply_case(M, C)
    _, s0, refs = bwd_refs(c, True, True, chained=True)
    dy, mask, x, ms = dbf(c["dy"]), dbf(c["mask"]), dbf(c["x"]), d32(c["ms"])
    red, dx = guarded_flat((C, 2), DEV), GuardedBf16((M, C), DEV)
    dg, db = guarded_flat((C,), DEV, init=s0[0]), guarded_flat((C,), DEV, init=s0[1])
    K.bn_bwd_reduce(dy, mask, x, ms, red.view)
    K.bn_bwd_apply(dy, mask, x, ms, d32(c["gamma"]), red.view, dx.view, dg.view, db.view, True)
    what = f"bn_bwd_reduce -> bn_bwd_apply[M={M}, C={C}]"
    red.check(what)
    dx.check(what)
    assert_fp64_parity(red.view, refs[0]["red"], refs[1]["red"], what=f"{what} red")
    assert_bf16_parity(dx.view, refs[0]["dx"], refs[1]["dx"], what=f"{what} dx")
    check_param_grads(what, dg, db, s0, refs, ("dgamma", "dbeta"))


@pytest.mark.parametrize("batch_stats", [True, False])
@pytest.mark.parametrize("C", APPLY_C)
@pytest.mark.parametrize("M", APPLY_M)
def test_bn_bwd_apply2(M, C, batch_stats):
    """Both outputs against the reference, not against two launches."""
    c = apply_case(M, C)
    ra, sa, refs_a = bwd_refs(c, True, batch_stats)
    rb, sb, refs_b = bwd_refs(c, True, batch_stats, second=True)
    dy, mask = dbf(c["dy"]), dbf(c["mask"])
    for want_a, want_b in ((("dgamma", "dbeta"), ("dgamma", "dbeta")), (("dbeta",), ("dgamma",)), ((), ())):
        what = f"bn_bwd_apply2[M={M}, C={C}, batch_stats {batch_stats}, {want_a} / {want_b}]"
        dx, dx2 = GuardedBf16((M, C), DEV), GuardedBf16((M, C), DEV)
        g = [guarded_flat((C,), DEV, init=s) for s in (sa[0], sa[1], sb[0], sb[1])]
        K.bn_bwd_apply2(dy, mask, dbf(c["x"]), d32(c["ms"]), d32(c["gamma"]), d32(ra), dx.view,
                        g[0].view if "dgamma" in want_a else None, g[1].view if "dbeta" in want_a else None,
                        dbf(c["x2"]), d32(c["ms2"]), d32(c["gamma2"]), d32(rb), dx2.view,
                        g[2].view if "dgamma" in want_b else None, g[3].view if "dbeta" in want_b else None,
                        batch_stats)
        dx.check(what)
        dx2.check(what)
        assert_bf16_parity(dx.view, refs_a[0]["dx"], refs_a[1]["dx"], what=f"{what} dx")
        assert_bf16_parity(dx2.view, refs_b[0]["dx"], refs_b[1]["dx"], what=f"{what} dx2")
        check_param_grads(f"{what} first", g[0], g[1], sa, refs_a, want_a)
        check_param_grads(f"{what} second", g[2], g[3], sb, refs_b, want_b)


def test_bn_bwd_apply2_refuses_in_place():
    M, C = 33, 64
    c = apply_case(M, C)
    red = torch.zeros(C, 2, device=DEV)
    for alias in (0, 1):
        outs = [GuardedBf16((M, C), DEV), GuardedBf16((M, C), DEV)]
        dy = outs[alias].view
        with pytest.raises(MerKernelError):
            K.bn_bwd_apply2(dy, dbf(c["mask"]), dbf(c["x"]), d32(c["ms"]), d32(c["gamma"]), red, outs[0].view, None,
                            None, dbf(c["x2"]), d32(c["ms2"]), d32(c["gamma2"]), red, outs[1].view, None, None, True)
        torch.cuda.synchronize()
        for o in outs:
            o.check("bn_bwd_apply2 in place", written=False)


# ---------------------------------------------------------------------------------------------------------
# maxpool_fwd / maxpool_bwd
# ---------------------------------------------------------------------------------------------------------
POOL_HW = [(1, 1), (1, 2), (2, 1), (5, 4), (8, 8), (9, 7)]
POOL_C = [8, 72]


@functools.lru_cache(maxsize=None)
def pool_case(H, W, C):
    """N = 2, five bf16 values only, so nearly every window has ties; image 0 is negative throughout, image 1 has one
    pixel of -inf."""
    g = gen(17000 + 100 * H + 10 * W + C)
    idx = torch.randint(0, 5, (2, H, W, C), generator=g)
    x = torch.tensor([-1.5, -0.25, 0.0, 0.75, 2.0])[idx]
    x[0] = torch.tensor([-3.0, -2.0, -1.5, -1.0, -0.5])[idx[0]]
    x[1, H // 2, W // 2, :] = -float("inf")
    dy = bf16_values(g, 2, kp.maxpool_out(H), kp.maxpool_out(W), C)
    return x, dy, both(lambda dt: kp.ref_maxpool(x, dy, dt))


@pytest.mark.parametrize("C", POOL_C)
@pytest.mark.parametrize("H,W", POOL_HW)
def test_maxpool(H, W, C):
    x, dy, (r64, r32) = pool_case(H, W, C)
    what = f"maxpool[2x{H}x{W}x{C}]"
    Ho, Wo = kp.maxpool_out(H), kp.maxpool_out(W)
    y, arg = GuardedBf16((2, Ho, Wo, C), DEV), GuardedBf16((2, Ho, Wo, C), DEV, dtype=torch.uint8)
    K.maxpool_fwd(dbf(x), y.view, arg.view)
    y.check(f"{what} y")
    arg.check(f"{what} arg")
    assert torch.equal(y.view.cpu(), to_bf16(r64["y"])), f"{what}: y differs from the reference"
    assert torch.equal(arg.view.cpu(), r64["arg"].to(torch.uint8)), f"{what}: the argmax is not the first maximum"
    dx = GuardedBf16((2, H, W, C), DEV)
    K.maxpool_bwd(dbf(dy), arg.view, dx.view)
    dx.check(f"{what} dx")  # every element written, the pixels no window selects too
    assert_bf16_parity(dx.view, r64["dx"], r32["dx"], what=f"{what} dx")
    assert bool((dx.view.cpu()[r64["dx"] == 0] == 0).all()), f"{what}: a pixel no window selects must be an exact zero"


def test_maxpool_refuses_c_12():
    x = torch.zeros(2, 5, 4, 12, dtype=BF16, device=DEV)
    y, arg = GuardedBf16((2, 3, 2, 12), DEV), GuardedBf16((2, 3, 2, 12), DEV, dtype=torch.uint8)
    dx = GuardedBf16((2, 5, 4, 12), DEV)
    with pytest.raises(MerKernelError):
        K.maxpool_fwd(x, y.view, arg.view)
    with pytest.raises(MerKernelError):
        K.maxpool_bwd(torch.zeros(2, 3, 2, 12, dtype=BF16, device=DEV),
                      torch.zeros(2, 3, 2, 12, dtype=torch.uint8, device=DEV), dx.view)
    torch.cuda.synchronize()
    for o in (y, arg, dx):
        o.check("maxpool C=12", written=False)


# ---------------------------------------------------------------------------------------------------------
# the fused stem tail: stem_bnrelu_maxpool / stem_pool_bn_bwd
# ---------------------------------------------------------------------------------------------------------
def stem_chain_refs(dp, arg, mask, x, ms, gamma, batch_stats, s0, H, W):
    """The backward chain restated: the pool gather through the kernels' argmax, rounded to bf16 as maxpool_bwd
    stores it, then the BatchNorm backward under the kernels' ReLU mask -- a tie or a sign decision is an input."""
    def chain(dt):
        da = to_bf16(kp.maxpool_gather(dp, arg, H, W, dt)).to(dt)
        return kp.ref_bn_bwd(da, mask, x, ms, gamma, batch_stats, dt, dgamma0=s0[0], dbeta0=s0[1])
    return both(chain)


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("C", [8, 64])
@pytest.mark.parametrize("H,W", [(1, 1), (5, 4), (9, 7)])
def test_fused_stem_tail(H, W, C, training):
    N = 4
    g = gen(19007 + 100 * H + C)
    what = f"stem tail[{N}x{H}x{W}x{C}, batch_stats {training}]"
    x = bf16_values(g, N, H, W, C)
    ms, gamma, beta = bn_params(g, C, mean_shift=0.1)
    Ho, Wo = kp.maxpool_out(H), kp.maxpool_out(W)
    dp, s0 = bf16_values(g, N, Ho, Wo, C, shift=0.7), randn(g, 2, C)  # (a mean: see apply_case)
    xd, msd, gd, bd = dbf(x), d32(ms), d32(gamma), d32(beta)
    a = torch.empty_like(xd)
    K.bn_apply(xd, msd, gd, bd, a, relu=True)
    p_ref, arg_ref = GuardedBf16((N, Ho, Wo, C), DEV), GuardedBf16((N, Ho, Wo, C), DEV, dtype=torch.uint8)
    K.maxpool_fwd(a, p_ref.view, arg_ref.view)
    p, arg = GuardedBf16((N, Ho, Wo, C), DEV), GuardedBf16((N, Ho, Wo, C), DEV, dtype=torch.uint8)
    K.stem_bnrelu_maxpool(xd, msd, gd, bd, p.view, arg.view)
    for o in (p_ref, arg_ref, p, arg):
        o.check(what)
    assert torch.equal(p.view, p_ref.view) and torch.equal(arg.view, arg_ref.view), f"{what}: fused != unfused"
    # the unfused forward is itself the reference's: y of bn_apply, then the first-maximum pool of that
    a_cpu = a.float().cpu()
    pool = kp.ref_maxpool(a_cpu, None, F64)
    assert torch.equal(p.view.cpu(), to_bf16(pool["y"])) and torch.equal(arg.view.cpu(), pool["arg"].to(torch.uint8))
    red, dx = guarded_flat((C, 2), DEV), GuardedBf16((N, H, W, C), DEV)
    dg, db = guarded_flat((C,), DEV, init=s0[0]), guarded_flat((C,), DEV, init=s0[1])
    K.stem_pool_bn_bwd(dbf(dp), arg.view, xd, msd, gd, bd, red.view, dx.view, dg.view, db.view, training)
    red.check(what)
    dx.check(what)
    refs = stem_chain_refs(dp, arg.view.cpu(), a_cpu, x, ms, gamma, training, s0, H, W)
    assert_bf16_parity(dx.view, refs[0]["dx"], refs[1]["dx"], what=f"{what} dx")
    assert_fp64_parity(red.view, refs[0]["red"], refs[1]["red"], what=f"{what} red")
    check_param_grads(what, dg, db, s0, refs, ("dgamma", "dbeta"))


# ---------------------------------------------------------------------------------------------------------
# avgpool_fwd / avgpool_bwd
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [8, 200, 520])  # the C tail of the 256-thread block
@pytest.mark.parametrize("H,W", [(1, 1), (7, 7), (5, 10)])
def test_avgpool(H, W, C):
    g = gen(23000 + H * W + C)
    N = 3
    x, dy = bf16_values(g, N, H, W, C, shift=0.3), randn(g, N, C)
    what = f"avgpool[{N}x{H}x{W}x{C}]"
    y, dx = guarded_flat((N, C), DEV), GuardedBf16((N, H, W, C), DEV)
    K.avgpool_fwd(dbf(x), y.view)
    K.avgpool_bwd(d32(dy), dx.view)
    y.check(what)
    dx.check(what)
    r64, r32 = both(lambda dt: kp.ref_avgpool(x, dy, dt))
    assert_fp64_parity(y.view, r64["y"], r32["y"], what=f"{what} y")
    assert_bf16_parity(dx.view, r64["dx"], r32["dx"], what=f"{what} dx")


# ---------------------------------------------------------------------------------------------------------
# Index range: the pooling kernels index 16-byte chunks, pixels x C / 8 of them.  The launchers admit pixels < 2^22;
# the chunk index then passes 2^23, where csrc/common.h fdiv (a float-reciprocal divide, exact below 2^22) returns
# q + 1 for the last chunk of every pixel (tests/test_kernel_parity_cpu.py).  These are the only large allocations.
# ---------------------------------------------------------------------------------------------------------
BWD_SHAPE = (3, 600, 592, 64)  # 1,065,600 pixels, 8,524,800 chunks
FWD_SHAPE = (2, 1030, 1030, 128)  # 2,121,800 pixels; 530,450 output pixels, 8,487,200 output chunks


def first_row_past_2_23(shape, image):
    """The first row of ``image`` ([N, rows, cols, C]) that holds a chunk index >= 2^23."""
    N, R, Wd, C = shape
    pixel = (1 << 23) // (C // 8)
    assert image * R * Wd < pixel < (image + 1) * R * Wd, "2^23 must fall inside the image the reference covers"
    return (pixel - image * R * Wd) // Wd


def by_rows(shape, image):
    r = first_row_past_2_23(shape, image)
    return ((f"rows 0..{r - 1} of image {image} (chunk indices below 2^23)", slice(0, r)),
            (f"rows {r}..{shape[1] - 1} of image {image} (chunk indices from 2^23 on)", slice(r, shape[1])))


@pytest.fixture(scope="module")
def big_bwd():
    """dp [3, 300, 296, 64], non-zero only in image 2, a random argmax, and the gather restated for image 2 (pooling
    is per image)."""
    N, H, W, C = BWD_SHAPE
    Ho, Wo = kp.maxpool_out(H), kp.maxpool_out(W)
    g = torch.Generator(device=DEV).manual_seed(29)
    dp = torch.zeros(N, Ho, Wo, C, dtype=BF16, device=DEV)
    dp[2] = torch.randn(Ho, Wo, C, generator=g, device=DEV).to(BF16)
    arg = torch.randint(0, 9, (N, Ho, Wo, C), generator=g, device=DEV, dtype=torch.uint8)
    dp2, arg2 = dp[2:3].float().cpu(), arg[2:3].cpu()
    da64, da32 = both(lambda dt: kp.maxpool_gather(dp2, arg2, H, W, dt)[0])
    yield dict(dp=dp, arg=arg, da64=da64, da32=da32)


def test_maxpool_bwd_beyond_2_23_chunks(big_bwd):
    N, H, W, C = BWD_SHAPE
    assert N * H * W < 1 << 22 < 1 << 23 < N * H * W * (C // 8)
    dx = GuardedBf16(BWD_SHAPE, DEV)
    K.maxpool_bwd(big_bwd["dp"], big_bwd["arg"], dx.view)  # under the pixel guard: must compute, not refuse
    dx.check("maxpool_bwd beyond 2^23 chunks")
    assert bool((dx.view[:2] == 0).all()), "images 0 and 1 receive no gradient and must be exact zeros"
    got = dx.view[2].cpu()
    for name, rows in by_rows(BWD_SHAPE, 2):
        assert_bf16_parity(got[rows], big_bwd["da64"][rows], big_bwd["da32"][rows], what=f"maxpool_bwd {name}")


def test_stem_pool_bn_bwd_beyond_2_23_chunks(big_bwd):
    """batch_stats=False: dx of image 2 depends on image 2 alone, and red / dgamma / dbeta are sums over image 2,
    dp being zero elsewhere."""
    N, H, W, C = BWD_SHAPE
    g = torch.Generator(device=DEV).manual_seed(31)
    x = torch.randn(BWD_SHAPE, generator=g, device=DEV).to(BF16)
    cg = gen(31)
    ms, gamma, beta = bn_params(cg, C, mean_shift=0.1)
    s0 = randn(cg, 2, C)
    msd, gd, bd = d32(ms), d32(gamma), d32(beta)
    a2 = torch.empty_like(x[2])
    K.bn_apply(x[2], msd, gd, bd, a2, relu=True)  # the ReLU mask of image 2 as the kernels round it
    red, dx = guarded_flat((C, 2), DEV), GuardedBf16(BWD_SHAPE, DEV)
    dg, db = guarded_flat((C,), DEV, init=s0[0]), guarded_flat((C,), DEV, init=s0[1])
    K.stem_pool_bn_bwd(big_bwd["dp"], big_bwd["arg"], x, msd, gd, bd, red.view, dx.view, dg.view, db.view, False)
    what = "stem_pool_bn_bwd beyond 2^23 chunks"
    red.check(what)
    dx.check(what)
    assert bool((dx.view[:2] == 0).all()), "images 0 and 1 receive no gradient and must be exact zeros"
    x2, mask2 = x[2].float().cpu(), a2.float().cpu()
    refs = both(lambda dt: kp.ref_bn_bwd(to_bf16(big_bwd["da64"]).to(dt), mask2, x2, ms, gamma, False, dt,
                                         dgamma0=s0[0], dbeta0=s0[1]))
    got = dx.view[2].cpu()
    for name, rows in by_rows(BWD_SHAPE, 2):
        assert_bf16_parity(got[rows], refs[0]["dx"].view(H, W, C)[rows], refs[1]["dx"].view(H, W, C)[rows],
                           what=f"stem_pool_bn_bwd {name} dx")
    assert_fp64_parity(red.view, refs[0]["red"], refs[1]["red"], what=f"{what} red")
    check_param_grads(what, dg, db, s0, refs, ("dgamma", "dbeta"))


@pytest.fixture(scope="module")
def big_fwd():
    """x [2, 1030, 1030, 128] of the values 0..4 (ties everywhere) and the first-maximum pool of image 1, restated
    in slabs of output rows.  y and arg are copies, so float32 restates them exactly."""
    N, H, W, C = FWD_SHAPE
    Ho, Wo = kp.maxpool_out(H), kp.maxpool_out(W)
    g = torch.Generator(device=DEV).manual_seed(37)
    x = torch.randint(0, 5, FWD_SHAPE, generator=g, device=DEV, dtype=torch.int8).to(BF16)
    x1 = x[1].cpu()
    y = torch.empty(Ho, Wo, C, dtype=BF16)
    arg = torch.empty(Ho, Wo, C, dtype=torch.uint8)
    for o0 in range(0, Ho, 64):
        o1 = min(Ho, o0 + 64)
        i0, i1 = 2 * o0 - 1, 2 * o1  # input rows i0 .. i1 inclusive, -inf outside the frame
        xp = torch.full((1, i1 - i0 + 1, W + 2, C), -float("inf"), dtype=F32)
        lo, hi = max(i0, 0), min(i1, H - 1)
        xp[0, lo - i0:hi - i0 + 1, 1:W + 1] = x1[lo:hi + 1].to(F32)
        ys, as_ = kp.maxpool_taps(xp, o1 - o0, Wo)
        y[o0:o1], arg[o0:o1] = ys[0].to(BF16), as_[0]
    small = kp.ref_maxpool(x1[:9, :7].to(F32)[None], None, F64)  # the slabs agree with the plain restatement
    assert torch.equal(small["y"][0, :4, :3].to(BF16), y[:4, :3]) and torch.equal(
        small["arg"][0, :4, :3].to(torch.uint8), arg[:4, :3])
    yield dict(x=x, y=y.to(DEV), arg=arg.to(DEV))


def check_big_fwd(what, call, want_y, want_arg):
    """The call either returns the reference's y and arg of image 1 exactly or refuses; silently wrong output is the
    only failure."""
    N, H, W, C = FWD_SHAPE
    Ho, Wo = kp.maxpool_out(H), kp.maxpool_out(W)
    assert N * H * W < 1 << 22 and N * Ho * Wo * (C // 8) > 1 << 23
    y, arg = GuardedBf16((N, Ho, Wo, C), DEV), GuardedBf16((N, Ho, Wo, C), DEV, dtype=torch.uint8)
    try:
        call(y.view, arg.view)
    except MerKernelError:
        torch.cuda.synchronize()
        y.check(what, written=False)
        arg.check(what, written=False)
        return
    y.check(what)
    arg.check(what)
    for name, rows in by_rows((N, Ho, Wo, C), 1):
        assert torch.equal(y.view[1, rows], want_y[rows]), f"{what}: y differs from the reference in {name}"
        assert torch.equal(arg.view[1, rows], want_arg[rows]), f"{what}: arg differs from the reference in {name}"


def test_maxpool_fwd_beyond_2_23_chunks(big_fwd):
    check_big_fwd("maxpool_fwd beyond 2^23 chunks", lambda y, arg: K.maxpool_fwd(big_fwd["x"], y, arg), big_fwd["y"],
                  big_fwd["arg"])


def test_stem_bnrelu_maxpool_beyond_2_23_chunks(big_fwd):
    """BatchNorm with mean 0, rstd 1, beta 0 and a power of two for gamma: on the non-negative x the activation is
    x gamma exactly, so the pool's argmax is that of x and its y is the reference's times gamma (the BatchNorm
    arithmetic itself is test_fused_stem_tail's)."""
    C = FWD_SHAPE[3]
    gamma = torch.tensor([1.0, 2.0, 0.5, 4.0]).repeat(C // 4)
    ms = torch.stack([torch.zeros(C), torch.ones(C)], 1).contiguous()
    want_y = (big_fwd["y"].float() * gamma.to(DEV)).to(BF16)
    assert torch.equal(want_y.float(), big_fwd["y"].float() * gamma.to(DEV))
    check_big_fwd("stem_bnrelu_maxpool beyond 2^23 chunks",
                  lambda y, arg: K.stem_bnrelu_maxpool(big_fwd["x"], d32(ms), d32(gamma), d32(torch.zeros(C)), y, arg),
                  want_y, big_fwd["arg"])

"""CPU only: pins the float64 references of tests/rowwise_refs.py and shows that the tolerances of the GPU parity tests admit a correct
kernel.

1. every reference agrees with the torch functional of the same operation in float64 to 1e-12;
2. an fp32 restatement of each kernel's arithmetic, in the kernel's own order of additions (each of 64 lanes adds its 16-byte chunks in
   sequence, then the xor butterfly of wave_sum; for the column reductions 32 row-strided partial sums, then a sequential sum of the 32),
   stays within ONE QUARTER of the fp32 allowance that the GPU test grants beyond one bf16 rounding (parity tolerances)."""
import math

import torch
import torch.nn.functional as F

from tests import rowwise_refs as R


def _rnd(shape, seed, std=2.0, mean=0.5, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * std + mean).to(dtype)


# ------------------------------------------------------------------------------------------------ 1. references vs torch, float64
def test_layernorm_refs_match_torch_float64():
    x, w, b, dy = _rnd((37, 520), 1), _rnd((520,), 2, dtype=torch.float32), _rnd((520,), 3, dtype=torch.float32), _rnd((37, 520), 4)
    y, mean, rstd = R.layernorm_ref(x, w, b, 1e-5)
    xd = x.double().requires_grad_(True)
    wd, bd = w.double().requires_grad_(True), b.double().requires_grad_(True)
    ref = F.layer_norm(xd, (520,), wd, bd, 1e-5)
    assert (y - ref).abs().max() < 1e-12
    assert (mean - x.double().mean(-1)).abs().max() < 1e-12
    assert (rstd - 1.0 / torch.sqrt(x.double().var(-1, unbiased=False) + 1e-5)).abs().max() < 1e-12
    yg = R.layernorm_ref(x, w, b, 1e-5, gelu=True)[0]
    assert (yg - F.gelu(ref)).abs().max() < 1e-12
    ref.backward(dy.double())
    dx, dg, db = R.layernorm_bwd_ref(x, w, dy)
    # the closed form the kernel implements, against autograd
    xh = (x.double() - mean[:, None]) * rstd[:, None]
    g = dy.double() * w.double()
    closed = rstd[:, None] * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    assert (dx - xd.grad).abs().max() < 1e-12 and (dx - closed).abs().max() < 1e-12
    assert (dg - wd.grad).abs().max() < 1e-12 and (dg - (dy.double() * xh).sum(0)).abs().max() < 1e-10
    assert (db - bd.grad).abs().max() < 1e-12


def test_rmsnorm_refs_match_torch_float64():
    x, w, dy, dres = _rnd((9, 896), 5), 1 + 0.1 * _rnd((896,), 6, dtype=torch.float32), _rnd((9, 896), 7), _rnd((9, 896), 8)
    y, rstd = R.rmsnorm_ref(x, w, 1e-6)
    xd = x.double().requires_grad_(True)
    r = torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + 1e-6)
    assert (rstd - r[:, 0]).abs().max() < 1e-12
    assert (y - w.double() * (xd * r).float().bfloat16().double()).abs().max() < 1e-12      # HF: weight * hidden.to(input_dtype)
    # without the inner rounding the reference is within one bf16 rounding of it
    assert ((y - w.double() * (xd * r)).abs() <= R.U_BF16 * (w.double() * xd * r).abs() + 1e-12).all()
    (w.double() * (xd * r)).backward(dy.double())
    for dres_, scale in ((dres, 0.5), (dres, None), (None, 0.5), (None, None)):
        want = xd.grad * (scale if scale is not None else 1.0) + (dres_.double() if dres_ is not None else 0.0)
        assert (R.rmsnorm_bwd_ref(x, w, dy, dres_, scale, eps=1e-6) - want).abs().max() < 1e-12


def test_gelu_colsum_refs_match_torch_float64():
    x, dy = _rnd((40, 64), 9, std=3.0, mean=0.0), _rnd((40, 64), 10)
    xd = x.double().requires_grad_(True)
    ref = F.gelu(xd)
    assert (R.gelu_ref(x) - ref).abs().max() < 1e-12
    ref.backward(dy.double())
    assert (R.gelu_bwd_ref(x, dy) - xd.grad).abs().max() < 1e-12
    assert (R.colsum_ref(x) - x.double().sum(0)).abs().max() < 1e-12
    # the left tail, where 1 + erf cancels: x Phi(x) against the asymptotic series -phi(x) (1 - 1/x^2 + 3/x^4 - 15/x^6)
    t = torch.tensor([-12.0, -20.0], dtype=torch.float64)
    series = -torch.exp(-0.5 * t * t) / math.sqrt(2 * math.pi) * (1 - 1 / t ** 2 + 3 / t ** 4 - 15 / t ** 6)
    assert ((R.gelu_ref(t) - series).abs() <= 1e-3 * series.abs()).all()


def test_ce_ref_matches_torch_float64():
    V = 264
    lg = _rnd((6, V), 11, std=3.0, mean=0.0)
    lg[1, 8:16] = float("-inf")
    lg[2, 5] = lg[2, 100] = lg[2, V - 1] = 30.0          # a three-way tie of the maximum
    t = torch.tensor([3, 20, 100, 7, -1, 263])
    loss, dl, am, mean = R.ce_ref(lg, t)
    ld = lg.double().requires_grad_(True)
    ref = F.cross_entropy(ld, t.masked_fill(t < 0, -100), ignore_index=-100)
    ref.backward()
    per_row = F.cross_entropy(lg.double(), t.masked_fill(t < 0, -100), ignore_index=-100, reduction="none")
    assert torch.isfinite(loss).all() and (loss - per_row).abs().max() < 1e-12 and abs(float(mean) - float(ref.detach())) < 1e-12
    assert (dl - ld.grad).abs().max() < 1e-12 and (dl[4] == 0).all() and (dl[1, 8:16] == 0).all()
    assert int(am[2]) == 5 and torch.equal(am, lg.double().argmax(-1))
    assert math.isnan(float(R.ce_ref(lg, torch.full((6,), -1))[3]))


def test_bf16_sweep_contents():
    s = R.bf16_sweep()
    assert s.numel() == 20484 and s.dtype == torch.bfloat16
    bits = s.view(torch.int16).int() & 0xFFFF
    assert bits.unique().numel() == 20484
    assert (bits == 0).sum() == 1 and (bits == 0x8000).sum() == 1          # +0 and -0
    a = s.double().abs()
    nz = a[a > 0]
    assert float(nz.min()) == 2.0 ** -40 and float(nz.max()) == 2.0 ** 40 and torch.isfinite(s.float()).all()
    m = R.sweep_matrix("cpu")
    assert m.shape == (21, 1024) and torch.equal(m.flatten()[:20484].view(torch.int16), s.view(torch.int16)) and (m.flatten()[20484:] == 0).all()


def test_helpers_catch_what_they_are_for():
    import pytest
    ref = torch.tensor([1.0, -2.0, 0.0], dtype=torch.float64)
    R.assert_one_rounding(torch.tensor([1.0 + 2.0 ** -8, -2.0, 0.0]), ref, 0.0, "at the bound")
    for bad in ([1.0 + 2.0 ** -7, -2.0, 0.0], [1.0, float("nan"), 0.0], [1.0, -2.0, 1e-30], [1.0, float("inf"), 0.0]):
        with pytest.raises(AssertionError):
            R.assert_one_rounding(torch.tensor(bad), ref, 0.0, "beyond")
    v = R.padded((3, 16), 8, "cpu")
    assert v.shape == (3, 16) and v.stride() == (24, 1) and torch.isnan(v.float()).all()
    v.zero_()
    R.assert_padding_untouched(v)
    v._base[1, 16] = 0
    with pytest.raises(AssertionError):
        R.assert_padding_untouched(v)
    f = R.padded((10,), 8, "cpu", dtype=torch.float32)
    f.zero_()
    R.assert_padding_untouched(f)
    f._base[10] = 1.0
    with pytest.raises(AssertionError):
        R.assert_padding_untouched(f)


# ------------------------------------------------------------------------------------------------ 2. fp32 restatements in kernel order
def _wave_sum_rows(v):
    """v [M, d] fp32 -> [M]: lane l adds the elements of its chunks l, l + 64, ... in order, then the xor butterfly (lane 0's value)"""
    M, d = v.shape
    nch = d // 8
    I = (nch + 63) // 64
    p = torch.zeros((M, I * 64, 8), dtype=torch.float32)
    p[:, :nch] = v.view(M, nch, 8)            # (adding the +0 of a missing chunk changes no fp32 sum)
    p = p.view(M, I, 64, 8)
    acc = torch.zeros((M, 64), dtype=torch.float32)
    for i in range(I):
        for e in range(8):
            acc = acc + p[:, i, :, e]
    lanes = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lanes ^ o]
    return acc[:, 0]


def _col_sum_rows(v):
    """v [M, N] fp32 -> [N]: partial sum ty = rows ty, ty + 32, ... in order; then the 32 partials in order"""
    M, N = v.shape
    G_ = (M + 31) // 32
    p = torch.zeros((G_ * 32, N), dtype=torch.float32)
    p[:M] = v
    p = p.view(G_, 32, N)
    acc = torch.zeros((32, N), dtype=torch.float32)
    for g in range(G_):
        acc = acc + p[g]
    s = torch.zeros((N,), dtype=torch.float32)
    for r in range(32):
        s = s + acc[r]
    return s


def _ln_fwd_f32(x, w, b, eps, gelu):
    xf, d = x.float(), x.shape[1]
    mean = _wave_sum_rows(xf) / d
    c = xf - mean[:, None]
    rstd = torch.rsqrt(_wave_sum_rows(c * c) / d + eps)
    t = c * rstd[:, None] * w + b
    if gelu:
        t = 0.5 * t * (1.0 + torch.erf(t * 0.70710678118654752440))
    return t.bfloat16(), mean, rstd


def _quarter(got, ref, allowance, what):
    return R.assert_one_rounding(got, ref, 0.25 * allowance, what)


def test_fp32_layernorm_forward_is_within_a_quarter_of_the_allowances():
    for (M, d), gelu in (((37, 520), False), ((37, 520), True), ((7, 4104), False), ((3, 8200), True)):
        x, w, b = _rnd((M, d), 21), _rnd((d,), 22, std=1.0, mean=0.0, dtype=torch.float32), _rnd((d,), 23, std=1.0, mean=0.0, dtype=torch.float32)
        y, mean, rstd = _ln_fwd_f32(x, w, b, 1e-5, gelu)
        ry, rmean, rrstd = R.layernorm_ref(x, w, b, 1e-5, gelu)
        xh = (x.double() - rmean[:, None]) * rrstd[:, None]
        allow = 2.0 ** -20 * ((w.double() * xh).abs() + b.double().abs())
        if gelu:
            allow = 1.13 * allow + 2.0 ** -22 * (xh * w.double() + b.double()).abs()
        _quarter(y, ry, allow, "host ln y")
        R.assert_within(mean, rmean, 0.25 * 2.0 ** -18 * x.double().abs().mean(-1), "host ln mean")
        R.assert_within(rstd, rrstd, 0.25 * 2.0 ** -18 * rrstd, "host ln rstd")
        assert ((rstd.double() - rrstd).abs() / rrstd).max() < 2.0 ** -22      # about two fp32 ulps


def test_fp32_layernorm_backward_is_within_a_quarter_of_the_allowances():
    for M, d in ((31, 72), (130, 1288), (70, 5128), (1030, 64)):
        x, w, dy = _rnd((M, d), 31), _rnd((d,), 32, std=1.0, mean=0.0, dtype=torch.float32), _rnd((M, d), 33)
        _, mean, rstd = _ln_fwd_f32(x, w, torch.zeros(d), 1e-5, False)
        xf, gf = x.float(), dy.float() * w
        xh = (xf - mean[:, None]) * rstd[:, None]
        s1, s2 = _wave_sum_rows(gf) / d, _wave_sum_rows(gf * xh) / d
        dx = (rstd[:, None] * (gf - s1[:, None] - xh * s2[:, None])).bfloat16()
        dg, db = _col_sum_rows(dy.float() * xh), _col_sum_rows(dy.float())
        rdx, rdg, rdb = R.layernorm_bwd_ref(x, w, dy)
        _, rmean, rrstd = R.layernorm_ref(x, w, torch.zeros(d), 1e-5)
        scale = rrstd * (dy.double() * w.double()).abs().max(-1).values
        _quarter(dx, rdx, (2.0 ** -20 * scale)[:, None], "host ln dx")
        assert float((R.excess_over_one_rounding(dx, rdx) / scale[:, None]).max()) <= 3e-9
        rxh = (x.double() - rmean[:, None]) * rrstd[:, None]
        tg, tb = (dy.double() * rxh).abs().sum(0), dy.double().abs().sum(0)
        R.assert_within(dg, rdg, 0.25 * 2.0 ** -18 * tg, "host ln dgamma")
        R.assert_within(db, rdb, 0.25 * 2.0 ** -18 * tb, "host ln dbeta")
        assert float(((dg.double() - rdg).abs() / tg).max()) < 2.0 ** -22 and float(((db.double() - rdb).abs() / tb).max()) < 2.0 ** -22


def test_fp32_rmsnorm_is_within_a_quarter_of_the_allowances():
    for M, d in ((5, 896), (130, 3584), (130, 4104)):
        x, w, dy, dres = _rnd((M, d), 41), 1 + 0.1 * _rnd((d,), 42, std=1.0, mean=0.0, dtype=torch.float32), _rnd((M, d), 43), _rnd((M, d), 44)
        xf = x.float()
        rstd = torch.rsqrt(_wave_sum_rows(xf * xf) / d + 1e-6)
        y = (w * (xf * rstd[:, None]).bfloat16().float()).bfloat16()
        ry, rrstd = R.rmsnorm_ref(x, w, 1e-6)
        R.assert_within(rstd, rrstd, 0.25 * 2.0 ** -18 * rrstd, "host rms rstd")
        allow = 2.0 ** -20 * ry.abs()
        # two roundings: nothing beyond (2^-8 + 2^-7)|ref|, and where the inner roundings agree (all but a few 1e-5 of the elements) one rounding
        R.assert_within(y, ry, (R.U_BF16 + 2.0 ** -7) * ry.abs() + 0.25 * allow, "host rms y (two roundings)")
        beyond = (R.excess_over_one_rounding(y, ry) > allow).double().mean()
        assert float(beyond) <= 4.2e-5, float(beyond)
        xh = xf * rstd[:, None]
        for dres_, scale in ((dres, 0.5), (None, None)):
            dot = _wave_sum_rows(dy.float() * w * xf * rstd[:, None]) / d
            t = rstd[:, None] * (dy.float() * w - xh * dot[:, None]) * (scale if scale is not None else 1.0)
            if dres_ is not None:
                t = t + dres_.float()
            rdx = R.rmsnorm_bwd_ref(x, w, dy, dres_, scale, eps=1e-6)
            sc = (rrstd * (dy.double() * w.double()).abs().max(-1).values)[:, None] * (scale if scale is not None else 1.0)
            _quarter(t.bfloat16(), rdx, 2.0 ** -20 * sc, "host rms dx")


def test_fp32_gelu_over_the_sweep_is_within_a_quarter_of_the_allowances():
    x = R.bf16_sweep()
    xf = x.float()
    y = (0.5 * xf * (1.0 + torch.erf(xf * 0.70710678118654752440))).bfloat16()
    ref = R.gelu_ref(x)
    _quarter(y, ref, 2.0 ** -22 * x.double().abs(), "host gelu fwd")
    # the issue's own figure for the cancelling tail: the worst element uses 0.975 of 2^-8 |ref| + 2^-23 |x|
    assert R.assert_within(y, ref, R.U_BF16 * ref.abs() + 2.0 ** -23 * x.double().abs(), "host gelu fwd (2^-23)") <= 1.0
    for dy in (torch.ones_like(x), _rnd((x.numel(),), 51, std=1.0, mean=0.0)):
        cdf = 0.5 * (1.0 + torch.erf(xf * 0.70710678118654752440))
        pdf = 0.3989422804014327 * torch.exp(-0.5 * xf * xf)
        dz = (dy.float() * (cdf + xf * pdf)).bfloat16()
        rdz = R.gelu_bwd_ref(x, dy)
        _quarter(dz, rdz, 2.0 ** -20 * dy.double().abs(), "host gelu bwd")
        assert float(R.excess_over_one_rounding(dz, rdz).max()) <= 2.3e-8 * float(dy.double().abs().max())


def test_fp32_colsum_is_within_a_quarter_of_the_allowance():
    for M, N in ((31, 72), (1000, 520), (4101, 1288)):
        x = _rnd((M, N), 61)
        R.assert_within(_col_sum_rows(x.float()), R.colsum_ref(x), 0.25 * 2.0 ** -18 * x.double().abs().sum(0), "host colsum")

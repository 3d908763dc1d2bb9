"""float64 references and shared helpers for the per-kernel parity tests of the row kernels (csrc/norm.hip, the elementwise kernels of
csrc/elementwise.hip, the CE kernel of csrc/loss_optim.hip).  Plain module, no GPU: tests/test_rowwise_refs_host.py pins every function
here against the torch functional of the same operation, so a wrong reference cannot quietly loosen a GPU test.

The rule the GPU tests apply (parity tolerances): these kernels compute in fp32 from bf16-valued inputs and round ONCE to
bf16, so |got - ref| <= 2^-8 |ref| (round-to-nearest-even of an 8-bit significand) plus a stated fp32 allowance per kernel."""
import math

import numpy as np
import torch
import torch.nn.functional as F

U_BF16 = 2.0 ** -8            # one bf16 rounding, relative
SENTINEL_BF16 = 0x7FA5        # a NaN pattern: padding that a kernel READS poisons its result, padding it WRITES changes these bits
SENTINEL_F32 = 0x7FC5A5A5
SHARES = {}                   # what -> worst measured share of its bound (assert_one_rounding / assert_within), for profiles/rowwise_parity.md


def f64(t):
    return t.detach().to("cpu", torch.float64)


# ------------------------------------------------------------------------------------------------ references
def layernorm_ref(x, w, b, eps=1e-5, gelu=False):
    """y, mean, rstd in float64 (biased variance, as F.layer_norm); gelu: the exact-erf GELU applied to y"""
    x, w, b = f64(x), f64(w), f64(b)
    mean = x.mean(-1)
    rstd = torch.rsqrt(((x - mean[:, None]) ** 2).mean(-1) + eps)
    y = (x - mean[:, None]) * rstd[:, None] * w + b
    return (gelu_ref(y) if gelu else y), mean, rstd


def layernorm_bwd_ref(x, w, dy, eps=1e-5):
    """dx, dgamma, dbeta: autograd of F.layer_norm in float64"""
    x, w, dy = f64(x).requires_grad_(True), f64(w).requires_grad_(True), f64(dy)
    b = torch.zeros_like(w).requires_grad_(True)
    F.layer_norm(x, (x.shape[-1],), w, b, eps).backward(dy)
    return x.grad, w.grad, b.grad


def rmsnorm_ref(x, w, eps):
    """y, rstd.  HF LlamaRMSNorm rounds twice: w * bf16(x * rstd), then the product.  The inner rounding is done here, the outer one is
    left to the caller's bound."""
    x, w = f64(x), f64(w)
    rstd = torch.rsqrt((x * x).mean(-1) + eps)
    xn = (x * rstd[:, None]).float().bfloat16().double()
    return w * xn, rstd


def rmsnorm_bwd_ref(x, w, dy, dres=None, scale=None, eps=1e-5):
    """dx = scale * rstd (g - xhat mean(g xhat)) + dres,  g = dy w, xhat = x rstd  (no inner rounding: the backward is fp32 throughout)"""
    x, w, dy = f64(x), f64(w), f64(dy)
    rstd = torch.rsqrt((x * x).mean(-1, keepdim=True) + eps)
    g, xh = dy * w, x * rstd
    dx = rstd * (g - xh * (g * xh).mean(-1, keepdim=True))
    if scale is not None:
        dx = dx * float(scale)
    if dres is not None:
        dx = dx + f64(dres)
    return dx


def _Phi(x):
    return 0.5 * torch.special.erfc(-x / math.sqrt(2.0))     # erfc: no cancellation in the left tail, unlike 1 + erf


def gelu_ref(x):
    x = f64(x)
    return x * _Phi(x)


def gelu_bwd_ref(x, dy):
    x = f64(x)
    return f64(dy) * (_Phi(x) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi))


def colsum_ref(x):
    return f64(x).sum(0)


def ce_ref(logits, targets):
    """per-row loss (0 for rows whose target is < 0), dlogits of the MEAN loss over the labelled rows (ignored rows 0), the FIRST index
    of each row's maximum, and the mean loss (NaN when no row carries a label)"""
    lg, t = f64(logits), targets.detach().cpu().long()
    valid = t >= 0
    n = int(valid.sum())
    m = lg.max(-1, keepdim=True).values
    lse = m[:, 0] + torch.log(torch.exp(lg - m).sum(-1))
    tc = t.clamp(min=0)
    loss = torch.where(valid, lse - lg.gather(1, tc[:, None])[:, 0], torch.zeros_like(lse))
    p = torch.exp(lg - lse[:, None])
    p[torch.arange(lg.shape[0]), tc] -= 1.0
    dlogits = torch.where(valid[:, None], p / max(n, 1), torch.zeros_like(p))
    cols = torch.arange(lg.shape[1]).expand_as(lg)
    argmax = torch.where(lg == m, cols, torch.full_like(cols, lg.shape[1])).min(-1).values
    mean = loss.sum() / n if n else torch.tensor(float("nan"), dtype=torch.float64)
    return loss, dlogits, argmax, mean


# ------------------------------------------------------------------------------------------------ inputs
def bf16_sweep():
    """every finite bf16 bit pattern with 2^-40 <= |x| <= 2^40, plus +0 and -0: 2 * (80 * 128 + 1) + 2 = 20484 values.  Subnormals and
    huge values are left out on purpose (x * x must stay finite in fp32 for the GELU derivative)."""
    bits = torch.from_numpy(np.arange(65536, dtype=np.uint16).view(np.int16).copy())
    v = bits.view(torch.bfloat16)
    a = v.double().abs()
    keep = ((a >= 2.0 ** -40) & (a <= 2.0 ** 40)) | (a == 0)
    return v[keep].clone()


def sweep_matrix(dev, rows=21, cols=1024):
    """bf16_sweep() zero-padded to [rows, cols]"""
    s = bf16_sweep()
    m = torch.zeros(rows * cols, dtype=torch.bfloat16)
    m[: s.numel()] = s
    return m.view(rows, cols).to(dev)


def _sentinel(dtype, sentinel_bits=None):
    if dtype == torch.bfloat16:
        return torch.int16, SENTINEL_BF16 if sentinel_bits is None else sentinel_bits
    assert dtype == torch.float32
    return torch.int32, SENTINEL_F32 if sentinel_bits is None else sentinel_bits


def padded(shape, pad_cols, dev, sentinel_bits=None, dtype=torch.bfloat16):
    """a view of `shape` ([rows, cols] or [n]) into a buffer whose row pitch is cols + pad_cols (1-D: a tail of pad_cols elements);
    the WHOLE buffer, view included, starts as the sentinel bit pattern.  assert_padding_untouched(view) checks the padding afterwards."""
    assert pad_cols % 8 == 0 and pad_cols > 0
    it, bits = _sentinel(dtype, sentinel_bits)
    if len(shape) == 1:
        buf = torch.full((shape[0] + pad_cols,), bits, dtype=it, device=dev).view(dtype)
        return buf[: shape[0]]
    rows, cols = shape
    buf = torch.full((rows, cols + pad_cols), bits, dtype=it, device=dev).view(dtype)
    return buf[:, :cols]


def padded_like(t, pad_cols=8):
    """a strided copy of t (2-D) with sentinel padding: the same values behind a row pitch of cols + pad_cols"""
    v = padded(tuple(t.shape), pad_cols, t.device, dtype=t.dtype)
    v.copy_(t)
    return v


def assert_padding_untouched(view, sentinel_bits=None, what=""):
    it, bits = _sentinel(view.dtype, sentinel_bits)
    buf = view._base
    assert buf is not None, "not a view made by padded()"
    pad = buf[view.shape[0]:] if view.dim() == 1 else buf[:, view.shape[1]:]
    assert pad.numel() > 0
    bad = pad.contiguous().view(it) != bits
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} padding elements were overwritten"


# ------------------------------------------------------------------------------------------------ assertions
def _record(what, share):
    SHARES[what] = max(SHARES.get(what, 0.0), share)
    print(f"ROWWISE-SHARE\t{what}\t{share:.4f}")


def assert_within(got, ref64, bound, what):
    """|got - ref| <= bound elementwise (a NaN or inf in got fails; where the bound is 0 the values must be equal).  Returns and records
    the worst ratio of error to bound."""
    got, ref64 = f64(got), f64(ref64)
    bound = f64(bound).expand_as(ref64) if torch.is_tensor(bound) else torch.full_like(ref64, float(bound))
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    err = (got - ref64).abs()
    ok = err <= bound
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp(min=1e-300))
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    i = int(ratio.argmax())
    worst = float(ratio.flatten()[i])
    assert bool(ok.all()), (f"{what}: {int((~ok).sum())}/{ok.numel()} elements outside the bound; worst error/bound {worst:.3f} at flat index {i}: "
                            f"got {float(got.flatten()[i])!r} ref {float(ref64.flatten()[i])!r} bound {float(bound.flatten()[i]):.3e}")
    _record(what, worst)
    return worst


def assert_one_rounding(got, ref64, atol_terms, what):
    """one bf16 rounding of the exact result plus the kernel's fp32 allowance: |got - ref| <= 2^-8 |ref| + atol_terms"""
    ref64 = f64(ref64)
    at = f64(atol_terms) if torch.is_tensor(atol_terms) else float(atol_terms)
    return assert_within(got, ref64, U_BF16 * ref64.abs() + at, what)


def excess_over_one_rounding(got, ref64):
    """max(|got - ref| - 2^-8 |ref|, 0) elementwise, float64"""
    got, ref64 = f64(got), f64(ref64)
    return ((got - ref64).abs() - U_BF16 * ref64.abs()).clamp(min=0)

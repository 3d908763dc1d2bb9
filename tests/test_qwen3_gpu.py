"""GPU: Qwen3 LLMs (per-head q/k RMSNorm fused with RoPE in the training forward and prefill, its backward, the norm inside the decode
attention kernel) and the Llama-3.1 `llama3` RoPE tables on the HIP path -- the kernels against torch restatements, the tiny geometries
against the reference's fixtures (tools/make_golden_qwen3.py) and true widths against the fp32 restatement of tests/qwen3_cases.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import slam_oracle as O
from tests import golden_util as G
from tests.qwen3_cases import (CASES, GEN_RUNS, GENERATE_CASE, LLAMA31_CASE, LLAMA31_NAME, P, gen_key, head_rmsnorm, qwen3_embeds,
                               qwen3_forward, qwen3_weights)

pytestmark = pytest.mark.gpu
EPS = 1e-6
U = 2.0 ** -7       # largest relative spacing of bf16 (8 significant bits): one rounding moves a value by at most U * |value|


def _bf(t):
    return t.to(torch.bfloat16).float()


# ------------------------------------------------------------------------------------------------ fused norm + RoPE kernel
def _norm_rope_reference(x, wq, wk, Hq, cos, sin):
    """x [M, H, D] fp32 (bf16 values), cos / sin [M, D/2]: Qwen3RMSNorm with its two roundings (cast back to bf16, then the weight), then
    rotate-half RoPE rounded once.  Returns (out, y = the normed un-rotated heads, rstd [M, H])."""
    M, H, D = x.shape
    rstd = torch.rsqrt(x.pow(2).mean(-1) + EPS)
    w = torch.cat([wq[None].expand(Hq, D), wk[None].expand(H - Hq, D)])[None]
    y = _bf(w * _bf(x * rstd[..., None]))
    a, b = y[..., : D // 2], y[..., D // 2:]
    c, s = cos[:, None], sin[:, None]
    return _bf(torch.cat([a * c - b * s, b * c + a * s], -1)), y, rstd


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Hq,Hkv", [(2, 1), (8, 2), (32, 8)])
@pytest.mark.parametrize("with_positions", [False, True])
def test_head_rmsnorm_rope_matches_restatement(dev, D, Hq, Hkv, with_positions):
    """H = 3, 8+2, 32+8 heads inside a wider buffer (v columns and 24 LoRA-A columns behind them: ld is not H * D), M = 3 x 37 rows (no
    multiple of the 256 / (D/16) heads a workgroup covers), with and without explicit positions, with and without the training stash.
    Bound: the restatement rounds at the same three places, so the kernel may differ from it only where a last-bit difference of rstd
    (hardware rsqrt, another summation order) flips a rounding: one flip of bf16(x rstd) moves y = bf16(w xn) by <= 2 U |y|, both
    inputs of a rotated pair carry that, and the final rounding may flip once more: |err| <= 3 U (|y1| + |y2|)."""
    from slam_llm_amd import ops
    B, T, H = 3, 37, Hq + Hkv
    M, N = B * T, (Hq + 2 * Hkv) * D
    g = torch.Generator(device=dev).manual_seed(D + H)
    buf = (torch.randn(M, N + 24, generator=g, device=dev) * 1.7).to(torch.bfloat16)
    wq = 1 + 0.3 * torch.randn(D, generator=g, device=dev)
    wk = 1 + 0.3 * torch.randn(D, generator=g, device=dev)
    cos, sin = [t[:, : D // 2].contiguous().to(dev) for t in O.rope_tables(T + 9, D, 1e6)]
    positions = None
    if with_positions:
        positions = torch.randint(0, T + 9, (M,), generator=g, device=dev).to(torch.int32)
    pos = positions.long() if with_positions else torch.arange(M, device=dev) % T
    ref, y, rstd_ref = _norm_rope_reference(buf[:, : H * D].float().view(M, H, D), wq, wk, Hq, cos[pos], sin[pos])
    bound = 3 * U * (y[..., : D // 2].abs() + y[..., D // 2:].abs()).repeat(1, 1, 2) + 1e-30
    outs = []
    for stash in (False, True):
        q = buf.clone()
        rstd, x = ops.head_rmsnorm_rope(q, 0, B, T, Hq, Hkv, D, wq, wk, EPS, cos, sin, positions=positions, stash=stash)
        torch.cuda.synchronize()
        assert torch.equal(q[:, H * D:], buf[:, H * D:]), "columns behind the q|k heads were written"
        err = (q[:, : H * D].float().view(M, H, D) - ref).abs()
        assert bool((err <= bound).all()), (D, H, stash, float((err / bound).max()))
        if stash:
            assert torch.equal(x, buf[:, : H * D]) and x.is_contiguous()
            # fp32 rstd: the hardware rsqrt (~1 ulp) and another order of the D-term sum
            assert torch.allclose(rstd, rstd_ref, rtol=1e-5, atol=0), float(((rstd - rstd_ref) / rstd_ref).abs().max())
        else:
            assert rstd is None and x is None
        outs.append(q)
    assert torch.equal(outs[0], outs[1]), "the stash outputs changed the result"
    # the norm is far outside the bound of a plain RoPE: this test cannot pass on rope_inplace
    plain = buf.clone()
    ops.rope_inplace(plain, 0, B, T, H, D, cos, sin, positions=positions)
    assert float(((plain[:, : H * D].float().view(M, H, D) - ref).abs() / bound).max()) > 10


def test_head_rmsnorm_rope_rejects_bad_arguments(dev):
    from slam_llm_amd import lib, ops
    q = torch.zeros(8, 3 * 64 + 8, dtype=torch.bfloat16, device=dev)
    w = torch.ones(64, device=dev)
    cos, sin = [t[:, :32].contiguous().to(dev) for t in O.rope_tables(8, 64, 1e4)]
    p = ops._p
    with pytest.raises(lib.SlamHipError, match="head_dim"):
        lib.call("slam_head_rmsnorm_rope", p(q), q.stride(0), 0, p(w), p(w), EPS, p(cos), p(sin), None, None, None, 1, 8, 2, 1, 96, ops._s())
    with pytest.raises(lib.SlamHipError, match="must fit in a row"):
        lib.call("slam_head_rmsnorm_rope", p(q), q.stride(0), 64, p(w), p(w), EPS, p(cos), p(sin), None, None, None, 1, 8, 2, 1, 64, ops._s())
    with pytest.raises(lib.SlamHipError, match="both be set or both null"):
        r = torch.zeros(8, 3, device=dev)
        lib.call("slam_head_rmsnorm_rope", p(q), q.stride(0), 0, p(w), p(w), EPS, p(cos), p(sin), None, p(r), None, 1, 8, 2, 1, 64, ops._s())
    with pytest.raises(lib.SlamHipError, match="null norm weight"):
        lib.call("slam_head_rmsnorm_bwd", p(q), q.stride(0), 0, p(q), p(w), p(w), None, 8, 2, 1, 64, ops._s())


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Hq,Hkv", [(2, 1), (8, 2), (32, 8)])
def test_head_rmsnorm_bwd_matches_autograd(dev, D, Hq, Hkv):
    """dx against torch autograd of the fp32 norm on the stash the forward kernel wrote; the result is one bf16 rounding of an fp32
    expression whose cancelling term x^ mean(g x^) is itself exact to fp32: |err| <= U |ref| + 1e-5 max|ref|.  v and the LoRA-A columns
    keep their bits."""
    from slam_llm_amd import ops
    B, T, H = 2, 53, Hq + Hkv
    M, N = B * T, (Hq + 2 * Hkv) * D
    g = torch.Generator(device=dev).manual_seed(7 * D + H)
    buf = (torch.randn(M, N + 24, generator=g, device=dev) * 1.7).to(torch.bfloat16)
    dqkv = torch.randn(M, N + 24, generator=g, device=dev).to(torch.bfloat16)
    wq = 1 + 0.3 * torch.randn(D, generator=g, device=dev)
    wk = 1 + 0.3 * torch.randn(D, generator=g, device=dev)
    cos, sin = [t[:, : D // 2].contiguous().to(dev) for t in O.rope_tables(T, D, 1e6)]
    rstd, x = ops.head_rmsnorm_rope(buf.clone(), 0, B, T, Hq, Hkv, D, wq, wk, EPS, cos, sin, stash=True)
    xr = x.float().view(M, H, D).requires_grad_(True)
    w = torch.cat([wq[None].expand(Hq, D), wk[None].expand(Hkv, D)])[None]
    head_rmsnorm(xr, w, EPS).backward(dqkv[:, : H * D].float().view(M, H, D))
    ref = xr.grad
    got = dqkv.clone()
    ops.head_rmsnorm_bwd(got, 0, x, rstd, Hq, Hkv, D, wq, wk)
    torch.cuda.synchronize()
    assert torch.equal(got[:, H * D:], dqkv[:, H * D:]), "v / LoRA-A columns were written"
    err = (got[:, : H * D].float().view(M, H, D) - ref).abs()
    bound = U * ref.abs() + 1e-5 * float(ref.abs().max())
    assert bool((err <= bound).all()), (D, H, float((err / bound).max()))
    # not the identity, and not the weight alone: both are far outside the bound
    assert float(((dqkv[:, : H * D].float().view(M, H, D) * w * rstd[..., None] - ref).abs() / bound).max()) > 10


# ------------------------------------------------------------------------------------------------ decode attention
def _decode_case(dev, D, rep, lora, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    Hkv, B, beams, Tp, G_, n_prev = 2, 2, 2, 9, 6, 3
    Hq, R = Hkv * rep, B * beams
    N = (Hq + 2 * Hkv) * D
    lr = 12 if lora else 0
    qkv = torch.randn(R, N + lr, generator=g, device=dev).to(torch.bfloat16)
    lora_b = (torch.randn(N, 16, generator=g, device=dev) * 0.3).to(torch.bfloat16) if lora else None
    bias = _bf(torch.randn(N, generator=g, device=dev))
    wq = 1 + 0.3 * torch.randn(D, generator=g, device=dev)
    wk = 1 + 0.3 * torch.randn(D, generator=g, device=dev)
    cos, sin = [t[:, : D // 2].contiguous().to(dev) for t in O.rope_tables(Tp + G_, D, 1e6)]
    start = torch.tensor([0, 3], dtype=torch.int32, device=dev)
    pos = torch.tensor([Tp + n_prev, Tp + n_prev, Tp - 3 + n_prev, Tp - 3 + n_prev], dtype=torch.int32, device=dev)
    Kp = torch.randn(B, Tp, Hkv * D, generator=g, device=dev).to(torch.bfloat16)
    Vp = torch.randn(B, Tp, Hkv * D, generator=g, device=dev).to(torch.bfloat16)
    Kg = torch.randn(R, G_, Hkv * D, generator=g, device=dev).to(torch.bfloat16)
    Vg = torch.randn(R, G_, Hkv * D, generator=g, device=dev).to(torch.bfloat16)
    anc = torch.tensor([[0, 1, 1, 0, 0, 0], [1, 0, 1, 1, 1, 1], [2, 2, 3, 2, 2, 2], [3, 3, 3, 3, 3, 3]], dtype=torch.int32, device=dev)
    return dict(qkv=qkv, lora_b=lora_b, lr=lr, bias=bias, wq=wq, wk=wk, cos=cos, sin=sin, start=start, pos=pos, Kp=Kp, Vp=Vp, Kg=Kg,
                Vg=Vg, anc=anc, Hq=Hq, Hkv=Hkv, D=D, B=B, beams=beams, R=R, Tp=Tp, G=G_, n_prev=n_prev, N=N)


def _run_decode(c, bias, qk_norm, raw=False):
    """raw: through the C entry point slam_attn_decode_qknorm itself (null norm weights included)"""
    from slam_llm_amd import lib, ops
    Kg, Vg, anc = c["Kg"].clone(), c["Vg"].clone(), c["anc"].clone()
    O_ = torch.empty(c["R"], c["Hq"] * c["D"], dtype=torch.bfloat16, device=c["qkv"].device)
    if not raw:
        ops.attn_decode(c["qkv"], c["lora_b"], c["lr"], c["cos"], c["sin"], c["pos"], c["Kp"], c["Vp"], c["start"], Kg, Vg, anc, None,
                        c["n_prev"], c["beams"], c["Hq"], c["Hkv"], c["D"], c["D"] ** -0.5, O_, qkv_bias=bias, qk_norm=qk_norm)
    else:
        q, lb, p = c["qkv"], c["lora_b"], ops._p
        wq, wk, eps = qk_norm if qk_norm is not None else (None, None, 0.0)
        lib.call("slam_attn_decode_qknorm", p(q), q.stride(0), p(lb), lb.stride(0) if lb is not None else 0, c["lr"], p(c["cos"]),
                 p(c["sin"]), p(c["pos"]), p(c["Kp"]), p(c["Vp"]), p(c["start"]), p(Kg), p(Vg), p(anc), None, c["n_prev"], p(O_),
                 O_.stride(0), c["R"], c["beams"], c["Tp"], c["G"], c["Hq"], c["Hkv"], c["D"], c["D"] ** -0.5, p(bias), p(wq), p(wk), eps,
                 ops._s())
    torch.cuda.synchronize()
    return O_, Kg, Vg, anc


def _decode_reference(c, bias, qk_norm):
    """the new token's prelude in HF's order under peft -- bias, LoRA delta, per-head RMSNorm, RoPE -- then attention over
    [prompt KV | generated KV via the ancestor table | the new token]"""
    D, Hq, Hkv, N, R, n = c["D"], c["Hq"], c["Hkv"], c["N"], c["R"], c["n_prev"]
    x = c["qkv"][:, :N].float()
    if bias is not None:
        x = _bf(x + bias)
    if c["lora_b"] is not None:
        u = c["qkv"][:, N: N + c["lr"]].float()
        x = _bf(x + _bf(u @ c["lora_b"][:, : c["lr"]].float().t()))
    x = x.view(R, Hq + 2 * Hkv, D)
    qk = x[:, : Hq + Hkv]
    if qk_norm is not None:
        wq, wk, eps = qk_norm
        w = torch.cat([wq[None].expand(Hq, D), wk[None].expand(Hkv, D)])[None]
        qk = _bf(w * _bf(qk * torch.rsqrt(qk.pow(2).mean(-1, keepdim=True) + eps)))
    cos, sin = c["cos"][c["pos"].long()][:, None], c["sin"][c["pos"].long()][:, None]
    a, b = qk[..., : D // 2], qk[..., D // 2:]
    qk = _bf(torch.cat([a * cos - b * sin, b * cos + a * sin], -1))
    q, k_new, v_new = qk[:, :Hq], qk[:, Hq:], _bf(x[:, Hq + Hkv:])
    out = torch.empty(R, Hq, D, device=x.device)
    for r in range(R):
        item = r // c["beams"]
        s = int(c["start"][item])
        ks = [c["Kp"][item, s:].float().view(-1, Hkv, D)] + [c["Kg"][int(c["anc"][r, j]), j].float().view(1, Hkv, D) for j in range(n)]
        vs = [c["Vp"][item, s:].float().view(-1, Hkv, D)] + [c["Vg"][int(c["anc"][r, j]), j].float().view(1, Hkv, D) for j in range(n)]
        Kt = torch.cat(ks + [k_new[r:r + 1]])
        Vt = torch.cat(vs + [v_new[r:r + 1]])
        rep = Hq // Hkv
        Kt, Vt = Kt.repeat_interleave(rep, 1), Vt.repeat_interleave(rep, 1)     # [L, Hq, D]
        att = torch.softmax(torch.einsum("hd,lhd->hl", q[r], Kt) * D ** -0.5, -1)
        out[r] = torch.einsum("hl,lhd->hd", att, Vt)
    return out.reshape(R, Hq * D), k_new, v_new


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("rep", [1, 2, 3, 4, 5, 6, 7, 8])
def test_attn_decode_qknorm_every_gqa_ratio(dev, D, rep):
    """same bounds as the q|k|v bias test of the decode kernel (tests/test_qwen2_gpu.py): bf16 outputs of an attention over ~13 keys"""
    for lora in (False, True):
        c = _decode_case(dev, D, rep, lora, seed=rep)
        qk = (c["wq"], c["wk"], EPS)
        for bias in (None, c["bias"]):
            O_, Kg, Vg, anc = _run_decode(c, bias, qk)
            ref, k_new, v_new = _decode_reference(c, bias, qk)
            err = float((O_.float() - ref).abs().max())
            assert err < 2e-2 * float(ref.abs().max()) + 1e-2, (D, rep, lora, bias is not None, err)
            n = c["n_prev"]
            for r in range(c["R"]):
                assert float((Kg[r, n].float().view(c["Hkv"], D) - k_new[r]).abs().max()) <= 1e-2 * float(k_new.abs().max()) + 1e-3
                assert float((Vg[r, n].float().view(c["Hkv"], D) - v_new[r]).abs().max()) <= 1e-2 * float(v_new.abs().max()) + 1e-3
                assert int(anc[r, n]) == r
            # the norm moves the result, and the appended key, by more than the tolerance
            ref0, k0, _ = _decode_reference(c, bias, None)
            assert float((ref0 - ref).abs().max()) > 2 * (2e-2 * float(ref.abs().max()) + 1e-2)
            assert float((k0 - k_new).abs().max()) > 2 * (1e-2 * float(k_new.abs().max()) + 1e-3)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("rep", [1, 2, 3, 4, 5, 6, 7, 8])
def test_attn_decode_qknorm_null_weights_are_bit_identical_to_attn_decode_bias(dev, D, rep):
    for lora in (False, True):
        c = _decode_case(dev, D, rep, lora, seed=20 + rep)
        for bias in (None, c["bias"]):
            a = _run_decode(c, bias, None)                # slam_attn_decode / slam_attn_decode_bias
            b = _run_decode(c, bias, None, raw=True)      # slam_attn_decode_qknorm with null norm weights
            for x, y in zip(a, b):
                assert torch.equal(x, y)


def test_attn_decode_qknorm_rejects_through_the_c_abi(dev):
    from slam_llm_amd import lib
    c = _decode_case(dev, 64, 1, False)
    c9 = dict(c, Hq=9 * c["Hkv"])
    with pytest.raises(lib.SlamHipError, match=r"slam_attn_decode_qknorm: Hq/Hkv must be in \[1, 8\]"):
        _run_decode(c9, None, (c["wq"], c["wk"], EPS), raw=True)
    with pytest.raises(lib.SlamHipError, match="both be set or both null"):
        _run_decode(c, None, (c["wq"], None, EPS), raw=True)


# ------------------------------------------------------------------------------------------------ tiny geometries vs the reference
ALL_CASES = dict(CASES, **{LLAMA31_NAME: LLAMA31_CASE})


def _build(case, dev, W=None):
    from slam_llm_amd.model import SlamHipModel
    cfg = case["cfg"]
    W = W if W is not None else qwen3_weights(cfg, seed=42, norm_scale=case["norm_scale"])
    return SlamHipModel(dict(cfg, lora_dropout=0.0), dev).load_weights(W), W


def _batch(fx, dev, prefix="batch."):
    return {k[len(prefix):]: torch.from_numpy(fx[k]).to(dev) for k in fx.files if k.startswith(prefix)}


def _rel(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max() / (np.abs(ref).max() + 1e-12))


@pytest.mark.parametrize("name", list(ALL_CASES))
def test_forward_matches_reference_fixture(dev, name):
    """loss (1e-2, the tolerance the fixtures' comparison losses are sized against), accuracy, and every logit of every label row and
    every 5th other row (golden_util.check_logits) against the reference's slam_model over HF Qwen3 / Llama with llama3 RoPE"""
    fx = G.load(name)
    case = ALL_CASES[name]
    cfg = case["cfg"]
    model, W = _build(case, dev)
    assert (model.llm.layers[0].q_norm is not None) == bool(cfg["llm_qk_norm"])
    if cfg["tie_embeddings"]:
        assert model.llm.lm_head.data_ptr() == model.llm.embed.data_ptr()
    model.train()
    b = _batch(fx, dev)
    enc = model.encoder.forward_btc(b["audio_mel"].float().contiguous())
    g, a = G.sub(fx, "encoder_out", enc.float().cpu().numpy())
    assert _rel(a, g) < 2e-2
    model._refresh()
    proj = model.encoder_projector.forward_hip(enc, None)
    g, a = G.sub(fx, "projector_out", proj.float().cpu().numpy())
    assert _rel(a, g) < 2e-2
    model.return_logits = True
    outputs, acc = model(**{k: v.clone() for k, v in b.items()})
    other = "loss_with_unit_qk_norm" if cfg["llm_qk_norm"] else "loss_with_default_rope"
    print(f"{name}: loss {float(outputs.loss.detach()):.6f} fixture {float(fx['loss.0']):.6f} ({other} {float(fx[other]):.6f}) acc {float(acc):.4f}")
    assert abs(float(outputs.loss) - float(fx["loss.0"])) < 1e-2, (float(outputs.loss), float(fx["loss.0"]))
    G.check_logits(outputs.logits, torch.from_numpy(fx["logits_full"]), b["attention_mask"], b["labels"], f"{name} vs fixture")
    assert abs(float(acc) - float(fx["acc.0"])) <= 1.0 / max(1, int((b["labels"][:, 1:] != -100).sum()))


@pytest.mark.parametrize("name", list(ALL_CASES))
def test_gradients_and_training_steps_match_reference(dev, name):
    """every trainable gradient (cosine floor of the frozen-LLM family, norm within 3 %), the losses of three steps, and the parameters
    after the three AdamW steps.  Adam's first real step is lr * sign(g): an element whose gradient is below the bf16 noise may move
    the other way, so the parameters are compared by the direction of the whole update -- with gradient cosines >= 0.999 the noise is
    <= 4.5 % of the gradient rms, which flips the sign of <= 1.5 % of Gaussian elements, 1 - cos <= 0.03 for a sign step: floor 0.95 --
    and elementwise by the largest distance two runs of these steps can reach (2 x the sum of the learning rates)."""
    from slam_llm_amd.model import SlamAdamW
    fx = G.load(name)
    case = ALL_CASES[name]
    model, W = _build(case, dev)
    model.train()
    b = _batch(fx, dev)
    opt = SlamAdamW(model, lr=1e-2, weight_decay=0.01)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda s: O.lr_lambda(s, 2, 10))
    init = {n: p.detach().float().cpu().numpy().copy() for n, p in model.store.params.items()}
    losses, lr_sum, worst_grad = [], 0.0, (1.0, "")
    for step in range(3):
        outputs, acc = model(**{k: v.clone() for k, v in b.items()})
        outputs.loss.backward()
        if step == 0:
            for n, p in model.store.params.items():
                g = p.grad.float().cpu().numpy()
                gold, mine = G.sub(fx, "grad." + n, g)
                worst_grad = min(worst_grad, (G.cosine(gold, mine), n))
                G.floor_check(G.cosine(gold, mine), G.FLOORS["frozen"], f"grad {n}")
                gn = float(fx["grad." + n + ".__norm"])
                assert abs(float(np.sqrt((g.astype(np.float64) ** 2).sum())) - gn) < 3e-2 * gn + 1e-7, n
        lr_sum += float(sched.get_last_lr()[0])
        opt.step(); sched.step(); opt.zero_grad()
        losses.append(float(outputs.loss))
    assert abs(losses[0] - losses[1]) < 1e-6
    for s in range(3):
        assert abs(losses[s] - float(fx[f"loss.{s}"])) < 3e-2, (s, losses[s], float(fx[f"loss.{s}"]))
    assert set(model.state_dict().keys()) == set(O.trainable_names(W))
    worst = 1.0
    for n, p in model.store.params.items():
        gold, mine = G.sub(fx, "param." + n, p.detach().float().cpu().numpy())
        _, p0 = G.sub(fx, "param." + n, init[n])
        assert float(np.abs(gold - mine).max()) <= 2 * lr_sum + 1e-6, (n, float(np.abs(gold - mine).max()), lr_sum)
        if np.abs(gold - p0).max() > 0:
            cs = G.cosine(gold - p0, mine - p0)
            worst = min(worst, cs)
            assert cs >= 0.95, (n, cs)
    print(f"{name}: losses {losses}, worst gradient cosine {worst_grad[0]:.6f} ({worst_grad[1]}), worst update cosine {worst:.5f}")


def test_state_dict_without_qk_norm_weights_is_refused(dev):
    case = CASES["step_qwen3_tied"]
    W = qwen3_weights(case["cfg"], seed=42)
    del W[P + "model.layers.1.self_attn.k_norm.weight"]
    with pytest.raises(KeyError, match="k_norm"):
        _build(case, dev, W)


def test_pure_bf16_route_rounds_the_qk_norm_weights(dev):
    case = CASES["step_qwen3_untied"]
    W = qwen3_weights(case["cfg"], seed=42)
    model, _ = _build(case, dev, W)
    L = model.llm.layers[0]
    q0, k0 = L.q_norm.clone(), L.k_norm.clone()
    model.to(torch.bfloat16)
    for w0, w in ((q0, L.q_norm), (k0, L.k_norm)):
        assert w.dtype == torch.float32 and torch.equal(w, w0.to(torch.bfloat16).float()) and not torch.equal(w, w0)


def test_existing_configs_draw_the_same_random_weights(dev):
    """init_random draws q_norm / k_norm last: a config without llm_qk_norm, and everything drawn before them in one with it, stay"""
    from slam_llm_amd.model import SlamHipModel
    cfg = dict(CASES["step_qwen3_tied"]["cfg"], lora_dropout=0.0)
    a, b = SlamHipModel(dict(cfg, llm_qk_norm=False), dev), SlamHipModel(cfg, dev)
    a.init_random(5)
    b.init_random(5)
    assert a.llm.layers[0].q_norm is None and b.llm.layers[1].k_norm is not None
    assert torch.equal(a.llm.embed, b.llm.embed) and torch.equal(a.llm.norm_w, b.llm.norm_w)
    assert torch.equal(a.llm.layers[1].ln2, b.llm.layers[1].ln2) and torch.equal(a.llm.layers[1].down.Wext, b.llm.layers[1].down.Wext)


# ------------------------------------------------------------------------------------------------ generate
def _ref_logits_fn(W, cfg, cpu):
    embeds_ref = qwen3_embeds(W, cfg, cpu)
    emb_w = W[P + "model.embed_tokens.weight"]
    mask = cpu["attention_mask"].long()

    def ref_logits(toks):
        x = torch.cat([embeds_ref, F.embedding(toks, emb_w)], dim=1)
        m = torch.cat([mask, torch.ones_like(toks)], dim=1)
        return qwen3_forward(W, cfg, x, m, None, position_ids=O.generate_position_ids(m))[1][:, -1, :]
    return ref_logits


@pytest.mark.parametrize("name", list(CASES))
def test_generate_matches_reference_tokens(dev, name):
    """greedy and beam 4 vs the reference's generate (fp32), margin-aware as tests/test_qwen2_gpu.py: a greedy row must match up to its
    first step whose fp32 top-2 margin is below 2 x the measured bf16 noise; a beam item either reproduces the reference hypothesis or
    one whose fp32 score is within the noise.  The beam-4 run is repeated on the batch tiled x6 (72 hypotheses > 64): the decode
    step's GEMM path, where the new q / k reach the attention kernel un-normed as well."""
    C = GENERATE_CASE
    cfg = CASES[name]["cfg"]
    fx = G.load("generate_qwen3")
    W = qwen3_weights(cfg, seed=42, norm_scale=C["norm_scale"])
    model, _ = _build(CASES[name], dev, W)
    model.eval()
    b = _batch(fx, dev, prefix=f"{name}.batch.")
    cpu = {k: v.cpu() for k, v in b.items()}
    eos, L = int(fx[f"{name}.eos"]), C["max_new_tokens"]
    ref_logits = _ref_logits_fn(W, cfg, cpu)
    embeds, am = model(**{k: v.clone() for k, v in b.items()}, inference_mode=True)
    B, T, d = embeds.shape
    lg0, _ = model.llm.prefill(embeds.reshape(B * T, d), B, T, am, L)
    noise = 3.0 * float((lg0.float().cpu() - ref_logits(torch.zeros((B, 0), dtype=torch.int64))).abs().max())
    compared = 0
    for nb, lp in GEN_RUNS:
        want = torch.from_numpy(fx[gen_key(name, nb, lp)])
        for tile in ((1, 6) if nb > 1 else (1,)):
            bt = {k: v.repeat(tile, *([1] * (v.dim() - 1))) for k, v in b.items()}
            got = model.generate(**bt, max_new_tokens=L, num_beams=nb, length_penalty=lp, eos_token_id=eos, pad_token_id=C["pad"]).cpu()
            assert (B * tile * nb > 64) == (tile > 1)
            got = got[:B]
            n = max(got.shape[1], want.shape[1])
            pad_to = lambda x: torch.cat([x, torch.full((B, n - x.shape[1]), C["pad"], dtype=torch.int64)], 1)  # noqa: E731
            got_p, want_p = pad_to(got), pad_to(want)
            # teacher-forced fp32 log-probs along both sequences
            lp_got, lp_want, margins = torch.zeros(B), torch.zeros(B), []
            alive_g, alive_w = torch.ones(B, dtype=torch.bool), torch.ones(B, dtype=torch.bool)
            len_g, len_w = torch.zeros(B), torch.zeros(B)
            for t in range(n):
                lw = F.log_softmax(ref_logits(want_p[:, :t]).float(), -1)
                top2 = lw.topk(2, -1).values
                margins.append(top2[:, 0] - top2[:, 1])
                lp_want += torch.where(alive_w, lw.gather(1, want_p[:, t:t + 1])[:, 0], torch.zeros(B))
                len_w += alive_w.float()
                alive_w &= want_p[:, t] != eos
                lg_ = F.log_softmax(ref_logits(got_p[:, :t]).float(), -1)
                lp_got += torch.where(alive_g, lg_.gather(1, got_p[:, t:t + 1])[:, 0], torch.zeros(B))
                len_g += alive_g.float()
                alive_g &= got_p[:, t] != eos
            margins = torch.stack(margins)
            for r in range(B):
                if torch.equal(got_p[r], want_p[r]):
                    compared += n
                    continue
                if nb == 1:
                    close = (margins[:, r] < 2 * noise).nonzero()
                    upto = int(close[0]) if close.numel() else n
                    assert torch.equal(got_p[r, :upto], want_p[r, :upto]), (name, tile, r, upto, got[r], want[r], noise)
                    compared += upto
                else:
                    sg, sw = float(lp_got[r] / len_g[r] ** lp), float(lp_want[r] / len_w[r] ** lp)
                    assert sg >= sw - 2 * noise, (name, tile, r, sg, sw, noise, got[r], want[r])
    assert compared > 0
    print(f"generate {name}: noise {noise:.4f}, token positions compared exactly: {compared}")


# ------------------------------------------------------------------------------------------------ true widths
TRUE_WIDTH = {
    "qwen3-8b": dict(lora_targets=("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj"), lora_r=16, lora_alpha=16),
    "qwen3-0.6b": dict(lora_targets=("q_proj", "k_proj", "v_proj", "o_proj"), lora_r=8, lora_alpha=32),
}
# Measured on MI355X (worst LoRA gradient's 1 - cosine and its tensor; |logit err| / bound over the label rows and every 5th other row;
# prefill and decode |err| / bound); each limit sits at >= 2x its measured deviation (the suite's rule, tools/margins_report.py):
TRUE_WIDTH_MEASURED = {
    "qwen3-8b": dict(grad_dev=1.78e-4, grad_worst="layers.1.self_attn.k_proj.lora_B", logit_frac=0.2105, prefill_frac=0.1831,
                     decode_frac=0.1885),
    "qwen3-0.6b": dict(grad_dev=4.05e-4, grad_worst="layers.1.self_attn.q_proj.lora_A", logit_frac=0.2172, prefill_frac=0.1929,
                       decode_frac=0.2086),
}
# grad_cos 0.999 = 1 - 2.5 x 4.05e-4 (5.6 x the 8B deviation; the frozen-LLM family's floor); frac 0.5 = 2.3 x 0.2172
TRUE_WIDTH_FLOOR = {"qwen3-8b": dict(grad_cos=0.999, frac=0.5), "qwen3-0.6b": dict(grad_cos=0.999, frac=0.5)}


def true_width_measure(dev, preset):
    """2 LLM layers at the checkpoint's true widths (vocab 151936, tied or untied), a small Whisper encoder, three 30 s clips: the eval
    logits, the LoRA gradients against the fp32 restatement run on the device over the HIP path's own inputs_embeds, and prefill of
    T - 1 positions + one decode step against the every-row forward's last two rows.  Returns the measured deviations."""
    from slam_llm_amd.model import PRESETS, SlamHipModel
    cfg = O.make_config(**{k: v for k, v in PRESETS[preset].items()}, **TRUE_WIDTH[preset])
    cfg.update(llm_layers=2)
    W = qwen3_weights(cfg, seed=7)
    model = SlamHipModel(dict(cfg, lora_dropout=0.0), dev).load_weights(W)
    audio = O.synth_audio(3, 30.0, seed=99)
    batch = O.synth_batch(cfg, audio, prompt_len=8, answer_lens=(12, 5, 20), seed=5, left_pad=True, pad_to_30s=True)
    b = {k: v.to(dev) for k, v in batch.items()}
    model.eval()
    embeds, am = model(**{k: v.clone() for k, v in b.items() if k != "labels"}, inference_mode=True)
    Wd = {k: v.to(dev) for k, v in W.items() if k.startswith(P)}
    x = embeds.float().detach()
    names = [n for n in Wd if ".lora_" in n]
    for n in names:
        Wd[n].requires_grad_(True)
    loss_ref, logits_ref = qwen3_forward(Wd, cfg, x, b["attention_mask"], b["labels"])
    loss_ref.backward()
    model.train()
    model.return_logits = True
    outputs, _ = model(**{k: v.clone() for k, v in b.items()})
    stats = G.check_logits(outputs.logits, logits_ref.detach(), b["attention_mask"], b["labels"], f"{preset} true width")
    outputs.loss.backward()
    cos = {n: G.cosine(model.store.params[n].grad.float().cpu().numpy(), Wd[n].grad.float().cpu().numpy()) for n in names}
    worst = min(cos, key=cos.get)
    model.eval()
    rows = torch.nonzero(b["attention_mask"].all(1)).flatten()
    assert rows.numel() >= 1
    e = embeds[rows]
    B, T, d = e.shape
    lg0, cache = model.llm.prefill(e[:, :-1].reshape(B * (T - 1), d).contiguous(), B, T - 1, am[rows][:, :-1], 2)
    lg1 = model.llm.decode_step(b["input_ids"][rows, -1], cache)
    ref_prev, ref_last = logits_ref[rows, -2].detach(), logits_ref[rows, -1].detach()
    bound = 6e-2 + 2e-2 * float(ref_last.abs().max())
    m = dict(loss=float(outputs.loss), loss_ref=float(loss_ref), grad_dev=1.0 - cos[worst], grad_worst=worst,
             logit_frac=stats["max_err"] / stats["bound"], prefill_frac=float((lg0.float() - ref_prev).abs().max()) / bound,
             decode_frac=float((lg1.float() - ref_last).abs().max()) / bound, cos=cos)
    print(f"{preset} measured: " + ", ".join(f"{k}={v:.4g}" if isinstance(v, float) else f"{k}={v}" for k, v in m.items() if k != "cos"))
    return m


@pytest.mark.parametrize("preset", list(TRUE_WIDTH))
def test_true_width_against_restatement(dev, preset):
    m = true_width_measure(dev, preset)
    assert abs(m["loss"] - m["loss_ref"]) < 2e-2 + 1e-2 * m["loss_ref"]
    floor = TRUE_WIDTH_FLOOR[preset]
    for n, cs in m["cos"].items():
        G.floor_check(cs, floor["grad_cos"], f"{preset} grad {n}")
    # the bf16 bound of golden_util.check_logits (6e-2 + 2e-2 max|ref|) holds on every compared logit, on the prefill's last row and
    # on the decode step's row; `frac` is how much of it may be used
    assert m["logit_frac"] <= floor["frac"] and m["prefill_frac"] <= floor["frac"] and m["decode_frac"] <= floor["frac"], m


# ------------------------------------------------------------------------------------------------ graphs
def test_graphed_train_step_is_bit_identical_on_qwen3(dev):
    from slam_llm_amd.model import SlamAdamW
    from slam_llm_amd.train import GraphedTrainStep, lr_lambda, train_step
    name = "step_qwen3_tied"
    fx = G.load(name)
    runs = []
    for graphed in (False, True):
        model, _ = _build(CASES[name], dev)
        model.train()
        model.llm.label_rows_cap = 64
        b = _batch(fx, dev)
        opt = SlamAdamW(model, lr=1e-2, weight_decay=0.01)
        sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda s: lr_lambda(s, 2, 10))
        stepper = GraphedTrainStep(model, opt, sched, label_rows_cap=64, warmup=1) if graphed else None
        losses = [float((stepper({k: v.clone() for k, v in b.items()}) if graphed else
                         train_step(model, {k: v.clone() for k, v in b.items()}, opt, sched))[0]) for _ in range(4)]
        torch.cuda.synchronize()
        runs.append((losses, model.store.flat.clone()))
        if graphed:
            assert stepper.replays == 3
    assert runs[0][0] == runs[1][0]
    assert torch.equal(runs[0][1], runs[1][1])


# ------------------------------------------------------------------------------------------------ recipe entry
@pytest.mark.parametrize("use_peft", [True, False])
def test_recipe_invocation_trains_through_model_factory(dev, use_peft):
    """`encoder_name=whisper llm_name=Qwen3-0.6B` with the aispeech peft_config, and `use_peft=false freeze_llm=true`, at tiny widths
    through arch_overrides: the preset's QK-norm / tie / theta / head_dim survive, and one step trains"""
    from slam_llm_amd.model import SlamAdamW
    from slam_llm_amd.slam_model_hip import model_factory
    peft = dict(peft_method="lora", r=8, lora_alpha=16, lora_dropout=0.0,
                target_modules=["q_proj", "k_proj", "v_proj", "o_proj", "up_proj", "gate_proj", "down_proj"])
    tc = dict(use_peft=use_peft, peft_config=peft, freeze_llm=True, freeze_encoder=True, seed=3)
    over = dict(enc_dim=128, enc_heads=2, enc_layers=2, n_mels=128, llm_dim=192, llm_layers=2, llm_heads=6, llm_kv_heads=2, llm_ffn=512,
                vocab=1024)
    mc = dict(encoder_name="whisper", encoder_path="large-v3", encoder_projector="linear", llm_name="Qwen3-0.6B",
              random_init=True, arch_overrides=over)
    model, _ = model_factory(tc, mc)
    cfg = model.cfg
    assert cfg["llm_qk_norm"] and not cfg["llm_qkv_bias"] and cfg["rope_theta"] == 1e6 and cfg["tie_embeddings"] and cfg["llm_head_dim"] == 128
    L0 = model.llm.layers[0]
    assert L0.bias is None and tuple(L0.q_norm.shape) == (128,) and bool((L0.q_norm - 1).abs().sum() > 0)
    assert any(".lora_A." in n for n in model.state_dict()) == use_peft
    audio = O.synth_audio(2, 2.0, seed=1)
    batch = {k: v.to(dev) for k, v in O.synth_batch(cfg, audio, prompt_len=6, answer_lens=(5, 9), seed=2, left_pad=False,
                                                      pad_to_30s=False).items()}
    model.train()
    opt = SlamAdamW(model, lr=1e-2)
    losses = []
    for _ in range(3):
        outputs, _ = model(**{k: v.clone() for k, v in batch.items()})
        outputs.loss.backward()
        opt.step(); opt.zero_grad()
        losses.append(float(outputs.loss))
    assert all(np.isfinite(losses)) and losses[2] < losses[0], losses

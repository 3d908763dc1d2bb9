"""GPU: Phi-3 / Phi-4 LLMs (fused qkv_proj / gate_up_proj with one adapter each, partial rotary embedding, longrope tables) on the HIP
path -- the partial-rotary kernels against torch restatements, the tiny geometries against the reference's fixtures
(tools/make_golden_phi3.py) and a Phi-4-mini-like width against the fp32 restatement of tests/phi3_cases.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import slam_oracle as O
from tests import golden_util as G
from tests import rightpad_cases as RP
from tests.phi3_cases import (CASES, EXPECT_GRAD_DEV, FUSED_FOUR, GEN_PADS, GEN_RUNS, GENERATE_CASE, P, gen_key, longrope, partial_rope,
                              phi3_embeds, phi3_forward, phi3_weights, trainable_names)

pytestmark = pytest.mark.gpu


def _bf(t):
    return t.to(torch.bfloat16).float()


def _tables(P_, D, rot, s, dev, theta=1e4):
    """[P_, D/2] fp32 tables in the kernels' convention (s cos / s sin, then 1 / 0) and the [P_, rot] pair HF's apply_rotary_pos_emb
    takes, built from the same fp32 values"""
    inv = 1.0 / (theta ** (torch.arange(0, rot, 2, dtype=torch.float32) / rot))
    fr = torch.arange(P_, dtype=torch.float32)[:, None] * inv[None, :]
    c, sn = fr.cos() * s, fr.sin() * s
    cosT = torch.cat([c, torch.ones(P_, (D - rot) // 2)], 1).contiguous().to(dev)
    sinT = torch.cat([sn, torch.zeros(P_, (D - rot) // 2)], 1).contiguous().to(dev)
    return cosT, sinT, torch.cat([c, c], 1).to(dev), torch.cat([sn, sn], 1).to(dev)


# ------------------------------------------------------------------------------------------------ 1. the elementwise kernel
GUARD = 8       # columns in front of the heads; 24 more behind them


def _pair_sum(x, rot):
    """|x1| + |x2| of the rotated pair every element of x[..., :rot] belongs to"""
    a = x[..., : rot // 2].abs() + x[..., rot // 2: rot].abs()
    return torch.cat([a, a], -1)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("rot_of", ["16", "D/2", "3D/4"])
@pytest.mark.parametrize("with_positions", [False, True])
@pytest.mark.parametrize("s", [1.0, 1.19])
def test_head_rope_partial_matches_restatement(dev, D, rot_of, with_positions, s):
    """B 2 x T 75 rows (150: no multiple of the 16 / 32 rows of a block), H 3 heads between guard columns.  Forward against HF
    apply_rotary_pos_emb in fp32 on the same bf16 inputs, inverse=True against torch autograd of it: the kernel rounds an fp32 result
    once (2^-8 |ref|), and its fp32 expression may contract a multiply and an add (1e-5 (|x1| + |x2|)).  Dims [rot, D) and the guard
    columns keep their bits."""
    from slam_llm_amd import ops
    rot = {"16": 16, "D/2": D // 2, "3D/4": 3 * D // 4}[rot_of]
    B, T, H = 2, 75, 3
    M = B * T
    g = torch.Generator(device=dev).manual_seed(D + rot)
    buf = (torch.randn(M, GUARD + H * D + 24, generator=g, device=dev) * 1.7).to(torch.bfloat16)
    cosT, sinT, cos_hf, sin_hf = _tables(T + 9, D, rot, s, dev)
    positions = torch.randint(0, T + 9, (M,), generator=g, device=dev).to(torch.int32) if with_positions else None
    pos = positions.long() if with_positions else torch.arange(M, device=dev) % T
    x = buf[:, GUARD: GUARD + H * D].float().view(M, H, D)
    for inverse in (False, True):
        if not inverse:
            ref = partial_rope(x, cos_hf[pos][:, None], sin_hf[pos][:, None])
        else:   # x plays dL/dy: the adjoint of the rotation
            xin = torch.zeros_like(x, requires_grad=True)
            partial_rope(xin, cos_hf[pos][:, None], sin_hf[pos][:, None]).backward(x)
            ref = xin.grad
        got = buf.clone()
        ops.rope_inplace(got, GUARD, B, T, H, D, cosT, sinT, positions=positions, inverse=inverse, rot_dim=rot)
        torch.cuda.synchronize()
        assert torch.equal(got[:, :GUARD], buf[:, :GUARD]) and torch.equal(got[:, GUARD + H * D:], buf[:, GUARD + H * D:]), "guard columns written"
        gv, bv = got[:, GUARD: GUARD + H * D].view(M, H, D), buf[:, GUARD: GUARD + H * D].view(M, H, D)
        assert torch.equal(gv[..., rot:], bv[..., rot:]), "dims [rot, D) must keep their bits"
        err = (gv[..., :rot].float() - ref[..., :rot]).abs()
        bound = 2.0 ** -8 * ref[..., :rot].abs() + 1e-5 * _pair_sum(x, rot)
        assert bool((err <= bound).all()), (D, rot, inverse, s, float((err / bound).max()))
        # a whole-head rotation, and the forward rotation where the adjoint is asked for, are far outside the bound
        wrong = buf.clone()
        if inverse:
            ops.rope_inplace(wrong, GUARD, B, T, H, D, cosT, sinT, positions=positions, inverse=False, rot_dim=rot)
        else:
            ops.rope_inplace(wrong, GUARD, B, T, H, D, cosT, sinT, positions=positions)
        werr = (wrong[:, GUARD: GUARD + H * D].view(M, H, D)[..., :rot].float() - ref[..., :rot]).abs()
        assert float((werr / bound).max()) > 10
    if s != 1.0:    # "restores the input" is NOT the property of the adjoint when the tables carry a factor
        back = buf.clone()
        ops.rope_inplace(back, GUARD, B, T, H, D, cosT, sinT, positions=positions, rot_dim=rot)
        ops.rope_inplace(back, GUARD, B, T, H, D, cosT, sinT, positions=positions, inverse=True, rot_dim=rot)
        assert not torch.allclose(back[:, GUARD: GUARD + rot].float(), buf[:, GUARD: GUARD + rot].float(), rtol=0.1, atol=0.05)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("inverse", [False, True])
def test_head_rope_partial_at_full_width_is_bit_identical_to_rope_inplace(dev, D, inverse):
    from slam_llm_amd import ops
    B, T, H = 2, 75, 5
    g = torch.Generator(device=dev).manual_seed(D)
    buf = (torch.randn(B * T, GUARD + H * D + 24, generator=g, device=dev) * 1.7).to(torch.bfloat16)
    cosT, sinT, _, _ = _tables(T + 9, D, D, 1.19, dev)
    for positions in (None, torch.randint(0, T + 9, (B * T,), generator=g, device=dev).to(torch.int32)):
        a, b = buf.clone(), buf.clone()
        ops.rope_inplace(a, GUARD, B, T, H, D, cosT, sinT, positions=positions, inverse=inverse)
        ops.head_rope_partial(b, GUARD, B, T, H, D, D, cosT, sinT, positions=positions, inverse=inverse)
        torch.cuda.synchronize()
        assert torch.equal(a, b) and not torch.equal(a, buf)


def test_head_rope_partial_rejects_bad_arguments(dev):
    from slam_llm_amd import lib, ops
    q = torch.zeros(8, 3 * 64 + 8, dtype=torch.bfloat16, device=dev)
    cos, sin, _, _ = _tables(8, 64, 32, 1.0, dev)
    p, st = ops._p, ops._s

    def call(ld=q.stride(0), col0=0, cosp=p(cos), H=3, D=64, rot=32):
        lib.call("slam_head_rope_partial", p(q), ld, col0, cosp, p(sin), 0, 1, 8, H, D, rot, None, st())

    call()
    for rot in (0, 8, 24, 80):
        with pytest.raises(lib.SlamHipError, match=r"rot_dim .* multiple of 16 in \[16, head_dim\]"):
            call(rot=rot)
    with pytest.raises(lib.SlamHipError, match="head_dim 96 unsupported"):
        call(D=96, rot=48)
    with pytest.raises(lib.SlamHipError, match="inside the row"):
        call(col0=16)
    with pytest.raises(lib.SlamHipError, match="inside the row"):
        call(H=4)
    with pytest.raises(lib.SlamHipError, match="multiples of 8"):
        call(col0=4)
    with pytest.raises(lib.SlamHipError, match="null pointer"):
        call(cosp=None)
    assert float(q.float().abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ 2. decode attention
def _decode_case(dev, D, rep, lora, rot, seed=0):
    """the case of tests/test_qwen3_gpu.py's decode tests with partial-rotary tables (attention factor 1.19)"""
    g = torch.Generator(device=dev).manual_seed(seed)
    Hkv, B, beams, Tp, G_, n_prev = 2, 2, 2, 9, 6, 3
    Hq, R = Hkv * rep, B * beams
    N = (Hq + 2 * Hkv) * D
    lr = 12 if lora else 0
    qkv = torch.randn(R, N + lr, generator=g, device=dev).to(torch.bfloat16)
    lora_b = (torch.randn(N, 16, generator=g, device=dev) * 0.3).to(torch.bfloat16) if lora else None
    bias = _bf(torch.randn(N, generator=g, device=dev))
    cos, sin, _, _ = _tables(Tp + G_, D, rot, 1.19, dev, theta=1e6)
    start = torch.tensor([0, 3], dtype=torch.int32, device=dev)
    end = torch.tensor([Tp, Tp - 1], dtype=torch.int32, device=dev)
    pos = torch.tensor([Tp + n_prev, Tp + n_prev, Tp - 3 + n_prev, Tp - 3 + n_prev], dtype=torch.int32, device=dev)
    Kp = torch.randn(B, Tp, Hkv * D, generator=g, device=dev).to(torch.bfloat16)
    Vp = torch.randn(B, Tp, Hkv * D, generator=g, device=dev).to(torch.bfloat16)
    Kg = torch.randn(R, G_, Hkv * D, generator=g, device=dev).to(torch.bfloat16)
    Vg = torch.randn(R, G_, Hkv * D, generator=g, device=dev).to(torch.bfloat16)
    anc = torch.tensor([[0, 1, 1, 0, 0, 0], [1, 0, 1, 1, 1, 1], [2, 2, 3, 2, 2, 2], [3, 3, 3, 3, 3, 3]], dtype=torch.int32, device=dev)
    return dict(qkv=qkv, lora_b=lora_b, lr=lr, bias=bias, cos=cos, sin=sin, start=start, end=end, pos=pos, Kp=Kp, Vp=Vp, Kg=Kg, Vg=Vg,
                anc=anc, Hq=Hq, Hkv=Hkv, D=D, B=B, beams=beams, R=R, Tp=Tp, G=G_, n_prev=n_prev, N=N, rot=rot)


def _run_decode(c, bias, rot, entry=None, end=None, qk_norm=None):
    """entry None: through ops.attn_decode(rot_dim=rot); else the named C entry point itself"""
    from slam_llm_amd import lib, ops
    Kg, Vg, anc = c["Kg"].clone(), c["Vg"].clone(), c["anc"].clone()
    O_ = torch.empty(c["R"], c["Hq"] * c["D"], dtype=torch.bfloat16, device=c["qkv"].device)
    if entry is None:
        ops.attn_decode(c["qkv"], c["lora_b"], c["lr"], c["cos"], c["sin"], c["pos"], c["Kp"], c["Vp"], c["start"], Kg, Vg, anc, None,
                        c["n_prev"], c["beams"], c["Hq"], c["Hkv"], c["D"], c["D"] ** -0.5, O_, qkv_bias=bias, prompt_end=end, rot_dim=rot)
    else:
        q, lb, p = c["qkv"], c["lora_b"], ops._p
        wq, wk, eps = qk_norm if qk_norm is not None else (None, None, 0.0)
        tail = (p(end), ops._s()) if entry == "slam_attn_decode_span" else (p(end), rot, ops._s())
        lib.call(entry, p(q), q.stride(0), p(lb), lb.stride(0) if lb is not None else 0, c["lr"], p(c["cos"]), p(c["sin"]), p(c["pos"]),
                 p(c["Kp"]), p(c["Vp"]), p(c["start"]), p(Kg), p(Vg), p(anc), None, c["n_prev"], p(O_), O_.stride(0), c["R"], c["beams"],
                 c["Tp"], c["G"], c["Hq"], c["Hkv"], c["D"], c["D"] ** -0.5, p(bias), p(wq), p(wk), eps, *tail)
    torch.cuda.synchronize()
    return O_, Kg, Vg, anc


def _decode_reference(c, bias, rot):
    """tests/test_qwen3_gpu.py's restatement (bias, LoRA delta, RoPE in HF's order under peft, then attention over [prompt KV | generated
    KV via the ancestor table | the new token]) with the rotation over the first rot dims of a head only"""
    D, Hq, Hkv, N, R, n = c["D"], c["Hq"], c["Hkv"], c["N"], c["R"], c["n_prev"]
    x = c["qkv"][:, :N].float()
    if bias is not None:
        x = _bf(x + bias)
    if c["lora_b"] is not None:
        u = c["qkv"][:, N: N + c["lr"]].float()
        x = _bf(x + _bf(u @ c["lora_b"][:, : c["lr"]].float().t()))
    x = x.view(R, Hq + 2 * Hkv, D)
    qk = x[:, : Hq + Hkv]
    cos, sin = c["cos"][c["pos"].long()][:, None, : rot // 2], c["sin"][c["pos"].long()][:, None, : rot // 2]
    a, b = qk[..., : rot // 2], qk[..., rot // 2: rot]
    qk = _bf(torch.cat([a * cos - b * sin, b * cos + a * sin, qk[..., rot:]], -1))
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
@pytest.mark.parametrize("rep", [1, 3, 4, 8])
@pytest.mark.parametrize("rot_of", ["D/2", "3D/4"])
def test_attn_decode_partial_rotary(dev, D, rep, rot_of):
    """the bounds of test_attn_decode_qknorm_every_gqa_ratio (bf16 outputs of an attention over ~13 keys); with and without the q|k|v
    bias and the LoRA delta, which the prologue reads at the same two elements as the rotation"""
    rot = D // 2 if rot_of == "D/2" else 3 * D // 4
    for lora in (False, True):
        c = _decode_case(dev, D, rep, lora, rot, seed=rep)
        for bias in (None, c["bias"]):
            O_, Kg, Vg, anc = _run_decode(c, bias, rot)
            ref, k_new, v_new = _decode_reference(c, bias, rot)
            err = float((O_.float() - ref).abs().max())
            assert err < 2e-2 * float(ref.abs().max()) + 1e-2, (D, rep, rot, lora, bias is not None, err)
            n = c["n_prev"]
            for r in range(c["R"]):
                assert float((Kg[r, n].float().view(c["Hkv"], D) - k_new[r]).abs().max()) <= 1e-2 * float(k_new.abs().max()) + 1e-3
                assert float((Vg[r, n].float().view(c["Hkv"], D) - v_new[r]).abs().max()) <= 1e-2 * float(v_new.abs().max()) + 1e-3
                assert int(anc[r, n]) == r
            # pairing (d, d + D/2) over the whole head moves the result, and the appended key, by more than the tolerance
            ref0, k0, _ = _decode_reference(c, bias, D)
            assert float((ref0 - ref).abs().max()) > 2 * (2e-2 * float(ref.abs().max()) + 1e-2)
            assert float((k0 - k_new).abs().max()) > 2 * (1e-2 * float(k_new.abs().max()) + 1e-3)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("rep", [1, 2, 3, 4, 5, 6, 7, 8])
def test_attn_decode_partial_at_full_width_is_bit_identical_to_span(dev, D, rep):
    for lora in (False, True):
        c = _decode_case(dev, D, rep, lora, D, seed=20 + rep)
        for bias in (None, c["bias"]):
            for end in (None, c["end"]):
                a = _run_decode(c, bias, D, entry="slam_attn_decode_span", end=end)
                b = _run_decode(c, bias, D, entry="slam_attn_decode_partial", end=end)
                for x, y in zip(a, b):
                    assert torch.equal(x, y)


def test_attn_decode_partial_rejects_through_the_c_abi(dev):
    from slam_llm_amd import lib
    c = _decode_case(dev, 64, 1, False, 32)
    _run_decode(c, None, 32, entry="slam_attn_decode_partial")
    for rot in (0, 8, 24, 80):
        with pytest.raises(lib.SlamHipError, match=r"slam_attn_decode_partial: rot_dim .* multiple of 16 in \[16, head_dim\]"):
            _run_decode(c, None, rot, entry="slam_attn_decode_partial")
    w = torch.ones(64, device=dev)
    with pytest.raises(lib.SlamHipError, match="partial rotary"):
        _run_decode(c, None, 32, entry="slam_attn_decode_partial", qk_norm=(w, w, 1e-6))
    _run_decode(c, None, 64, entry="slam_attn_decode_partial", qk_norm=(w, w, 1e-6))


# ------------------------------------------------------------------------------------------------ 3. tiny geometries vs the reference
def _build(case, dev, W=None, **over):
    from slam_llm_amd.model import SlamHipModel
    cfg = case["cfg"]
    W = W if W is not None else phi3_weights(cfg, seed=42, norm_scale=case["norm_scale"])
    return SlamHipModel(dict(cfg, lora_dropout=0.0, **over), dev).load_weights(W), W


def _batch(fx, dev, prefix="batch."):
    return {k[len(prefix):]: torch.from_numpy(fx[k]).to(dev) for k in fx.files if k.startswith(prefix)}


def _rel(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max() / (np.abs(ref).max() + 1e-12))


@pytest.mark.parametrize("name", list(CASES))
def test_forward_matches_reference_fixture(dev, name):
    """loss (1e-2, the tolerance the fixtures' comparison loss is sized against), accuracy, and every logit of every label row and every
    5th other row (golden_util.check_logits) against the reference's slam_model over HF Phi3ForCausalLM"""
    fx = G.load(name)
    case = CASES[name]
    cfg = case["cfg"]
    model, W = _build(case, dev)
    L0 = model.llm.layers[0]
    assert [n for n, _ in L0.qkv.parts] == ["qkv_proj"] and [n for n, _ in L0.gu.parts] == ["gate_up_proj"]
    assert model.llm.rot_dim == cfg["llm_rotary_dim"] < cfg["llm_head_dim"]
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
    other = "loss_with_full_default_rope"
    print(f"{name}: loss {float(outputs.loss.detach()):.6f} fixture {float(fx['loss.0']):.6f} ({other} {float(fx[other]):.6f}) acc {float(acc):.4f}")
    assert abs(float(outputs.loss) - float(fx["loss.0"])) < 1e-2, (float(outputs.loss), float(fx["loss.0"]))
    G.check_logits(outputs.logits, torch.from_numpy(fx["logits_full"]), b["attention_mask"], b["labels"], f"{name} vs fixture")
    assert abs(float(acc) - float(fx["acc.0"])) <= 1.0 / max(1, int((b["labels"][:, 1:] != -100).sum()))


def _three_steps(model, fx, b, name):
    """gradients of the first step and three AdamW steps against the fixture, under the bounds of tests/test_qwen3_gpu.py"""
    from slam_llm_amd.model import SlamAdamW
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
    return 1.0 - worst_grad[0]


@pytest.mark.parametrize("name", list(CASES))
def test_gradients_and_training_steps_match_reference(dev, name):
    """every trainable gradient (cosine floor of the frozen-LLM family, norm within 3 %), the losses of three steps, and the parameters
    after the three AdamW steps (direction of the whole update >= 0.95, elementwise within 2 x the sum of the learning rates: see
    tests/test_qwen3_gpu.py for the reasoning).  The adapter of qkv_proj receives its gradient through the stand-alone adjoint launch."""
    fx = G.load(name)
    model, W = _build(CASES[name], dev)
    model.train()
    assert set(model.state_dict().keys()) == set(trainable_names(W))
    dev_ = _three_steps(model, fx, _batch(fx, dev), name)
    G.drift_check(f"{name} worst gradient deviation", dev_, EXPECT_GRAD_DEV[name])


def test_packed_varlen_path_equals_the_padded_reference(dev):
    """cfg['varlen'] on the right-padded fixture batch: the LLM runs on the packed sequences with per-token rotary positions (forward
    launch and adjoint launch both take them) -- the fixture's bounds hold on every valid token, pad rows come back as zeros"""
    name = "step_phi3_untied"
    fx = G.load(name)
    model, W = _build(CASES[name], dev, varlen=True)
    model.train()
    b = _batch(fx, dev)
    assert not bool(b["attention_mask"].all())
    model.return_logits = True
    outputs, _ = model(**{k: v.clone() for k, v in b.items()})
    valid = b["attention_mask"].bool().cpu()
    got, want = outputs.logits.float().cpu(), torch.from_numpy(fx["logits_full"])
    assert float((got[valid] - want[valid]).abs().max()) < 6e-2 + 2e-2 * float(want[valid].abs().max())
    assert float(got[~valid].abs().max()) == 0.0
    model.return_logits = False
    model.zero_grad()
    _three_steps(model, fx, b, name + " packed")


def test_state_dict_with_separate_projections_is_refused(dev):
    case = CASES["step_phi3_tied"]
    W = O.init_weights(dict(case["cfg"], lora_targets=()), seed=42)
    with pytest.raises(KeyError, match="qkv_proj"):
        _build(case, dev, W)


def test_existing_configs_draw_the_same_random_weights(dev):
    """llm_rotary_dim draws nothing; llm_fused_proj draws each fused group in one call, everything drawn before the first layer stays"""
    from slam_llm_amd.model import SlamHipModel
    cfg = dict(O.make_config(llm_dim=384, llm_heads=6, llm_kv_heads=2, llm_head_dim=64, llm_ffn=512, lora_targets=()), lora_dropout=0.0)
    a = SlamHipModel(dict(cfg), dev)
    b = SlamHipModel(dict(cfg, llm_rotary_dim=32, llm_sliding_window=4096), dev)
    c = SlamHipModel(dict(cfg, llm_fused_proj=True, llm_rotary_dim=32), dev)
    for m in (a, b, c):
        m.init_random(5)
    assert a.llm.rot_dim == 64 and b.llm.rot_dim == 32 and not a.llm.fused_proj and c.llm.fused_proj
    for x, y in zip(a.llm.layers, b.llm.layers):
        for fa, fb in ((x.qkv, y.qkv), (x.o, y.o), (x.gu, y.gu), (x.down, y.down)):
            assert torch.equal(fa.Wext, fb.Wext)
        assert torch.equal(x.ln1, y.ln1) and torch.equal(x.ln2, y.ln2)
    assert torch.equal(a.llm.embed, b.llm.embed) and torch.equal(a.llm.lm_head, b.llm.lm_head) and torch.equal(a.llm.norm_w, b.llm.norm_w)
    assert torch.equal(a.llm.embed, c.llm.embed) and c.llm.layers[0].qkv.Wext.shape == a.llm.layers[0].qkv.Wext.shape


def test_adapter_directory_round_trip_under_the_fused_names(dev, tmp_path):
    from slam_llm_amd.slam_model_hip import read_peft_adapter, save_peft_adapter
    name = "step_phi3_untied"
    fx = G.load(name)
    case = CASES[name]
    model, W = _build(case, dev)
    keys = save_peft_adapter(model, str(tmp_path))
    assert len(keys) == 2 * 4 * case["cfg"]["llm_layers"]
    assert "base_model.model.model.layers.0.self_attn.qkv_proj.lora_A.weight" in keys
    assert "base_model.model.model.layers.1.mlp.gate_up_proj.lora_B.weight" in keys
    lora, state = read_peft_adapter(str(tmp_path))
    assert lora["lora_targets"] == FUSED_FOUR and lora["lora_r"] == 16
    own = model.state_dict()
    assert set(state) == {k for k in own if ".lora_" in k}
    W2 = {k: (torch.zeros_like(v) if ".lora_B." in k else v) for k, v in W.items()}
    other, _ = _build(case, dev, W2)
    other.load_state_dict(state, strict=False)
    other.mark_params_updated()
    b = _batch(fx, dev)
    model.eval(); other.eval()
    la, lb = model(**{k: v.clone() for k, v in b.items()})[0].loss, other(**{k: v.clone() for k, v in b.items()})[0].loss
    assert float(la) == float(lb) and abs(float(la) - float(fx["loss.0"])) < 1e-2


# ------------------------------------------------------------------------------------------------ 4. generate
@pytest.mark.parametrize("pad", GEN_PADS)
@pytest.mark.parametrize("name", list(CASES))
def test_generate_matches_reference_tokens(dev, name, pad):
    """greedy and beam 4 vs the reference's generate (fp32) on the left-padded and the right-padded prompt batch, margin-aware as
    tests/test_qwen3_gpu.py: a greedy row must match up to its first step whose fp32 top-2 margin is below 2 x the measured bf16 noise;
    a beam item either reproduces the reference hypothesis or one whose fp32 score is within the noise.  The beam-4 run is repeated on
    the batch tiled x6 (72 hypotheses > 64): the decode step's GEMM path."""
    C = GENERATE_CASE
    cfg = CASES[name]["cfg"]
    fx = G.load("generate_phi3")
    W = phi3_weights(cfg, seed=42, norm_scale=C["norm_scale"])
    model, _ = _build(CASES[name], dev, W)
    model.eval()
    b = _batch(fx, dev, prefix=f"{name}.{pad}.batch.")
    b.setdefault("audio_mel", torch.from_numpy(fx[f"{name}.left.batch.audio_mel"]).to(dev))
    cpu = {k: v.cpu() for k, v in b.items()}
    assert bool((cpu["attention_mask"][:, -1 if pad == "right" else 0] == 0).any()), "the batch must have padded rows on that side"
    eos, L = int(fx[f"{name}.{pad}.eos"]), C["max_new_tokens"]
    step_fn = RP.rule_step_fn(W, cfg, phi3_embeds(W, cfg, cpu), cpu["attention_mask"], forward=phi3_forward)
    ref_logits = lambda toks: step_fn(toks, None)  # noqa: E731
    embeds, am = model(**{k: v.clone() for k, v in b.items()}, inference_mode=True)
    B, T, d = embeds.shape
    lg0, _ = model.llm.prefill(embeds.reshape(B * T, d), B, T, am, L)
    noise = 3.0 * float((lg0.float().cpu() - ref_logits(torch.zeros((B, 0), dtype=torch.int64))).abs().max())
    compared = 0
    for nb, lp in GEN_RUNS:
        want = torch.from_numpy(fx[gen_key(name, pad, nb, lp)])
        for tile in ((1, 6) if nb > 1 else (1,)):
            bt = {k: v.repeat(tile, *([1] * (v.dim() - 1))) for k, v in b.items()}
            got = model.generate(**bt, max_new_tokens=L, num_beams=nb, length_penalty=lp, eos_token_id=eos, pad_token_id=C["pad"]).cpu()
            assert (B * tile * nb > 64) == (tile > 1)
            got = got[:B]
            n = max(got.shape[1], want.shape[1])
            pad_to = lambda x: torch.cat([x, torch.full((B, n - x.shape[1]), C["pad"], dtype=torch.int64)], 1)  # noqa: E731
            got_p, want_p = pad_to(got), pad_to(want)
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
                    assert torch.equal(got_p[r, :upto], want_p[r, :upto]), (name, pad, tile, r, upto, got[r], want[r], noise)
                    compared += upto
                else:
                    sg, sw = float(lp_got[r] / len_g[r] ** lp), float(lp_want[r] / len_w[r] ** lp)
                    assert sg >= sw - 2 * noise, (name, pad, tile, r, sg, sw, noise, got[r], want[r])
    assert compared > 0
    print(f"generate {name} {pad}: noise {noise:.4f}, token positions compared exactly: {compared}")


def test_generate_refuses_what_longrope_and_the_window_do_not_cover(dev):
    name = "step_phi3_untied"       # original_max_position_embeddings 128, window 256
    fx = G.load("generate_phi3")
    model, _ = _build(CASES[name], dev)
    model.eval()
    b = _batch(fx, dev, prefix=f"{name}.left.batch.")
    T = b["input_ids"].shape[1]
    with pytest.raises(NotImplementedError, match="original_max_position_embeddings=128"):
        model.generate(**b, max_new_tokens=129 - T, num_beams=1, eos_token_id=2, pad_token_id=0)
    model.llm.window = T + 3
    with pytest.raises(NotImplementedError, match="llm_sliding_window"):
        model.generate(**b, max_new_tokens=4, num_beams=1, eos_token_id=2, pad_token_id=0)


# ------------------------------------------------------------------------------------------------ 5. a true width
# Phi-4-mini-like: hidden 3072, 24 q / 8 kv heads of 128 dims of which 96 rotate, ffn 8192, longrope whose attention factor is
# Phi-4-mini's (sqrt(1 + ln 32 / ln 4096) = 1.19); 2 layers and a small vocabulary keep it quick.  The factor lists are not Phi-4-mini's.
PHI4_MINI_LIKE = dict(llm_dim=3072, llm_layers=2, llm_heads=24, llm_kv_heads=8, llm_head_dim=128, llm_rotary_dim=96, llm_ffn=8192,
                      vocab=8192, rope_theta=10000.0, rms_eps=1e-5, tie_embeddings=True, llm_fused_proj=True, llm_qkv_bias=False,
                      llm_qk_norm=False, llm_sliding_window=262144, rope_scaling=longrope(96, original_max=4096, max_pos=131072),
                      lora_targets=FUSED_FOUR, lora_r=16, lora_alpha=16)


def test_true_width_against_restatement(dev):
    """eval logits, loss and the LoRA gradients against the fp32 restatement run on the device over the HIP path's own inputs_embeds;
    prefill of T - 1 positions + one decode step against the every-row forward's last two rows.  Bounds: the bf16 logit bound of
    golden_util.check_logits (6e-2 + 2e-2 max|ref|) and the frozen-LLM family's gradient floor."""
    from slam_llm_amd.model import SlamHipModel
    cfg = O.make_config(**PHI4_MINI_LIKE)
    W = phi3_weights(cfg, seed=7)
    model = SlamHipModel(dict(cfg, lora_dropout=0.0), dev).load_weights(W)
    audio = O.synth_audio(2, 2.0, seed=99)
    batch = O.synth_batch(cfg, audio, prompt_len=8, answer_lens=(12, 5), seed=5, left_pad=True, pad_to_30s=False)
    b = {k: v.to(dev) for k, v in batch.items()}
    model.eval()
    embeds, am = model(**{k: v.clone() for k, v in b.items() if k != "labels"}, inference_mode=True)
    Wd = {k: v.to(dev) for k, v in W.items() if k.startswith(P)}
    names = [n for n in Wd if ".lora_" in n]
    for n in names:
        Wd[n].requires_grad_(True)
    loss_ref, logits_ref = phi3_forward(Wd, cfg, embeds.float().detach(), b["attention_mask"], b["labels"])
    loss_ref.backward()
    model.train()
    model.return_logits = True
    outputs, _ = model(**{k: v.clone() for k, v in b.items()})
    stats = G.check_logits(outputs.logits, logits_ref.detach(), b["attention_mask"], b["labels"], "phi-4-mini-like width")
    outputs.loss.backward()
    assert abs(float(outputs.loss) - float(loss_ref)) < 2e-2 + 1e-2 * float(loss_ref)
    cos = {n: G.cosine(model.store.params[n].grad.float().cpu().numpy(), Wd[n].grad.float().cpu().numpy()) for n in names}
    worst = min(cos, key=cos.get)
    for n, cs in cos.items():
        G.floor_check(cs, G.FLOORS["frozen"], f"phi-4-mini-like grad {n}")
    model.eval()
    rows = torch.nonzero(b["attention_mask"].all(1)).flatten()
    assert rows.numel() >= 1
    e = embeds[rows]
    B, T, d = e.shape
    lg0, cache = model.llm.prefill(e[:, :-1].reshape(B * (T - 1), d).contiguous(), B, T - 1, am[rows][:, :-1], 2)
    lg1 = model.llm.decode_step(b["input_ids"][rows, -1], cache)
    ref_prev, ref_last = logits_ref[rows, -2].detach(), logits_ref[rows, -1].detach()
    bound = 6e-2 + 2e-2 * float(ref_last.abs().max())
    pf, df = float((lg0.float() - ref_prev).abs().max()) / bound, float((lg1.float() - ref_last).abs().max()) / bound
    print(f"phi-4-mini-like measured: loss {float(outputs.loss):.5f} ref {float(loss_ref):.5f}, worst grad 1-cos {1 - cos[worst]:.3e} ({worst}), "
          f"logit frac {stats['max_err'] / stats['bound']:.4f}, prefill frac {pf:.4f}, decode frac {df:.4f}")
    assert pf <= 1.0 and df <= 1.0, (pf, df)


# ------------------------------------------------------------------------------------------------ graphs, recipe entry
def test_graphed_train_step_is_bit_identical_on_phi3(dev):
    from slam_llm_amd.model import SlamAdamW
    from slam_llm_amd.train import GraphedTrainStep, lr_lambda, train_step
    name = "step_phi3_untied"
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


@pytest.mark.parametrize("use_peft", [True, False])
def test_recipe_invocation_trains_through_model_factory(dev, use_peft):
    """the recipe entry with the Phi3 keys at tiny widths through arch_overrides (what the config.json of an llm_path directory sets:
    tests/test_phi3_host.py), the peft_config naming the fused Linears, and `use_peft=false freeze_llm=true`: one step trains"""
    from slam_llm_amd.model import SlamAdamW
    from slam_llm_amd.slam_model_hip import model_factory
    peft = dict(peft_method="lora", r=8, lora_alpha=16, lora_dropout=0.0, target_modules=["qkv_proj", "o_proj", "gate_up_proj", "down_proj"])
    tc = dict(use_peft=use_peft, peft_config=peft, freeze_llm=True, freeze_encoder=True, seed=3)
    over = dict(enc_dim=128, enc_heads=2, enc_layers=2, n_mels=128, llm_dim=256, llm_layers=2, llm_heads=4, llm_kv_heads=2, llm_head_dim=64,
                llm_ffn=512, vocab=1024, tie_embeddings=True, llm_fused_proj=True, llm_rotary_dim=48, llm_sliding_window=2047,
                rope_scaling=longrope(48))
    mc = dict(encoder_name="whisper", encoder_path="large-v3", encoder_projector="linear", llm_name="tinyllama-1.1b", random_init=True,
              arch_overrides=over)
    model, _ = model_factory(tc, mc)
    cfg = model.cfg
    assert cfg["llm_fused_proj"] and cfg["llm_rotary_dim"] == 48 and model.llm.rot_dim == 48 and model.llm.window == 2047
    names = [n for n in model.state_dict() if ".lora_A." in n]
    assert bool(names) == use_peft and all(("qkv_proj" in n) or ("o_proj" in n) or ("gate_up_proj" in n) or ("down_proj" in n) for n in names)
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

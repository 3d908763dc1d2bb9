"""GPU: Qwen2 / Qwen2.5 LLMs on the HIP path -- q/k/v bias in the GEMM epilogue and in the decode attention kernel, GQA ratios 1..8 in
decode, tied embeddings; the tiny geometries against the reference's fixtures (tools/make_golden_qwen2.py) and true widths against
the fp32 restatement of tests/qwen2_cases.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import slam_oracle as O
from tests import golden_util as G
from tests.qwen2_cases import CASES, GEN_RUNS, GENERATE_CASE, P, gen_key, qwen2_forward, qwen2_weights

pytestmark = pytest.mark.gpu


def _bf(t):
    return t.to(torch.bfloat16).float()


# ------------------------------------------------------------------------------------------------ GEMM epilogue bias
@pytest.mark.parametrize("N,K", [(1152, 896), (2048, 1536), (4608, 3584)])
def test_gemm_bias_at_qwen_qkv_shapes(dev, N, K):
    """every plan the auto rule picks for the q|k|v product (M = 1 .. 64 tiles, mid-M split-K, the C3-size row count) adds the bias
    exactly once: a bias of unit scale counted twice or not at all is ~30x the bf16 bound used here"""
    from slam_llm_amd import ops
    g = torch.Generator(device=dev).manual_seed(3)
    W = (torch.randn(N, K, generator=g, device=dev) * K ** -0.5).to(torch.bfloat16)
    bias = _bf(torch.randn(N, generator=g, device=dev))
    for M in (1, 5, 16, 33, 64, 672, 2048, 11780):
        x = torch.randn(M, K, generator=g, device=dev).to(torch.bfloat16)
        got = ops.gemm_nt(x, W, bias=bias).float()
        ref = x.float() @ W.float().t() + bias
        err = float((got - ref).abs().max())
        assert err <= 2e-2 * float(ref.abs().max()), (M, N, K, err, ops.gemm_kernel_name(M, N, K))


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
    cos, sin = [t.to(dev) for t in O.rope_tables(Tp + G_, D, 1e6)]
    cos, sin = cos[:, : D // 2].contiguous(), sin[:, : D // 2].contiguous()
    start = torch.tensor([0, 3], dtype=torch.int32, device=dev)
    pos = torch.tensor([Tp + n_prev, Tp + n_prev, Tp - 3 + n_prev, Tp - 3 + n_prev], dtype=torch.int32, device=dev)
    Kp = torch.randn(B, Tp, Hkv * D, generator=g, device=dev).to(torch.bfloat16)
    Vp = torch.randn(B, Tp, Hkv * D, generator=g, device=dev).to(torch.bfloat16)
    Kg = torch.randn(R, G_, Hkv * D, generator=g, device=dev).to(torch.bfloat16)
    Vg = torch.randn(R, G_, Hkv * D, generator=g, device=dev).to(torch.bfloat16)
    anc = torch.tensor([[0, 1, 1, 0, 0, 0], [1, 0, 1, 1, 1, 1], [2, 2, 3, 2, 2, 2], [3, 3, 3, 3, 3, 3]], dtype=torch.int32, device=dev)
    return dict(qkv=qkv, lora_b=lora_b, lr=lr, bias=bias, cos=cos, sin=sin, start=start, pos=pos, Kp=Kp, Vp=Vp, Kg=Kg, Vg=Vg, anc=anc,
                Hq=Hq, Hkv=Hkv, D=D, B=B, beams=beams, R=R, Tp=Tp, G=G_, n_prev=n_prev, N=N)


def _run_decode(c, bias, entry=None):
    from slam_llm_amd import ops
    Kg, Vg, anc = c["Kg"].clone(), c["Vg"].clone(), c["anc"].clone()
    O_ = torch.empty(c["R"], c["Hq"] * c["D"], dtype=torch.bfloat16, device=c["qkv"].device)
    args = (c["qkv"], c["lora_b"], c["lr"], c["cos"], c["sin"], c["pos"], c["Kp"], c["Vp"], c["start"], Kg, Vg, anc, None, c["n_prev"],
            c["beams"], c["Hq"], c["Hkv"], c["D"], c["D"] ** -0.5, O_)
    if entry is None:
        ops.attn_decode(*args, qkv_bias=bias)
    else:       # the new entry point with a NULL bias pointer
        from slam_llm_amd import lib
        q, lb, p = c["qkv"], c["lora_b"], ops._p
        lib.call("slam_attn_decode_bias", p(q), q.stride(0), p(lb), lb.stride(0) if lb is not None else 0, c["lr"], p(c["cos"]),
                 p(c["sin"]), p(c["pos"]), p(c["Kp"]), p(c["Vp"]), p(c["start"]), p(Kg), p(Vg), p(anc), None, c["n_prev"], p(O_),
                 O_.stride(0), c["R"], c["beams"], c["Tp"], c["G"], c["Hq"], c["Hkv"], c["D"], c["D"] ** -0.5, None, ops._s())
    torch.cuda.synchronize()
    return O_, Kg, Vg, anc


def _decode_reference(c, bias):
    D, Hq, Hkv, N, R, n = c["D"], c["Hq"], c["Hkv"], c["N"], c["R"], c["n_prev"]
    x = c["qkv"][:, :N].float()
    if bias is not None:
        x = _bf(x + bias)
    if c["lora_b"] is not None:
        u = c["qkv"][:, N: N + c["lr"]].float()
        x = _bf(x + _bf(u @ c["lora_b"][:, : c["lr"]].float().t()))
    x = x.view(R, Hq + 2 * Hkv, D)
    cos, sin = c["cos"][c["pos"].long()][:, None], c["sin"][c["pos"].long()][:, None]
    qk = x[:, : Hq + Hkv]
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
def test_attn_decode_bias_every_gqa_ratio(dev, D, rep):
    for lora in (False, True):
        c = _decode_case(dev, D, rep, lora, seed=rep)
        for bias in (None, c["bias"]):
            O_, Kg, Vg, anc = _run_decode(c, bias)
            ref, k_new, v_new = _decode_reference(c, bias)
            err = float((O_.float() - ref).abs().max())
            assert err < 2e-2 * float(ref.abs().max()) + 1e-2, (D, rep, lora, bias is not None, err)
            n = c["n_prev"]
            for r in range(c["R"]):
                assert float((Kg[r, n].float().view(c["Hkv"], D) - k_new[r]).abs().max()) <= 1e-2 * float(k_new.abs().max()) + 1e-3
                assert float((Vg[r, n].float().view(c["Hkv"], D) - v_new[r]).abs().max()) <= 1e-2 * float(v_new.abs().max()) + 1e-3
                assert int(anc[r, n]) == r
            if bias is not None:    # the bias moves the result by more than the tolerance
                ref0, _, _ = _decode_reference(c, None)
                assert float((ref0 - ref).abs().max()) > 2 * (2e-2 * float(ref.abs().max()) + 1e-2)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("rep", [1, 2, 4, 8])
def test_attn_decode_bias_null_is_bit_identical_to_attn_decode(dev, D, rep):
    for lora in (False, True):
        c = _decode_case(dev, D, rep, lora, seed=10 + rep)
        a = _run_decode(c, None)
        b = _run_decode(c, None, entry="bias")
        for x, y in zip(a, b):
            assert torch.equal(x, y)


def test_attn_decode_rejects_ratios_above_8(dev):
    from slam_llm_amd import lib
    c = _decode_case(dev, 64, 1, False)
    with pytest.raises(lib.SlamHipError, match=r"Hq/Hkv must be in \[1, 8\]"):
        from slam_llm_amd import ops
        ops.attn_decode(c["qkv"], None, 0, c["cos"], c["sin"], c["pos"], c["Kp"], c["Vp"], c["start"], c["Kg"], c["Vg"], c["anc"], None,
                        c["n_prev"], c["beams"], 9 * c["Hkv"], c["Hkv"], 64, 0.125, torch.empty(4, 9 * 2 * 64, dtype=torch.bfloat16,
                                                                                             device=dev), qkv_bias=None)


# ------------------------------------------------------------------------------------------------ tiny geometries vs the reference
def _build(cfg, dev, W=None):
    from slam_llm_amd.model import SlamHipModel
    W = W if W is not None else qwen2_weights(cfg, seed=42)
    return SlamHipModel(dict(cfg, lora_dropout=0.0), dev).load_weights(W), W


def _batch(fx, dev, prefix="batch."):
    return {k[len(prefix):]: torch.from_numpy(fx[k]).to(dev) for k in fx.files if k.startswith(prefix)}


def _rel(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max() / (np.abs(ref).max() + 1e-12))


@pytest.mark.parametrize("name", list(CASES))
def test_forward_matches_reference_fixture(dev, name):
    fx = G.load(name)
    cfg = CASES[name]["cfg"]
    model, W = _build(cfg, dev)
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
    assert abs(float(outputs.loss) - float(fx["loss.0"])) < 1e-2, (float(outputs.loss), float(fx["loss.0"]))
    Bn, T, V = [int(x) for x in fx["logits.shape"]]
    lg = outputs.logits.float().cpu().numpy()
    valid_rows = b["attention_mask"].cpu().numpy().astype(bool).reshape(-1)
    stride = int(fx["logits.__stride"])
    keep = valid_rows[np.arange(0, Bn * T * V, stride) // V]
    gl, al = fx["logits"][keep], lg.reshape(-1)[::stride][keep]
    assert np.abs(gl - al).max() < 6e-2 + 2e-2 * np.abs(gl).max(), np.abs(gl - al).max()
    assert abs(float(acc) - float(fx["acc.0"])) <= 1.0 / max(1, int((b["labels"][:, 1:] != -100).sum()))


@pytest.mark.parametrize("name", list(CASES))
def test_gradients_and_training_steps_match_reference(dev, name):
    from slam_llm_amd.model import SlamAdamW
    fx = G.load(name)
    cfg = CASES[name]["cfg"]
    model, W = _build(cfg, dev)
    model.train()
    b = _batch(fx, dev)
    opt = SlamAdamW(model, lr=1e-2, weight_decay=0.01)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda s: O.lr_lambda(s, 2, 10))
    losses = []
    for step in range(3):
        outputs, acc = model(**{k: v.clone() for k, v in b.items()})
        outputs.loss.backward()
        if step == 0:
            for n, p in model.store.params.items():
                g = p.grad.float().cpu().numpy()
                gold, mine = G.sub(fx, "grad." + n, g)
                G.floor_check(G.cosine(gold, mine), G.FLOORS["frozen"], f"grad {n}")
                gn = float(fx["grad." + n + ".__norm"])
                assert abs(float(np.sqrt((g.astype(np.float64) ** 2).sum())) - gn) < 3e-2 * gn + 1e-7, n
        opt.step(); sched.step(); opt.zero_grad()
        losses.append(float(outputs.loss))
    assert abs(losses[0] - losses[1]) < 1e-6
    for s in range(3):
        assert abs(losses[s] - float(fx[f"loss.{s}"])) < 3e-2, (s, losses[s], float(fx[f"loss.{s}"]))
    assert set(model.state_dict().keys()) == set(O.trainable_names(W))


def test_tied_state_dict_must_hold_the_embedding(dev):
    cfg = CASES["step_qwen2_tied"]["cfg"]
    W = qwen2_weights(cfg, seed=42)
    W[P + "lm_head.weight"] = W[P + "model.embed_tokens.weight"].clone()
    _build(cfg, dev, W)        # an explicit copy of the embedding is accepted
    W[P + "lm_head.weight"] = W[P + "lm_head.weight"] * 2
    with pytest.raises(ValueError, match="tie_embeddings"):
        _build(cfg, dev, W)


def test_pure_bf16_route_rounds_the_bias(dev):
    cfg = CASES["step_qwen2_untied"]["cfg"]
    W = qwen2_weights(cfg, seed=42)
    for k in list(W):
        if k.endswith("q_proj.bias"):
            W[k] = W[k] + 1e-3        # not bf16-representable
    model, _ = _build(cfg, dev, W)
    bias = model.llm.layers[0].bias.clone()
    model.to(torch.bfloat16)
    assert model.llm.layers[0].bias.dtype == torch.float32
    assert torch.equal(model.llm.layers[0].bias, bias.to(torch.bfloat16).float()) and not torch.equal(bias, model.llm.layers[0].bias)


# ------------------------------------------------------------------------------------------------ generate
def _ref_logits_fn(W, cfg, cpu):
    from tests.qwen2_cases import qwen2_embeds
    embeds_ref = qwen2_embeds(W, cfg, cpu)
    emb_w = W[P + "model.embed_tokens.weight"]
    mask = cpu["attention_mask"].long()

    def ref_logits(toks):
        x = torch.cat([embeds_ref, F.embedding(toks, emb_w)], dim=1)
        m = torch.cat([mask, torch.ones_like(toks)], dim=1)
        return qwen2_forward(W, cfg, x, m, None, position_ids=O.generate_position_ids(m))[1][:, -1, :]
    return ref_logits


@pytest.mark.parametrize("name", list(CASES))
def test_generate_matches_reference_tokens(dev, name):
    """greedy and beam 4 vs the reference's generate (fp32), margin-aware as tests/test_model_gpu.py's repetition-penalty test:
    a greedy row must match up to its first step whose fp32 top-2 margin is below 2 x the measured bf16 noise; a beam item either
    reproduces the reference hypothesis or one whose fp32 score is within the noise.  The beam-4 run is repeated on the batch tiled
    x6 (72 hypotheses > 64): the decode step's GEMM path, where the q|k|v bias is added only by the attention kernel."""
    C = GENERATE_CASE
    cfg = CASES[name]["cfg"]
    fx = G.load("generate_qwen2")
    W = qwen2_weights(cfg, seed=42, norm_scale=C["norm_scale"])
    model, _ = _build(cfg, dev, W)
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
    "qwen2.5-7b": dict(lora_targets=("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj"), lora_r=16,
                       lora_alpha=16),
    "qwen2.5-0.5b": dict(lora_targets=("q_proj", "v_proj"), lora_r=8, lora_alpha=32),
}
# 1 - cosine measured on MI355X for the LoRA gradients (worst tensor) and |logit err| / bound: the floors sit at >= 2x these
TRUE_WIDTH_FLOOR = {"qwen2.5-7b": 0.995, "qwen2.5-0.5b": 0.995}


@pytest.mark.parametrize("preset", list(TRUE_WIDTH))
def test_true_width_against_restatement(dev, preset):
    """2 LLM layers at the checkpoint's true widths (vocab 152064 untied / 151936 tied), a small Whisper encoder, three 30 s clips:
    eval logits (golden_util.check_logits), LoRA gradient cosines against the fp32 restatement run on the device over the HIP path's
    own inputs_embeds, and prefill + one decode step against the every-row forward"""
    from slam_llm_amd.model import PRESETS, SlamHipModel
    cfg = O.make_config(**{k: v for k, v in PRESETS[preset].items()}, **TRUE_WIDTH[preset])
    cfg.update(llm_layers=2)
    W = qwen2_weights(cfg, seed=7)
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
    loss_ref, logits_ref = qwen2_forward(Wd, cfg, x, b["attention_mask"], b["labels"])
    loss_ref.backward()
    model.train()
    model.return_logits = True
    outputs, _ = model(**{k: v.clone() for k, v in b.items()})
    stats = G.check_logits(outputs.logits, logits_ref.detach(), b["attention_mask"], b["labels"], f"{preset} true width")
    outputs.loss.backward()
    assert abs(float(outputs.loss) - float(loss_ref)) < 2e-2 + 1e-2 * float(loss_ref)
    for n in names:
        G.floor_check(G.cosine(model.store.params[n].grad.float().cpu().numpy(), Wd[n].grad.float().cpu().numpy()), TRUE_WIDTH_FLOOR[preset],
                      f"{preset} grad {n}")
    # prefill of the first T-1 positions + one decode step == the every-row forward's logits at the last two positions (bf16 tolerance),
    # on the rows without padding (this collator pads on the right)
    model.eval()
    rows = torch.nonzero(b["attention_mask"].all(1)).flatten()
    assert rows.numel() >= 1
    e = embeds[rows]
    B, T, d = e.shape
    lg0, cache = model.llm.prefill(e[:, :-1].reshape(B * (T - 1), d).contiguous(), B, T - 1, am[rows][:, :-1], 2)
    lg1 = model.llm.decode_step(b["input_ids"][rows, -1], cache)
    ref_prev, ref_last = logits_ref[rows, -2].detach(), logits_ref[rows, -1].detach()
    bound = 6e-2 + 2e-2 * float(ref_last.abs().max())
    err0, err1 = float((lg0.float() - ref_prev).abs().max()), float((lg1.float() - ref_last).abs().max())
    assert err0 <= bound and err1 <= bound, (err0, err1, bound)
    stats.update(prefill_err=err0, decode_err=err1)
    print(f"{preset}: {stats}")


# ------------------------------------------------------------------------------------------------ graphs
def test_graphed_train_step_is_bit_identical_on_qwen2(dev):
    from slam_llm_amd.model import SlamAdamW
    from slam_llm_amd.train import GraphedTrainStep, lr_lambda, train_step
    name = "step_qwen2_tied"
    fx = G.load(name)
    cfg = CASES[name]["cfg"]
    runs = []
    for graphed in (False, True):
        model, _ = _build(cfg, dev)
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
    """`encoder_name=whisper llm_name=Qwen2.5-7B-Instruct` with the aispeech peft_config, and `use_peft=false freeze_llm=true`,
    at tiny widths through arch_overrides: the preset's bias / tie / theta survive, and one step trains"""
    from slam_llm_amd.model import SlamAdamW
    from slam_llm_amd.slam_model_hip import model_factory
    peft = dict(peft_method="lora", r=8, lora_alpha=16, lora_dropout=0.0,
                target_modules=["q_proj", "k_proj", "v_proj", "o_proj", "up_proj", "gate_proj", "down_proj"])
    tc = dict(use_peft=use_peft, peft_config=peft, freeze_llm=True, freeze_encoder=True, seed=3)
    over = dict(enc_dim=128, enc_heads=2, enc_layers=2, n_mels=128, llm_dim=448, llm_layers=2, llm_heads=7, llm_kv_heads=1,
                llm_head_dim=64, llm_ffn=512, vocab=1024)
    mc = dict(encoder_name="whisper", encoder_path="large-v3", encoder_projector="linear", llm_name="Qwen2.5-7B-Instruct",
              random_init=True, arch_overrides=over)
    model, _ = model_factory(tc, mc)
    cfg = model.cfg
    assert cfg["llm_qkv_bias"] and cfg["rope_theta"] == 1e6 and not cfg["tie_embeddings"]
    assert model.llm.layers[0].bias is not None and bool(model.llm.layers[0].bias.abs().sum() > 0)
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

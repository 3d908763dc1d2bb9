"""GPU: generate() on right-padded prompt batches (MultiTaskDataset.collator in inference mode).

  a/b  the decode attention kernel over a prompt SPAN per item (slam_attn_decode_span) against a torch fp32 reference, and its null-end
       form bit for bit against the three older entry points;
  c/d  SlamHipModel.generate on tests/golden/generate_rightpad.npz: the reference's own tokens, and the KV-cache decode logits along the
       reference's greedy tokens against the fp32 restatement of the rule (tests/rightpad_cases.py);
  e    generate_right_pad_fix: every row as if alone and unpadded; no change on a left-padded batch;
  f    Qwen2 (q|k|v bias) and Qwen3 (per-head q/k norm) on a right-padded batch;
  g    the dataset plugin's own right-padded inference batch (batcher.make_sample / batcher.collate) decodes."""
import pytest
import torch
import torch.nn.functional as F

from oracle import slam_oracle as O
from oracle.make_golden_cases import GENERATE_CASE as C
from tests import golden_util as G
from tests import rightpad_cases as RP
from tests.test_oracle_golden import generate_case_weights

pytestmark = pytest.mark.gpu

BIG = 1.0e4     # what the prompt slots outside a span hold: a kernel that reads one fails by orders of magnitude, not by a rounding


def _bf(t):
    return t.to(torch.bfloat16).float()


def _rnd(shape, dev, seed, std=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * std).to(torch.bfloat16).to(dev)


# ------------------------------------------------------------------------------------------------ a / b: the kernel
def _kernel_case(dev, D, Hq, Hkv, lora, Tp, n, spans, B=2, beams=2, G_=6):
    """spans: [(start, end)] per item.  Prompt slots outside the span hold BIG in K and V."""
    from slam_llm_amd.host_tables import rope_tables
    R, HD, NQ = B * beams, Hkv * D, (Hq + 2 * Hkv) * D
    ld = NQ + (lora + 7) // 8 * 8
    c = dict(D=D, Hq=Hq, Hkv=Hkv, lora=lora, Tp=Tp, n=n, B=B, beams=beams, G=G_, R=R, NQ=NQ)
    c["qkv"] = _rnd((R, ld), dev, 6)
    c["lora_b"] = _rnd((NQ, 16), dev, 12, std=0.3) if lora else None
    Kp, Vp = _rnd((B, Tp, HD), dev, 7), _rnd((B, Tp, HD), dev, 8)
    for b, (s, e) in enumerate(spans):
        for t in (Kp, Vp):
            t[b, :s] = BIG
            t[b, e:] = BIG
    c["Kp"], c["Vp"] = Kp, Vp
    c["Kg"], c["Vg"] = _rnd((R, G_, HD), dev, 9), _rnd((R, G_, HD), dev, 10)
    c["start"] = torch.tensor([s for s, _ in spans], dtype=torch.int32, device=dev)
    c["end"] = torch.tensor([e for _, e in spans], dtype=torch.int32, device=dev)
    g = torch.Generator().manual_seed(11)
    c["anc"] = torch.stack([torch.randint(0, beams, (G_,), generator=g) + (r // beams) * beams for r in range(R)]).to(torch.int32).to(dev)
    c["pos"] = torch.tensor([spans[r // beams][1] - spans[r // beams][0] + n for r in range(R)], dtype=torch.int32, device=dev)
    cos, sin = rope_tables(Tp + G_, D, 10000.0)
    c["cos"], c["sin"] = cos.to(dev), sin.to(dev)
    c["bias"] = _bf(torch.randn(NQ, generator=torch.Generator().manual_seed(13))).to(dev)
    gw = torch.Generator().manual_seed(14)
    c["wq"], c["wk"] = (1 + 0.3 * torch.randn(D, generator=gw)).to(dev), (1 + 0.3 * torch.randn(D, generator=gw)).to(dev)
    return c


def _kernel_reference(c):
    """fp32, on the device: the new token as tests/test_ops_gpu.py::test_decode_attention_fused builds it (LoRA delta, RoPE, one bf16
    rounding each), attention over [the item's span of the prompt | generated slots through the ancestor table | the new token]"""
    D, Hq, Hkv, R, NQ, n, lora, beams = c["D"], c["Hq"], c["Hkv"], c["R"], c["NQ"], c["n"], c["lora"], c["beams"]
    y = c["qkv"][:, :NQ].float()
    if lora:
        y = _bf(y + _bf(c["qkv"][:, NQ:NQ + lora].float() @ c["lora_b"][:, :lora].float().T))
    pos = c["pos"].long()

    def rope(x):
        cs = torch.cat([c["cos"][pos], c["cos"][pos]], -1)[:, None, :].float()
        sn = torch.cat([c["sin"][pos], c["sin"][pos]], -1)[:, None, :].float()
        return _bf(x * cs + torch.cat([-x[..., D // 2:], x[..., : D // 2]], -1) * sn)

    qf = rope(y[:, : Hq * D].view(R, Hq, D))
    kf = rope(y[:, Hq * D:(Hq + Hkv) * D].view(R, Hkv, D))
    vf = y[:, (Hq + Hkv) * D:].view(R, Hkv, D)
    ref = torch.empty(R, Hq, D, device=y.device)
    rep = Hq // Hkv
    j = torch.arange(n, device=y.device)
    for r in range(R):
        it = r // beams
        s, e = int(c["start"][it]), int(c["end"][it])
        rows = c["anc"][r, :n].long()
        Kh = torch.cat([c["Kp"][it, s:e].float(), c["Kg"][rows, j].float()]).view(-1, Hkv, D)
        Vh = torch.cat([c["Vp"][it, s:e].float(), c["Vg"][rows, j].float()]).view(-1, Hkv, D)
        Kh = torch.cat([Kh, kf[r:r + 1]]).repeat_interleave(rep, 1)
        Vh = torch.cat([Vh, vf[r:r + 1]]).repeat_interleave(rep, 1)
        att = torch.softmax(torch.einsum("hd,lhd->hl", qf[r], Kh) * D ** -0.5, -1)
        ref[r] = torch.einsum("hl,lhd->hd", att, Vh)
    return ref, kf, vf


def _close(got, ref, atol, rtol, what):
    err = (got.float() - ref.float()).abs()
    bad = err > atol + rtol * ref.float().abs()
    assert not bool(bad.any()), f"{what}: {int(bad.sum())}/{bad.numel()} out of tolerance, max err {float(err.max()):.4e}"


@pytest.mark.parametrize("Tp", [70, 600])
@pytest.mark.parametrize("lora", [0, 12])
@pytest.mark.parametrize("D,Hq,Hkv", [(64, 4, 4), (64, 7, 1), (128, 8, 2)])
def test_attn_decode_span_matches_fp32_reference(dev, D, Hq, Hkv, lora, Tp):
    """one decode step through slam_attn_decode_span (ops.attn_decode(..., prompt_end=)) against the torch fp32 reference of
    test_decode_attention_fused, same tolerances (atol 2e-2, rtol 1e-2; the appended K / V within one bf16 ulp).  B = 2, beams = 2,
    0 and 3 generated tokens already cached; spans: right padding on one item, on the other, and an item with ONE prompt key.  At
    Tp = 600 a span crosses one sweep of the workgroup's key groups (512 keys at D = 64, 256 at D = 128), at 70 it sits inside one.
    The slots outside a span hold 1e4."""
    from slam_llm_amd import ops
    for n in (0, 3):
        for spans in ([(0, Tp), (5, Tp - 9)], [(0, Tp - 9), (5, Tp)], [(3, 4), (0, Tp)]):
            c = _kernel_case(dev, D, Hq, Hkv, lora, Tp, n, spans)
            Kg, Vg, anc = c["Kg"].clone(), c["Vg"].clone(), c["anc"].clone()
            out = torch.empty((c["R"], Hq * D), dtype=torch.bfloat16, device=dev)
            ops.attn_decode(c["qkv"], c["lora_b"], lora, c["cos"], c["sin"], c["pos"], c["Kp"], c["Vp"], c["start"], Kg, Vg, anc, None, n,
                            c["beams"], Hq, Hkv, D, D ** -0.5, out, prompt_end=c["end"])
            torch.cuda.synchronize()
            ref, kf, vf = _kernel_reference(c)
            what = f"D={D} Hq={Hq} Hkv={Hkv} lora={lora} Tp={Tp} n={n} spans={spans}"
            _close(Kg[:, n].view(c["R"], Hkv, D), kf, 1e-6, 2 ** -7, "K append " + what)
            _close(Vg[:, n].view(c["R"], Hkv, D), vf, 1e-6, 2 ** -7, "V append " + what)
            keep = torch.ones(c["G"], dtype=torch.bool)
            keep[n] = False
            assert torch.equal(Kg[:, keep], c["Kg"][:, keep]) and torch.equal(Vg[:, keep], c["Vg"][:, keep]), "other slots untouched"
            assert torch.equal(anc[:, n].cpu(), torch.arange(c["R"], dtype=torch.int32)) and torch.equal(anc[:, keep], c["anc"][:, keep])
            assert float(ref.abs().max()) < 10.0     # (the reference itself saw no slot outside a span)
            _close(out.view(c["R"], Hq, D), ref, 2e-2, 1e-2, "decode attention " + what)


def _run_entry(c, bias, qk_norm, span_raw):
    """span_raw: slam_attn_decode_span itself with a NULL prompt_end; else ops.attn_decode without an end, which takes the plain entry,
    slam_attn_decode_bias or slam_attn_decode_qknorm depending on what is set"""
    from slam_llm_amd import lib, ops
    Kg, Vg, anc = c["Kg"].clone(), c["Vg"].clone(), c["anc"].clone()
    out = torch.empty(c["R"], c["Hq"] * c["D"], dtype=torch.bfloat16, device=c["qkv"].device)
    if not span_raw:
        ops.attn_decode(c["qkv"], c["lora_b"], c["lora"], c["cos"], c["sin"], c["pos"], c["Kp"], c["Vp"], c["start"], Kg, Vg, anc, None,
                        c["n"], c["beams"], c["Hq"], c["Hkv"], c["D"], c["D"] ** -0.5, out, qkv_bias=bias, qk_norm=qk_norm)
    else:
        q, lb, p = c["qkv"], c["lora_b"], ops._p
        wq, wk, eps = qk_norm if qk_norm is not None else (None, None, 0.0)
        lib.call("slam_attn_decode_span", p(q), q.stride(0), p(lb), lb.stride(0) if lb is not None else 0, c["lora"], p(c["cos"]),
                 p(c["sin"]), p(c["pos"]), p(c["Kp"]), p(c["Vp"]), p(c["start"]), p(Kg), p(Vg), p(anc), None, c["n"], p(out),
                 out.stride(0), c["R"], c["beams"], c["Tp"], c["G"], c["Hq"], c["Hkv"], c["D"], c["D"] ** -0.5, p(bias), p(wq), p(wk), eps,
                 None, ops._s())
    torch.cuda.synchronize()
    return out, Kg, Vg, anc


@pytest.mark.parametrize("D,Hq,Hkv", [(64, 7, 1), (128, 8, 2)])
def test_attn_decode_span_null_end_is_bit_identical_to_the_older_entry_points(dev, D, Hq, Hkv):
    """slam_attn_decode_span(prompt_end = NULL) against slam_attn_decode (no bias, no norm), slam_attn_decode_bias (bias) and
    slam_attn_decode_qknorm (norm, with and without bias): output, appended K / V and the ancestor write, bit for bit"""
    for lora in (0, 12):
        c = _kernel_case(dev, D, Hq, Hkv, lora, 70, 3, [(0, 70), (5, 70)])     # left padding: what the older entries can express
        for bias in (None, c["bias"]):
            for qk in (None, (c["wq"], c["wk"], 1e-6)):
                a = _run_entry(c, bias, qk, span_raw=False)
                b = _run_entry(c, bias, qk, span_raw=True)
                for x, y in zip(a, b):
                    assert torch.equal(x, y), (D, Hq, Hkv, lora, bias is not None, qk is not None)
                assert bool(torch.isfinite(a[0].float()).all())


# ------------------------------------------------------------------------------------------------ c / d / e: the model
def _to(batch, dev):
    return {k: v.to(dev) for k, v in batch.items()}


def _fixture_batch(fx):
    return {k[len("batch."):]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("batch.")}


def _setup(dev, scale, fixture="generate_rightpad", **cfg_extra):
    from slam_llm_amd.model import SlamHipModel
    fx = G.load(fixture)
    W = generate_case_weights(scale)
    model = SlamHipModel(dict(C["cfg"], lora_dropout=0.0, **cfg_extra), dev).load_weights(W)
    model.eval()
    return fx, W, model, _fixture_batch(fx)


# runs whose reference decision sits inside the bf16 logit noise (measured, see the test's docstring): (scale, beams, length_penalty, pad)
MARGIN_RUNS = {(5.0, 4, 1.0, 0)}


@pytest.mark.parametrize("nb,lp,pad", RP.RUNS)
@pytest.mark.parametrize("scale", [24.0, 5.0])
def test_generate_right_padded_matches_reference_tokens(dev, scale, nb, lp, pad):
    """SlamHipModel.generate (default mode) on the right-padded fixture batch == the token ids the reference's slam_model.generate -> HF
    generate produced in fp32 on it: greedy, beam 4 (length_penalty 1 and 2) and beam 3 (length_penalty 0), both lm_head scales,
    bit-exact, as test_generate_matches_reference_tokens states it for the left-padded fixture.

    One run falls back to the margin-aware beam statement of test_generate_with_repetition_penalty_margin_aware (MARGIN_RUNS): scale 5.0,
    beam 4, length_penalty 1.  There item 2 returns [216 260 349 307 224 306 216 260 349 307 eos] (the hypothesis the reference itself
    returns for beam 3 / length_penalty 0) where the fp32 reference returns [216 124 454] x 4; items 0 and 1 are the reference's.
    Measured on MI355X: fp32 score -0.51757 against the reference's -0.51709, noise 0.388.  The
    statement, with that test's noise measure and nothing else: noise = 3 x the measured |HIP - fp32 restatement| on the prompt's
    next-token logits; an item either reproduces the reference hypothesis or returns one whose fp32 score (sum of log-probs /
    length**length_penalty, teacher-forced through the restatement) is within 2 x noise of the reference's."""
    fx, W, model, batch = _setup(dev, scale)
    b, eos, L = _to(batch, dev), int(fx[f"s{scale}.eos"]), C["max_new_tokens"]
    got = model.generate(**{k: v.clone() for k, v in b.items()}, max_new_tokens=L, num_beams=nb, length_penalty=lp,
                         eos_token_id=eos, pad_token_id=pad).cpu()
    want = torch.from_numpy(fx[RP.gen_key(scale, nb, lp, pad)])
    print(f"scale {scale} beams {nb} lp {lp}: got\n{got.numpy()}\nwant\n{want.numpy()}")
    if (scale, nb, lp, pad) not in MARGIN_RUNS:
        assert got.shape == want.shape and torch.equal(got, want), (nb, lp, pad, got, want)
        return
    cfg = C["cfg"]
    step_fn = RP.rule_step_fn(W, cfg, RP.rule_embeds(W, cfg, batch), batch["attention_mask"])
    embeds, am = model(**{k: v.clone() for k, v in b.items()}, inference_mode=True)
    B, T, d = embeds.shape
    lg0, _ = model.llm.prefill(embeds.reshape(B * T, d), B, T, am, L)
    noise = 3.0 * float((lg0.float().cpu() - step_fn(torch.zeros((B, 0), dtype=torch.int64), None)).abs().max())

    def score(seq_rows):        # teacher-forced fp32 score of one hypothesis per item
        total, length, alive = torch.zeros(B), torch.zeros(B), torch.ones(B, dtype=torch.bool)
        for t in range(seq_rows.shape[1]):
            lpr = F.log_softmax(step_fn(seq_rows[:, :t], None).float(), -1)
            tok = seq_rows[:, t]
            total += torch.where(alive, lpr.gather(1, tok[:, None])[:, 0], torch.zeros(B))
            length += alive.float()
            alive = alive & (tok != eos)
        return total / length.clamp(min=1) ** lp

    n = max(got.shape[1], want.shape[1])
    fill = pad or eos
    pad_to = lambda x: torch.cat([x, torch.full((B, n - x.shape[1]), fill, dtype=torch.int64)], 1)  # noqa: E731
    got_p, want_p = pad_to(got), pad_to(want)
    s_got, s_want = score(got_p), score(want_p)
    same = 0
    for r in range(B):
        print(f"item {r}: same {torch.equal(got_p[r], want_p[r])} fp32 score got {float(s_got[r]):.5f} reference {float(s_want[r]):.5f} noise {noise:.5f}")
        if torch.equal(got_p[r], want_p[r]):
            same += 1
        else:
            assert float(s_got[r]) >= float(s_want[r]) - 2 * noise, (scale, r, float(s_got[r]), float(s_want[r]), noise, got[r], want[r])
    assert same > 0, "no item reproduced the reference: the margin criterion would be vacuous"


def test_right_padded_kv_cache_logits_match_restatement_teacher_forced(dev):
    """prefill + decode_step logits along the reference's greedy tokens of the right-padded fixture against the fp32 restatement of the
    rule re-running the full sequence (no cache), every row (two of the three are padded): the bound of
    test_kv_cache_decode_logits_match_oracle_teacher_forced, 6e-2 + 2e-2 * max|logit|.  Token equality alone can miss a wrong position."""
    scale = 5.0
    fx, W, model, batch = _setup(dev, scale)
    cfg, b = C["cfg"], _to(batch, dev)
    toks = torch.from_numpy(fx[RP.gen_key(scale, 1, 1.0, 0)])      # rows that ended carry the pad id: still valid input ids
    step_fn = RP.rule_step_fn(W, cfg, RP.rule_embeds(W, cfg, batch), batch["attention_mask"])
    embeds, am = model(**{k: v.clone() for k, v in b.items()}, inference_mode=True)
    B, T, d = embeds.shape
    logits, cache = model.llm.prefill(embeds.reshape(B * T, d), B, T, am, toks.shape[1])
    assert int((cache.end < T).sum()) == 2 and cache.next_pos.tolist() == [int(x) for x in RP.rule_positions(batch["attention_mask"], 1)[:, -1]]
    worst = 0.0
    for t in range(toks.shape[1]):
        ref = step_fn(toks[:, :t], None)
        err = (logits.float().cpu() - ref).abs().amax(-1)
        bound = 6e-2 + 2e-2 * ref.abs().max().item()
        worst = max(worst, float(err.max()) / bound)
        print(f"step {t}: err per row {err.tolist()} bound {bound:.4f}")
        assert float(err.max()) < bound, f"step {t}: logits err {err.tolist()} > {bound}"
        logits = model.llm.decode_step(toks[:, t].to(dev), cache)
    print("right-padded teacher-forced decode: worst err/bound", worst)


def _row_alone(batch, i):
    """row i of the right-padded batch as a batch of one without pad tokens (the encoder input stays the row's mel as the batch holds it)"""
    n = int(batch["attention_mask"][i].sum())
    out = {k: batch[k][i:i + 1, :n].clone() for k in ("input_ids", "attention_mask", "modality_mask")}
    out["audio_mel"] = batch["audio_mel"][i:i + 1].clone()
    return out


def test_right_pad_fix_decodes_every_row_as_if_alone(dev):
    """generate_right_pad_fix=True (the kwarg, and the config key): each row's tokens == O.slam_generate on that row alone (B = 1, no
    padding), lm_head scale 24, greedy and beam 4; the default mode gives other tokens on this batch"""
    scale = 24.0
    fx, W, model, batch = _setup(dev, scale)
    b, eos, L = _to(batch, dev), int(fx[f"s{scale}.eos"]), C["max_new_tokens"]
    from slam_llm_amd.model import SlamHipModel
    by_cfg = SlamHipModel(dict(C["cfg"], lora_dropout=0.0, generate_right_pad_fix=True), dev).load_weights(W).eval()
    for nb in (1, 4):
        kw = dict(max_new_tokens=L, num_beams=nb, length_penalty=1.0, eos_token_id=eos, pad_token_id=C["pad"])
        got = model.generate(**{k: v.clone() for k, v in b.items()}, generate_right_pad_fix=True, **kw).cpu()
        assert torch.equal(by_cfg.generate(**{k: v.clone() for k, v in b.items()}, **kw).cpu(), got)
        assert torch.equal(by_cfg.generate(**{k: v.clone() for k, v in b.items()}, generate_right_pad_fix=False, **kw).cpu(),
                           torch.from_numpy(fx[RP.gen_key(scale, nb, 1.0, C["pad"])]))
        differs = False
        for i in range(got.shape[0]):
            want = O.slam_generate(W, C["cfg"], _row_alone(batch, i), max_new_tokens=L, num_beams=nb, length_penalty=1.0, eos=eos,
                                   pad=C["pad"])[0]
            n = want.shape[0]
            fill = C["pad"] if nb == 1 else (C["pad"] or eos)
            print(f"beams {nb} row {i}: got {got[i].tolist()} want {want.tolist()}")
            assert got.shape[1] >= n and torch.equal(got[i, :n], want) and bool((got[i, n:] == fill).all()), (nb, i, got[i], want)
            ref_mode = torch.from_numpy(fx[RP.gen_key(scale, nb, 1.0, C["pad"])])[i]
            differs = differs or not torch.equal(ref_mode[:n], want[: ref_mode.shape[0]])
        assert differs, "the fixture's padded rows must tell the two modes apart"


@pytest.mark.parametrize("scale", [24.0, 5.0])
def test_right_pad_fix_changes_nothing_on_a_left_padded_batch(dev, scale):
    """tests/golden/generate.npz (left padded) with the flag set: the reference's tokens, bit for bit, as without it"""
    from tests.test_oracle_golden import GEN_RUNS, gen_key
    fx, W, model, batch = _setup(dev, scale, fixture="generate")
    b, eos = _to(batch, dev), int(fx[f"s{scale}.eos"])
    for nb, lp, pad, rp in GEN_RUNS:
        if rp != 1.0:
            continue
        got = model.generate(**{k: v.clone() for k, v in b.items()}, max_new_tokens=C["max_new_tokens"], num_beams=nb, length_penalty=lp,
                             eos_token_id=eos, pad_token_id=pad, generate_right_pad_fix=True)
        want = fx[gen_key(scale, nb, lp, pad, rp)]
        assert tuple(got.shape) == want.shape and (got.cpu().numpy() == want).all(), (nb, lp, pad, got, want)


def test_right_padding_warning_is_logged_once_and_names_the_flag(dev, caplog):
    import logging
    from slam_llm_amd import model as M
    fx, W, model, batch = _setup(dev, 24.0)
    b, eos = _to(batch, dev), int(fx["s24.0.eos"])
    kw = dict(max_new_tokens=2, num_beams=1, eos_token_id=eos, pad_token_id=0)
    M._RIGHT_PAD_WARNED[0] = False
    with caplog.at_level(logging.WARNING, logger=M.logger.name):
        model.generate(**{k: v.clone() for k, v in b.items()}, generate_right_pad_fix=True, **kw)       # fixed: nothing to warn about
        left = _to(_fixture_batch(G.load("generate")), dev)
        model.generate(**left, **kw)                                                                     # left padded: nothing either
        assert not [r for r in caplog.records if "generate_right_pad_fix" in r.getMessage()]
        model.generate(**{k: v.clone() for k, v in b.items()}, **kw)
        model.generate(**{k: v.clone() for k, v in b.items()}, **kw)
    hits = [r for r in caplog.records if "generate_right_pad_fix" in r.getMessage()]
    assert len(hits) == 1 and hits[0].levelno == logging.WARNING


def test_generate_rejects_masks_with_holes_and_empty_rows(dev):
    fx, W, model, batch = _setup(dev, 24.0)
    b = _to(batch, dev)
    holes = {k: v.clone() for k, v in b.items()}
    holes["attention_mask"][0, 3] = 0
    with pytest.raises(ValueError, match="contiguous"):
        model.generate(**holes, max_new_tokens=2, num_beams=1, eos_token_id=2, pad_token_id=0)
    empty = {k: v.clone() for k, v in b.items()}
    empty["attention_mask"][1] = 0
    with pytest.raises(ValueError, match="no real token"):
        model.generate(**empty, max_new_tokens=2, num_beams=1, eos_token_id=2, pad_token_id=0)


# ------------------------------------------------------------------------------------------------ f: families
def _family(name):
    if name == "step_qwen2_tied":
        from tests import qwen2_cases as Q
        return Q.CASES[name]["cfg"], Q.qwen2_weights(Q.CASES[name]["cfg"], seed=42, norm_scale=Q.GENERATE_CASE["norm_scale"]), Q.qwen2_forward, Q.GENERATE_CASE
    from tests import qwen3_cases as Q
    return Q.CASES[name]["cfg"], Q.qwen3_weights(Q.CASES[name]["cfg"], seed=42, norm_scale=Q.GENERATE_CASE["norm_scale"]), Q.qwen3_forward, Q.GENERATE_CASE


@pytest.mark.parametrize("name", ["step_qwen2_tied", "step_qwen3_tied"])
def test_families_decode_right_padded_batches(dev, name):
    """Qwen2 (tied head; the q|k|v bias reaches the new token only through the decode kernel) and Qwen3 (per-head q/k RMSNorm) on the
    right-padded batch of their GENERATE_CASE, greedy, default mode, against the restated rule over the family's fp32 forward
    (tests/qwen2_cases.py, tests/qwen3_cases.py).  No reference fixture exists for these; the comparison is the margin-aware greedy
    statement of those files' own generate tests: noise = 3 x the measured |HIP - fp32| on the prompt's next-token logits, and a row
    either reproduces the restatement's tokens or equals them up to (excluding) its first step whose fp32 top-2 margin is below
    2 x noise; at least one token position must have been compared."""
    from slam_llm_amd.model import SlamHipModel
    cfg, W, forward, QC = _family(name)
    audio = O.synth_audio(len(QC["clip_samples"]), 2.0, seed=1234)
    batch = RP.rightpad_batch(cfg, audio, QC["clip_samples"], QC["prompt_lens"])
    assert int((batch["attention_mask"][:, -1] == 0).sum()) == 2
    model = SlamHipModel(dict(cfg, lora_dropout=0.0), dev).load_weights(W)
    model.eval()
    b, L, eos = _to(batch, dev), QC["max_new_tokens"], cfg["vocab"] - 1
    step_fn = RP.rule_step_fn(W, cfg, RP.rule_embeds(W, cfg, batch), batch["attention_mask"], forward)
    trace = []
    want = O.greedy_search(step_fn, 3, L, eos, QC["pad"], 1, trace=trace)
    embeds, am = model(**{k: v.clone() for k, v in b.items()}, inference_mode=True)
    B, T, d = embeds.shape
    lg0, _ = model.llm.prefill(embeds.reshape(B * T, d), B, T, am, L)
    noise = 3.0 * float((lg0.float().cpu() - step_fn(torch.zeros((B, 0), dtype=torch.int64), None)).abs().max())
    got = model.generate(**{k: v.clone() for k, v in b.items()}, max_new_tokens=L, num_beams=1, eos_token_id=eos, pad_token_id=QC["pad"]).cpu()
    margins = torch.stack([t["margin"] for t in trace])
    compared = 0
    n = max(got.shape[1], want.shape[1])
    pad_to = lambda x: torch.cat([x, torch.full((B, n - x.shape[1]), QC["pad"], dtype=torch.int64)], 1)  # noqa: E731
    got_p, want_p = pad_to(got), pad_to(want)
    for r in range(B):
        print(f"{name} row {r}: noise {noise:.4f} got {got_p[r].tolist()} want {want_p[r].tolist()}")
        if torch.equal(got_p[r], want_p[r]):      # (as in those tests: a row that reproduces the restatement is compared whole)
            compared += n
            continue
        close = (margins[:, r] < 2 * noise).nonzero()
        upto = int(close[0]) if close.numel() else n
        assert torch.equal(got_p[r, :upto], want_p[r, :upto]), (name, r, upto, got[r], want[r], noise)
        compared += upto
    assert compared > 0, "nothing was comparable: the margin criterion is vacuous here"


# ------------------------------------------------------------------------------------------------ g: the plugin's own batch
def test_plugin_right_padded_inference_batch_decodes(dev):
    """inference samples from batcher.make_sample, collated with batcher.collate(..., left_pad_prompt=False) as MultiTaskDataset does in
    inference_mode (raw audio, clips and prompts of different lengths, pad_or_trim off): generate() runs and returns the tokens of the
    hand-built batch of the same rows"""
    from slam_llm_amd import batcher
    from slam_llm_amd.model import SlamHipModel
    W = generate_case_weights(24.0)
    model = SlamHipModel(dict(C["cfg"], lora_dropout=0.0, pad_or_trim=False), dev).load_weights(W)
    model.eval()
    audio = O.synth_audio(3, 2.0, seed=77)
    clips = [audio[0][:32000], audio[1][:22400], audio[2][:28800]]
    prompts = [[5, 17, 301, 42, 9, 88], [7, 250, 31, 6], [400, 3, 12, 77, 140, 9, 55]]
    alens = [batcher.whisper_audio_length(len(a), 5, pad_to_30s=False) for a in clips]
    samples = [batcher.make_sample(a, p, None, 2, n) for a, p, n in zip(clips, prompts, alens)]
    coll = batcher.collate(samples, 0, False, pad_or_trim=False)
    rows = [n + len(p) for n, p in zip(alens, prompts)]
    T = max(rows)
    assert len(set(rows)) == 3 and len(set(alens)) == 3
    # the same rows by hand: [audio placeholders, prompt] at the front, pad id 0 behind
    ids = torch.zeros((3, T), dtype=torch.int64)
    mask = torch.zeros((3, T), dtype=torch.bool)
    mod = torch.zeros((3, T), dtype=torch.bool)
    wav = torch.zeros((3, 32000))
    for i, (a, p, n) in enumerate(zip(clips, prompts, alens)):
        ids[i, :n] = -1
        ids[i, n:n + len(p)] = torch.tensor(p)
        mask[i, :n + len(p)] = True
        mod[i, :n] = True
        wav[i, :len(a)] = a
    assert torch.equal(coll["input_ids"], ids) and torch.equal(coll["attention_mask"], mask) and torch.equal(coll["modality_mask"], mod)
    hand = dict(input_ids=ids, attention_mask=mask, modality_mask=mod, audio=wav, audio_len=torch.tensor([32000, 22400, 28800], dtype=torch.int32),
                audio_len_list=[32000, 22400, 28800])
    kw = dict(max_new_tokens=8, eos_token_id=int(G.load("generate_rightpad")["s24.0.eos"]), pad_token_id=0)
    for nb in (1, 4):
        got = model.generate(**{k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in coll.items()}, num_beams=nb, **kw)
        want = model.generate(**{k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in hand.items()}, num_beams=nb, **kw)
        assert got.shape[0] == 3 and 1 <= got.shape[1] <= 8 and torch.equal(got, want)

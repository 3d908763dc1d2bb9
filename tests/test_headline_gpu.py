"""GPU: parity at the HEADLINE geometry -- the shapes bench.py's C3 line is measured on.

* whole step, B = 31 clips padded to 30 s, T = 380 (M = 11 780 LLM rows: 46 full 256-row tiles + the thin 4-row tail tile; three
  lm_head chunks of 4096 rows; T_e = 1500 encoder frames with the full positional table; 2576-tile products through the XCD remap),
  Whisper-large-v3 widths x 1 layer -> Llama-3-8B widths x 1 layer, raw audio in (GPU log-mel), default chunking, AUTO GEMM rule,
  against the CPU oracle (reference arithmetic in fp32);
* C4 widths (HuBERT-large conv 512 / d 1024 -> Q-Former 768 x 32 queries -> Vicuna-7B MHA 32 x 128, ffn 11008, V 32000), 1 + 1 + 1
  layers, B = 2 x 2 s waveforms;
* the single kernels at exactly the bench's shapes (GEMM cfg 12 at 11780 x 4096 x 4096 and 11780 x 6144 x 4160 with bias / residual,
  attention forward (B 4, T 1500, H 20, D 64), attention backward (B 8, T 380, 32q / 8kv, D 128)) against fp32 torch on the device
  (row / head samples where the full fp32 reference would be slow).
Tolerances are written at each assert; they are the ones of tests/test_boundary_gpu.py::test_true_width_step_matches_oracle."""
import os

import numpy as np
import pytest
import torch

from oracle import slam_oracle as O
from tests import golden_util as G

pytestmark = pytest.mark.gpu


LAST_LOGITS = {}


def _eval_logits_check(model, gb, ob, what, **kw):
    """the every-row EVAL forward of the HIP model (the training forward of a labelled batch hands no logits out) against the oracle's
    logits of the same batch -- SURVEY 8(c) "logits compared on a sampled subset", north_star "loss/logits"."""
    ref = LAST_LOGITS.pop("ref")
    was = model.training
    model.eval()
    try:
        with torch.no_grad():
            out_eval, _ = model(**{k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in gb.items()})
    finally:
        model.train(was)
    assert out_eval.logits is not None, "eval forward returned no logits"
    return G.check_logits(out_eval.logits, ref, ob["attention_mask"], ob["labels"], what, **kw)


def _oracle_grads(W, cfg, ob, fwd):
    names = O.trainable_names(W)
    for n in names:
        W[n].requires_grad_(True)
    torch.set_num_threads(min(64, os.cpu_count()))
    res = fwd()
    loss_ref, acc_ref = res[0], res[1]
    if len(res) > 2:        # the oracle's logits [B, T, V], kept for G.check_logits (VERDICT r5 missing #1)
        LAST_LOGITS["ref"] = res[2].detach()
    loss_ref.backward()
    grads = {n: W[n].grad.detach().clone() for n in names}
    for n in names:
        W[n].requires_grad_(False)
        W[n].grad = None
    return float(loss_ref.detach()), float(acc_ref), grads


def _check_grads(model, grads, cos_min=0.999, norm_tol=3e-2, table=None, expected=None):
    """table: a list that receives (name, cosine, relative norm deviation) of every tensor BEFORE the asserts fire;
    expected: the worst 1 - cosine measured when `cos_min` was set (tests/golden_util.EXPECT): drift alarm outside [0.5, 1.5] x it"""
    worst = 1.0
    gmax = max(float(g.norm()) for g in grads.values())
    if table is not None:
        for n, p in model.store.params.items():
            gn = float(grads[n].norm())
            table.append((n, G.cosine(grads[n].numpy(), p.grad.float().cpu().numpy()), abs(float(p.grad.float().norm()) - gn) / (gn + 1e-30)))
    for n, p in model.store.params.items():
        if n.endswith("key.bias") and float(grads[n].norm()) < 1e-4 * gmax:
            # attention key biases: mathematically zero gradient (softmax is invariant to a per-query constant); the oracle's value is
            # fp32 cancellation noise, the HIP one bf16 rounding noise of the dK column sum (same rule as tests/test_model_gpu.py:404)
            assert float(p.grad.float().abs().max()) < 3e-2, n
            continue
        cs = G.cosine(grads[n].numpy(), p.grad.float().cpu().numpy())
        worst = min(worst, cs)
        G.floor_check(cs, cos_min, f"grad {n}: cosine {cs}")
        gn, mn = float(grads[n].norm()), float(p.grad.float().norm())
        assert abs(mn - gn) <= norm_tol * gn + 1e-9, f"grad {n}: norm {mn} vs {gn}"
    if expected is not None:
        G.drift_check(os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0] + " worst gradient cosine", 1.0 - worst, expected)
    return worst


@pytest.mark.timeout(2400)
@pytest.mark.parametrize("encoder,B", [("whisper-large-v3", 31), ("whisper-base", 8)])
def test_headline_geometry_step_matches_oracle(dev, encoder, B):
    """The bench geometries as whole steps: C3 (BASELINE configs[2], the headline: 31 x 30 s clips) and C2 (configs[1]: Whisper-base,
    8 x 30 s clips), T = 380, true widths, 1 + 1 layers, raw audio in: loss abs <= 1e-2, accuracy within one token, every trainable
    gradient cosine >= 0.999 and norm within 3 % of the fp32 oracle; the auto GEMM rule must have picked the kernels the bench lines
    are quoted on (4-wave hand-ordered kernel for the LLM products, persistent descriptor-DMA kernel for the K <= 2048 encoder products)."""
    _headline_case(dev, encoder, B, 1, 1)


@pytest.mark.timeout(2400)
def test_c3_full_depth_step_matches_oracle(dev):
    """VERDICT r4 missing #5: the headline model at FULL depth -- all 32 Whisper-large-v3 layers and all 32 Llama-3-8B layers at true
    widths (the bf16 residual stream at d 4096 through 32 layers has otherwise only met the oracle at C1's widths), B = 2 clips x 30 s,
    T = 380, raw audio in, LoRA r16 on q, v: loss abs <= 1e-2, accuracy within one token; gradients: cosine >= FULL_DEPTH_COS (0.985) / norm within
    FULL_DEPTH_NORM (8 %) of the FP32 oracle -- NOT the 0.999 / 3 % of the 1-layer cases: see the block comment below and the bf16-emulation
    check (tests/test_emulation_gpu.py), which shows the fp32 arithmetic of the oracle under this path's bf16 formats deviating as much.
    The fp32 oracle holds 8.6 G parameters (34 GB) on the host: skipped on a box with less than 160 GB of free RAM."""
    import psutil
    if psutil.virtual_memory().available < 160 * 2 ** 30:
        pytest.skip("needs 160 GB of host RAM for the fp32 oracle at full depth")
    _headline_case(dev, "whisper-large-v3", 2, 32, 32, keep=FULL_DEPTH_CACHE)


FULL_DEPTH_CACHE = {}      # what the full-depth case leaves for the emulation test right behind it (fp32 weights, batch, both gradient sets)


def _family_stats(dev_by_name):
    fam = {}
    for n, d in dev_by_name.items():
        key = ("q_proj.lora_A" if "q_proj.lora_A" in n else "q_proj.lora_B" if "q_proj.lora_B" in n else "v_proj.lora_A" if "v_proj.lora_A" in n
               else "v_proj.lora_B" if "v_proj.lora_B" in n else "projector")
        fam.setdefault(key, []).append(d)
    return {k: (float(np.mean(v)), float(np.max(v))) for k, v in fam.items()}


@pytest.mark.timeout(3000)
def test_c3_full_depth_bf16_emulation_explains_the_q_proj_floor(dev):
    """VERDICT r5 next #1b / ADVICE r5 (medium): the 0.985 floor of the full-depth case, backed by a test instead of prose.

    The oracle's fp32 ARITHMETIC is run again under this path's bf16 number FORMATS (oracle/bf16_emulation.py: a rounding at every tensor
    the HIP path materialises in bf16, forward and backward; bf16 frozen weights), twice: once as is, once with every contraction summed in
    another order (what any second correct implementation does).  Measured (8-core container, profiles/r06_bf16_emulation_cpu.json; the
    GPU box's host draws other numbers -- 4.0e-3 / 3.6e-3 -- because its BLAS sums in yet another order; this test re-measures):
      * emulated vs fp32: q_proj adapters fall to 1 - cos = 7.1e-3 (lora_A, layer 12) while v_proj / projector stay <= 1.7e-4 -- the HIP
        path's own profile (4.4e-3 .. 5.6e-3 / <= 4.4e-4): the degradation is a property of bf16 formats on THIS input (Whisper's output for 30 s of
        noise is nearly constant over time -- frame-to-frame cosine 0.998 -- so the keys of a deep random-init LLM share one large common
        component), not of the kernels;
      * the two emulations are 9.1e-3 APART from each other on q_proj.lora_A: bf16 roundings flip on 1e-7 differences and the flips
        cascade through 32 layers, so two correct bf16 implementations are no closer to each other than either is to fp32.  The
        "HIP vs emulation >= 0.9995" form of the check is therefore unattainable BY THE EMULATION ITSELF; what can be asserted is that the
        HIP path behaves like one more member of that family:
          (a) per tensor family (q/v x lora_A/lora_B, projector), HIP-vs-fp32 mean and max deviation <= 1.5x / 2x the larger of the
              two emulations' (HIP is no noisier than the reference arithmetic in bf16 formats);
          (b) HIP-vs-emulation <= 2.5x emulation-vs-reordered-emulation, mean and max (the twins share their input and their first
              roundings, HIP shares neither: measured 1.6x on q_proj.lora_A -- the sum of two independent deviations; the factor leaves
              room for another host's BLAS drawing closer twins);
          (c) the emulation reproduces at least half of HIP's worst q_proj deviation (the explanation accounts for the floor).
      * single sites (CPU run): without the dS rounding 7.2e-3, without the residual-stream rounding 5.0e-3, without the RMSNorm-output
        rounding 6.8e-3: no single site carries it, and a higher-precision dS operand (round 5's suspicion) buys NOTHING.
    A depth-dependent defect in the q path (RoPE backward, LoRA-extension dX, Delta) would break (a) and (b)."""
    import psutil
    from oracle import bf16_emulation as E
    if not FULL_DEPTH_CACHE:
        if psutil.virtual_memory().available < 160 * 2 ** 30:
            pytest.skip("needs 160 GB of host RAM for the fp32 oracle at full depth")
        _headline_case(dev, "whisper-large-v3", 2, 32, 32, keep=FULL_DEPTH_CACHE)
    C = FULL_DEPTH_CACHE
    W, cfg, ob, enc, g32, ghip = C["W"], C["cfg"], C["ob"], C["enc"], C["grads"], C["hip_grads"]
    C = dict(loss_ref=C["loss_ref"], loss_hip=C["loss_hip"])
    try:
        for n, t in W.items():          # the frozen matrices take their bf16 values in place (what the HIP model loaded)
            if not any(m in n for m in O.TRAINABLE_MARKERS) and t.dim() >= 2:
                t.copy_(E.rb(t))
        sites = E.ALL_SITES - {"weights"}
        emb_w = W["llm.base_model.model.model.embed_tokens.weight"]

        def emulated(reorder):
            def f():
                proj = E.projector_concat_emulated(W, E.rb(enc), cfg["ds_rate"], sites=sites, reorder=reorder)
                emb = O.embed_splice(emb_w, ob["input_ids"].clone(), ob["modality_mask"].bool(), proj)
                loss, logits = E.llama_forward_emulated(W, cfg, emb, ob["attention_mask"], ob["labels"], sites=sites, reorder=reorder)
                return loss, torch.zeros(())
            return f
        l_em, _, g_em = _oracle_grads(W, cfg, ob, emulated(False))
        l_re, _, g_re = _oracle_grads(W, cfg, ob, emulated(True))
    finally:
        FULL_DEPTH_CACHE.clear()
    names = [n for n in g32 if not n.endswith("key.bias")]
    dev_of = lambda a, b: {n: 1.0 - G.cosine(a[n].numpy(), b[n].numpy()) for n in names}  # noqa: E731
    S = {k: _family_stats(v) for k, v in dict(hip_fp32=dev_of(ghip, g32), emu_fp32=dev_of(g_em, g32), re_fp32=dev_of(g_re, g32),
                                              hip_emu=dev_of(ghip, g_em), emu_re=dev_of(g_em, g_re)).items()}
    lines = [f"full depth, B = 2: loss fp32 {C['loss_ref']:.5f} | HIP {C['loss_hip']:.5f} | emulated {l_em:.5f} | emulated, re-ordered sums {l_re:.5f}",
             "family\tHIP-vs-fp32 mean / max\temulated-vs-fp32\tre-ordered-vs-fp32\tHIP-vs-emulated\temulated-vs-re-ordered"]
    for fam in sorted(S["hip_fp32"]):
        lines.append(fam + "\t" + "\t".join(f"{S[k][fam][0]:.2e} / {S[k][fam][1]:.2e}" for k in ("hip_fp32", "emu_fp32", "re_fp32", "hip_emu", "emu_re")))
    print("\n".join(lines))
    if os.environ.get("SLAM_TEST_REPORT"):
        with open(os.environ["SLAM_TEST_REPORT"] + ".emulation.tsv", "a") as f:
            f.write("\n".join(lines) + "\n")
    assert abs(l_em - C["loss_ref"]) <= 1e-2 and abs(l_re - C["loss_ref"]) <= 1e-2
    # below this a family is "clean" (v_proj, projector: <= 4.4e-4 on the HIP side, which also carries the bf16 ENCODER the emulation does
    # not emulate -- it starts from the fp32 encoder output rounded once); ratios of such small numbers are not compared
    FLOOR = 5e-4
    for fam in S["hip_fp32"]:
        hm, hx = S["hip_fp32"][fam]
        em, ex = (max(S["emu_fp32"][fam][i], S["re_fp32"][fam][i]) for i in (0, 1))
        assert hm <= 1.5 * em + FLOOR and hx <= 2.0 * ex + FLOOR, f"(a) {fam}: HIP-vs-fp32 {hm:.2e} / {hx:.2e} vs emulations {em:.2e} / {ex:.2e}"
        dm, dx = S["hip_emu"][fam]
        tm, tx = S["emu_re"][fam]
        assert dm <= 2.5 * tm + FLOOR and dx <= 2.5 * tx + FLOOR, f"(b) {fam}: HIP-vs-emulated {dm:.2e} / {dx:.2e} vs emulated-vs-re-ordered {tm:.2e} / {tx:.2e}"
    worst_q_hip = max(S["hip_fp32"]["q_proj.lora_A"][1], S["hip_fp32"]["q_proj.lora_B"][1])
    worst_q_emu = max(S[k][f][1] for k in ("emu_fp32", "re_fp32") for f in ("q_proj.lora_A", "q_proj.lora_B"))
    assert worst_q_emu >= 0.5 * worst_q_hip, f"(c) the emulation's worst q_proj deviation {worst_q_emu:.2e} does not account for HIP's {worst_q_hip:.2e}"


# Full depth (profiles/r05_c3_full_depth.md, 132 tensors): loss 12.23417 vs 12.23254; every v_proj adapter and the projector >= 0.9996 at
# every depth; the q_proj adapters fall with depth to 0.9944 (layer 30 lora_A), norms within 3.3 %.  v and q see the same residual stream,
# the same LoRA plumbing and the same recomputed P -- what only q sees is dQ = sum_k dS_k K_k with sum_k dS_k = 0: a CANCELLING sum over
# keys that share a large common component at depth under random-init weights (token representations of a deep random transformer
# collapse towards each other), so the bf16 rounding of the dS operand (and of Delta = sum dO O) is amplified by |mean key| / |key spread|.
# A property of bf16 attention backward in this regime (torch SDPA in bf16 has it too), not of depth bookkeeping: dV = P^T dO has no such
# structure and stays at 0.9998.  The worst q_proj adapter is a noisy quantity: three builds of round 5 whose attention arithmetic differs
# only in roundings (score scale applied in the softmax / folded into Q in the kernel / folded into the frozen query projection) measured
# 1 - cos 0.0056, 0.0054 and 0.0067 (layer 30 lora_A each time), norm deviations 0.033 .. 0.037.  Floors = 2x the worst measured:
# 1 - cos 0.0067 -> 0.985 (rounded down), norm 0.037 -> 0.08.
FULL_DEPTH_COS, FULL_DEPTH_NORM = 0.985, 8e-2


def _headline_case(dev, encoder, B, enc_layers, llm_layers, keep=None):
    from slam_llm_amd import ops
    from slam_llm_amd.model import SlamHipModel, make_config
    PROMPT, ANSWER = 16, 64
    cfg = make_config(encoder, "llama-3-8b", enc_layers=enc_layers, llm_layers=llm_layers, lora_r=16, lora_alpha=32,
                      lora_targets=("q_proj", "v_proj"), lora_dropout=0.0)
    W = O.init_weights(cfg, seed=42)
    audio = O.synth_audio(B, 30.0, seed=1234)
    ob = O.synth_batch(cfg, audio, prompt_len=PROMPT, answer_lens=(ANSWER,), seed=1236, left_pad=False, pad_to_30s=True)
    assert ob["input_ids"].shape == (B, 380) and ob["audio_mel"].shape == (B, 3000, cfg["n_mels"])

    def fwd():
        with torch.no_grad():   # frozen encoder: no graph through the 31 x 20 x 1500 x 1500 attention
            enc = O.whisper_encoder(W, cfg, ob["audio_mel"].permute(0, 2, 1))
        if keep is not None:
            keep["enc"] = enc
        proj = O.projector_concat(W, enc, cfg["ds_rate"])
        emb = O.embed_splice(W["llm.base_model.model.model.embed_tokens.weight"], ob["input_ids"].clone(), ob["modality_mask"].bool(), proj)
        loss, logits = O.llama_forward(W, cfg, emb, ob["attention_mask"], ob["labels"])
        acc = O.compute_accuracy(torch.argmax(logits, -1)[:, :-1], ob["labels"][:, 1:], -100)
        return loss, acc, logits

    loss_ref, acc_ref, grads = _oracle_grads(W, cfg, ob, fwd)
    model = SlamHipModel(dict(cfg), dev).load_weights(W)
    if keep is not None:
        keep.update(W=W, cfg=dict(cfg), ob=ob, grads=grads, loss_ref=loss_ref)
    del W
    model.train()
    assert ops.lib.raw().slam_gemm_get_config() == 0, "the headline test runs under the AUTO GEMM rule"
    gb = {k: v.to(dev) for k, v in ob.items() if k != "audio_mel"}
    gb["audio"] = audio.to(dev)                                   # GPU log-mel front end, like bench.py
    ops.TIMER = ops.KernelTimer()
    try:
        outputs, acc = model(**gb)
        outputs.loss.backward()
        torch.cuda.synchronize()
    finally:
        used = set(ops.TIMER.rec)
        ops.TIMER = None
    M = B * 380
    assert model.llm.lm_head_chunk_rows is None and ((1 << 29) // cfg["vocab"]) // 256 * 256 == 4096   # default chunking: lm_head chunks of 4096 rows
    if B >= 8:      # the bench batch sizes: the auto rule must have picked the kernels the bench lines are quoted on
        assert -(-M // 4096) == (3 if B == 31 else 1)
        assert "w4" in ops.gemm_kernel_name(M, 4096, 4096) and "w4" in ops.gemm_kernel_name(M, 6144, 4160)
        assert "persist2" in ops.gemm_kernel_name(B * 1500, 3 * cfg["enc_dim"], cfg["enc_dim"])
        assert any("gemm_nt_w4_kernel" in k for k in used) and any("gemm_nt_persist2_kernel" in k for k in used), sorted(used)
    n_valid = int((ob["labels"][:, 1:] != -100).sum())
    got = float(outputs.loss)
    if keep is not None:
        keep.update(loss_hip=got, hip_grads={n: p.grad.float().cpu() for n, p in model.store.params.items()})
    assert abs(got - loss_ref) <= 1e-2, (got, loss_ref)
    assert abs(float(acc) - acc_ref) <= 1.0 / n_valid + 1e-6
    table = []
    try:
        # full depth: 32 layers of bf16 residual stream (each layer's output rounded to 8 mantissa bits before it is added on) under the
        # fp32 oracle; the floor is set from the measured table (profiles/r05_c3_full_depth.md), not from the 1-layer case
        worst = _check_grads(model, grads, table=table, **(dict(cos_min=FULL_DEPTH_COS, norm_tol=FULL_DEPTH_NORM, expected=G.EXPECT["c3_full_depth"])
                                                           if llm_layers > 1 else {}))
    finally:
        if os.environ.get("SLAM_TEST_REPORT") and table:
            with open(os.environ["SLAM_TEST_REPORT"] + ".grads.tsv", "a") as f:
                f.write(f"# {encoder} x {B}, {enc_layers} + {llm_layers} layers: loss {got:.5f} vs oracle {loss_ref:.5f}\n")
                for n, cs, nr in table:
                    f.write(f"{n}\t{cs:.6f}\t{nr:.5f}\n")
    print(f"{encoder} x {B} ({enc_layers} + {llm_layers} layers): loss {got:.4f} vs {loss_ref:.4f}, acc {float(acc):.4f} vs {acc_ref:.4f}, worst gradient cosine {worst:.6f}")
    # logits of the every-row eval forward vs the oracle's, every label row + every 5th other valid row x all 128 256 columns
    _eval_logits_check(model, gb, ob, f"{encoder} x {B}, {enc_layers} + {llm_layers} layers")
    if os.environ.get("SLAM_TEST_REPORT"):      # (tools: append the measured numbers to a file that is committed under profiles/)
        with open(os.environ["SLAM_TEST_REPORT"], "a") as f:
            f.write(f"{encoder} x {B}, {enc_layers} + {llm_layers} layers, T = 380: loss {got:.5f} vs oracle {loss_ref:.5f}; accuracy {float(acc):.4f} vs "
                    f"{acc_ref:.4f}; worst gradient cosine {worst:.6f} over {len(grads)} tensors\n")


@pytest.mark.timeout(1500)
def test_c4_true_width_step_matches_oracle(dev):
    """BASELINE configs[3] at its true widths, 1 HuBERT layer + 1 Q-Former layer + 1 Vicuna layer, two 2 s waveforms: loss abs <= 1e-2, accuracy within one token, gradients cosine >= 0.998 / norm 3 % (the Q-Former
    fixtures' tolerance, tests/test_model_gpu.py)."""
    from slam_llm_amd.model import SlamHipModel
    from slam_llm_amd.slam_model_hip import build_config
    mc = dict(encoder_name="hubert", encoder_path="hubert_large_ll60k.pt", llm_name="vicuna-7b-v1.5", encoder_dim=1024,
              encoder_projector="q-former", qformer_layers=1, query_len=32)
    cfg = build_config(dict(use_peft=True, peft_config=dict(r=32, lora_alpha=32, target_modules=["q_proj", "v_proj"], lora_dropout=0.0),
                            seed=42, freeze_encoder=True), mc)
    cfg = dict(cfg, hub_layers=1, llm_layers=1, lora_dropout=0.0, qf_dropout=0.0)
    assert (cfg["hub_dim"], cfg["hub_conv_dim"][0], cfg["qf_dim"], cfg["qf_queries"], cfg["llm_heads"], cfg["llm_kv_heads"], cfg["llm_head_dim"],
            cfg["llm_ffn"], cfg["vocab"], cfg["lora_r"]) == (1024, 512, 768, 32, 32, 32, 128, 11008, 32000, 32)
    c = dict(cfg)
    W = {k: v for k, v in O.init_weights(c, seed=42).items() if not k.startswith(("encoder.", "encoder_projector."))}
    W.update(O.init_hubert_weights(c, seed=7))
    W.update(O.init_qformer_weights(c, c["enc_dim"], c["llm_dim"], seed=11))
    audio = O.synth_audio(2, 2.0, seed=77)
    wav = torch.nn.functional.layer_norm(audio, (audio.shape[1],))   # dataset_config.normalize (speech_dataset.py:96-97)
    Q = c["qf_queries"]
    g = torch.Generator().manual_seed(1236)
    samples = [O.make_sample(Q, torch.randint(3, c["vocab"], (12,), generator=g).tolist(),
                             torch.randint(3, c["vocab"], (al - 1,), generator=g).tolist(), 2) for al in (20, 9)]
    ob = O.collate_right_pad(samples, pad_id=2)

    def fwd():
        with torch.no_grad():
            enc = O.hubert_encoder(W, c, wav)
        proj = O.projector_qformer(W, c, enc, None)
        emb = O.embed_splice(W["llm.base_model.model.model.embed_tokens.weight"], ob["input_ids"].clone(), ob["modality_mask"].bool(), proj)
        loss, logits = O.llama_forward(W, c, emb, ob["attention_mask"], ob["labels"])
        acc = O.compute_accuracy(torch.argmax(logits, -1)[:, :-1], ob["labels"][:, 1:], -100)
        return loss, acc, logits

    loss_ref, acc_ref, grads = _oracle_grads(W, c, ob, fwd)
    model = SlamHipModel(dict(cfg), dev).load_weights(W)
    del W
    model.train()
    gb = {k: v.to(dev) for k, v in ob.items()}
    gb["audio"] = wav.to(dev)
    outputs, acc = model(**gb)
    outputs.loss.backward()
    n_valid = int((ob["labels"][:, 1:] != -100).sum())
    got = float(outputs.loss)
    assert abs(got - loss_ref) <= 1e-2, (got, loss_ref)
    assert abs(float(acc) - acc_ref) <= 1.0 / n_valid + 1e-6
    worst = _check_grads(model, grads, cos_min=0.998)
    print(f"C4 true widths: loss {got:.4f} vs {loss_ref:.4f}, worst gradient cosine {worst:.6f}")
    _eval_logits_check(model, gb, ob, "C4 true widths (HuBERT-large -> Q-Former -> Vicuna-7B, 1 + 1 + 1 layers)", other_stride=1)


# ------------------------------------------------------------------------------------------------ single kernels at the bench's shapes
def _rand_bf16(shape, dev, seed, scale=1.0):
    g = torch.Generator(device=dev).manual_seed(seed)
    return (torch.randn(shape, generator=g, device=dev) * scale).to(torch.bfloat16)


@pytest.mark.parametrize("M,N,K,bias,res", [(11780, 4096, 4096, False, True), (11780, 6144, 4160, True, False),
                                            (11780, 14336, 4096, False, False), (46500, 1280, 1280, True, True)])
def test_gemm_at_bench_shapes(dev, M, N, K, bias, res):
    """many tiles AND long K together, through the XCD remap (736 / 1104 / 2576 tiles incl. the thin M-tail row; the K = 1280 shape
    runs the persistent kernel over 182 x 5 tiles), under the auto rule: every 97th row and the last 8 rows against an fp32 matmul of
    the same bf16 operands; |err| <= 2e-2 * (1 + |ref|) (bf16 output rounding of O(1..60) values: 2^-8 relative)."""
    from slam_llm_amd import ops
    a = _rand_bf16((M, K), dev, 1, 1.0)
    b = _rand_bf16((N, K), dev, 2, K ** -0.5)
    bias_t = torch.randn(N, device=dev) if bias else None
    res_t = _rand_bf16((M, N), dev, 3) if res else None
    assert ops.lib.raw().slam_gemm_get_config() == 0
    name = ops.gemm_kernel_name(M, N, K)
    assert ("persist2" in name) if K <= 2048 else ("w4" in name), name
    out = ops.gemm_nt(a, b, bias=bias_t, residual=res_t)
    rows = torch.cat([torch.arange(0, M, 97, device=dev), torch.arange(M - 8, M, device=dev)]).unique()
    ref = a[rows].float() @ b.float().t()
    if bias:
        ref += bias_t
    if res:
        ref += res_t[rows].float()
    err = (out[rows].float() - ref).abs()
    tol = 2e-2 * (1 + ref.abs())
    assert bool((err <= tol).all()), f"{name}: max err {float(err.max()):.4f} at {int(err.argmax())}"
    # every output element written exactly once with a finite value (a non-bijective tile map would leave holes of the fill value)
    out2 = torch.full_like(out, float("nan"))
    ops.gemm_nt(a, b, out=out2, bias=bias_t, residual=res_t)
    assert bool(torch.isfinite(out2).all()) and torch.equal(out2, out)


def _attn_ref(q, k, v, causal, scale):
    """fp32 softmax attention for [T, D] slices of one (batch, head)"""
    s = (q.float() @ k.float().t()) * scale
    if causal:
        T = q.shape[0]
        s = s.masked_fill(~torch.tril(torch.ones(T, T, dtype=torch.bool, device=q.device)), float("-inf"))
    p = torch.softmax(s, -1)
    return p @ v.float(), torch.logsumexp(s, -1), p


def test_attn_fwd_at_whisper_bench_shape(dev):
    """(B 4, T 1500, H 20, D 64) bidirectional -- the C3 encoder's attention launch (12 query blocks per head, 24 key tiles, ragged
    last tile: 1500 = 23 x 64 + 28), XCD-aware workgroup order: O within 2e-2 abs (values O(1)), LSE within 2e-3 of fp32 on
    every 3rd (batch, head)."""
    from slam_llm_amd import ops
    B, T, H, D = 4, 1500, 20, 64
    Tp = ops.round_up(T, 64)
    qkv = _rand_bf16((B * T, 3 * H * D), dev, 11, 1.0)
    q2d, k2d, v2d = qkv[:, : H * D], qkv[:, H * D: 2 * H * D], qkv[:, 2 * H * D:]
    scale = D ** -0.5
    out, lse = ops.attn_fwd(q2d, k2d, v2d, B, T, H, H, D, False, scale)     # V row-major: the kernel reads V^T with transposing LDS reads
    torch.cuda.synchronize()
    worst_o = worst_l = 0.0
    for bh in range(0, B * H, 3):
        b, h = divmod(bh, H)
        sl = slice(h * D, (h + 1) * D)
        o_ref, lse_ref, _ = _attn_ref(q2d[b * T:(b + 1) * T, sl], k2d[b * T:(b + 1) * T, sl], v2d[b * T:(b + 1) * T, sl], False, scale)
        worst_o = max(worst_o, float((out[b * T:(b + 1) * T, sl].float() - o_ref).abs().max()))
        worst_l = max(worst_l, float((lse.view(B, H, -1)[b, h, :T] - lse_ref).abs().max()))
    assert worst_o <= 2e-2 and worst_l <= 2e-3, (worst_o, worst_l)


def test_attn_bwd_at_llama_bench_shape(dev):
    """(B 8, T 380, 32 q / 8 kv heads, D 128) causal GQA, fused RoPE gradient off: dQ / dK / dV of the transposed-read ring kernels (XCD-aware
    workgroup order, all key blocks of one (b, kv head) on one XCD) against fp32 autograd on every batch, 2 kv groups each:
    cosine >= 0.999 and max |err| <= 3e-2 * max |ref| per tensor."""
    from slam_llm_amd import ops
    B, T, Hq, Hkv, D = 8, 380, 32, 8, 128
    G_ = Hq // Hkv
    Tp = ops.round_up(T, 64)
    q2d = _rand_bf16((B * T, Hq * D), dev, 21)
    k2d = _rand_bf16((B * T, Hkv * D), dev, 22)
    v2d = _rand_bf16((B * T, Hkv * D), dev, 23)
    do2d = _rand_bf16((B * T, Hq * D), dev, 24)
    scale = D ** -0.5

    def tr(x2d, H):   # [B*T, H*D] -> [B, H, D, Tp] zero padded
        t = torch.zeros((B, H, D, Tp), dtype=torch.bfloat16, device=dev)
        t[..., :T] = x2d.view(B, T, H, D).permute(0, 2, 3, 1)
        return t

    o2d, lse = ops.attn_fwd(q2d, k2d, v2d, B, T, Hq, Hkv, D, True, scale)     # no [B,H,D,Tp] copies anywhere: forward and backward read row-major tiles
    dq, dk, dv = torch.empty_like(q2d), torch.empty_like(k2d), torch.empty_like(v2d)
    ops.attn_bwd(q2d, k2d, v2d, o2d, do2d, lse, dq, dk, dv, B, T, Hq, Hkv, D, True, scale)
    torch.cuda.synchronize()
    for b in range(B):
        for hk in (b % Hkv, (b + 3) % Hkv):
            r = slice(b * T, (b + 1) * T)
            kk = k2d[r, hk * D:(hk + 1) * D].float().requires_grad_(True)
            vv = v2d[r, hk * D:(hk + 1) * D].float().requires_grad_(True)
            dq_ref = []
            for gq in range(G_):
                h = hk * G_ + gq
                qq = q2d[r, h * D:(h + 1) * D].float().requires_grad_(True)
                s = (qq @ kk.t()) * scale
                s = s.masked_fill(~torch.tril(torch.ones(T, T, dtype=torch.bool, device=dev)), float("-inf"))
                o = torch.softmax(s, -1) @ vv
                (o * do2d[r, h * D:(h + 1) * D].float()).sum().backward()
                dq_ref.append((h, qq.grad))
            for name, got, ref in [("dK", dk[r, hk * D:(hk + 1) * D], kk.grad), ("dV", dv[r, hk * D:(hk + 1) * D], vv.grad)] + \
                                  [(f"dQ[h={h}]", dq[r, h * D:(h + 1) * D], gr) for h, gr in dq_ref]:
                cs = G.cosine(ref.cpu().numpy(), got.float().cpu().numpy())
                err = float((got.float() - ref).abs().max())
                G.floor_check(cs, 0.999, f"{name} b={b} hk={hk}: cosine {cs}, max err {err}")
                assert err <= 3e-2 * float(ref.abs().max()), f"{name} b={b} hk={hk}: cosine {cs}, max err {err}"


def test_attn_xcd_order_is_bit_identical_to_hardware_order(dev):
    """the XCD-aware renumbering only changes WHICH workgroup computes a block: forward and backward outputs are bit-identical
    with the knob off (slam_attn_set_fwd_qf 20) and on (21), for a grid whose size is not a multiple of 8."""
    from slam_llm_amd import ops
    from slam_llm_amd.lib import call
    B, T, Hq, Hkv, D = 3, 200, 6, 2, 64     # 3 x 6 x 2 = 36 forward workgroups (QF 2), 3 x 2 x 2 = 12 dK/dV workgroups
    Tp = ops.round_up(T, 64)
    q2d, k2d, v2d, do2d = (_rand_bf16((B * T, H * D), dev, s) for s, H in ((31, Hq), (32, Hkv), (33, Hkv), (34, Hq)))

    def tr(x2d, H):
        t = torch.zeros((B, H, D, Tp), dtype=torch.bfloat16, device=dev)
        t[..., :T] = x2d.view(B, T, H, D).permute(0, 2, 3, 1)
        return t

    res = []
    try:
        for knob in (20, 21):
            call("slam_attn_set_fwd_qf", knob)
            o, lse = ops.attn_fwd(q2d, k2d, v2d, B, T, Hq, Hkv, D, True, D ** -0.5)
            dq, dk, dv = torch.empty_like(q2d), torch.empty_like(k2d), torch.empty_like(v2d)
            ops.attn_bwd(q2d, k2d, v2d, o, do2d, lse, dq, dk, dv, B, T, Hq, Hkv, D, True, D ** -0.5)
            torch.cuda.synchronize()
            res.append((o.clone(), lse[..., :T].clone(), dq, dk, dv))     # (LSE columns past T are never written)
    finally:
        call("slam_attn_set_fwd_qf", 21)
    for a, b_ in zip(*res):
        assert torch.equal(a, b_)


@pytest.mark.parametrize("B,T,Hq,Hkv,D", [(3, 380, 8, 2, 128), (2, 200, 6, 2, 64), (1, 1100, 4, 4, 128)])
def test_attn_heaviest_block_first_order_is_bit_identical_to_id_order(dev, B, T, Hq, Hkv, D):
    """Round 5: causal launches start each XCD's heaviest sequence blocks first (attn_blk: the i-th workgroup an XCD starts takes the
    i-th id of its run sorted by block weight).  A pure renumbering: forward output, LSE and dQ / dK / dV must be bit-identical with the
    knob off (slam_attn_set_fwd_qf 50) and on (51), for grids of 3, 4 and 9 / 18 sequence blocks whose sizes are not multiples of 8."""
    from slam_llm_amd import ops
    from slam_llm_amd.host_tables import rope_tables
    from slam_llm_amd.lib import call
    q2d, k2d, v2d, do2d = (_rand_bf16((B * T, H * D), dev, s) for s, H in ((41, Hq), (42, Hkv), (43, Hkv), (44, Hq)))
    cos, sin = (t.to(dev) for t in rope_tables(T, D, 10000.0))
    res = []
    try:
        for knob in (50, 51):
            call("slam_attn_set_fwd_qf", knob)
            o, lse = ops.attn_fwd(q2d, k2d, v2d, B, T, Hq, Hkv, D, True, D ** -0.5)
            dq, dk, dv = torch.empty_like(q2d), torch.empty_like(k2d), torch.empty_like(v2d)
            ops.attn_bwd(q2d, k2d, v2d, o, do2d, lse, dq, dk, dv, B, T, Hq, Hkv, D, True, D ** -0.5, rope=(cos, sin))
            torch.cuda.synchronize()
            res.append((o.clone(), lse[..., :T].clone(), dq, dk, dv))
    finally:
        call("slam_attn_set_fwd_qf", 51)
    for a, b_ in zip(*res):
        assert torch.isfinite(a.float()).all() and torch.equal(a, b_)


@pytest.mark.timeout(2400)
def test_headline_width_training_trajectory_tracks_oracle(dev):
    """the LOOP at true widths ("3 optimizer steps track the reference losses"; so far pinned at fixture widths only): 3 steps of
    AdamW + LambdaLR on Whisper-large-v3 x 1 -> Llama-3-8B x 1, B = 4 x 30 s clips, T = 380, two alternating batches, against the oracle's
    `train_steps` (torch.optim.AdamW on fp32 masters, utils/train_utils.py:112-169 + pipeline/finetune.py:247-260): every loss within
    3e-2, and the UPDATE each trainable tensor received over the three steps (p_after - p_before) agrees with the oracle's in direction
    (cosine >= 0.965: Adam's sign-like first steps turn a gradient angle a into a / pi sign flips) -- the fused optimizer, the LoRA re-pack of (alpha / r) B and the derived transposes are in that path at d = 4096."""
    from slam_llm_amd.model import SlamAdamW, SlamHipModel, make_config
    from slam_llm_amd.train import lr_lambda, train_step
    cfg = make_config("whisper-large-v3", "llama-3-8b", enc_layers=1, llm_layers=1, lora_r=16, lora_alpha=32,
                      lora_targets=("q_proj", "v_proj"), lora_dropout=0.0)
    W = O.init_weights(cfg, seed=42)
    obs = []
    for i in range(2):
        audio = O.synth_audio(4, 30.0, seed=4321 + i)
        obs.append(O.synth_batch(cfg, audio, prompt_len=16, answer_lens=(64,), seed=77 + i, left_pad=False, pad_to_30s=True))
    seq = [obs[0], obs[1], obs[0]]
    model = SlamHipModel(dict(cfg), dev).load_weights(W)
    model.train()
    before = {n: p.detach().float().cpu().clone() for n, p in model.store.params.items()}
    opt = SlamAdamW(model, lr=1e-3, weight_decay=0.0)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda s: lr_lambda(s + 1, 2, 10))     # (s + 1: a non-zero lr from the first step on)
    losses = []
    for ob in seq:
        loss, _ = train_step(model, {k: v.to(dev) for k, v in ob.items()}, opt, sched)
        losses.append(float(loss))
    after = {n: p.detach().float().cpu() for n, p in model.store.params.items()}
    del model
    torch.cuda.empty_cache()
    torch.set_num_threads(min(64, os.cpu_count()))
    Wt = {k: v.clone() for k, v in W.items()}
    names = O.trainable_names(Wt)
    params = [Wt[n].requires_grad_(True) for n in names]
    ropt = torch.optim.AdamW(params, lr=1e-3, weight_decay=0.0)
    rsched = torch.optim.lr_scheduler.LambdaLR(ropt, lr_lambda=lambda s: lr_lambda(s + 1, 2, 10))
    ref_losses = []
    for ob in seq:
        with torch.no_grad():
            enc = O.whisper_encoder(Wt, cfg, ob["audio_mel"].permute(0, 2, 1))
        proj = O.projector_concat(Wt, enc, cfg["ds_rate"])
        emb = O.embed_splice(Wt["llm.base_model.model.model.embed_tokens.weight"], ob["input_ids"].clone(), ob["modality_mask"].bool(), proj)
        loss, _ = O.llama_forward(Wt, cfg, emb, ob["attention_mask"], ob["labels"])
        loss.backward()
        ropt.step(); rsched.step(); ropt.zero_grad()
        ref_losses.append(float(loss.detach()))
    for s, (a, b) in enumerate(zip(losses, ref_losses)):
        assert abs(a - b) <= 3e-2, (s, losses, ref_losses)
    worst = 1.0
    for n in names:
        du_hip, du_ref = (after[n] - before[n]).numpy(), (Wt[n].detach() - W[n]).numpy()
        cs = G.cosine(du_ref, du_hip)
        worst = min(worst, cs)
        # Adam normalises every element's first steps to ~lr: the update is a SIGN-like field, and two gradients at an angle a disagree in
        # sign on a fraction a / pi of the elements -- gradient cosines of 0.9999 .. 0.9996 (what the 1-layer geometry measures) give
        # update cosines of 0.991 .. 0.982; the floor leaves the usual 2x
        assert cs >= 0.965, f"update of {n}: cosine {cs}"
    print(f"true-width trajectory: losses {losses} vs oracle {ref_losses}; worst update cosine {worst:.5f}")

"""Write tests/golden/step_qwen3_*.npz, generate_qwen3.npz and step_llama31_rope.npz by running the REFERENCE -- TEST INFRASTRUCTURE.

Run once in the authoring environment (`python tools/make_golden_qwen3.py`), where the reference checkout is importable; the
fixtures are committed and the tests read only them.  What runs (oracle/make_golden.py describes the same setup for Llama):
  * `slam_llm.models.slam_model.slam_model.forward` / `.generate` imported UNMODIFIED
  * the reference's EncoderProjectorConcat and WhisperWrappedEncoder (through oracle/make_golden.py's adapter)
  * HF `Qwen3ForCausalLM` (per-head q_norm / k_norm, no bias, head_dim independent of hidden_size, tied or untied head), or HF
    `LlamaForCausalLM` with `rope_parameters = {rope_type: llama3, ...}`, under a LoRA wrapper equal to peft 0.6.0's Linear
The case table (geometries, seeds, the norm-weight initialiser) is tests/qwen3_cases.py."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import make_golden as MG  # noqa: E402  (installs the import stubs and puts the reference on the path)
from oracle import slam_oracle as O  # noqa: E402
from tests.qwen3_cases import (CASES, GEN_RUNS, GENERATE_CASE, LLAMA31_CASE, LLAMA31_NAME, P, gen_key, head_weight,  # noqa: E402
                               qwen3_weights, rope_bands)
from transformers import LlamaConfig, LlamaForCausalLM, Qwen3Config, Qwen3ForCausalLM  # noqa: E402

ATTN = ("q_proj", "k_proj", "v_proj", "o_proj")


def build_llm_reference(cfg, W):
    """slam_model over HF Qwen3ForCausalLM (cfg['llm_qk_norm']) or LlamaForCausalLM with cfg['rope_scaling']: the encoder and
    projector as oracle/make_golden.py builds them, the LLM replaced"""
    Wl = dict(W)
    Wl[P + "lm_head.weight"] = head_weight(W)
    model = MG.build_reference(dict(cfg, lora_targets=()), Wl)
    common = dict(vocab_size=cfg["vocab"], hidden_size=cfg["llm_dim"], intermediate_size=cfg["llm_ffn"],
                  num_hidden_layers=cfg["llm_layers"], num_attention_heads=cfg["llm_heads"], num_key_value_heads=cfg["llm_kv_heads"],
                  head_dim=cfg["llm_head_dim"], rms_norm_eps=cfg["rms_eps"], max_position_embeddings=4096,
                  tie_word_embeddings=bool(cfg["tie_embeddings"]), attention_dropout=0.0, attention_bias=False)
    rope = dict(cfg.get("rope_scaling") or dict(rope_type="default"), rope_theta=cfg["rope_theta"])
    if cfg.get("llm_qk_norm"):
        hc = Qwen3Config(use_sliding_window=False, **common)
        hc.rope_parameters = rope
        hc._attn_implementation = "eager"
        llm = Qwen3ForCausalLM(hc)
        att = llm.model.layers[0].self_attn
        assert att.q_proj.bias is None and tuple(att.q_norm.weight.shape) == (cfg["llm_head_dim"],)
        assert all(t == "full_attention" for t in llm.config.layer_types)
    else:
        hc = LlamaConfig(mlp_bias=False, **common)
        hc.rope_parameters = rope
        hc._attn_implementation = "eager"
        llm = LlamaForCausalLM(hc)
    assert llm.config.rope_parameters["rope_theta"] == cfg["rope_theta"]
    assert llm.config.rope_parameters["rope_type"] == rope["rope_type"] == llm.model.rotary_emb.rope_type
    assert float(llm.model.rotary_emb.attention_scaling) == 1.0
    sd = {k[len(P):]: v for k, v in W.items() if k.startswith(P) and ".lora_" not in k}
    missing, unexpected = llm.load_state_dict(sd, strict=False)
    assert not unexpected and set(missing) <= {"lm_head.weight"}, (missing, unexpected)
    if cfg["tie_embeddings"]:
        assert llm.lm_head.weight.data_ptr() == llm.model.embed_tokens.weight.data_ptr()
    for p_ in llm.parameters():
        p_.requires_grad = False
    llm.eval()
    for i, l in enumerate(llm.model.layers):   # get_peft_model(LoraConfig(target_modules=...)) equivalent
        for nme in cfg["lora_targets"]:
            mod = l.self_attn if nme in ATTN else l.mlp
            pre = f"{P}model.layers.{i}.{'self_attn' if mod is l.self_attn else 'mlp'}.{nme}."
            ll = MG.LoraLinear(getattr(mod, nme), cfg["lora_r"], cfg["lora_alpha"])
            with torch.no_grad():
                ll.lora_A["default"].weight.copy_(W[pre + "lora_A.default.weight"])
                ll.lora_B["default"].weight.copy_(W[pre + "lora_B.default.weight"])
            setattr(mod, nme, ll)
    model.llm = llm
    return model


def trainables(model, cfg):
    out = {}
    for n in ("linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias"):
        out["encoder_projector." + n] = model.encoder_projector.get_parameter(n)
    for i, l in enumerate(model.llm.model.layers):
        for nme in cfg["lora_targets"]:
            sub = "self_attn" if nme in ATTN else "mlp"
            m = getattr(getattr(l, sub), nme)
            p = f"{P}model.layers.{i}.{sub}.{nme}."
            out[p + "lora_A.default.weight"] = m.lora_A["default"].weight
            out[p + "lora_B.default.weight"] = m.lora_B["default"].weight
    return out


LOSS_TOL = 1e-2     # the tests' tolerance on the forward loss; the comparison losses below must differ by far more (> 10x)


def gen_step(name, cfg, clip_seconds, answer_lens, left_pad, norm_scale, n_steps=3):
    torch.manual_seed(0)
    W = qwen3_weights(cfg, seed=42, norm_scale=norm_scale)
    model = build_llm_reference(cfg, W)
    audio = O.synth_audio(len(answer_lens), clip_seconds, seed=1234)
    batch = O.synth_batch(cfg, audio, prompt_len=6, answer_lens=answer_lens, seed=1236, left_pad=left_pad, pad_to_30s=False)
    tr = trainables(model, cfg)
    for p_ in tr.values():
        p_.requires_grad = True
    opt = torch.optim.AdamW(list(tr.values()), lr=1e-2, weight_decay=0.01)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda s: O.lr_lambda(s, 2, 10))
    # small on purpose: the batch (its mel included) and the logits are stored whole, everything else as a strided subsample + norm + sum
    fx = {"weights_sha256": np.array(MG.wsum(W))}
    for k, v in batch.items():
        fx["batch." + k] = v.numpy()
    # the same batch without the feature under test: how far it moves the loss (the fixture must show it)
    if cfg.get("llm_qk_norm"):
        other, what = build_llm_reference(cfg, qwen3_weights(cfg, seed=42, norm_scale=norm_scale, unit_qk_norm=True)), "loss_with_unit_qk_norm"
    else:
        T = batch["input_ids"].shape[1]
        sc = cfg["rope_scaling"]
        bands = rope_bands(cfg["llm_head_dim"], cfg["rope_theta"], sc)
        assert min(bands) >= 1, f"the llama3 rule must meet all three frequency bands, got {bands}"
        assert T >= 1.5 * sc["original_max_position_embeddings"], (T, sc)
        fx["rope_bands"] = np.array(bands)
        other, what = build_llm_reference(dict(cfg, rope_scaling=None), W), "loss_with_default_rope"
    with torch.no_grad():
        fx[what] = np.float32(other(**{k: v.clone() for k, v in batch.items()})[0].loss.item())
    for step in range(n_steps):
        outputs, acc = model(**{k: v.clone() for k, v in batch.items()})  # the reference forward, unmodified
        loss = outputs.loss
        loss.backward()
        if step == 0:
            fx["logits_full"] = outputs.logits.detach().float().numpy()
            with torch.no_grad():
                enc = model.encoder.extract_variable_length_features(batch["audio_mel"].permute(0, 2, 1))
                MG.pack(fx, "encoder_out", enc.numpy(), limit=16384)
                MG.pack(fx, "projector_out", model.encoder_projector(enc).numpy(), limit=16384)
            for n, p_ in tr.items():
                MG.pack(fx, "grad." + n, p_.grad.detach().numpy(), limit=2048)
            # the norm must move the loss by > 10x the tolerance; the RoPE rule (stored for comparison) by > 3x
            assert abs(loss.item() - float(fx[what])) > (10 if cfg.get("llm_qk_norm") else 3) * LOSS_TOL, (what, loss.item(), float(fx[what]))
        fx[f"loss.{step}"] = np.float32(loss.item())
        fx[f"acc.{step}"] = np.float32(float(acc))
        opt.step(); sched.step(); opt.zero_grad()
        print(f"{name} step {step}: loss {loss.item():.6f} acc {float(acc):.4f} ({what}: {float(fx[what]):.6f})")
    for n, p_ in tr.items():    # the parameters after the n_steps AdamW steps
        MG.pack(fx, "param." + n, p_.detach().numpy(), limit=2048)
    np.savez_compressed(os.path.join(MG.GOLD, name + ".npz"), **fx)
    print(name + ".npz written")


def gen_generate():
    """slam_model.generate UNMODIFIED -> HF Qwen3ForCausalLM.generate (fp32), greedy and beam 4, both geometries"""
    C = GENERATE_CASE
    fx = {}
    for name, case in CASES.items():
        cfg = case["cfg"]
        audio = O.synth_audio(len(C["clip_samples"]), 2.0, seed=1234)
        batch = O.synth_infer_batch(cfg, audio, C["clip_samples"], C["prompt_lens"])
        for k, v in batch.items():
            fx[f"{name}.batch." + k] = v.numpy()
        W = qwen3_weights(cfg, seed=42, norm_scale=C["norm_scale"])
        fx[f"{name}.weights_sha256"] = np.array(MG.wsum(W))
        model = build_llm_reference(cfg, W)
        model.eval()

        def run(eos, nb, lp=1.0):
            model.tokenizer = types.SimpleNamespace(bos_token_id=C["bos"], eos_token_id=eos, pad_token_id=C["pad"])
            with torch.no_grad():
                return model.generate(**{k: v.clone() for k, v in batch.items()}, max_new_tokens=C["max_new_tokens"], num_beams=nb,
                                      length_penalty=lp)

        # eos: a token a greedy row emits mid-sequence, so that rows finish at different lengths -- and never as any row's FIRST token
        # (whether min_length=1 bans eos at the first step differs between transformers versions when generate() gets only inputs_embeds)
        free = run(cfg["vocab"] - 1, 1)
        for eos in dict.fromkeys(free[:, 2:].flatten().tolist()):
            outs = {(nb, lp): run(eos, nb, lp) for nb, lp in GEN_RUNS}
            if all(not bool((o[:, 0] == eos).any()) for o in outs.values()) and any(bool((o == eos).any()) for o in outs.values()):
                break
        else:
            raise RuntimeError(f"{name}: no usable eos")
        fx[f"{name}.eos"] = np.int64(eos)
        for (nb, lp), out in outs.items():
            print(f"generate {name} eos={eos} beams={nb} lp={lp}:\n{out.numpy()}")
            fx[gen_key(name, nb, lp)] = out.numpy()
    np.savez_compressed(os.path.join(MG.GOLD, "generate_qwen3.npz"), **fx)
    print("generate_qwen3.npz written")


if __name__ == "__main__":
    if sys.argv[1:] == ["generate"]:
        gen_generate()
        sys.exit(0)
    for nme, c in CASES.items():
        gen_step(nme, **c)
    gen_step(LLAMA31_NAME, **LLAMA31_CASE)
    gen_generate()

"""Write tests/golden/step_phi3_*.npz and generate_phi3.npz by running the REFERENCE -- TEST INFRASTRUCTURE.

Run once in the authoring environment (`python tools/make_golden_phi3.py`), where the reference checkout is importable; the fixtures
are committed and the tests read only them.  What runs (oracle/make_golden.py describes the same setup for Llama):
  * `slam_llm.models.slam_model.slam_model.forward` / `.generate` imported UNMODIFIED
  * the reference's EncoderProjectorConcat and WhisperWrappedEncoder (through oracle/make_golden.py's adapter)
  * HF `Phi3ForCausalLM` (fused qkv_proj / gate_up_proj, partial_rotary_factor, default or longrope frequencies, a sliding window above
    the sequence length, tied or untied head) under a LoRA wrapper equal to peft 0.6.0's Linear on the FUSED Linears
The case table (geometries, seeds, the factor lists) is tests/phi3_cases.py."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import make_golden as MG  # noqa: E402  (installs the import stubs and puts the reference on the path)
from oracle import slam_oracle as O  # noqa: E402
from tests.phi3_cases import CASES, GEN_PADS, GEN_RUNS, GENERATE_CASE, P, attention_factor_restated, gen_key, phi3_weights  # noqa: E402
from tests.rightpad_cases import rightpad_batch  # noqa: E402
from transformers import Phi3Config, Phi3ForCausalLM  # noqa: E402

ATTN = ("qkv_proj", "o_proj")


def build_llm_reference(cfg, W):
    """slam_model over HF Phi3ForCausalLM: the encoder and projector as oracle/make_golden.py builds them, the LLM replaced"""
    model = MG.build_reference(dict(cfg, lora_targets=()), O.init_weights(dict(cfg, lora_targets=()), seed=42))
    with torch.no_grad():   # the encoder and projector of THIS state dict (equal to the seed-42 draw; copied so that it cannot drift)
        for n in ("linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias"):
            model.encoder_projector.get_parameter(n).copy_(W["encoder_projector." + n])
    D, rot, sc = cfg["llm_head_dim"], cfg["llm_rotary_dim"], cfg.get("rope_scaling")
    assert cfg["llm_dim"] == cfg["llm_heads"] * D, "Phi3Config derives head_dim from hidden_size / heads"
    rope = dict(rope_type="default", rope_theta=cfg["rope_theta"], partial_rotary_factor=rot / D)
    extra = {}
    if sc:
        rope.update(rope_type="longrope", short_factor=sc["short_factor"], long_factor=sc["long_factor"],
                    original_max_position_embeddings=sc["original_max_position_embeddings"])
        extra = dict(original_max_position_embeddings=sc["original_max_position_embeddings"], max_position_embeddings=sc["max_position_embeddings"])
    else:
        extra = dict(max_position_embeddings=4096)
    hc = Phi3Config(vocab_size=cfg["vocab"], hidden_size=cfg["llm_dim"], intermediate_size=cfg["llm_ffn"],
                    num_hidden_layers=cfg["llm_layers"], num_attention_heads=cfg["llm_heads"], num_key_value_heads=cfg["llm_kv_heads"],
                    rms_norm_eps=cfg["rms_eps"], tie_word_embeddings=bool(cfg["tie_embeddings"]), attention_dropout=0.0, resid_pdrop=0.0,
                    embd_pdrop=0.0, sliding_window=cfg.get("llm_sliding_window"), partial_rotary_factor=rot / D, pad_token_id=0,
                    bos_token_id=1, eos_token_id=2, rope_parameters=rope, **extra)
    hc._attn_implementation = "eager"
    llm = Phi3ForCausalLM(hc)
    emb = llm.model.rotary_emb
    assert emb.rope_type == rope["rope_type"] and emb.inv_freq.numel() == rot // 2
    assert abs(float(emb.attention_scaling) - attention_factor_restated(sc)) < 1e-12
    att = llm.model.layers[0].self_attn
    assert tuple(att.qkv_proj.weight.shape) == ((cfg["llm_heads"] + 2 * cfg["llm_kv_heads"]) * D, cfg["llm_dim"])
    sd = {k[len(P):]: v for k, v in W.items() if k.startswith(P) and ".lora_" not in k}
    missing, unexpected = llm.load_state_dict(sd, strict=False)
    assert not unexpected and set(missing) <= {"lm_head.weight"}, (missing, unexpected)
    if cfg["tie_embeddings"]:
        assert llm.lm_head.weight.data_ptr() == llm.model.embed_tokens.weight.data_ptr()
    for p_ in llm.parameters():
        p_.requires_grad = False
    llm.eval()
    for i, l in enumerate(llm.model.layers):   # get_peft_model(LoraConfig(target_modules=...)) equivalent, on the fused Linears
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


LOSS_TOL = 1e-2     # the tests' tolerance on the forward loss; the comparison loss below must differ by more than 3x that


def gen_step(name, cfg, clip_seconds, answer_lens, left_pad, norm_scale, n_steps=3):
    torch.manual_seed(0)
    W = phi3_weights(cfg, seed=42, norm_scale=norm_scale)
    model = build_llm_reference(cfg, W)
    audio = O.synth_audio(len(answer_lens), clip_seconds, seed=1234)
    batch = O.synth_batch(cfg, audio, prompt_len=6, answer_lens=answer_lens, seed=1236, left_pad=left_pad, pad_to_30s=False)
    T = batch["input_ids"].shape[1]
    if cfg.get("rope_scaling"):
        assert T <= cfg["rope_scaling"]["original_max_position_embeddings"] and T <= cfg["llm_sliding_window"], T
    tr = trainables(model, cfg)
    for p_ in tr.values():
        p_.requires_grad = True
    opt = torch.optim.AdamW(list(tr.values()), lr=1e-2, weight_decay=0.01)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda s: O.lr_lambda(s, 2, 10))
    fx = {"weights_sha256": np.array(MG.wsum(W))}
    for k, v in batch.items():
        fx["batch." + k] = v.numpy()
    # the same batch with the whole head rotated under plain frequencies: how far partial rotary (and longrope) move the loss
    other = build_llm_reference(dict(cfg, llm_rotary_dim=cfg["llm_head_dim"], rope_scaling=None), W)
    what = "loss_with_full_default_rope"
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
                MG.pack(fx, "grad." + n, p_.grad.detach().numpy(), limit=1536)
            assert abs(loss.item() - float(fx[what])) > 3 * LOSS_TOL, (what, loss.item(), float(fx[what]))
        fx[f"loss.{step}"] = np.float32(loss.item())
        fx[f"acc.{step}"] = np.float32(float(acc))
        opt.step(); sched.step(); opt.zero_grad()
        print(f"{name} step {step}: T {T} loss {loss.item():.6f} acc {float(acc):.4f} ({what}: {float(fx[what]):.6f})")
    for n, p_ in tr.items():    # the parameters after the n_steps AdamW steps
        MG.pack(fx, "param." + n, p_.detach().numpy(), limit=1536)
    np.savez_compressed(os.path.join(MG.GOLD, name + ".npz"), **fx)
    print(name + ".npz written")


def gen_generate():
    """slam_model.generate UNMODIFIED -> HF Phi3ForCausalLM.generate (fp32), greedy and beam 4, both geometries, the prompt batch padded
    on the left (speech dataset collator) and on the right (multitask collator)"""
    C = GENERATE_CASE
    fx = {}
    for name, case in CASES.items():
        cfg = case["cfg"]
        audio = O.synth_audio(len(C["clip_samples"]), 2.0, seed=1234)
        batches = dict(left=O.synth_infer_batch(cfg, audio, C["clip_samples"], C["prompt_lens"]),
                       right=rightpad_batch(cfg, audio, C["clip_samples"], C["prompt_lens"]))
        W = phi3_weights(cfg, seed=42, norm_scale=C["norm_scale"])
        fx[f"{name}.weights_sha256"] = np.array(MG.wsum(W))
        model = build_llm_reference(cfg, W)
        model.eval()
        for pad in GEN_PADS:
            batch = batches[pad]
            T = batch["input_ids"].shape[1]
            if cfg.get("rope_scaling"):
                assert T + C["max_new_tokens"] <= cfg["rope_scaling"]["original_max_position_embeddings"]
            for k, v in batch.items():
                if pad == "right" and k == "audio_mel":     # the same clips: stored once, under the left batch
                    assert torch.equal(v, batches["left"][k])
                    continue
                fx[f"{name}.{pad}.batch." + k] = v.numpy()

            def run(eos, nb, lp=1.0):
                model.tokenizer = types.SimpleNamespace(bos_token_id=C["bos"], eos_token_id=eos, pad_token_id=C["pad"])
                with torch.no_grad():
                    return model.generate(**{k: v.clone() for k, v in batch.items()}, max_new_tokens=C["max_new_tokens"], num_beams=nb,
                                          length_penalty=lp)

            # eos: a token a greedy row emits mid-sequence, so that rows finish at different lengths -- and never as any row's FIRST token
            free = run(cfg["vocab"] - 1, 1)
            for eos in dict.fromkeys(free[:, 2:].flatten().tolist()):
                outs = {(nb, lp): run(eos, nb, lp) for nb, lp in GEN_RUNS}
                if all(not bool((o[:, 0] == eos).any()) for o in outs.values()) and any(bool((o == eos).any()) for o in outs.values()):
                    break
            else:
                raise RuntimeError(f"{name} {pad}: no usable eos")
            fx[f"{name}.{pad}.eos"] = np.int64(eos)
            for (nb, lp), out in outs.items():
                print(f"generate {name} {pad} eos={eos} beams={nb} lp={lp}:\n{out.numpy()}")
                fx[gen_key(name, pad, nb, lp)] = out.numpy()
    np.savez_compressed(os.path.join(MG.GOLD, "generate_phi3.npz"), **fx)
    print("generate_phi3.npz written")


if __name__ == "__main__":
    if sys.argv[1:] == ["generate"]:
        gen_generate()
        sys.exit(0)
    for nme, c in CASES.items():
        gen_step(nme, **c)
    gen_generate()

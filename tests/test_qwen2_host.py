"""CPU: Qwen2 / Qwen2.5 LLMs -- presets and the recipes' spellings, geometry from an HF config.json, HF -> reference weight names,
and the fp32 Qwen2 restatement (tests/qwen2_cases.py) against the fixtures the reference wrote (tools/make_golden_qwen2.py)."""
import json
import types

import numpy as np
import pytest
import torch

from oracle import slam_oracle as O
from tests import golden_util as G
from tests.qwen2_cases import CASES, P, qwen2_weights, slam_qwen2_forward


def _build_config(**mc):
    from slam_llm_amd.slam_model_hip import build_config
    return build_config(types.SimpleNamespace(use_peft=False), dict(dict(encoder_name="whisper", encoder_path="large-v3"), **mc))


@pytest.mark.parametrize("name,want", [
    ("Qwen2.5-1.5B-Instruct", "qwen2.5-1.5b"), ("Qwen2.5-7B-Instruct", "qwen2.5-7b"), ("Qwen2-7B", "qwen2-7b"),
    ("qwen2-0.5b", "qwen2-0.5b"), ("Qwen2-0.5b", "qwen2-0.5b"), ("Qwen2.5-3B-Instruct", "qwen2.5-3b"),
    ("/models/Qwen2.5-7B-Instruct/", "qwen2.5-7b"), ("/data/model/Qwen2-7B", "qwen2-7b"),
    ("/m/models--Qwen--Qwen2-0.5B/snapshots/ff3a49fac17555b8dfc4db6709f480cc8f16a9fe", "qwen2-0.5b"),
    ("vicuna-7b-v1.5", "vicuna-7b"),
])
def test_recipe_spellings_map_to_the_right_preset(name, want):
    cfg = _build_config(llm_name=name)
    from slam_llm_amd.model import PRESETS
    for k, v in PRESETS[want].items():
        assert cfg[k] == v, (name, k, cfg[k], v)


def test_qwen2_7b_and_qwen25_7b_never_cross_match():
    from slam_llm_amd.model import PRESETS
    from slam_llm_amd.slam_model_hip import _guess_preset
    llm = {k: v for k, v in PRESETS.items() if not k.startswith("whisper")}
    assert _guess_preset("Qwen2-7B", llm) == "qwen2-7b"
    assert _guess_preset("Qwen2.5-7B", llm) == "qwen2.5-7b"
    assert _guess_preset("qwen2-7b-instruct", llm) == "qwen2-7b"
    assert _guess_preset("qwen2.5-7b-instruct", llm) == "qwen2.5-7b"
    # only the Qwen2.5 line has a 3B: a Qwen2 spelling must not fall through to it
    with pytest.raises(ValueError):
        _guess_preset("Qwen2-3B", llm)


def test_presets_and_defaults():
    from slam_llm_amd.model import PRESETS, make_config
    for k in ("qwen2-0.5b", "qwen2-1.5b", "qwen2-7b", "qwen2.5-0.5b", "qwen2.5-1.5b", "qwen2.5-3b", "qwen2.5-7b"):
        p = PRESETS[k]
        assert p["llm_qkv_bias"] is True and p["rope_theta"] == 1e6 and p["rms_eps"] == 1e-6
        assert p["tie_embeddings"] is (not k.endswith("7b"))
        assert p["llm_heads"] % p["llm_kv_heads"] == 0 and p["llm_heads"] // p["llm_kv_heads"] in (6, 7, 8)
        assert p["llm_dim"] == p["llm_heads"] * p["llm_head_dim"]
    assert PRESETS["qwen2.5-7b"]["vocab"] == 152064 and PRESETS["qwen2.5-0.5b"]["vocab"] == 151936
    for k in ("llama-3-8b", "vicuna-7b", "tinyllama-1.1b", None):
        c = make_config("whisper-large-v3", k)
        assert c["llm_qkv_bias"] is False and c["tie_embeddings"] is False


def _hf_dir(tmp_path, **over):
    hc = dict(model_type="qwen2", architectures=["Qwen2ForCausalLM"], hidden_size=448, num_hidden_layers=3, num_attention_heads=7,
              num_key_value_heads=1, intermediate_size=512, vocab_size=1024, rms_norm_eps=1e-6, tie_word_embeddings=True,
              rope_parameters=dict(rope_type="default", rope_theta=1e6), use_sliding_window=False)
    hc.update(over)
    (tmp_path / "config.json").write_text(json.dumps(hc))
    return str(tmp_path)


def test_build_config_reads_an_hf_directory(tmp_path):
    d = _hf_dir(tmp_path)
    # config.json wins over the name guess (even over a name that maps to another preset, or none)
    for name in ("Qwen2.5-7B-Instruct", "Qwen", ""):
        cfg = _build_config(llm_name=name, llm_path=d)
        assert (cfg["llm_dim"], cfg["llm_layers"], cfg["llm_heads"], cfg["llm_kv_heads"], cfg["llm_head_dim"], cfg["llm_ffn"],
                cfg["vocab"]) == (448, 3, 7, 1, 64, 512, 1024)
        assert cfg["rope_theta"] == 1e6 and cfg["rms_eps"] == 1e-6 and cfg["llm_qkv_bias"] and cfg["tie_embeddings"]
    # the older spelling: rope_theta at the top level
    cfg = _build_config(llm_path=_hf_dir(tmp_path, rope_parameters=None, rope_theta=5e5, tie_word_embeddings=False))
    assert cfg["rope_theta"] == 5e5 and not cfg["tie_embeddings"]
    # a Llama directory: no bias
    cfg = _build_config(llm_path=_hf_dir(tmp_path, model_type="llama", rope_theta=5e5))
    assert cfg["llm_qkv_bias"] is False
    # explicit arch_llm / arch_overrides win over config.json
    d = _hf_dir(tmp_path)
    assert _build_config(llm_path=d, arch_llm="qwen2.5-7b")["llm_dim"] == 3584
    assert _build_config(llm_path=d, arch_overrides={"llm_layers": 1})["llm_layers"] == 1
    # llm_dim is checked against the geometry as before
    with pytest.raises(ValueError, match="do not match"):
        _build_config(llm_path=d, llm_dim=3584)
    assert _build_config(llm_path=d, llm_dim=448)["llm_dim"] == 448


def test_unknown_model_type_is_refused(tmp_path):
    with pytest.raises(NotImplementedError, match="model_type 'mistral'"):
        _build_config(llm_name="Qwen2.5-7B-Instruct", llm_path=_hf_dir(tmp_path, model_type="mistral"))
    with pytest.raises(NotImplementedError, match="sliding-window"):
        _build_config(llm_path=_hf_dir(tmp_path, use_sliding_window=True))


def test_hf_names_map_to_reference_names(tmp_path):
    from slam_llm_amd.slam_model_hip import hf_to_reference_names, load_hf_llm_state
    t = torch.zeros(2)
    sd = {"model.embed_tokens.weight": t, "model.layers.0.self_attn.q_proj.weight": t, "model.layers.0.self_attn.q_proj.bias": t,
          "model.layers.0.self_attn.rotary_emb.inv_freq": t, "model.norm.weight": t, "lm_head.weight": t}
    got = hf_to_reference_names(sd)
    assert set(got) == {P + "model.embed_tokens.weight", P + "model.layers.0.self_attn.q_proj.weight",
                        P + "model.layers.0.self_attn.q_proj.bias", P + "model.norm.weight", P + "lm_head.weight"}
    # a tied checkpoint: no lm_head.weight, and none is invented
    tied = {k: v for k, v in sd.items() if k != "lm_head.weight"}
    assert P + "lm_head.weight" not in hf_to_reference_names(tied)
    # model.safetensors and a sharded index
    from safetensors.torch import save_file
    a = {"model.embed_tokens.weight": torch.arange(4.0), "model.norm.weight": torch.ones(3)}
    b = {"model.layers.0.self_attn.k_proj.bias": torch.full((2,), 5.0)}
    save_file(a, str(tmp_path / "model-00001-of-00002.safetensors"))
    save_file(b, str(tmp_path / "model-00002-of-00002.safetensors"))
    idx = {"weight_map": {**{k: "model-00001-of-00002.safetensors" for k in a}, **{k: "model-00002-of-00002.safetensors" for k in b}}}
    (tmp_path / "model.safetensors.index.json").write_text(json.dumps(idx))
    W = load_hf_llm_state(str(tmp_path))
    assert set(W) == {P + k for k in list(a) + list(b)}
    assert torch.equal(W[P + "model.layers.0.self_attn.k_proj.bias"], b["model.layers.0.self_attn.k_proj.bias"])


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_reproduces_reference_fixture(name):
    """the fp32 Qwen2 restatement == the reference's slam_model over HF Qwen2ForCausalLM: loss, logits, first-step gradients"""
    fx = G.load(name)
    cfg = CASES[name]["cfg"]
    W = qwen2_weights(cfg, seed=42)
    batch = {k[len("batch."):]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("batch.")}
    names = O.trainable_names(W)
    for n in names:
        W[n] = W[n].clone().requires_grad_(True)
    loss, logits, acc = slam_qwen2_forward(W, cfg, batch)
    loss.backward()
    assert abs(float(loss) - float(fx["loss.0"])) < 1e-4, (float(loss), float(fx["loss.0"]))
    assert abs(float(fx["loss.0"]) - float(fx["loss_without_bias"])) > 2e-2, "the fixture's biases do not move the loss"
    G.check_packed(fx, "logits", logits.detach().numpy(), atol=2e-4, rtol=1e-4)
    assert abs(float(acc) - float(fx["acc.0"])) < 1e-6
    assert len(names) == sum(1 for k in fx.files if k.startswith("grad.") and not k.endswith(("__stride", "__norm", "__sum")))
    for n in names:
        g, m = G.sub(fx, "grad." + n, W[n].grad.numpy())
        assert G.cosine(g, m) > 0.99999, (n, G.cosine(g, m))
        assert np.allclose(float(np.sqrt((W[n].grad.double() ** 2).sum())), float(fx["grad." + n + ".__norm"]), rtol=1e-4)

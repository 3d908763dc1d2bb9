"""CPU: Qwen3 LLMs and Llama-3.1 / 3.2 scaled RoPE -- presets and the recipes' spellings, geometry from an HF config.json, the
llama3 / linear RoPE frequency rules against the installed transformers, HF -> reference weight names, and the fp32 restatement
(tests/qwen3_cases.py) against the fixtures the reference wrote (tools/make_golden_qwen3.py)."""
import json
import types

import numpy as np
import pytest
import torch

from oracle import slam_oracle as O
from tests import golden_util as G
from tests.qwen3_cases import (CASES, LLAMA31_CASE, LLAMA31_NAME, P, inv_freq_restated, qwen3_weights, rope_bands,
                               slam_qwen3_forward)

ALL_CASES = dict(CASES, **{LLAMA31_NAME: LLAMA31_CASE})


def _build_config(**mc):
    from slam_llm_amd.slam_model_hip import build_config
    return build_config(types.SimpleNamespace(use_peft=False), dict(dict(encoder_name="whisper", encoder_path="large-v3"), **mc))


def _llm_presets():
    from slam_llm_amd.model import PRESETS
    return {k: v for k, v in PRESETS.items() if not k.startswith("whisper")}


@pytest.mark.parametrize("name,want", [
    ("Qwen3-0.6B", "qwen3-0.6b"), ("Qwen3-1.7B", "qwen3-1.7b"), ("Qwen3-4B-Instruct-2507", "qwen3-4b"), ("qwen3-8b", "qwen3-8b"),
    ("Qwen3-8B-Instruct", "qwen3-8b"), ("/models/Qwen3-0.6B/", "qwen3-0.6b"),
    ("/m/models--Qwen--Qwen3-1.7B/snapshots/70d244cc86ccca08cf5af4e1e306ecf908b1ad5e", "qwen3-1.7b"),
    ("Meta-Llama-3.1-8B-Instruct", "llama-3.1-8b"), ("Llama-3.1-8B", "llama-3.1-8b"), ("Llama-3.2-1B-Instruct", "llama-3.2-1b"),
    ("/data/models--meta-llama--Llama-3.2-3B/snapshots/13afe5124825b4f3751f836b40dafda64c1ed062", "llama-3.2-3b"),
    ("Meta-Llama-3-8B", "llama-3-8b"), ("Qwen2.5-7B-Instruct", "qwen2.5-7b"), ("Qwen2-7B", "qwen2-7b"),
])
def test_recipe_spellings_map_to_the_right_preset(name, want):
    from slam_llm_amd.model import PRESETS
    cfg = _build_config(llm_name=name)
    for k, v in PRESETS[want].items():
        assert cfg[k] == v, (name, k, cfg[k], v)
    assert cfg["llm_qk_norm"] is want.startswith("qwen3")
    assert (cfg["rope_scaling"] is not None) == want.startswith(("llama-3.1", "llama-3.2"))


def test_neighbouring_families_never_cross_match():
    from slam_llm_amd.slam_model_hip import _guess_preset
    llm = _llm_presets()
    for name, want in (("Llama-3-8B", "llama-3-8b"), ("Llama-3.1-8B", "llama-3.1-8b"), ("llama-3-8b-instruct", "llama-3-8b"),
                       ("llama-3.1-8b-instruct", "llama-3.1-8b"), ("Qwen2-7B", "qwen2-7b"), ("Qwen2.5-7B", "qwen2.5-7b"),
                       ("Qwen3-8B", "qwen3-8b"), ("Qwen2-0.5B", "qwen2-0.5b"), ("Qwen2.5-0.5B", "qwen2.5-0.5b"),
                       ("Qwen3-0.6B", "qwen3-0.6b"), ("Qwen2-1.5B", "qwen2-1.5b"), ("Qwen3-1.7B", "qwen3-1.7b")):
        assert _guess_preset(name, llm) == want, name
    # sizes a line does not have must not fall through to a neighbouring line
    for name in ("Qwen2-3B", "Qwen3-7B", "Qwen3-3B", "Qwen2.5-8B", "Llama-3.1-1B", "Llama-3.2-8B"):
        with pytest.raises(ValueError):
            _guess_preset(name, llm)


def test_presets_and_defaults():
    from slam_llm_amd.model import PRESETS, make_config
    geo = {"qwen3-0.6b": (1024, 28, 16, 8, 3072, True), "qwen3-1.7b": (2048, 28, 16, 8, 6144, True),
           "qwen3-4b": (2560, 36, 32, 8, 9728, True), "qwen3-8b": (4096, 36, 32, 8, 12288, False)}
    for k, (d, n, hq, hkv, ffn, tied) in geo.items():
        p = PRESETS[k]
        assert (p["llm_dim"], p["llm_layers"], p["llm_heads"], p["llm_kv_heads"], p["llm_ffn"], p["tie_embeddings"]) == (d, n, hq, hkv, ffn, tied)
        assert p["llm_head_dim"] == 128 and p["vocab"] == 151936 and p["rope_theta"] == 1e6 and p["rms_eps"] == 1e-6
        assert p["llm_qk_norm"] is True and not p.get("llm_qkv_bias", False) and p.get("rope_scaling") is None
    assert PRESETS["qwen3-0.6b"]["llm_heads"] * 128 != PRESETS["qwen3-0.6b"]["llm_dim"]
    l31, l3 = PRESETS["llama-3.1-8b"], PRESETS["llama-3-8b"]
    assert {k: v for k, v in l31.items() if k != "rope_scaling"} == l3 and "rope_scaling" not in l3
    assert l31["rope_scaling"] == dict(rope_type="llama3", factor=8.0, low_freq_factor=1.0, high_freq_factor=4.0,
                                       original_max_position_embeddings=8192)
    for k, (d, n, hq, D) in {"llama-3.2-1b": (2048, 16, 32, 64), "llama-3.2-3b": (3072, 28, 24, 128)}.items():
        p = PRESETS[k]
        assert (p["llm_dim"], p["llm_layers"], p["llm_heads"], p["llm_kv_heads"], p["llm_head_dim"], p["llm_ffn"]) == (d, n, hq, 8, D, 8192)
        assert p["tie_embeddings"] is True and p["rope_scaling"]["factor"] == 32.0 and p["rope_scaling"]["rope_type"] == "llama3"
    for k in ("llama-3-8b", "vicuna-7b", "tinyllama-1.1b", "qwen2.5-7b", None):
        c = make_config("whisper-large-v3", k)
        assert c["llm_qk_norm"] is False and c["rope_scaling"] is None


def _hf_dir(tmp_path, **over):
    hc = dict(model_type="qwen3", architectures=["Qwen3ForCausalLM"], hidden_size=192, num_hidden_layers=3, num_attention_heads=6,
              num_key_value_heads=2, head_dim=64, intermediate_size=512, vocab_size=512, rms_norm_eps=1e-6, tie_word_embeddings=True,
              attention_bias=False, rope_parameters=dict(rope_type="default", rope_theta=1e6), use_sliding_window=False,
              layer_types=["full_attention"] * 3)
    hc.update(over)
    (tmp_path / "config.json").write_text(json.dumps(hc))
    return str(tmp_path)


LLAMA3 = dict(rope_type="llama3", factor=8.0, low_freq_factor=1.0, high_freq_factor=4.0, original_max_position_embeddings=8192)


def test_build_config_reads_a_qwen3_directory(tmp_path):
    cfg = _build_config(llm_name="Qwen3-8B", llm_path=_hf_dir(tmp_path))
    assert (cfg["llm_dim"], cfg["llm_layers"], cfg["llm_heads"], cfg["llm_kv_heads"], cfg["llm_head_dim"], cfg["llm_ffn"],
            cfg["vocab"]) == (192, 3, 6, 2, 64, 512, 512)        # head_dim from config.json, not hidden_size / heads = 32
    assert cfg["llm_qk_norm"] is True and cfg["llm_qkv_bias"] is False and cfg["tie_embeddings"] and cfg["rope_scaling"] is None
    assert cfg["rope_theta"] == 1e6 and cfg["rms_eps"] == 1e-6
    assert _build_config(llm_path=_hf_dir(tmp_path, attention_bias=True))["llm_qkv_bias"] is True
    # a Qwen2 directory still has the bias and no norm
    q2 = _build_config(llm_path=_hf_dir(tmp_path, model_type="qwen2", head_dim=None, hidden_size=384))
    assert q2["llm_qkv_bias"] is True and q2["llm_qk_norm"] is False


def test_sliding_attention_layers_are_refused(tmp_path):
    with pytest.raises(NotImplementedError, match="sliding_attention"):
        _build_config(llm_path=_hf_dir(tmp_path, layer_types=["full_attention", "sliding_attention", "full_attention"]))
    with pytest.raises(NotImplementedError, match="sliding-window"):
        _build_config(llm_path=_hf_dir(tmp_path, use_sliding_window=True))


def test_rope_scaling_types_in_a_directory(tmp_path):
    llama = dict(model_type="llama", architectures=["LlamaForCausalLM"], head_dim=None, hidden_size=384, layer_types=None)
    # both spellings of a Llama-3.1 config.json are accepted and passed on
    new = _build_config(llm_path=_hf_dir(tmp_path, **llama, rope_parameters=dict(LLAMA3, rope_theta=5e5)))
    old = _build_config(llm_path=_hf_dir(tmp_path, **llama, rope_parameters=None, rope_theta=5e5, rope_scaling=dict(LLAMA3)))
    for cfg in (new, old):
        assert cfg["rope_scaling"] == LLAMA3 and cfg["rope_theta"] == 5e5 and not cfg["llm_qk_norm"] and not cfg["llm_qkv_bias"]
    lin = _build_config(llm_path=_hf_dir(tmp_path, **llama, rope_parameters=None, rope_theta=1e4, rope_scaling=dict(type="linear", factor=4.0)))
    assert lin["rope_scaling"] == dict(rope_type="linear", factor=4.0)
    for kind in ("yarn", "dynamic", "longrope"):
        with pytest.raises(NotImplementedError, match=kind):
            _build_config(llm_path=_hf_dir(tmp_path, rope_parameters=dict(rope_type=kind, factor=4.0, rope_theta=1e6)))
        with pytest.raises(NotImplementedError, match=kind):
            _build_config(llm_path=_hf_dir(tmp_path, rope_scaling=dict(type=kind, factor=4.0)))
    with pytest.raises(ValueError, match="original_max_position_embeddings"):
        _build_config(llm_path=_hf_dir(tmp_path, rope_scaling=dict(rope_type="llama3", factor=8.0, low_freq_factor=1.0, high_freq_factor=4.0)))


def _hf_inv_freq(D, theta, scaling):
    from transformers import LlamaConfig
    from transformers.modeling_rope_utils import ROPE_INIT_FUNCTIONS
    hc = LlamaConfig(hidden_size=D * 2, num_attention_heads=2, head_dim=D, max_position_embeddings=131072)
    hc.rope_parameters = dict(scaling, rope_theta=theta)
    inv, attention_factor = ROPE_INIT_FUNCTIONS[scaling["rope_type"]](hc, "cpu")
    assert attention_factor == 1.0
    return inv


@pytest.mark.parametrize("D,theta,scaling", [
    (128, 5e5, LLAMA3), (64, 5e5, dict(LLAMA3, factor=32.0)), (128, 5e5, dict(LLAMA3, factor=32.0)),
    (64, 1e4, LLAMA31_CASE["cfg"]["rope_scaling"]), (128, 1e4, dict(rope_type="linear", factor=4.0)),
    (64, 1e6, dict(rope_type="linear", factor=2.5)),
])
def test_rope_tables_equal_hf_inv_freq_bitwise(D, theta, scaling):
    """BITWISE: host_tables.rope_inv_freq performs HF's operations in HF's order (ROPE_INIT_FUNCTIONS of the installed transformers),
    and the tables are cos / sin of the same fp32 outer product HF's rotary module forms"""
    from slam_llm_amd.host_tables import rope_inv_freq, rope_tables
    want = _hf_inv_freq(D, theta, scaling)
    got = rope_inv_freq(D, theta, scaling)
    assert got.dtype == torch.float32 and torch.equal(got, want)
    T = 300
    cos, sin = rope_tables(T, D, theta, scaling)
    fr = torch.arange(T, dtype=torch.float32)[:, None] * want[None, :]
    assert torch.equal(cos, fr.cos()) and torch.equal(sin, fr.sin())
    # and the independent fp64 restatement the GPU tests use agrees to the rounding of the fp32 power (a few ulp)
    assert torch.allclose(got.double(), inv_freq_restated(D, theta, scaling), rtol=2e-6, atol=0)
    if scaling["rope_type"] == "llama3":
        plain = rope_inv_freq(D, theta, None)
        hi, mid, lo = rope_bands(D, theta, scaling)
        assert torch.equal(got[:hi], plain[:hi]) and torch.equal(got[D // 2 - lo:], plain[D // 2 - lo:] / scaling["factor"])
        assert bool(((got[hi:hi + mid] < plain[hi:hi + mid]) & (got[hi:hi + mid] > plain[hi:hi + mid] / scaling["factor"])).all())


def test_rope_tables_without_scaling_are_bitwise_unchanged():
    from slam_llm_amd.host_tables import rope_tables
    for T, D, theta in ((77, 64, 1e4), (300, 128, 5e5), (33, 128, 1e6)):
        inv = 1.0 / (theta ** (torch.arange(0, D, 2, dtype=torch.float32) / D))     # the expression the tables were built from before
        fr = torch.arange(T, dtype=torch.float32)[:, None] * inv[None, :]
        for sc in (None, {}, dict(rope_type="default")):
            cos, sin = rope_tables(T, D, theta, sc) if sc is not None else rope_tables(T, D, theta)
            assert torch.equal(cos, fr.cos()) and torch.equal(sin, fr.sin())
        o_cos, o_sin = O.rope_tables(T, D, theta)
        assert torch.equal(cos, o_cos[:, : D // 2]) and torch.equal(sin, o_sin[:, : D // 2])
    with pytest.raises(NotImplementedError, match="yarn"):
        rope_tables(8, 64, 1e4, dict(rope_type="yarn", factor=4.0))


def test_hf_names_map_the_qk_norm_weights():
    from slam_llm_amd.slam_model_hip import hf_to_reference_names
    t = torch.zeros(2)
    sd = {"model.embed_tokens.weight": t, "model.layers.0.self_attn.q_norm.weight": t, "model.layers.0.self_attn.k_norm.weight": t,
          "model.layers.0.self_attn.q_proj.weight": t, "model.norm.weight": t}
    assert set(hf_to_reference_names(sd)) == {P + k for k in sd}


@pytest.mark.parametrize("name", list(ALL_CASES))
def test_restatement_reproduces_reference_fixture(name):
    """the fp32 restatement == the reference's slam_model over HF Qwen3ForCausalLM / LlamaForCausalLM (llama3 RoPE): loss, every
    logit, first-step gradients; and the fixture shows that the feature under test moves the loss by far more than the GPU tests'
    loss tolerance (1e-2)"""
    fx = G.load(name)
    case = ALL_CASES[name]
    cfg = case["cfg"]
    W = qwen3_weights(cfg, seed=42, norm_scale=case["norm_scale"])
    batch = {k[len("batch."):]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("batch.")}
    names = O.trainable_names(W)
    for n in names:
        W[n] = W[n].clone().requires_grad_(True)
    loss, logits, acc = slam_qwen3_forward(W, cfg, batch)
    loss.backward()
    assert abs(float(loss) - float(fx["loss.0"])) < 1e-4, (float(loss), float(fx["loss.0"]))
    other = "loss_with_unit_qk_norm" if cfg["llm_qk_norm"] else "loss_with_default_rope"
    far = 10 if cfg["llm_qk_norm"] else 3       # x the GPU tests' 1e-2 (tools/make_golden_qwen3.py asserts the same)
    assert abs(float(fx["loss.0"]) - float(fx[other])) > far * 1e-2, f"the fixture's {other} is too close to its loss"
    if not cfg["llm_qk_norm"]:
        assert min(int(x) for x in fx["rope_bands"]) >= 1
        assert batch["input_ids"].shape[1] >= 1.5 * cfg["rope_scaling"]["original_max_position_embeddings"]
    ref = torch.from_numpy(fx["logits_full"])
    assert tuple(ref.shape) == tuple(logits.shape)
    valid = batch["attention_mask"].bool()
    assert float((logits.detach() - ref)[valid].abs().max()) < 2e-4 + 1e-4 * float(ref[valid].abs().max())
    assert abs(float(acc) - float(fx["acc.0"])) < 1e-6
    assert len(names) == sum(1 for k in fx.files if k.startswith("grad.") and not k.endswith(("__stride", "__norm", "__sum")))
    for n in names:
        g, m = G.sub(fx, "grad." + n, W[n].grad.numpy())
        assert G.cosine(g, m) > 0.99999, (n, G.cosine(g, m))
        assert np.allclose(float(np.sqrt((W[n].grad.double() ** 2).sum())), float(fx["grad." + n + ".__norm"]), rtol=1e-4)

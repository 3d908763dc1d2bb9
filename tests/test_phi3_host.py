"""CPU: Phi-3 / Phi-4 LLMs -- geometry from an HF config.json (fused projections, partial rotary, longrope, sliding window), what is
refused, the longrope / partial-rotary cos/sin tables against the installed transformers bit for bit, the adapter names, the length
guards, and the fp32 restatement (tests/phi3_cases.py) against the fixtures the reference wrote (tools/make_golden_phi3.py)."""
import json
import types

import numpy as np
import pytest
import torch

from oracle import slam_oracle as O
from tests import golden_util as G
from tests.phi3_cases import (CASES, FUSED_FOUR, P, attention_factor_restated, inv_freq_restated, longrope, phi3_tables, phi3_weights,
                              slam_phi3_forward, trainable_names)


def _build_config(peft=None, **mc):
    from slam_llm_amd.slam_model_hip import build_config
    tc = types.SimpleNamespace(use_peft=peft is not None, peft_config=peft)
    return build_config(tc, dict(dict(encoder_name="whisper", encoder_path="large-v3"), **mc))


LONG = dict(rope_type="longrope", short_factor=[1.0 + 0.01 * i for i in range(48)], long_factor=[1.0 + 0.5 * i for i in range(48)])


def _hf_dir(tmp_path, **over):
    """Phi-4-mini's config.json layout at small widths: top-level partial_rotary_factor / rope_theta / original_max, rope_scaling"""
    hc = dict(model_type="phi3", architectures=["Phi3ForCausalLM"], hidden_size=1024, num_hidden_layers=3, num_attention_heads=8,
              num_key_value_heads=2, intermediate_size=2048, vocab_size=512, rms_norm_eps=1e-5, tie_word_embeddings=True,
              partial_rotary_factor=0.75, rope_theta=10000.0, max_position_embeddings=131072, original_max_position_embeddings=4096,
              sliding_window=262144, resid_pdrop=0.0, embd_pdrop=0.0, attention_dropout=0.0,
              rope_scaling=dict(LONG, type="longrope"))
    hc.update(over)
    hc = {k: v for k, v in hc.items() if v is not None}
    (tmp_path / "config.json").write_text(json.dumps(hc))
    return str(tmp_path)


def test_build_config_reads_a_phi3_directory_in_both_spellings(tmp_path):
    old = _build_config(llm_path=_hf_dir(tmp_path))
    new = _build_config(llm_path=_hf_dir(tmp_path, partial_rotary_factor=None, rope_theta=None, rope_scaling=None,
                                         rope_parameters=dict(LONG, rope_theta=10000.0, partial_rotary_factor=0.75,
                                                              original_max_position_embeddings=4096)))
    for cfg in (old, new):
        assert (cfg["llm_dim"], cfg["llm_layers"], cfg["llm_heads"], cfg["llm_kv_heads"], cfg["llm_head_dim"], cfg["llm_ffn"],
                cfg["vocab"]) == (1024, 3, 8, 2, 128, 2048, 512)
        assert cfg["llm_fused_proj"] is True and cfg["llm_rotary_dim"] == 96 and cfg["llm_sliding_window"] == 262144
        assert cfg["tie_embeddings"] and not cfg["llm_qk_norm"] and not cfg["llm_qkv_bias"] and cfg["rope_theta"] == 10000.0
        sc = cfg["rope_scaling"]
        assert sc["rope_type"] == "longrope" and sc["short_factor"] == LONG["short_factor"] and sc["long_factor"] == LONG["long_factor"]
        assert sc["original_max_position_embeddings"] == 4096 and sc["max_position_embeddings"] == 131072
        assert abs(attention_factor_restated(sc) - 1.1902) < 1e-4      # Phi-4-mini's: sqrt(1 + ln 32 / ln 4096)
    assert old == new
    # default RoPE, D = 64 at factor 0.5, an explicit attention_factor / factor, no window
    plain = _build_config(llm_path=_hf_dir(tmp_path, hidden_size=512, partial_rotary_factor=0.5, rope_scaling=None, sliding_window=None))
    assert plain["llm_head_dim"] == 64 and plain["llm_rotary_dim"] == 32 and plain["rope_scaling"] is None and plain["llm_sliding_window"] is None
    full = _build_config(llm_path=_hf_dir(tmp_path, partial_rotary_factor=None, rope_scaling=None))
    assert full["llm_rotary_dim"] == 128 and full["llm_fused_proj"] is True
    lf = dict(LONG, short_factor=LONG["short_factor"] + [2.0] * 16, long_factor=LONG["long_factor"] + [3.0] * 16)
    af = _build_config(llm_path=_hf_dir(tmp_path, partial_rotary_factor=None, rope_scaling=dict(lf, factor=8.0, attention_factor=1.25)))
    assert af["rope_scaling"]["attention_factor"] == 1.25 and af["rope_scaling"]["factor"] == 8.0
    assert "max_position_embeddings" not in af["rope_scaling"]


def test_phi3_refusals(tmp_path):
    with pytest.raises(NotImplementedError, match="head_dim 96"):      # Phi-3-mini: 3072 / 32
        _build_config(llm_path=_hf_dir(tmp_path, hidden_size=768, rope_scaling=None))
    with pytest.raises(NotImplementedError, match="multiple of 16"):   # 128 * 0.4 = 51
        _build_config(llm_path=_hf_dir(tmp_path, partial_rotary_factor=0.4, rope_scaling=None))
    for k in ("resid_pdrop", "embd_pdrop", "attention_dropout"):
        with pytest.raises(NotImplementedError, match=k):
            _build_config(llm_path=_hf_dir(tmp_path, **{k: 0.1}))
    with pytest.raises(ValueError, match="short_factor"):
        _build_config(llm_path=_hf_dir(tmp_path, rope_scaling=dict(type="longrope", long_factor=LONG["long_factor"])))
    with pytest.raises(ValueError, match="long_factor"):
        _build_config(llm_path=_hf_dir(tmp_path, rope_scaling=dict(LONG, long_factor=LONG["long_factor"][:32])))
    with pytest.raises(ValueError, match="original_max_position_embeddings"):
        _build_config(llm_path=_hf_dir(tmp_path, original_max_position_embeddings=None))
    with pytest.raises(NotImplementedError, match="sliding-window"):
        _build_config(llm_path=_hf_dir(tmp_path, model_type="qwen2", use_sliding_window=True, rope_scaling=None))
    with pytest.raises(NotImplementedError, match="yarn"):
        _build_config(llm_path=_hf_dir(tmp_path, rope_scaling=dict(type="yarn", factor=4.0)))


def test_longrope_stays_refused_for_other_model_types(tmp_path):
    for mt in ("llama", "qwen3", "qwen2"):
        with pytest.raises(NotImplementedError, match="longrope"):
            _build_config(llm_path=_hf_dir(tmp_path, model_type=mt, partial_rotary_factor=None, rope_scaling=dict(LONG)))
        with pytest.raises(NotImplementedError, match="longrope"):
            _build_config(llm_path=_hf_dir(tmp_path, model_type=mt, partial_rotary_factor=None, rope_scaling=None,
                                           rope_parameters=dict(rope_type="longrope", factor=4.0, rope_theta=1e6)))
    from slam_llm_amd.host_tables import ROPE_SCALING_TYPES
    assert "longrope" not in ROPE_SCALING_TYPES


def _llm(cfg):
    from slam_llm_amd.model import HipLlamaLora, TrainableStore, make_config
    return HipLlamaLora(dict(make_config(), **cfg), TrainableStore("cpu"), "cpu")


def test_fused_groups_and_adapter_names():
    cfg = CASES["step_phi3_untied"]["cfg"]
    llm = _llm(cfg)
    Hq, Hkv, D, Fd, d, r = cfg["llm_heads"], cfg["llm_kv_heads"], cfg["llm_head_dim"], cfg["llm_ffn"], cfg["llm_dim"], cfg["lora_r"]
    L = llm.layers[0]
    assert L.qkv.parts == [("qkv_proj", (Hq + 2 * Hkv) * D)] and L.gu.parts == [("gate_up_proj", 2 * Fd)]
    assert L.o.parts == [("o_proj", d)] and L.down.parts == [("down_proj", d)]
    shapes = {n: s for n, s, _ in llm.store.entries}
    W = phi3_weights(cfg)
    assert set(shapes) == {n for n in trainable_names(W) if ".lora_" in n}
    for n, s in shapes.items():
        assert tuple(W[n].shape) == s, n
    p = P + "model.layers.1."
    assert shapes[p + "self_attn.qkv_proj.lora_B.default.weight"] == ((Hq + 2 * Hkv) * D, r)
    assert shapes[p + "self_attn.qkv_proj.lora_A.default.weight"] == (r, d)
    assert shapes[p + "mlp.gate_up_proj.lora_B.default.weight"] == (2 * Fd, r)
    assert len(L.qkv.adapters) == 1 and L.qkv.adapters[0]["rows"] == (Hq + 2 * Hkv) * D and len(L.gu.adapters) == 1
    # a config without the new keys keeps the seven separate names
    plain = _llm(dict(lora_targets=("q_proj", "up_proj")))
    assert [n for n, _ in plain.layers[0].qkv.parts] == ["q_proj", "k_proj", "v_proj"]
    assert [n for n, _ in plain.layers[0].gu.parts] == ["gate_proj", "up_proj"] and plain.rot_dim == 64 and plain.window is None


def test_bad_targets_and_qk_norm_with_partial_rotary_are_refused():
    cfg = CASES["step_phi3_tied"]["cfg"]
    for bad in (("q_proj", "v_proj"), ("qkv_proj", "gate_proj"), ("up_proj",)):
        with pytest.raises(ValueError, match=r"valid targets: \['qkv_proj', 'o_proj', 'gate_up_proj', 'down_proj'\]"):
            _llm(dict(cfg, lora_targets=bad))
    for ok in ((), FUSED_FOUR, ("down_proj",)):
        _llm(dict(cfg, lora_targets=ok))
    with pytest.raises(NotImplementedError, match="llm_qk_norm"):
        _llm(dict(cfg, llm_qk_norm=True))
    _llm(dict(cfg, llm_qk_norm=True, llm_rotary_dim=64))      # the whole head: nothing partial about it
    with pytest.raises(NotImplementedError, match="multiple of 16"):
        _llm(dict(cfg, llm_rotary_dim=24))


def test_peft_adapter_directory_uses_the_fused_names(tmp_path):
    from slam_llm_amd.slam_model_hip import PEFT_PREFIX, read_peft_adapter
    ac = dict(peft_type="LORA", r=8, lora_alpha=32, target_modules=["qkv_proj", "gate_up_proj"], lora_dropout=0.0, bias="none")
    (tmp_path / "adapter_config.json").write_text(json.dumps(ac))
    key = "base_model.model.model.layers.0.self_attn.qkv_proj.lora_A.weight"
    torch.save({key: torch.ones(8, 4)}, str(tmp_path / "adapter_model.bin"))
    lora, state = read_peft_adapter(str(tmp_path))
    assert lora["lora_targets"] == ("qkv_proj", "gate_up_proj")
    assert list(state) == [PEFT_PREFIX + "base_model.model.model.layers.0.self_attn.qkv_proj.lora_A.default.weight"]
    assert list(state)[0] == P + "model.layers.0.self_attn.qkv_proj.lora_A.default.weight"


# ------------------------------------------------------------------------------------------------ tables
def _hf_rotary(D, rot, theta, scaling, T):
    """Phi3RotaryEmbedding of the installed transformers over positions arange(T): (inv_freq used, cos, sin) fp32 [T, rot]"""
    from transformers import Phi3Config
    from transformers.models.phi3.modeling_phi3 import Phi3RotaryEmbedding
    rope = dict(rope_type="default", rope_theta=theta, partial_rotary_factor=rot / D)
    extra = dict(max_position_embeddings=4096)
    if scaling:
        rope.update(rope_type="longrope", short_factor=scaling["short_factor"], long_factor=scaling["long_factor"],
                    original_max_position_embeddings=scaling["original_max_position_embeddings"])
        extra = dict(max_position_embeddings=scaling["max_position_embeddings"],
                     original_max_position_embeddings=scaling["original_max_position_embeddings"])
    hc = Phi3Config(hidden_size=2 * D, num_attention_heads=2, num_key_value_heads=2, partial_rotary_factor=rot / D, rope_parameters=rope,
                    pad_token_id=0, vocab_size=32064, **extra)
    emb = Phi3RotaryEmbedding(hc)
    cos, sin = emb(torch.zeros(1, T, 2 * D), torch.arange(T)[None])
    return emb.inv_freq.clone(), cos[0], sin[0], float(emb.attention_scaling)


@pytest.mark.parametrize("D,rot", [(128, 96), (64, 32), (128, 128)])
@pytest.mark.parametrize("kind", ["default", "longrope"])
@pytest.mark.parametrize("T", [100, 300])      # <= and > original_max_position_embeddings = 128
def test_rope_tables_equal_hf_bitwise(D, rot, kind, T):
    """BITWISE against Phi3RotaryEmbedding: the frequencies in use at this length (short_factor up to original_max, long_factor beyond:
    HF's longrope_frequency_update), cos . s and sin . s in fp32 on the first rot/2 columns, exactly 1 and 0 behind them"""
    from slam_llm_amd.host_tables import rope_inv_freq, rope_tables
    sc = longrope(rot) if kind == "longrope" else None
    inv_hf, cos_hf, sin_hf, s_hf = _hf_rotary(D, rot, 10000.0, sc, T)
    inv = rope_inv_freq(rot, 10000.0, sc, seq_len=T)
    assert inv.dtype == torch.float32 and torch.equal(inv, inv_hf)
    if sc:
        other = rope_inv_freq(rot, 10000.0, sc, seq_len=428 - T)
        assert not torch.equal(inv, other), "short and long factors must give different frequencies"
        assert s_hf != 1.0 and abs(s_hf - attention_factor_restated(sc)) < 1e-12
    cos, sin = rope_tables(T, D, 10000.0, sc, rot_dim=None if rot == D else rot)
    assert cos.shape == sin.shape == (T, D // 2) and cos.dtype == torch.float32 and cos.is_contiguous() and sin.is_contiguous()
    assert torch.equal(cos[:, : rot // 2], cos_hf[:, : rot // 2]) and torch.equal(sin[:, : rot // 2], sin_hf[:, : rot // 2])
    fr = torch.arange(T, dtype=torch.float32)[:, None] * inv_hf[None, :]
    assert torch.equal(cos[:, : rot // 2], fr.cos() * s_hf) and torch.equal(sin[:, : rot // 2], fr.sin() * s_hf)
    assert bool((cos[:, rot // 2:] == 1).all()) and bool((sin[:, rot // 2:] == 0).all())
    # the independent fp64 restatement the GPU tests use agrees to the rounding of the fp32 power
    assert torch.allclose(inv.double(), inv_freq_restated(rot, 10000.0, sc, seq_len=T), rtol=2e-6, atol=0)
    rc, rs = phi3_tables(dict(llm_head_dim=D, llm_rotary_dim=rot, rope_theta=10000.0, rope_scaling=sc), T)
    assert torch.allclose(rc[:, : rot // 2], cos[:, : rot // 2], atol=3e-5 * T) and torch.allclose(rs[:, : rot // 2], sin[:, : rot // 2], atol=3e-5 * T)


def test_tables_without_the_new_keys_are_bitwise_unchanged():
    from slam_llm_amd.host_tables import rope_tables
    llama3 = dict(rope_type="llama3", factor=8.0, low_freq_factor=1.0, high_freq_factor=4.0, original_max_position_embeddings=32)
    for T, D, theta in ((77, 64, 1e4), (300, 128, 5e5)):
        inv = 1.0 / (theta ** (torch.arange(0, D, 2, dtype=torch.float32) / D))     # the expression the tables were built from before
        fr = torch.arange(T, dtype=torch.float32)[:, None] * inv[None, :]
        for kw in ({}, dict(rot_dim=None), dict(rot_dim=D)):
            cos, sin = rope_tables(T, D, theta, None, **kw)
            assert torch.equal(cos, fr.cos()) and torch.equal(sin, fr.sin())
        a, b = rope_tables(T, D, theta, llama3), rope_tables(T, D, theta, llama3, rot_dim=None)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not torch.equal(a[0], fr.cos())
    llm = _llm({})
    cos, sin = llm.rope(50)
    o_cos, o_sin = O.rope_tables(50, 64, 10000.0)
    assert torch.equal(cos, o_cos[:, :32]) and torch.equal(sin, o_sin[:, :32])


def test_longrope_factor_lists_must_match_the_rotary_dims():
    from slam_llm_amd.host_tables import rope_tables
    with pytest.raises(ValueError, match="48 values"):
        rope_tables(16, 128, 1e4, longrope(64), rot_dim=96)
    with pytest.raises(NotImplementedError, match="longrope"):       # a dict without factor lists: the type is not a general one
        rope_tables(16, 128, 1e4, dict(rope_type="longrope", factor=4.0))


# ------------------------------------------------------------------------------------------------ guards
def test_window_and_longrope_length_guards():
    cfg = CASES["step_phi3_untied"]["cfg"]     # window 256, original_max 128
    llm = _llm(dict(cfg, llm_sliding_window=40))
    d = cfg["llm_dim"]
    with pytest.raises(NotImplementedError, match="llm_sliding_window=40"):
        llm.forward_hip(torch.zeros(2 * 41, d), 2, 41, None, None, None, False, False)
    with pytest.raises(NotImplementedError, match="llm_sliding_window=40"):   # packed: the longest sequence counts
        llm.forward_hip(torch.zeros(60, d), 1, 60, None, None, None, False, False, packed=(None, None, None, 41))
    with pytest.raises(NotImplementedError, match="llm_sliding_window=40"):
        llm.prefill(torch.zeros(2 * 36, d), 2, 36, torch.ones(2, 36, dtype=torch.int64), 5)
    llm._check_window(40, "x")
    llm = _llm(cfg)
    with pytest.raises(NotImplementedError, match="original_max_position_embeddings=128"):
        llm.prefill(torch.zeros(2 * 120, d), 2, 120, torch.ones(2, 120, dtype=torch.int64), 9)
    llm._check_longrope(128)
    llm._check_window(256, "x")
    _llm(CASES["step_phi3_tied"]["cfg"])._check_longrope(10 ** 6)      # default RoPE: no such limit


# ------------------------------------------------------------------------------------------------ restatement vs the reference
@pytest.mark.parametrize("name", list(CASES))
def test_restatement_reproduces_reference_fixture(name):
    """the fp32 restatement == the reference's slam_model over HF Phi3ForCausalLM with LoRA on the fused Linears: loss, every logit,
    first-step gradients; and the fixture shows that partial rotary (and longrope) move the loss by more than 3x the GPU tests' loss
    tolerance (1e-2) against a whole-head plain RoPE"""
    fx = G.load(name)
    case = CASES[name]
    cfg = case["cfg"]
    W = phi3_weights(cfg, seed=42, norm_scale=case["norm_scale"])
    batch = {k[len("batch."):]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("batch.")}
    names = trainable_names(W)
    assert sorted(O.trainable_names(W)) == names
    for n in names:
        W[n] = W[n].clone().requires_grad_(True)
    loss, logits, acc = slam_phi3_forward(W, cfg, batch)
    loss.backward()
    assert abs(float(loss) - float(fx["loss.0"])) < 1e-4, (float(loss), float(fx["loss.0"]))
    assert abs(float(fx["loss.0"]) - float(fx["loss_with_full_default_rope"])) > 3e-2
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

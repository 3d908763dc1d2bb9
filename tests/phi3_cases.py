"""Phi-3 / Phi-4 case table shared by tools/make_golden_phi3.py and the tests -- TEST INFRASTRUCTURE.

Also holds the fp32 torch restatement of the HF Phi3ForCausalLM decoder under peft: ONE Linear qkv_proj (rows [q; k; v]) and ONE
gate_up_proj (rows [gate; up]), each with one LoRA adapter over all its rows; rotary embedding over the first `rot` dims of a head only
(pairs (i, i + rot/2), dims [rot, D) pass through); the `longrope` frequency rule (1 / (f_i theta^(2i/rot)) with the short or the long
factor list, cos and sin multiplied by the attention factor), written from its definition in fp64 and not from
slam_llm_amd.host_tables.  tests/test_phi3_host.py pins the restatement against the fixtures the reference wrote, so that the GPU
tests can use it at widths no fixture covers."""
import math

import torch
import torch.nn.functional as F

from oracle import slam_oracle as O
from tests.qwen2_cases import P, _lin, head_weight

FUSED_FOUR = ("qkv_proj", "o_proj", "gate_up_proj", "down_proj")
PHI3 = dict(rope_theta=10000.0, rms_eps=1e-5, llm_qkv_bias=False, llm_qk_norm=False, llm_fused_proj=True)


def longrope(rot, original_max=128, max_pos=512):
    """a longrope dict with factor lists that differ from 1 and from each other (both grow with the dim index, as the published ones do);
    max_pos / original_max = 4 gives the attention factor sqrt(1 + ln 4 / ln 128) = 1.134"""
    return dict(rope_type="longrope", short_factor=[1.0 + 0.02 * i for i in range(rot // 2)],
                long_factor=[1.0 + 0.25 * i for i in range(rot // 2)], original_max_position_embeddings=original_max,
                max_position_embeddings=max_pos)


# A random decoder's loss is nearly blind to its attention pattern, so the step cases sharpen the logits through model.norm.weight
# (as tests/qwen3_cases.py does); tools/make_golden_phi3.py asserts that the loss of each case moves by > 3x the tests' loss tolerance
# when the rotary embedding covers the whole head with plain frequencies instead
STEP_NORM_SCALE = 2.0

CASES = {
    # (a) 6 q / 2 kv heads at hd 64, rot 32 (partial_rotary_factor 0.5), default RoPE, tied head, LoRA r8 on qkv_proj + o_proj, left-padded
    "step_phi3_tied": dict(cfg=O.make_config(llm_dim=384, llm_heads=6, llm_kv_heads=2, llm_head_dim=64, llm_ffn=512, vocab=512,
                                             tie_embeddings=True, lora_r=8, lora_alpha=32, lora_targets=("qkv_proj", "o_proj"),
                                             llm_rotary_dim=32, rope_scaling=None, llm_sliding_window=None, **PHI3),
                           clip_seconds=2.0, answer_lens=(5, 9), left_pad=True, norm_scale=STEP_NORM_SCALE),
    # (b) Phi-4-mini structure: 8 q / 2 kv heads at hd 128, rot 96 (0.75), longrope with an attention factor of 1.134, a sliding window
    # above T, untied head, LoRA r16 alpha 16 on all four Linears, 128 mel bins, right-padded
    "step_phi3_untied": dict(cfg=O.make_config(n_mels=128, llm_dim=1024, llm_heads=8, llm_kv_heads=2, llm_head_dim=128, llm_ffn=1024,
                                               vocab=512, tie_embeddings=False, lora_r=16, lora_alpha=16, lora_targets=FUSED_FOUR,
                                               llm_rotary_dim=96, rope_scaling=longrope(96), llm_sliding_window=256, **PHI3),
                             clip_seconds=1.5, answer_lens=(7, 3, 11), left_pad=False, norm_scale=STEP_NORM_SCALE),
}

# worst 1 - cosine of a first-step gradient against the fixture, measured on MI355X (profiles/phi3_margins.md): the GPU test warns (drift
# alarm, never a failure) when a run leaves [0.5, 1.5] x this value; the floor itself is the frozen-LLM family's (golden_util.FLOORS)
EXPECT_GRAD_DEV = {"step_phi3_tied": 1.6e-4, "step_phi3_untied": 2.5e-4}

GENERATE_CASE = dict(norm_scale=6.0, clip_samples=(32000, 22400, 28800), prompt_lens=(6, 4, 7), max_new_tokens=10, pad=0, bos=1)
GEN_RUNS = ((1, 1.0), (4, 1.0))     # (num_beams, length_penalty)
GEN_PADS = ("left", "right")        # O.synth_infer_batch (the speech dataset's collator) and tests/rightpad_cases.rightpad_batch (the multitask one)


def gen_key(case, pad, nb, lp):
    return f"{case}.{pad}.tokens.b{nb}.lp{lp}"


def phi3_weights(cfg, seed=42, norm_scale=1.0):
    """O.init_weights' frozen tensors with q|k|v and gate|up stacked under the Phi3 names, plus one adapter per fused target drawn from a
    generator of its own (lora_B non-zero so that the adapters contribute); a tied config drops lm_head.weight, as the HF checkpoints
    do, and scales the embedding to the head's scale"""
    W = O.init_weights(dict(cfg, lora_targets=()), seed=seed)
    g = torch.Generator().manual_seed(seed + 3)
    r = cfg["lora_r"]
    for i in range(cfg["llm_layers"]):
        p = f"{P}model.layers.{i}."
        W[p + "self_attn.qkv_proj.weight"] = torch.cat([W.pop(p + f"self_attn.{n}.weight") for n in ("q_proj", "k_proj", "v_proj")])
        W[p + "mlp.gate_up_proj.weight"] = torch.cat([W.pop(p + f"mlp.{n}.weight") for n in ("gate_proj", "up_proj")])
        for n in cfg["lora_targets"]:
            base = p + ("mlp." if n in ("gate_up_proj", "down_proj") else "self_attn.") + n
            o, ii = W[base + ".weight"].shape
            W[base + ".lora_A.default.weight"] = torch.randn(r, ii, generator=g) * ii ** -0.5
            W[base + ".lora_B.default.weight"] = torch.randn(o, r, generator=g) * 0.02
    if cfg.get("tie_embeddings"):
        W[P + "model.embed_tokens.weight"] = W[P + "model.embed_tokens.weight"] * cfg["llm_dim"] ** -0.5
        del W[P + "lm_head.weight"]
    W[P + "model.norm.weight"] = W[P + "model.norm.weight"] * norm_scale
    return W


def attention_factor_restated(scaling):
    if not scaling or scaling.get("rope_type") != "longrope":
        return 1.0
    if scaling.get("attention_factor") is not None:
        return float(scaling["attention_factor"])
    orig = scaling["original_max_position_embeddings"]
    f = scaling["factor"] if scaling.get("factor") is not None else scaling["max_position_embeddings"] / orig
    return 1.0 if f <= 1.0 else math.sqrt(1.0 + math.log(f) / math.log(orig))


def inv_freq_restated(rot, theta, scaling=None, seq_len=0):
    """theta^(-2i/rot), i < rot/2, in fp64; longrope divides frequency i by short_factor[i], or by long_factor[i] once the sequence is
    longer than original_max_position_embeddings"""
    f = 1.0 / (float(theta) ** (torch.arange(0, rot, 2, dtype=torch.float64) / rot))
    if scaling and scaling.get("rope_type") == "longrope":
        ext = scaling["long_factor" if seq_len > scaling["original_max_position_embeddings"] else "short_factor"]
        f = f / torch.tensor(ext, dtype=torch.float64)
    return f


def partial_rope(x, cos, sin):
    """HF Phi3 apply_rotary_pos_emb: the first rot = cos.shape[-1] dims of x [..., D] rotate (rotate_half over those rot dims), the rest
    pass through"""
    rot = cos.shape[-1]
    xr, xp = x[..., :rot], x[..., rot:]
    return torch.cat([xr * cos + O._rot_half(xr) * sin, xp], -1)


def phi3_tables(cfg, T, dev="cpu"):
    """cos / sin [T, rot] fp32 (the frequencies repeated over both halves, times the attention factor)"""
    D = cfg["llm_head_dim"]
    rot, sc = int(cfg.get("llm_rotary_dim") or D), cfg.get("rope_scaling")
    inv = inv_freq_restated(rot, cfg["rope_theta"], sc, seq_len=T).float()
    fr = torch.arange(T, dtype=torch.float32)[:, None] * inv[None, :]
    s = attention_factor_restated(sc)
    return (torch.cat([fr, fr], -1).cos() * s).to(dev), (torch.cat([fr, fr], -1).sin() * s).to(dev)


def phi3_forward(W, cfg, inputs_embeds, attention_mask, labels=None, position_ids=None):
    """HF Phi3ForCausalLM(inputs_embeds, attention_mask, labels) in fp32 under peft LoRA on cfg['lora_targets'] (names of the fused
    Linears).  A sliding window that covers the sequence leaves the causal mask as it is (asserted).  Returns (loss, logits)."""
    B, T, d = inputs_embeds.shape
    Hq, Hkv, D, eps, Fd = cfg["llm_heads"], cfg["llm_kv_heads"], cfg["llm_head_dim"], cfg["rms_eps"], cfg["llm_ffn"]
    assert not cfg.get("llm_sliding_window") or T <= cfg["llm_sliding_window"]
    dev = inputs_embeds.device
    cos, sin = phi3_tables(cfg, T, dev)
    if position_ids is not None:
        cos, sin = cos[position_ids][:, None], sin[position_ids][:, None]
    allowed = torch.tril(torch.ones(T, T, dtype=torch.bool, device=dev))[None, None] & attention_mask.bool()[:, None, None, :]
    add_mask = torch.zeros(B, 1, T, T, device=dev).masked_fill(~allowed, torch.finfo(torch.float32).min)
    h = inputs_embeds
    for i in range(cfg["llm_layers"]):
        p = f"{P}model.layers.{i}."
        x = O._rmsnorm(h, W[p + "input_layernorm.weight"], eps)
        qkv = _lin(W, p + "self_attn.qkv_proj", x, cfg)
        q = qkv[..., : Hq * D].view(B, T, Hq, D).transpose(1, 2)
        k = qkv[..., Hq * D: (Hq + Hkv) * D].view(B, T, Hkv, D).transpose(1, 2)
        v = qkv[..., (Hq + Hkv) * D:].view(B, T, Hkv, D).transpose(1, 2)
        q, k = partial_rope(q, cos, sin), partial_rope(k, cos, sin)
        rep = Hq // Hkv
        k = k[:, :, None].expand(B, Hkv, rep, T, D).reshape(B, Hq, T, D)
        v = v[:, :, None].expand(B, Hkv, rep, T, D).reshape(B, Hq, T, D)
        att = F.softmax((q @ k.transpose(2, 3)) * D ** -0.5 + add_mask, dim=-1, dtype=torch.float32)
        h = h + _lin(W, p + "self_attn.o_proj", (att @ v).transpose(1, 2).reshape(B, T, Hq * D), cfg)
        x = O._rmsnorm(h, W[p + "post_attention_layernorm.weight"], eps)
        gu = _lin(W, p + "mlp.gate_up_proj", x, cfg)
        h = h + _lin(W, p + "mlp.down_proj", gu[..., Fd:] * F.silu(gu[..., :Fd]), cfg)
    logits = F.linear(O._rmsnorm(h, W[P + "model.norm.weight"], eps), head_weight(W))
    loss = None
    if labels is not None:
        sl = F.pad(labels, (0, 1), value=-100)[..., 1:].contiguous()
        loss = F.cross_entropy(logits.float().view(-1, logits.shape[-1]), sl.view(-1), ignore_index=-100)
    return loss, logits


def phi3_embeds(W, cfg, batch):
    enc = O.whisper_encoder(W, cfg, batch["audio_mel"].permute(0, 2, 1))
    proj = O.projector_concat(W, enc, cfg["ds_rate"])
    return O.embed_splice(W[P + "model.embed_tokens.weight"], batch["input_ids"].clone(), batch["modality_mask"].bool(), proj)


def slam_phi3_forward(W, cfg, batch):
    """slam_model.forward (whisper + linear projector branch) over the restatement: (loss, logits, acc)"""
    loss, logits = phi3_forward(W, cfg, phi3_embeds(W, cfg, batch), batch["attention_mask"], batch.get("labels"))
    acc = None
    if batch.get("labels") is not None:
        acc = O.compute_accuracy(torch.argmax(logits, -1)[:, :-1], batch["labels"][:, 1:], -100)
    return loss, logits, acc


def trainable_names(W):
    return sorted(k for k in W if k.startswith("encoder_projector.") or ".lora_" in k)

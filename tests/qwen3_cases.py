"""Qwen3 and Llama-3.1 (scaled RoPE) case table shared by tools/make_golden_qwen3.py and the tests -- TEST INFRASTRUCTURE.

Also holds the fp32 torch restatement of the decoder these cases need on top of tests/qwen2_cases.py: HF Qwen3ForCausalLM's per-head
RMSNorm of q and k (q_norm / k_norm over head_dim, behind the projection and its LoRA delta, before RoPE) and the `llama3` / `linear`
RoPE frequency rules, written from their definitions (piecewise, in fp64) and not from slam_llm_amd.host_tables.
tests/test_qwen3_host.py pins the restatement against the fixtures the reference wrote, so that the GPU tests can use it at widths no
fixture covers."""
import math

import torch
import torch.nn.functional as F

from oracle import slam_oracle as O
from tests.qwen2_cases import P, _lin, head_weight

ATTN_FOUR = ("q_proj", "k_proj", "v_proj", "o_proj")
ALL_SEVEN = ATTN_FOUR + ("gate_proj", "up_proj", "down_proj")
QWEN3 = dict(rope_theta=1e6, rms_eps=1e-6, llm_qkv_bias=False, llm_qk_norm=True)
LLAMA3_ROPE = dict(rope_type="llama3", factor=8.0, low_freq_factor=1.0, high_freq_factor=4.0, original_max_position_embeddings=32)

# A random decoder's loss is nearly blind to its attention pattern (flat softmax over a few dozen keys), so the step cases sharpen the
# logits through model.norm.weight (x2) and draw the q_norm / k_norm weights from a seed under which the loss of both geometries
# moves by > 0.15 against unit weights (tools/make_golden_qwen3.py asserts > 10x the tests' loss tolerance)
STEP_NORM_SCALE = 2.0
QK_NORM_SEED_OFFSET = 2026

CASES = {
    # (a) Qwen3-0.6B structure: Hq * D = 384 != hidden_size 192, GQA 6q/2kv at hd 64, tied head, LoRA r8 on q/k/v/o (the adapter
    # gradient of q and k passes through the per-head norm), left-padded batch
    "step_qwen3_tied": dict(cfg=O.make_config(llm_dim=192, llm_heads=6, llm_kv_heads=2, llm_head_dim=64, llm_ffn=512, vocab=512,
                                              tie_embeddings=True, lora_r=8, lora_alpha=32, lora_targets=ATTN_FOUR, **QWEN3),
                            clip_seconds=2.0, answer_lens=(5, 9), left_pad=True, norm_scale=STEP_NORM_SCALE),
    # (b) Qwen3-8B structure: GQA 8q/1kv at hd 128 (Hq * D = 1024 != 512), untied head, LoRA r16 alpha 16, 128 mel bins, right-padded
    "step_qwen3_untied": dict(cfg=O.make_config(n_mels=128, llm_dim=512, llm_heads=8, llm_kv_heads=1, llm_head_dim=128, llm_ffn=1024,
                                                vocab=512, tie_embeddings=False, lora_r=16, lora_alpha=16, lora_targets=ATTN_FOUR,
                                                **QWEN3),
                              clip_seconds=1.5, answer_lens=(7, 3, 11), left_pad=False, norm_scale=STEP_NORM_SCALE),
}
# Llama-3.1 RoPE: the toy Llama geometry with the llama3 rule at original_max_position_embeddings = 32; 4 s clips give T ~ 55, and with
# theta 1e4 / hd 64 the wavelengths 2 pi theta^(2i/D) fall in all three bands (i = 0 unchanged, 1..5 interpolated, the rest / factor)
LLAMA31_CASE = dict(cfg=O.make_config(tie_embeddings=False, llm_qkv_bias=False, llm_qk_norm=False, rope_scaling=dict(LLAMA3_ROPE)),
                    clip_seconds=4.0, answer_lens=(5, 9), left_pad=True, norm_scale=1.0)
LLAMA31_NAME = "step_llama31_rope"
NORM_STD = 0.3      # q_norm / k_norm weights are 1 + NORM_STD * N(0, 1): far enough from 1 to move the loss visibly

GENERATE_CASE = dict(norm_scale=6.0, clip_samples=(32000, 22400, 28800), prompt_lens=(6, 4, 7), max_new_tokens=10, pad=0, bos=1)
GEN_RUNS = ((1, 1.0), (4, 1.0))     # (num_beams, length_penalty)


def gen_key(case, nb, lp):
    return f"{case}.tokens.b{nb}.lp{lp}"


def qwen3_weights(cfg, seed=42, norm_scale=1.0, unit_qk_norm=False):
    """O.init_weights plus q_norm / k_norm per layer when cfg['llm_qk_norm'] (drawn from their own generator; unit_qk_norm=True: all
    ones, the comparison run of the fixture); a tied config drops lm_head.weight, as the HF checkpoints do, and scales the embedding
    to the head's scale (logits stay O(1))"""
    W = O.init_weights(cfg, seed=seed)
    g = torch.Generator().manual_seed(seed + QK_NORM_SEED_OFFSET)
    D = cfg["llm_head_dim"]
    if cfg.get("llm_qk_norm"):
        for i in range(cfg["llm_layers"]):
            p = f"{P}model.layers.{i}.self_attn."
            for n in ("k_norm", "q_norm"):
                w = 1 + NORM_STD * torch.randn(D, generator=g)
                W[p + n + ".weight"] = torch.ones(D) if unit_qk_norm else w
    if cfg.get("tie_embeddings"):
        W[P + "model.embed_tokens.weight"] = W[P + "model.embed_tokens.weight"] * cfg["llm_dim"] ** -0.5
        del W[P + "lm_head.weight"]
    W[P + "model.norm.weight"] = W[P + "model.norm.weight"] * norm_scale
    return W


def inv_freq_restated(D, theta, scaling=None):
    """theta^(-2i/D) under the `linear` / `llama3` rules, from their definitions in fp64: linear divides every frequency by factor;
    llama3 keeps wavelengths below L / high_freq_factor, divides those above L / low_freq_factor by factor, and in between blends
    (1 - s) f / factor + s f with s = (L / wavelength - low) / (high - low)"""
    f = 1.0 / (float(theta) ** (torch.arange(0, D, 2, dtype=torch.float64) / D))
    kind = (scaling or {}).get("rope_type", "default")
    if kind == "default":
        return f
    if kind == "linear":
        return f / scaling["factor"]
    assert kind == "llama3", kind
    fac, lo, hi, L = scaling["factor"], scaling["low_freq_factor"], scaling["high_freq_factor"], scaling["original_max_position_embeddings"]
    out = []
    for x in f.tolist():
        wl = 2 * math.pi / x
        if wl < L / hi:
            out.append(x)
        elif wl > L / lo:
            out.append(x / fac)
        else:
            s = (L / wl - lo) / (hi - lo)
            out.append((1 - s) * x / fac + s * x)
    return torch.tensor(out, dtype=torch.float64)


def rope_bands(D, theta, scaling):
    """how many of the D/2 frequencies the llama3 rule leaves, interpolates and divides: (unchanged, medium, scaled)"""
    L, lo, hi = scaling["original_max_position_embeddings"], scaling["low_freq_factor"], scaling["high_freq_factor"]
    wl = 2 * math.pi / inv_freq_restated(D, theta)
    high, low = int((wl < L / hi).sum()), int((wl > L / lo).sum())
    return high, D // 2 - high - low, low


def head_rmsnorm(x, w, eps):
    """HF Qwen3RMSNorm over the last dimension (head_dim), fp32"""
    return w * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps))


def qwen3_forward(W, cfg, inputs_embeds, attention_mask, labels=None, position_ids=None):
    """HF Qwen3ForCausalLM / LlamaForCausalLM(inputs_embeds, attention_mask, labels) in fp32 under peft LoRA on cfg['lora_targets']:
    tests/qwen2_cases.qwen2_forward plus the per-head q / k RMSNorm (when the state dict carries q_norm / k_norm) and
    cfg['rope_scaling'].  Returns (loss, logits)."""
    B, T, d = inputs_embeds.shape
    Hq, Hkv, D, eps = cfg["llm_heads"], cfg["llm_kv_heads"], cfg["llm_head_dim"], cfg["rms_eps"]
    dev = inputs_embeds.device     # (runs on the CPU for the fixtures, on the device at true widths)
    inv = inv_freq_restated(D, cfg["rope_theta"], cfg.get("rope_scaling")).float()
    fr = torch.arange(T, dtype=torch.float32)[:, None] * inv[None, :]
    cos, sin = torch.cat([fr, fr], -1).cos().to(dev), torch.cat([fr, fr], -1).sin().to(dev)
    if position_ids is not None:
        cos, sin = cos[position_ids][:, None], sin[position_ids][:, None]
    allowed = torch.tril(torch.ones(T, T, dtype=torch.bool, device=dev))[None, None] & attention_mask.bool()[:, None, None, :]
    add_mask = torch.zeros(B, 1, T, T, device=dev).masked_fill(~allowed, torch.finfo(torch.float32).min)
    h = inputs_embeds
    for i in range(cfg["llm_layers"]):
        p = f"{P}model.layers.{i}."
        x = O._rmsnorm(h, W[p + "input_layernorm.weight"], eps)
        q = _lin(W, p + "self_attn.q_proj", x, cfg).view(B, T, Hq, D).transpose(1, 2)
        k = _lin(W, p + "self_attn.k_proj", x, cfg).view(B, T, Hkv, D).transpose(1, 2)
        v = _lin(W, p + "self_attn.v_proj", x, cfg).view(B, T, Hkv, D).transpose(1, 2)
        if p + "self_attn.q_norm.weight" in W:
            q = head_rmsnorm(q, W[p + "self_attn.q_norm.weight"], eps)
            k = head_rmsnorm(k, W[p + "self_attn.k_norm.weight"], eps)
        q = q * cos + O._rot_half(q) * sin
        k = k * cos + O._rot_half(k) * sin
        rep = Hq // Hkv
        k = k[:, :, None].expand(B, Hkv, rep, T, D).reshape(B, Hq, T, D)
        v = v[:, :, None].expand(B, Hkv, rep, T, D).reshape(B, Hq, T, D)
        att = F.softmax((q @ k.transpose(2, 3)) * D ** -0.5 + add_mask, dim=-1, dtype=torch.float32)
        h = h + _lin(W, p + "self_attn.o_proj", (att @ v).transpose(1, 2).reshape(B, T, Hq * D), cfg)
        x = O._rmsnorm(h, W[p + "post_attention_layernorm.weight"], eps)
        h = h + _lin(W, p + "mlp.down_proj", F.silu(_lin(W, p + "mlp.gate_proj", x, cfg)) * _lin(W, p + "mlp.up_proj", x, cfg), cfg)
    logits = F.linear(O._rmsnorm(h, W[P + "model.norm.weight"], eps), head_weight(W))
    loss = None
    if labels is not None:
        sl = F.pad(labels, (0, 1), value=-100)[..., 1:].contiguous()
        loss = F.cross_entropy(logits.float().view(-1, logits.shape[-1]), sl.view(-1), ignore_index=-100)
    return loss, logits


def qwen3_embeds(W, cfg, batch):
    enc = O.whisper_encoder(W, cfg, batch["audio_mel"].permute(0, 2, 1))
    proj = O.projector_concat(W, enc, cfg["ds_rate"])
    return O.embed_splice(W[P + "model.embed_tokens.weight"], batch["input_ids"].clone(), batch["modality_mask"].bool(), proj)


def slam_qwen3_forward(W, cfg, batch):
    """slam_model.forward (whisper + linear projector branch) over the restatement: (loss, logits, acc)"""
    loss, logits = qwen3_forward(W, cfg, qwen3_embeds(W, cfg, batch), batch["attention_mask"], batch.get("labels"))
    acc = None
    if batch.get("labels") is not None:
        acc = O.compute_accuracy(torch.argmax(logits, -1)[:, :-1], batch["labels"][:, 1:], -100)
    return loss, logits, acc

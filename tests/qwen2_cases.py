"""Qwen2 / Qwen2.5 case table shared by tools/make_golden_qwen2.py and the tests -- TEST INFRASTRUCTURE.

Also holds the fp32 torch restatement of the Qwen2 decoder (HF Qwen2ForCausalLM: RMSNorm, q/k/v with bias, rotate-half RoPE,
causal GQA with a key mask, SwiGLU, tied or untied head) under peft LoRA.  tests/test_qwen2_host.py pins it against the fixtures
the reference wrote, so that the GPU tests can use it at widths no fixture covers."""
import torch
import torch.nn.functional as F

from oracle import slam_oracle as O

P = "llm.base_model.model."
ALL_SEVEN = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
QWEN2 = dict(rope_theta=1e6, rms_eps=1e-6, llm_qkv_bias=True)

CASES = {
    # (a) Qwen2-0.5B structure: GQA 7q/1kv at hd 64, tied head, LoRA r8 on q and v, left-padded batch
    "step_qwen2_tied": dict(cfg=O.make_config(llm_dim=448, llm_heads=7, llm_kv_heads=1, llm_head_dim=64, llm_ffn=512, vocab=1024,
                                              tie_embeddings=True, lora_r=8, lora_alpha=32, lora_targets=("q_proj", "v_proj"),
                                              **QWEN2),
                            clip_seconds=2.0, answer_lens=(5, 9), left_pad=True),
    # (b) Qwen2.5-1.5B / 7B structure: GQA 6q/1kv at hd 128, untied head, LoRA r16 alpha 16 on all seven projections (the aispeech
    # recipe's target set), 128 mel bins, right-padded batch
    "step_qwen2_untied": dict(cfg=O.make_config(n_mels=128, llm_dim=768, llm_heads=6, llm_kv_heads=1, llm_head_dim=128, llm_ffn=1024,
                                                vocab=1024, tie_embeddings=False, lora_r=16, lora_alpha=16, lora_targets=ALL_SEVEN,
                                                **QWEN2),
                              clip_seconds=1.5, answer_lens=(7, 3, 11), left_pad=False),
}
BIAS_STD = 0.5      # projections are O(1): a bias of this size moves the loss visibly

# generate: both geometries; the logits are sharpened through model.norm.weight (geometry (a) ties lm_head to the input embedding)
GENERATE_CASE = dict(norm_scale=6.0, clip_samples=(32000, 22400, 28800), prompt_lens=(6, 4, 7), max_new_tokens=10, pad=0, bos=1)
GEN_RUNS = ((1, 1.0), (4, 1.0))     # (num_beams, length_penalty)


def gen_key(case, nb, lp):
    return f"{case}.tokens.b{nb}.lp{lp}"


def qwen2_weights(cfg, seed=42, norm_scale=1.0):
    """O.init_weights plus a q/k/v bias per layer (drawn from its own generator); a tied config drops lm_head.weight, as the HF
    checkpoints do, and scales the embedding to the head's scale (logits stay O(1))"""
    W = O.init_weights(cfg, seed=seed)
    g = torch.Generator().manual_seed(seed + 1000)
    Hq, Hkv, D = cfg["llm_heads"], cfg["llm_kv_heads"], cfg["llm_head_dim"]
    for i in range(cfg["llm_layers"]):
        p = f"{P}model.layers.{i}.self_attn."
        for n, rows in (("q_proj", Hq * D), ("k_proj", Hkv * D), ("v_proj", Hkv * D)):
            W[p + n + ".bias"] = torch.randn(rows, generator=g) * BIAS_STD
    if cfg.get("tie_embeddings"):
        W[P + "model.embed_tokens.weight"] = W[P + "model.embed_tokens.weight"] * cfg["llm_dim"] ** -0.5
        del W[P + "lm_head.weight"]
    W[P + "model.norm.weight"] = W[P + "model.norm.weight"] * norm_scale
    return W


def head_weight(W):
    return W.get(P + "lm_head.weight", W[P + "model.embed_tokens.weight"])


def _lin(W, name, x, cfg):
    y = O.lora_linear(W, name, x, cfg)
    b = W.get(name + ".bias")
    return y if b is None else y + b


def qwen2_forward(W, cfg, inputs_embeds, attention_mask, labels=None, position_ids=None):
    """HF Qwen2ForCausalLM(inputs_embeds, attention_mask, labels) in fp32 (peft LoRA on cfg['lora_targets']).  Returns (loss, logits)."""
    B, T, d = inputs_embeds.shape
    Hq, Hkv, D, eps = cfg["llm_heads"], cfg["llm_kv_heads"], cfg["llm_head_dim"], cfg["rms_eps"]
    dev = inputs_embeds.device     # (runs on the CPU for the fixtures, on the device at true widths)
    cos, sin = [t.to(dev) for t in O.rope_tables(T, D, cfg["rope_theta"])]
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


def qwen2_embeds(W, cfg, batch):
    enc = O.whisper_encoder(W, cfg, batch["audio_mel"].permute(0, 2, 1))
    proj = O.projector_concat(W, enc, cfg["ds_rate"])
    return O.embed_splice(W[P + "model.embed_tokens.weight"], batch["input_ids"].clone(), batch["modality_mask"].bool(), proj)


def slam_qwen2_forward(W, cfg, batch):
    """slam_model.forward (whisper + linear projector branch) over the Qwen2 restatement: (loss, logits, acc)"""
    loss, logits = qwen2_forward(W, cfg, qwen2_embeds(W, cfg, batch), batch["attention_mask"], batch.get("labels"))
    acc = None
    if batch.get("labels") is not None:
        acc = O.compute_accuracy(torch.argmax(logits, -1)[:, :-1], batch["labels"][:, 1:], -100)
    return loss, logits, acc

"""Small host-side constant tables (built once with torch on CPU, uploaded to HBM by the caller)."""
import math

import torch


def sinusoids(length: int, channels: int, max_timescale: float = 10000.0) -> torch.Tensor:
    """openai-whisper's fixed encoder positional embedding (model.py `sinusoids`), [length, channels] fp32."""
    inc = math.log(max_timescale) / (channels // 2 - 1)
    inv = torch.exp(-inc * torch.arange(channels // 2))
    t = torch.arange(length)[:, None] * inv[None, :]
    return torch.cat([t.sin(), t.cos()], dim=1)


ROPE_SCALING_TYPES = ("default", "llama3", "linear")
LONGROPE = "longrope"     # accepted for model_type phi3 only (slam_model_hip.hf_rope_scaling); never listed among the general types


def rope_scaling_type(scaling) -> str:
    """`rope_type` of an HF rope_scaling / rope_parameters dict (older configs spell the key `type`); None -> "default" """
    if not scaling:
        return "default"
    return str(scaling.get("rope_type", scaling.get("type", "default")) or "default")


def longrope_attention_factor(scaling) -> float:
    """HF _compute_longrope_parameters: the factor cos and sin are multiplied by.  `attention_factor` when the dict carries one, else
    sqrt(1 + ln(factor) / ln(original_max)) with factor = the dict's `factor` or max_position_embeddings / original_max (1 for
    factor <= 1)."""
    af = scaling.get("attention_factor")
    if af is not None:
        return af
    orig = scaling["original_max_position_embeddings"]
    factor = scaling.get("factor")
    if factor is None:
        factor = scaling["max_position_embeddings"] / orig
    return 1.0 if factor <= 1.0 else math.sqrt(1 + math.log(factor) / math.log(orig))


def rope_inv_freq(D: int, theta: float, scaling=None, seq_len=None) -> torch.Tensor:
    """inverse frequencies [D/2] fp32 (D: the rotary dims of a head).  scaling: None, or an HF rope_scaling dict of type
      * `linear` (HF _compute_linear_scaling_rope_parameters): inv_freq / factor;
      * `llama3` (HF _compute_llama3_parameters, Llama-3.1 / 3.2): wavelengths above original_max_position_embeddings / low_freq_factor
        are divided by factor, those below original_max_position_embeddings / high_freq_factor stay, the band between is a smooth
        interpolation of the two;
      * `longrope` (HF _compute_longrope_parameters, Phi-3 / Phi-4; only where the caller accepted it, see LONGROPE): 1 / (f_i theta^(2i/D))
        with f = long_factor when seq_len > original_max_position_embeddings, else short_factor.
    The operations and their order are HF's, so the result is bit-identical to the `inv_freq` buffer of the HF rotary module.
    Any other type (yarn, dynamic, ...) raises."""
    kind = rope_scaling_type(scaling)
    if kind == LONGROPE and scaling.get("short_factor") is not None:
        long = bool(seq_len) and seq_len > scaling["original_max_position_embeddings"]
        ext = torch.tensor(scaling["long_factor" if long else "short_factor"], dtype=torch.float32)
        if ext.numel() != D // 2:
            raise ValueError(f"longrope: short_factor / long_factor must hold {D // 2} values (rotary dims / 2), got {ext.numel()}")
        shape = torch.arange(0, D, 2, dtype=torch.int64).float() / D
        return 1.0 / (ext * theta ** shape)
    inv = 1.0 / (theta ** (torch.arange(0, D, 2, dtype=torch.float32) / D))
    if kind == "default":
        return inv
    if kind == "linear":
        return inv / scaling["factor"]
    if kind == "llama3":
        factor, low, high = scaling["factor"], scaling["low_freq_factor"], scaling["high_freq_factor"]
        old_len = scaling["original_max_position_embeddings"]
        low_wavelen, high_wavelen = old_len / low, old_len / high
        wavelen = 2 * math.pi / inv
        inv_l = torch.where(wavelen > low_wavelen, inv / factor, inv)
        smooth = (old_len / wavelen - low) / (high - low)
        smoothed = (1 - smooth) * inv_l / factor + smooth * inv_l
        medium = ~(wavelen < high_wavelen) * ~(wavelen > low_wavelen)
        return torch.where(medium, smoothed, inv_l)
    raise NotImplementedError(f"rope_scaling type {kind!r} is not implemented (the RoPE tables cover {list(ROPE_SCALING_TYPES)})")


def rope_tables(T: int, D: int, theta: float, scaling=None, rot_dim=None):
    """HF LlamaRotaryEmbedding: cos/sin of pos * inv_freq, [T, D/2] fp32 each (inv_freq = theta^(-2i/D), rescaled by `scaling`, see
    rope_inv_freq; the attention factor of llama3 / linear is 1); positions are arange(T) for every row because the reference never
    passes position_ids.
    rot_dim < D (HF partial_rotary_factor, Phi-3 / Phi-4): the frequencies are those of a rot_dim-wide head and fill columns
    [0, rot_dim/2); columns [rot_dim/2, D/2) hold cos = 1, sin = 0, under which the kernels' rotation returns a pair unchanged.
    longrope: a table of length T takes long_factor iff T > original_max_position_embeddings, and cos / sin are multiplied by the
    attention factor in fp32, as Phi3RotaryEmbedding.forward does."""
    rot = D if rot_dim is None else int(rot_dim)
    if not scaling:
        inv = 1.0 / (theta ** (torch.arange(0, rot, 2, dtype=torch.float32) / rot))
    else:
        inv = rope_inv_freq(rot, theta, scaling, seq_len=T)
    fr = torch.arange(T, dtype=torch.float32)[:, None] * inv[None, :]
    cos, sin = fr.cos(), fr.sin()
    if rope_scaling_type(scaling) == LONGROPE:
        s = longrope_attention_factor(scaling)
        cos, sin = cos * s, sin * s
    if rot < D:
        cos = torch.cat([cos, torch.ones(T, (D - rot) // 2)], 1)
        sin = torch.cat([sin, torch.zeros(T, (D - rot) // 2)], 1)
    return cos.contiguous(), sin.contiguous()


def wavlm_relative_buckets(T: int, num_buckets: int, max_distance: int) -> torch.Tensor:
    """bucket index of every relative distance k - q in [-(T-1), T-1] (entry i <-> distance i - (T-1)), WavLM's bidirectional
    T5-style bucketing (src/slam_llm/models/wavlm/modules.py:417-442): one half of the buckets per sign, distances below
    num_buckets/4 exact, beyond that log-spaced up to max_distance and clamped to the last bucket.  int64 [2T-1]."""
    import math
    rel = torch.arange(-(T - 1), T)
    half = num_buckets // 2
    exact = half // 2
    a = rel.abs()
    log_part = exact + (torch.log(a.float() / exact) / math.log(max_distance / exact) * (half - exact)).to(torch.long)
    log_part = torch.clamp(log_part, max=half - 1)
    return (rel > 0).to(torch.long) * half + torch.where(a < exact, a, log_part)

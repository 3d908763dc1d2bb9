"""generate() on RIGHT-padded prompt batches: case table and fp32 restatement shared by tools/make_golden_generate_rightpad.py and the
tests -- TEST INFRASTRUCTURE.

The batch is GENERATE_CASE's clips and prompt lengths, collated the way MultiTaskDataset.collator does in inference mode
(O.collate_right_pad: [audio, prompt] at the front of the row, pad ids behind it).  What the reference's slam_model.generate -> HF
generate (transformers 5.x, inputs_embeds prompt) does with such a batch, restated (tests/test_generate_rightpad_host.py pins it against
the tokens the reference wrote):
  prefill positions   cumsum(mask) - 1 on real slots, 0 on pad slots; the key mask is the attention mask
  first new token     from the logits of the LAST slot T - 1 (a pad query on a padded row)
  generated token t   position positions[T - 1] + 1 + t; pad slots stay masked as keys; generated keys follow the prompt"""
import torch
import torch.nn.functional as F

from oracle import slam_oracle as O

RUNS = ((1, 1.0, 0), (4, 1.0, 0), (4, 2.0, 1), (3, 0.0, 1))     # (num_beams, length_penalty, pad id): the rp = 1.0 runs of generate.npz
EMB = "llm.base_model.model.model.embed_tokens.weight"


def gen_key(scale, nb, lp, pad):
    return f"s{scale}.tokens.b{nb}.lp{lp}.pad{pad}"


def rightpad_batch(cfg, audio: torch.Tensor, clip_samples, prompt_lens, seed=1237, pad_id=2) -> dict:
    """O.synth_infer_batch's rows (same clips, same prompt ids), collated with O.collate_right_pad; no labels"""
    g = torch.Generator().manual_seed(seed)
    samples, mels = [], []
    for i in range(audio.shape[0]):
        n = clip_samples[i % len(clip_samples)] // O.HOP * O.HOP
        mel = O.log_mel_spectrogram(audio[i][:n], cfg["n_mels"]).permute(1, 0)
        mels.append(mel)
        alen = ((mel.shape[0] + 1) // 2) // cfg["ds_rate"]
        pids = torch.randint(3, cfg["vocab"], (prompt_lens[i % len(prompt_lens)],), generator=g)
        ids = torch.cat([torch.zeros(alen, dtype=torch.int64), pids])
        samples.append({"input_ids": ids, "labels": torch.full_like(ids, -100), "attention_mask": torch.ones_like(ids).bool(),
                        "audio_length": alen, "prompt_length": len(pids)})
    out = O.collate_right_pad(samples, pad_id=pad_id, mels=mels)
    del out["labels"]
    return out


def rule_positions(mask: torch.Tensor, n_new: int) -> torch.Tensor:
    """position ids [B, T + n_new] of the prompt slots and of n_new generated tokens under the rule above"""
    m = mask.long()
    pos = (m.cumsum(-1) - 1) * m
    new = pos[:, -1:] + 1 + torch.arange(n_new)[None, :]
    return torch.cat([pos, new], dim=1)


def rule_step_fn(W, cfg, embeds: torch.Tensor, mask: torch.Tensor, forward=O.llama_forward, emb_w=None):
    """step_fn(tokens [R, t], src_rows) -> next-token logits [R, V] fp32 for O.greedy_search / O.beam_search and decode.py's loops: the
    full sequence is re-run every step (no KV cache).  `forward` is O.llama_forward or a family's restatement of the same signature."""
    emb_w = W[EMB] if emb_w is None else emb_w
    B = embeds.shape[0]
    mask = mask.long()

    def step_fn(tokens, src_rows):
        R, t = tokens.shape
        item = torch.arange(R) // (R // B)
        x = torch.cat([embeds[item], F.embedding(tokens, emb_w)], dim=1)
        m = torch.cat([mask[item], torch.ones_like(tokens)], dim=1)
        logits = forward(W, cfg, x, m, None, position_ids=rule_positions(mask[item], t))[1]
        return logits[:, -1, :]     # t == 0: slot T - 1, whatever the row's padding

    return step_fn


def rule_embeds(W, cfg, batch):
    enc = O.whisper_encoder(W, cfg, batch["audio_mel"].permute(0, 2, 1))
    proj = O.projector_concat(W, enc, cfg["ds_rate"])
    return O.embed_splice(W[EMB], batch["input_ids"].clone(), batch["modality_mask"].bool(), proj)


def rule_generate(W, cfg, batch, max_new_tokens, num_beams, length_penalty, eos, pad, forward=O.llama_forward):
    step_fn = rule_step_fn(W, cfg, rule_embeds(W, cfg, batch), batch["attention_mask"], forward)
    B = batch["input_ids"].shape[0]
    if num_beams == 1:
        return O.greedy_search(step_fn, B, max_new_tokens, eos, pad, 1)
    return O.beam_search(step_fn, B, num_beams, max_new_tokens, eos, pad, 1, length_penalty)

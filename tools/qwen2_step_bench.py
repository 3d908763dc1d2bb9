"""GPU: one training step of Whisper-large-v3 -> Qwen2.5 (random weights at true widths), LoRA r64 alpha 16 on all seven
projections (the aispeech_asr recipe's target set), 31 x 30 s clips.  Prints one JSON line: ms per step and audio-s/s.
For the decode step at Qwen2.5-7B widths: tools/decode_bench.py --llm qwen2.5-7b."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--llm", default="Qwen2.5-7B-Instruct")
    ap.add_argument("--clips", type=int, default=31)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import bench
    from slam_llm_amd.model import SlamAdamW, SlamHipModel
    from slam_llm_amd.slam_model_hip import build_config
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    peft = dict(peft_method="lora", r=64, lora_alpha=16, lora_dropout=0.05,
                target_modules=["q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj"])
    cfg = build_config(dict(use_peft=True, peft_config=peft, freeze_encoder=True),
                       dict(encoder_name="whisper", encoder_path="large-v3", encoder_projector="linear", llm_name=args.llm))
    model = SlamHipModel(cfg, dev).init_random(42)
    model.train()
    opt = SlamAdamW(model, lr=1e-4)
    batch, _, _ = bench.make_batch(cfg, args.clips, dev, seed=1)

    def step():
        outputs, _ = model(**batch)
        outputs.loss.backward()
        opt.step()
        opt.zero_grad()
        return outputs.loss

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(args.steps):
        loss = step()
    t1.record()
    torch.cuda.synchronize()
    ms = t0.elapsed_time(t1) / args.steps
    print(json.dumps(dict(llm=args.llm, clips=args.clips, clip_s=30.0, lora="r64 a16 all seven", ms_per_step=round(ms, 2),
                          audio_s_per_s=round(args.clips * 30.0 / (ms * 1e-3), 1), loss=float(loss),
                          geometry={k: cfg[k] for k in ("llm_dim", "llm_layers", "llm_heads", "llm_kv_heads", "llm_ffn", "vocab",
                                                        "tie_embeddings")})))


if __name__ == "__main__":
    main()

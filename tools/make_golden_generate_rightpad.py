"""Write tests/golden/generate_rightpad.npz by running the REFERENCE -- TEST INFRASTRUCTURE.

Run once in the authoring environment (`python tools/make_golden_generate_rightpad.py`), where the reference checkout is importable;
the fixture is committed and the tests read only it.  What runs: `slam_llm.models.slam_model.slam_model.generate` imported UNMODIFIED
(through oracle/make_golden.py's build_reference: HF LlamaForCausalLM.generate in fp32, transformers 5.x) on GENERATE_CASE's clips
and prompt lengths, collated on the RIGHT like MultiTaskDataset.collator (O.collate_right_pad; tests/rightpad_cases.py builds the
batch).  Data only: the audio, the batch, the eos id per lm_head scale and the token ids of the greedy / beam runs."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import make_golden as MG  # noqa: E402  (installs the import stubs and puts the reference on the path)
from oracle import slam_oracle as O  # noqa: E402
from oracle.make_golden_cases import GENERATE_CASE as C  # noqa: E402
from tests.rightpad_cases import RUNS, gen_key, rightpad_batch, rule_generate  # noqa: E402


def main():
    cfg = C["cfg"]
    audio = O.synth_audio(len(C["clip_samples"]), 2.0, seed=1234)
    batch = rightpad_batch(cfg, audio, C["clip_samples"], C["prompt_lens"])
    assert not bool(batch["attention_mask"].all()), "the batch must have padded rows"
    fx = {"audio": audio.numpy()}
    for k, v in batch.items():
        fx["batch." + k] = v.numpy()
    for scale in C["lm_head_scales"]:
        W = O.init_weights(cfg, seed=42)
        W["llm.base_model.model.lm_head.weight"] = W["llm.base_model.model.lm_head.weight"] * scale
        model = MG.build_reference(cfg, W)
        model.eval()
        fx[f"s{scale}.weights_sha256"] = np.array(MG.wsum(W))

        def run(eos, nb, lp, pad):
            model.tokenizer = types.SimpleNamespace(bos_token_id=C["bos"], eos_token_id=eos, pad_token_id=pad)
            with torch.no_grad():
                return model.generate(**{k: v.clone() for k, v in batch.items()}, max_new_tokens=C["max_new_tokens"], num_beams=nb,
                                      length_penalty=lp)

        # eos: a token a greedy row emits mid-sequence, so that rows (and beams) finish at different lengths -- and never as any row's
        # FIRST token (whether min_length=1 bans eos at the first step differs between transformers versions for inputs_embeds prompts)
        free = run(cfg["vocab"] - 1, 1, 1.0, C["pad"])
        for eos in dict.fromkeys(free[:, 2:].flatten().tolist()):
            outs = {r: run(eos, *r) for r in RUNS}
            if all(not bool((o[:, 0] == eos).any()) for o in outs.values()) and any(bool((o == eos).any()) for o in outs.values()):
                break
        else:
            raise RuntimeError(f"scale {scale}: no usable eos")
        fx[f"s{scale}.eos"] = np.int64(eos)
        for (nb, lp, pad), out in outs.items():
            mine = rule_generate(W, cfg, {k: v.clone() for k, v in batch.items()}, C["max_new_tokens"], nb, lp, eos, pad)
            old = O.slam_generate(W, cfg, {k: v.clone() for k, v in batch.items()}, max_new_tokens=C["max_new_tokens"], num_beams=nb,
                                  length_penalty=lp, eos=eos, pad=pad)
            same = lambda a: a.shape == out.shape and bool((a == out).all())  # noqa: E731
            print(f"generate right-pad scale={scale} eos={eos} beams={nb} lp={lp} pad={pad}: restated rule matches {same(mine)}, "
                  f"O.slam_generate matches {same(old)}\n{out.numpy()}")
            fx[gen_key(scale, nb, lp, pad)] = out.numpy()
    np.savez_compressed(os.path.join(MG.GOLD, "generate_rightpad.npz"), **fx)
    print("generate_rightpad.npz written")


if __name__ == "__main__":
    main()

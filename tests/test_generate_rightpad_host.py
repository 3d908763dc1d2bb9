"""CPU: generate() on right-padded prompt batches (MultiTaskDataset.collator in inference mode) -- the rule the reference follows,
restated in fp32 (tests/rightpad_cases.py), the product's greedy / beam bookkeeping driven by it, and decode.prompt_spans, against the
tokens the reference's slam_model.generate wrote into tests/golden/generate_rightpad.npz."""
import pytest
import torch

from oracle import slam_oracle as O
from oracle.make_golden_cases import GENERATE_CASE as C
from tests import golden_util as G
from tests import rightpad_cases as RP
from tests.test_oracle_golden import generate_case_weights

SCALES = [24.0, 5.0]


def fixture_batch(fx):
    return {k[len("batch."):]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("batch.")}


def test_fixture_is_the_case_it_names():
    """the stored batch is GENERATE_CASE's clips and prompts collated on the right, two of its three rows padded; four runs per scale"""
    fx = G.load("generate_rightpad")
    batch = fixture_batch(fx)
    want = RP.rightpad_batch(C["cfg"], torch.from_numpy(fx["audio"]), C["clip_samples"], C["prompt_lens"])
    assert set(batch) == set(want)
    for k in want:
        assert torch.equal(batch[k], want[k]), k
    m = batch["attention_mask"].long()
    assert bool((m[:, :-1] >= m[:, 1:]).all()) and int((m[:, -1] == 0).sum()) == 2 and bool(m[:, 0].all())
    for scale in SCALES:
        for run in RP.RUNS:
            assert RP.gen_key(scale, *run) in fx.files


@pytest.mark.parametrize("scale", SCALES)
def test_restated_rule_matches_reference_generate(scale):
    """positions cumsum - 1 / 0 on pads, first logits from slot T - 1, new positions from positions[T - 1] + 1: token for token what the
    reference produced, greedy and beams, on both lm_head scales; O.slam_generate's rule (pad slots at position 1, new tokens at
    n_real + t) does NOT describe the padded rows"""
    fx = G.load("generate_rightpad")
    W, batch, eos = generate_case_weights(scale), fixture_batch(fx), int(fx[f"s{scale}.eos"])
    for nb, lp, pad in RP.RUNS:
        got = RP.rule_generate(W, C["cfg"], {k: v.clone() for k, v in batch.items()}, C["max_new_tokens"], nb, lp, eos, pad)
        want = fx[RP.gen_key(scale, nb, lp, pad)]
        assert tuple(got.shape) == want.shape and (got.numpy() == want).all(), (nb, lp, pad, got, want)
    old = O.slam_generate(W, C["cfg"], {k: v.clone() for k, v in batch.items()}, max_new_tokens=C["max_new_tokens"], num_beams=1,
                          eos=eos, pad=0)
    want = fx[RP.gen_key(scale, 1, 1.0, 0)]
    assert tuple(old.shape) != want.shape or not (old.numpy() == want).all()


@pytest.mark.parametrize("scale", SCALES)
def test_decode_bookkeeping_matches_reference_generate_right_padded(scale):
    """slam_llm_amd/decode.py's greedy and beam loops, driven on the CPU by the restated fp32 step, reproduce the reference's tokens"""
    from slam_llm_amd import decode
    fx = G.load("generate_rightpad")
    W, batch, eos = generate_case_weights(scale), fixture_batch(fx), int(fx[f"s{scale}.eos"])
    step_fn = RP.rule_step_fn(W, C["cfg"], RP.rule_embeds(W, C["cfg"], batch), batch["attention_mask"])
    B = batch["input_ids"].shape[0]
    for nb, lp, pad in RP.RUNS:
        if nb == 1:
            got = decode.greedy_search(step_fn, B, C["max_new_tokens"], eos, pad, 1, "cpu")
        else:
            got = decode.beam_search(step_fn, B, nb, C["max_new_tokens"], eos, pad, 1, lp, "cpu")
        want = fx[RP.gen_key(scale, nb, lp, pad)]
        assert tuple(got.shape) == want.shape and (got.numpy() == want).all(), (nb, lp, pad, got, want)


MASK = torch.tensor([[1, 1, 1, 1, 1, 1],      # unpadded
                     [0, 0, 1, 1, 1, 1],      # left
                     [1, 1, 1, 0, 0, 0],      # right
                     [0, 1, 1, 1, 0, 0],      # both sides
                     [0, 0, 0, 0, 0, 1],      # one token, at the end
                     [1, 0, 0, 0, 0, 0]])     # one token, at the front
POS = [[0, 1, 2, 3, 4, 5], [0, 0, 0, 1, 2, 3], [0, 1, 2, 0, 0, 0], [0, 0, 1, 2, 0, 0], [0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0]]


@pytest.mark.parametrize("dtype", [torch.int64, torch.int32, torch.bool, torch.uint8])
def test_prompt_spans_values(dtype):
    from slam_llm_amd import decode
    ref = decode.prompt_spans(MASK.to(dtype))
    fix = decode.prompt_spans(MASK.to(dtype), fix=True)
    for sp in (ref, fix):
        assert sp.start.tolist() == [0, 2, 0, 1, 5, 0] and sp.end.tolist() == [6, 6, 3, 4, 6, 1]
        assert sp.positions.tolist() == POS
        assert sp.start.dtype == sp.end.dtype == sp.positions.dtype == sp.next_pos.dtype == torch.int32 and sp.first_row.dtype == torch.int64
    # reference: the last slot gives the first logits, new positions continue from ITS position (0 on a pad slot)
    assert ref.first_row.tolist() == [5] * 6 and ref.next_pos.tolist() == [6, 4, 1, 1, 1, 1]
    # fix: the row's last real slot, new positions continue the row
    assert fix.first_row.tolist() == [5, 5, 2, 3, 5, 0] and fix.next_pos.tolist() == [6, 4, 3, 3, 1, 1]
    # rows that end at T (unpadded, left padded) are the same in both modes
    ends = MASK[:, -1].bool()
    assert torch.equal(ref.next_pos[ends], fix.next_pos[ends]) and torch.equal(ref.first_row[ends], fix.first_row[ends])
    # and the reference-mode values are the restatement's
    assert torch.equal(RP.rule_positions(MASK, 3)[:, :6], ref.positions.long())
    assert torch.equal(RP.rule_positions(MASK, 3)[:, 6], ref.next_pos.long())


@pytest.mark.parametrize("fix", [False, True])
def test_prompt_spans_rejects_empty_rows_and_holes(fix):
    from slam_llm_amd import decode
    with pytest.raises(ValueError, match="no real token"):
        decode.prompt_spans(torch.tensor([[1, 1, 1], [0, 0, 0]]), fix=fix)
    for holes in ([1, 0, 1, 1], [0, 1, 0, 1], [1, 1, 0, 1], [1, 0, 0, 1]):
        with pytest.raises(ValueError, match="contiguous"):
            decode.prompt_spans(torch.tensor([[1, 1, 1, 1], holes]), fix=fix)


def test_generate_right_pad_fix_is_a_generate_key_and_a_recipe_switch():
    """the kwarg is consumed by generate() (never forwarded to forward()); ++model_config.generate_right_pad_fix reaches the model's cfg
    and defaults to the reference's behaviour"""
    import types
    from slam_llm_amd import decode
    from slam_llm_amd.slam_model_hip import build_config
    assert "generate_right_pad_fix" in decode.GENERATE_KEYS
    mc = dict(encoder_name="whisper", encoder_path="large-v3", llm_name="vicuna-7b-v1.5")
    tc = types.SimpleNamespace(use_peft=False)
    assert build_config(tc, mc)["generate_right_pad_fix"] is False
    assert build_config(tc, dict(mc, generate_right_pad_fix=True))["generate_right_pad_fix"] is True

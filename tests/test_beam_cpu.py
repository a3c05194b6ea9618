"""CPU side of the beam-search tests: the preconditions under which tests/test_gpu_beam.py may demand equal tokens from the
device path -- the fp64 restatements' own margins on the seeded inputs, the mixed caption lengths of the end-to-end fixture --
and the option plumbing that needs no device."""
import pytest
import torch

import test_gpu_beam as G


@pytest.mark.parametrize("shape", G.STEP_SHAPES)
def test_step_seeds_keep_the_margin(shape):
    want = G.step_restatement(*G.step_inputs(*shape, G.STEP_SEEDS[shape]))
    assert float(want["gap"].min()) >= G.STEP_GAP
    n, W, V = shape
    if W > 1:                                                      # finished beams take part, and some survive
        fin = G.step_inputs(*shape, G.STEP_SEEDS[shape])[2]
        assert fin.any() and not fin.all()


def test_start_and_tie_cases_are_what_they_claim():
    n, W, V, seed = G.START_CASE
    want = G.step_restatement(*G.step_inputs(n, W, V, seed, start=True))
    assert float(want["gap"].min()) >= G.STEP_GAP and int(want["parent"].max()) == 0
    assert all(len(set(row)) == W for row in want["token"].tolist())
    tie = G.step_restatement(*G.tie_inputs())
    assert tie["parent"].tolist() == [[0, 1, 0]] * 4 and float(tie["gap"][:, 1].min()) >= G.STEP_GAP
    assert float(tie["gap"][:, 0].max()) == 0.0 == float(tie["gap"][:, 2].max())


def test_oracle_search_on_the_fixture_has_mixed_lengths_and_wide_margins():
    """the figures the end-to-end comparison rests on: margins against E2E_DELTA, mixed lengths, a penalty that matters, and an
    fp32 evaluation of the same oracle that takes the same tokens and parents"""
    rec, score, margin = G.oracle(0.75)
    assert int((margin < G.E2E_DELTA).sum()) == 0
    assert int(rec["fin"][-1].sum()) == 35
    r0, r1 = G.oracle_rank(rec, score, 0.0), G.oracle_rank(rec, score, 1.0)
    assert sorted(set(r0["lengths"].view(-1).tolist())) == [0, 1, 2, 4, 6]
    assert int(r0["lengths"][:, 0].max()) == 0                      # penalty 0: every best caption is empty
    assert int((r0["order"][:, 0] != r1["order"][:, 0]).sum()) == 8
    assert float(r0["gap"].min()) >= 2.8 and float(r1["gap"].min()) >= 2.29e-2
    rec32, score32, _ = G.oracle_search(G.cpu_inputs(torch.float32), G.E2E_W, 6, 0.75)
    assert torch.equal(rec32["token"], rec["token"]) and torch.equal(rec32["parent"], rec["parent"])
    rec, score, margin = G.oracle(0.25)
    assert int((margin < G.E2E_DELTA).sum()) == 2 == G.E2E_MAX_LOOSE
    r0 = G.oracle_rank(rec, score, 0.0)
    assert {0, 1, 6} <= set(r0["lengths"][:, 0].tolist())
    assert float(r0["gap"].min()) >= 2.7e-3


def test_beam_options_need_no_device():
    from gvl_amd.config import make_opt
    from gvl_amd.CaptioningHead import build_captioner
    opt = make_opt(vocab_size=40, max_caption_len=6, device="cpu")
    assert (opt.beam_size, opt.beam_length_penalty) == (1, 0.0)
    cap = build_captioner(opt).eval()
    with torch.no_grad():
        for bad in (0, 9):
            with pytest.raises(ValueError, match="beam_size"):
                cap.beam_search(None, None, None, bad)
        with pytest.raises(ValueError, match="sample_max"):
            cap.sample(None, None, None, {"beam_size": 2, "sample_max": 0})

"""The capture cache both caption heads share (gvl_amd/CaptioningHead/decoding.py: DecodingHead._decode_graphed) on the GPU: what
tests/test_gpu_transformer_beam.py and tests/test_gpu_transformer_cap.py assert of the Transformer-DSA head's cache, of the LSTM-DSA
head's; and the Transformer-DSA head's decode without a padding mask through it."""
import copy

import pytest
import torch

from test_gpu_beam import cap_setup, raised_end_bias  # noqa: F401  (cap_setup: B = 2, Q = 8, vocabulary 40, T = 6)
from test_gpu_transformer_cap import gpu_head, gpu_inputs

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def same(got, want):
    return all(torch.equal(g_, w_) for g_, w_ in zip(got, want))


def test_lstm_head_capture_cache(cap_setup):  # noqa: F811
    """greedy and beam graphs side by side under one cache, keyed on the beam pair; a replay is the eager result bit for bit; a
    parameter update kills every graph and changes the last element of the key alone"""
    cap, hs, reference, others = cap_setup
    args = (hs, reference, others)
    bump = torch.linspace(-1.0, 1.0, cap.logit.bias.numel(), device=DEV)
    cap.__dict__.pop("_decode_graphs", None)
    with torch.no_grad(), raised_end_bias(cap, 0.25):
        greedy = cap.sample(*args)
        beam = {k: v.clone() for k, v in cap.beam_search(*args, 3, 1.0).items()}
        assert isinstance(greedy[0], torch.Tensor) and greedy[0].shape[1] >= 1
        cap.graph_decode = True
        try:
            assert same(cap.sample(*args), greedy) and len(cap._decode_graphs) == 1
            key0 = next(iter(cap._decode_graphs))
            got = cap.beam_search(*args, 3, 1.0)
            assert len(cap._decode_graphs) == 2 and all(torch.equal(got[k], beam[k]) for k in beam)
            assert same(cap.sample(*args), greedy) and len(cap._decode_graphs) == 2
            got = cap.beam_search(*args, 3, 1.0)
            assert len(cap._decode_graphs) == 2 and all(torch.equal(got[k], beam[k]) for k in beam)
            cap.beam_search(*args, 2, 1.0)
            assert len(cap._decode_graphs) == 3
            cap.logit.bias.add_(bump)
            try:
                seq_g, lp_g = cap.sample(*args)
                assert len(cap._decode_graphs) == 1
                key1 = next(iter(cap._decode_graphs))
                assert key1 != key0 and key1[:-1] == key0[:-1] and key1[-1] != key0[-1]
                cap.graph_decode = False
                seq_e, lp_e = cap.sample(*args)
                assert torch.equal(seq_g, seq_e) and torch.equal(lp_g, lp_e)
                assert not torch.equal(lp_e, greedy[1])                      # the update was seen
            finally:
                cap.logit.bias.sub_(bump)
        finally:
            cap.graph_decode = False
            cap.__dict__.pop("_decode_graphs", None)


def no_mask(others):
    return {**others, "mask_flatten": None}


def test_transformer_head_graph_decode_without_a_padding_mask():
    """mask_flatten = None is part of the key and of the static inputs: the replay is the eager decode bit for bit, for other inputs
    of the same shape too, beside the graph of the masked decode"""
    _, base = gpu_head("a6")
    head = copy.deepcopy(base)
    a, b = gpu_inputs("a6", 1), gpu_inputs("a6", 2)
    eager = [head.sample(i_["hs"], i_["reference"], no_mask(i_["others"])) for i_ in (a, b)]
    masked = head.sample(a["hs"], a["reference"], a["others"])
    with torch.no_grad():
        beam = {k: v.clone() for k, v in head.beam_search(a["hs"], a["reference"], no_mask(a["others"]), 3, 1.0).items()}
    head.graph_decode = True
    for i_, want in zip((a, b, a), eager + eager[:1]):
        assert same(head.sample(i_["hs"], i_["reference"], no_mask(i_["others"])), want)
    assert len(head._decode_graphs) == 1
    assert same(head.sample(a["hs"], a["reference"], a["others"]), masked) and len(head._decode_graphs) == 2
    with torch.no_grad():
        got = head.beam_search(a["hs"], a["reference"], no_mask(a["others"]), 3, 1.0)
    assert len(head._decode_graphs) == 3 and all(torch.equal(got[k], beam[k]) for k in beam)


def test_lstm_head_graph_decode_without_a_padding_mask(cap_setup):  # noqa: F811
    """the shared cache gives the LSTM-DSA head the same: before it, its graphed decode cloned the mask unconditionally"""
    cap, hs, reference, others = cap_setup
    cap.__dict__.pop("_decode_graphs", None)
    with torch.no_grad():
        eager = cap.sample(hs, reference, no_mask(others))
        cap.graph_decode = True
        try:
            for _ in range(2):                                               # a capture, then a replay
                assert same(cap.sample(hs, reference, no_mask(others)), eager)
            assert len(cap._decode_graphs) == 1
        finally:
            cap.graph_decode = False
            cap.__dict__.pop("_decode_graphs", None)

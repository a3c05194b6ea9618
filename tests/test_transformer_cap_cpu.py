"""CPU side of the Transformer-DSA caption head (gvl_amd/CaptioningHead/Transformer_DSA.py): names and shapes against the
reference's (tests/golden/transformer_cap_*.npz), the position table, the dispatch, the refusals, and the host restatement of one
cached attention step (tests/transformer_cap_ref.py) against causal attention in one shot."""
import ast

import pytest
import torch

import transformer_cap_ref as R
from helpers import load, maxerr, t


def build(case, **over):
    from gvl_amd.CaptioningHead import build_captioner
    return build_captioner(R.head_opt(case, **over))


@pytest.mark.parametrize("case", sorted(R.HEAD_CASES))
def test_state_dict_names_shapes_and_position_table(case):
    f = load("transformer_cap_" + case)
    head = build(case)
    sd = head.state_dict()
    names = [str(n) for n in f["param_names"]]
    assert sorted(sd) == names
    for n, s in zip(names, f["param_shapes"]):
        assert tuple(sd[n].shape) == ast.literal_eval(str(s)), n
    assert torch.equal(head.pos_table, t(f["pos_table"]))
    # a reference state dict loads strictly
    head.load_state_dict({n: torch.zeros(ast.literal_eval(str(s))) for n, s in zip(names, f["param_shapes"])}, strict=True)
    layer = head.layers[0]
    assert layer.linear1.out_features == 1024 and layer.cross_attention.im2col_step == 500 and layer.activation is torch.nn.functional.relu
    assert not hasattr(layer.self_attention, "dense")                      # BertSelfAttention has no output projection


def test_no_transformers_import():
    import subprocess
    import sys
    code = ("import sys, transformer_cap_ref as R\nfrom gvl_amd.CaptioningHead import build_captioner\n"
            "build_captioner(R.head_opt('a6'))\nassert 'transformers' not in sys.modules\n")
    assert subprocess.run([sys.executable, "-c", code], env=_env()).returncode == 0


def _env():
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([os.path.dirname(here), here, os.path.join(here, "golden"), env.get("PYTHONPATH", "")])
    return env


def test_build_captioner_dispatch():
    from gvl_amd.CaptioningHead import build_captioner
    from gvl_amd.CaptioningHead.LSTM_DSA import LSTMDSACaptioner
    from gvl_amd.CaptioningHead.Transformer_DSA import TransformerDSACaptioner, TransformerDSACapLayer
    from gvl_amd.config import make_opt
    assert isinstance(build_captioner(make_opt(vocab_size=40, max_caption_len=6)), LSTMDSACaptioner)
    head = build_captioner(make_opt(vocab_size=40, max_caption_len=6, caption_decoder_type="transformer", cap_nheads=8))
    assert isinstance(head, TransformerDSACaptioner) and all(isinstance(l_, TransformerDSACapLayer) for l_ in head.layers)
    assert not hasattr(head, "core")                  # PDVC's one-pass / padded caption paths are for heads with a .core
    with pytest.raises(ValueError, match="light"):
        build_captioner(make_opt(vocab_size=40, max_caption_len=6, caption_decoder_type="light"))


def test_refusals_name_their_switch():
    head = build("a6")
    inp = R.head_inputs("a6")
    with pytest.raises(NotImplementedError, match="temperture"):                        # the reference's own (Transformer_DSA.py:235)
        head.sample(inp["hs"], inp["reference"], inp["others"], {"sample_max": 0})
    with pytest.raises(NotImplementedError, match="beam_size"):
        head.sample(inp["hs"], inp["reference"], inp["others"], {"beam_size": 3})
    with pytest.raises(ValueError, match="enable_pos_emb_for_captioner"):
        build("a6", enable_pos_emb_for_captioner=True)
    with pytest.raises(ValueError, match="input_encoding_size"):
        build("a6", input_encoding_size=64)
    few = build("a6", cap_num_feature_levels=2)
    with pytest.raises(NotImplementedError, match="cap_num_feature_levels"):
        few.sample(inp["hs"], inp["reference"], inp["others"])
    with pytest.raises(NotImplementedError, match="cap_num_feature_levels"):
        few(inp["hs"], inp["reference"], inp["others"], inp["seq"])


def test_build_loss_is_the_reference_formula():
    head = build("a6")
    inp = R.head_inputs("a6")
    V1 = R.HEAD_CASES["a6"]["V"] + 1
    logp = torch.log_softmax(inp["gout"], -1)
    target, mask = inp["seq"][:, 1:], inp["cap_mask"][:, 1:]
    x = logp[:, :-1]
    one_hot = torch.nn.functional.one_hot(target, V1)
    want = -(one_hot[:, :x.shape[1]] * x * mask[:, :x.shape[1], None]).sum(2).sum(1) / (mask.sum(1) + 1e-6)      # Transformer_DSA.py:165-170
    assert maxerr(head.build_loss(logp, target, mask), want) < 1e-6


@pytest.mark.parametrize("n,H,L", [(1, 1, 5), (5, 2, 35), (3, 8, 9)])
def test_cached_step_iterated_equals_causal_attention(n, H, L):
    """the restatement the GPU ops are held to: append, attend 0..t, residual, LayerNorm -- iterated over t it is causal attention"""
    C = 64 * H
    g = torch.Generator().manual_seed(n * 100 + H)
    qkv = torch.randn(n, L, 3 * C, generator=g, dtype=torch.float64)
    x = torch.randn(n, L, C, generator=g, dtype=torch.float64)
    w, b = torch.rand(C, generator=g, dtype=torch.float64) + 0.5, torch.randn(C, generator=g, dtype=torch.float64)
    want = R.full_causal_attention(qkv, x, H, w, b, 1e-5)
    cache = torch.full((2, n, L, C), float("nan"), dtype=torch.float64)
    for t_ in range(L):
        got = R.cached_attention_step(qkv[:, t_], x[:, t_], cache, t_, H, w, b, 1e-5)
        assert maxerr(got, want[:, t_]) < 1e-12, t_
    assert not torch.isnan(cache).any()


def test_attend_step_torch_form_equals_the_restatement():
    """the PyTorch formulation the head falls back to (attend_step_torch) is the restatement, in fp32"""
    from gvl_amd.CaptioningHead.Transformer_DSA import attend_step_torch
    n, H, C, L = 4, 4, 128, 6                                   # D = 32: outside the kernel's domain
    g = torch.Generator().manual_seed(5)
    w, b = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    c32, c64 = torch.zeros(2, n, L, C), torch.zeros(2, n, L, C, dtype=torch.float64)
    for t_ in range(L):
        qkv, x = torch.randn(n, 3 * C, generator=g), torch.randn(n, C, generator=g)
        got = attend_step_torch(qkv, x, c32, t_, H, w, b, 1e-5)
        want = R.cached_attention_step(qkv.double(), x.double(), c64, t_, H, w.double(), b.double(), 1e-5)
        assert maxerr(got, want) < 1e-5
    assert maxerr(c32, c64) == 0.0

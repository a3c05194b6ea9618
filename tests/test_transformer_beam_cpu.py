"""CPU side of the Transformer-DSA head's beam search over its KV cache: the host restatements of
tests/transformer_beam_ref.py -- the lineage update and one attention step read through a lineage table -- against the existing
restatement of a cached step (tests/transformer_cap_ref.py: cached_attention_step) run on a cache that is PHYSICALLY re-ordered by
parent beam after every token; the PyTorch formulation the head uses outside the kernel's domain; and the refusals."""
import pytest
import torch

import transformer_beam_ref as BR
import transformer_cap_ref as R
from helpers import maxerr


def build(case, **over):
    from gvl_amd.CaptioningHead import build_captioner
    return build_captioner(R.head_opt(case, **over))


def test_lineage_update_by_hand():
    lin = torch.tensor([[[0, 1, 9, 9], [1, 0, 9, 9], [2, 2, 9, 9]]], dtype=torch.uint8)         # n = 1, W = 3, P = 4, t = 2
    out = BR.lineage_update(lin, torch.tensor([[2, 0, 0]]), 2)
    assert out.tolist() == [[[2, 2, 2, 9], [0, 1, 0, 9], [0, 1, 0, 9]]]
    first = BR.lineage_update(torch.full((1, 3, 4), 7, dtype=torch.uint8), torch.tensor([[0, 0, 0]]), 0)
    assert first.tolist() == [[[0, 7, 7, 7]] * 3]                                                # t = 0: nothing of lin_in in front


@pytest.mark.parametrize("H", [1, 2])
@pytest.mark.parametrize("W", [1, 3, 8])
def test_lineage_steps_equal_cached_steps_on_a_reordered_cache(W, H):
    """L = 35 tokens of a search with random parents: reading the un-moved cache through the lineages gives what the plain cached
    step gives on a cache whose slots are copied by parent after every token (the copy this scheme removes)"""
    n, L, D = 2, 35, 16
    C, Rw = H * D, n * W
    g = torch.Generator().manual_seed(100 * W + H)
    w, b = torch.rand(C, generator=g, dtype=torch.float64) + 0.5, 0.1 * torch.randn(C, generator=g, dtype=torch.float64)
    cache_a = torch.full((2, Rw, L, C), float("nan"), dtype=torch.float64)
    cache_b = cache_a.clone()
    lin = torch.full((n, W, L), 255, dtype=torch.uint8)                    # (an unwritten byte would index out of the event)
    worst, moved = 0.0, 0
    for t in range(L):
        qkv, x = torch.randn(Rw, 3 * C, generator=g, dtype=torch.float64), torch.randn(Rw, C, generator=g, dtype=torch.float64)
        qkv[:, :C] *= 3.0
        ya = BR.lineage_attention_step(qkv, x, cache_a, lin, t, H, w, b, 1e-5)
        yb = R.cached_attention_step(qkv, x, cache_b, t, H, w, b, 1e-5)
        assert torch.isfinite(ya).all() and torch.isfinite(yb).all()
        worst = max(worst, maxerr(ya, yb))
        parent = torch.randint(0, W, (n, W), generator=g)
        moved += int((parent != torch.arange(W)[None]).sum())
        lin = BR.lineage_update(lin, parent, t)
        cache_b = cache_b[:, (torch.arange(n)[:, None] * W + parent).view(-1)]
    print(f"lineage vs re-ordered cache W={W} H={H}: worst error {worst:.3e}")
    assert worst <= 1e-12
    assert W == 1 or moved > L                                               # the parents were no identity


@pytest.mark.parametrize("W,H,t", [(1, 2, 0), (3, 2, 0), (3, 2, 1), (3, 1, 6), (8, 2, 33)])
def test_torch_formulation_equals_the_restatement(W, H, t):
    from gvl_amd.CaptioningHead.Transformer_DSA import attend_step_beam_torch
    n, P, D = 3, 35, 16
    C, Rw = H * D, n * W
    g = torch.Generator().manual_seed(7 * W + H + t)
    qkv, x = torch.randn(Rw, 3 * C, generator=g), torch.randn(Rw, C, generator=g)
    qkv[:, :C] *= 3.0
    cache = torch.randn(2, Rw, P, C, generator=g)
    cache[:, :, t:] = float("nan")                                          # nothing at or behind t may be read
    lin = BR.random_lineage(n, W, P, seed=t)
    cache[:, ~BR.named_positions(lin, t)] = float("nan")                     # ... nor a position no lineage names
    w, b = torch.rand(C, generator=g) + 0.5, 0.1 * torch.randn(C, generator=g)
    c64 = cache.double().clone()
    want = BR.lineage_attention_step(qkv.double(), x.double(), c64, lin, t, H, w.double(), b.double(), 1e-5)
    c32 = cache.clone()
    got = attend_step_beam_torch(qkv, x, c32, lin, t, H, w, b, 1e-5)
    assert torch.isfinite(got).all()
    assert maxerr(got, want) <= 1e-5
    expect = cache.clone()
    expect[0, :, t] = qkv[:, C:2 * C]
    expect[1, :, t] = qkv[:, 2 * C:]
    assert torch.equal(c32.view(torch.int32), expect.view(torch.int32))      # error 0.0, and written at (slot, t) only
    assert torch.equal(c32.view(torch.int32), c64.float().view(torch.int32))


def test_refusals():
    head = build("a6")
    inp = R.head_inputs("a6")
    args = (inp["hs"], inp["reference"], inp["others"])
    for bad in (0, 9, -1):
        with pytest.raises(ValueError, match="beam_size"):
            head.beam_search(*args, bad)
    with pytest.raises(ValueError, match="beam_size"):
        head.sample(*args, {"beam_size": 9})
    with pytest.raises(ValueError, match="exceeds"):
        build("a6", vocab_size=1).beam_search(*args, 3)
    # a CPU input: the search is built for the device alone -- and says which option asked for it
    with pytest.raises(NotImplementedError, match="beam_size"):
        head.beam_search(*args, 3)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="beam_size"):
        head.sample(*args, {"beam_size": 3})
    with pytest.raises(ValueError, match="sample_max"):
        head.sample(*args, {"beam_size": 3, "sample_max": 0})
    head.defer_trim = True
    with pytest.raises(NotImplementedError, match="defer_trim"):
        head.sample(*args, {"beam_size": 3})

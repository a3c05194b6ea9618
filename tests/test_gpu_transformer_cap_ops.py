"""The two kernels of the Transformer-DSA head's token step (gvl_amd/csrc/gvl_cap_tr.hip: k_capt_embed, k_capt_attend) through
their wrappers (gvl_amd.CaptioningHead.Transformer_DSA.embed_step / attend_step), against the fp64 restatement of
tests/transformer_cap_ref.py on the CPU.  Inputs are drawn in fp32 from fixed seeds and widened, so both sides see the same numbers.

Tolerance (the convention of tests/test_gpu_contrastive_ops.py): every output is held to
    max(FACTOR * err32, 16 * 2**-23 * scale),   FACTOR = 8,
err32 being the deviation of the SAME restatement evaluated in fp32 torch on the CPU and scale the largest magnitude of the fp64
result.  Every comparison prints "RATIO <case> <error / bound>" before it asserts (pytest -s).
"""
import pytest
import torch

import transformer_cap_ref as R
from helpers import path_census

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FACTOR, FLOOR = 8.0, 16 * 2.0 ** -23
POSITIONS = 64                         # the kernel's limit: T + 1 <= 64, so T = 63 is the last position
T_LAST = POSITIONS - 1


def hold(name, got, ref64, ref32):
    got, ref64, ref32 = got.double().cpu(), ref64.double(), ref32.double()
    assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
    assert torch.isfinite(got).all(), f"{name}: not finite"
    err32 = float((ref32 - ref64).abs().max())
    bound = max(FACTOR * err32, FLOOR * float(ref64.abs().max()))
    err = float((got - ref64).abs().max())
    print(f"RATIO {name} {err / bound if bound else 0.0:.3f}   (error {err:.3e}, err32 {err32:.3e}, bound {bound:.3e})")
    assert err <= bound, (name, err, bound)


def attend_case(n, H, t, D=64, positions=POSITIONS, seed=0):
    C = H * D
    g = torch.Generator().manual_seed(1000 * n + 10 * H + t + seed)
    qkv = torch.randn(n, 3 * C, generator=g)
    qkv[:, :C] *= 3.0                                                  # scores of a few units: a softmax that is not flat
    x = torch.randn(n, C, generator=g)
    cache = torch.randn(2, n, positions, C, generator=g)
    cache[:, :, t:] = float("nan")                                     # nothing at or behind t may be read
    w, b = torch.rand(C, generator=g) + 0.5, 0.1 * torch.randn(C, generator=g)
    return qkv, x, cache, w, b


def run_attend(n, H, t, D=64, positions=POSITIONS):
    from gvl_amd.CaptioningHead.Transformer_DSA import attend_step
    qkv, x, cache, w, b = attend_case(n, H, t, D, positions)
    C = H * D
    refs = {}
    for dt in (torch.float64, torch.float32):
        c_ = cache.to(dt).clone()
        refs[dt] = (R.cached_attention_step(qkv.to(dt), x.to(dt), c_, t, H, w.to(dt), b.to(dt), 1e-5), c_)
    dq, dx, dc, dw, db = (a.to(DEV) for a in (qkv, x, cache, w, b))
    keep = (dq.clone(), dx.clone())
    (y, am), tags = path_census(lambda: attend_step(dq, dx, dc, t, H, dw, db, 1e-5, want_amax=True))
    assert torch.equal(dq, keep[0]) and torch.equal(dx, keep[1]), "an input was written"
    name = f"attend/n{n}_H{H}_D{D}_t{t}"
    hold(name, y, refs[torch.float64][0], refs[torch.float32][0])
    assert torch.equal(am.cpu(), y.abs().amax(1).cpu()), name          # the row maxima of the rows as written
    # exactly row t of the cache was written, with k and v as they came: the whole cache, bit for bit (NaN included)
    want = cache.clone()
    want[0, :, t] = qkv[:, C:2 * C]
    want[1, :, t] = qkv[:, 2 * C:]
    assert torch.equal(dc.cpu().view(torch.int32), want.view(torch.int32)), name
    return tags


@pytest.mark.parametrize("t", [0, 1, 31, 32, 33, T_LAST])
@pytest.mark.parametrize("n,H", [(1, 1), (5, 2), (6, 8)])
def test_attend_step_kernel(n, H, t):
    tags = run_attend(n, H, t)
    assert tags["capt_attend"] == 1 and sum(tags.values()) == 1, tags


def test_attend_step_short_cache():
    """a cache of fewer positions than the kernel's limit, at its last one (the row stride of the cache is the positions argument)"""
    tags = run_attend(5, 2, 6, positions=7)
    assert tags["capt_attend"] == 1, tags


@pytest.mark.parametrize("t", [0, 5, 33])
def test_attend_step_fallback_outside_the_kernels_domain(t):
    """D = 32: the PyTorch formulation of the same step on the same cache, same bound, no launch of the kernel"""
    tags = run_attend(5, 4, t, D=32)
    assert tags["capt_attend"] == 0, tags


def test_attend_step_fallback_for_a_long_cache():
    tags = run_attend(3, 2, 70, positions=72)
    assert tags["capt_attend"] == 0, tags


def test_attend_refusals():
    from gvl_amd import _lib
    L = _lib.lib()
    assert L.gvl_capt_attend_applicable(8, 64, 64) == 1 and L.gvl_capt_attend_applicable(9, 64, 64) == 0
    assert L.gvl_capt_attend_applicable(8, 32, 64) == 0 and L.gvl_capt_attend_applicable(8, 64, 65) == 0
    rc = L.gvl_capt_attend_f32(None, 192, None, 64, None, 4, 8, 8, 1, None, None, 1e-5, None, None, None)
    assert rc != 0 and b"0 <= t < positions" in L.gvl_last_error()
    rc = L.gvl_capt_attend_f32(None, 192, None, 64, None, 4, 65, 8, 1, None, None, 1e-5, None, None, None)
    assert rc != 0 and b"positions <= 64" in L.gvl_last_error()


@pytest.mark.parametrize("t", [0, 1, 7, 8])
@pytest.mark.parametrize("n,C", [(1, 64), (5, 128), (6, 512)])
def test_embed_step_kernel(n, C, t):
    """x = embed[it] + pos_table[t]; t = 8 is beyond the table's 8 rows: the embedding alone (Transformer_DSA.py:203-206)"""
    from gvl_amd.CaptioningHead.Transformer_DSA import embed_step, TransformerDSACaptioner
    V1 = 41
    g = torch.Generator().manual_seed(n + C + t)
    emb = torch.randn(V1, C, generator=g)
    pos = TransformerDSACaptioner._get_sin_encoding_table(8, C)[0]
    it = torch.randint(0, V1, (n,), generator=g)
    it[0], it[-1] = V1 - 1, 0
    (x, am), tags = path_census(lambda: embed_step(emb.to(DEV), pos.to(DEV), it.to(DEV), t))
    assert tags["capt_embed"] == 1 and sum(tags.values()) == 1, tags
    x64, am64 = R.embed_ref(emb, pos, it, t)
    x32 = emb[it] + (pos[t] if t < pos.shape[0] else 0.0)
    hold(f"embed/n{n}_C{C}_t{t}", x, x64, x32)
    assert torch.equal(am.cpu(), x.abs().amax(1).cpu())
    if t >= pos.shape[0]:
        assert torch.equal(x.cpu(), emb[it])

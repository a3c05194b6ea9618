"""The two launches of the Transformer-DSA head's beam search through their wrappers:
  * MSDA.beam_step_lineage (gvl_amd/csrc/gvl_beam.hip: k_beam_step_lineage) against MSDA.beam_step on the same inputs -- the
    selection is one body of code, so every record is compared bit for bit -- and its lineage table against the restatement;
  * Transformer_DSA.attend_step_beam (gvl_amd/csrc/gvl_cap_tr.hip: k_capt_attend<true>) against the fp64 restatement of
    tests/transformer_beam_ref.py, under the bound of tests/test_gpu_transformer_cap_ops.py:
        max(8 * err32, 16 * 2**-23 * scale),
    err32 the deviation of the same restatement evaluated in fp32 on the CPU.  Every comparison prints "RATIO <case> <error /
    bound>" before it asserts (pytest -s)."""
import pytest
import torch

import test_gpu_beam as TB
import transformer_beam_ref as BR
from helpers import path_census
from test_gpu_transformer_cap_ops import hold

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENTINEL = 0xEE

# ---------------------------------------------------------------------------------------------------------------------------
# A. the selection with a lineage table
# ---------------------------------------------------------------------------------------------------------------------------
LINEAGE_SHAPES = [(7, 1, 41), (7, 3, 41), (2, 8, 8518)]                                 # (event rows, beams, vocabulary + 1)
LINEAGE_AT = [(64, 0), (64, 1), (64, 31), (64, 63), (7, 6), (35, 33)]                   # (cache positions P, position t)


def odd_table(n, W, P, fill=None, values=None):
    """an (n, W, P) uint8 table on the device that starts 3 bytes into its allocation: no alignment of the table is assumed"""
    flat = torch.empty(n * W * P + 3, dtype=torch.uint8, device=DEV)
    tab = flat[3:].view(n, W, P)
    assert tab.data_ptr() % 4 == 3 and tab.is_contiguous()
    if values is not None:
        tab.copy_(values)
    else:
        tab.fill_(fill)
    return tab


def run_lineage_step(logits, score, fin, lin_in, lin_out, t):
    from gvl_amd import MultiScaleDeformableAttention as MSDA
    n, W, V = logits.shape
    buf = torch.full((n * W, (V + 3) // 4 * 4), 1e30, device=DEV)       # (as test_gpu_beam.run_step: the padding is never read)
    dev_logits = buf[:, :V]
    dev_logits.copy_(logits.view(n * W, V))
    out = dict(score=torch.empty(n, W, device=DEV), fin=torch.empty(n, W, dtype=torch.uint8, device=DEV),
               parent=torch.empty(n, W, dtype=torch.int32, device=DEV), token=torch.empty(n, W, dtype=torch.long, device=DEV),
               logp=torch.empty(n, W, device=DEV), alive=torch.zeros(1, dtype=torch.int32, device=DEV))
    _, tags = path_census(lambda: MSDA.beam_step_lineage(dev_logits, score.to(DEV), fin.to(torch.uint8).to(DEV), lin_in, lin_out, t,
                                                         out["score"], out["fin"], out["parent"], out["token"], out["logp"],
                                                         out["alive"]))
    assert tags["beam_step_lineage"] == 1 and sum(tags.values()) == 1, tags
    return out


@pytest.mark.parametrize("P,t", LINEAGE_AT)
@pytest.mark.parametrize("shape", LINEAGE_SHAPES)
def test_beam_step_lineage_equals_beam_step_and_the_restatement(shape, P, t):
    n, W, V = shape
    logits, score, fin = TB.step_inputs(n, W, V, TB.STEP_SEEDS[shape])
    plain, _, _ = TB.run_step(logits, score, fin, 64, True)
    g = torch.Generator().manual_seed(17 * P + t + W)
    lin_cpu = torch.randint(0, W, (n, W, P), generator=g).to(torch.uint8)
    lin_in, lin_out = odd_table(n, W, P, values=lin_cpu), odd_table(n, W, P, fill=SENTINEL)
    got = run_lineage_step(logits, score, fin, lin_in, lin_out, t)
    for k in ("score", "logp"):                                              # one body of code: the same bits
        assert torch.equal(got[k].view(torch.int32), plain[k].view(torch.int32)), k
    for k in ("fin", "parent", "token", "alive"):
        assert torch.equal(got[k], plain[k]), k
    want = torch.full((n, W, P), SENTINEL, dtype=torch.uint8)
    want[:, :, :t + 1] = BR.lineage_update(lin_cpu, plain["parent"].cpu(), t)[:, :, :t + 1]
    assert torch.equal(lin_out.cpu(), want)                                  # the sentinel survives behind t
    assert torch.equal(lin_in.cpu(), lin_cpu)
    if W > 1 and t > 0:
        assert bool((plain["parent"].cpu() != torch.arange(W)[None]).any())  # the table was re-ordered, not copied


def test_beam_step_lineage_from_the_start_scores():
    """scores (0, -inf, ...) at t = 0: W continuations of beam 0, every lineage starts at slot 0, nothing else is written"""
    n, W, V, seed = TB.START_CASE
    logits, score, fin = TB.step_inputs(n, W, V, seed, start=True)
    lin_out = odd_table(n, W, 6, fill=SENTINEL)
    got = run_lineage_step(logits, score, fin, odd_table(n, W, 6, fill=SENTINEL), lin_out, 0)
    want = TB.step_restatement(logits, score, fin)
    assert torch.equal(got["token"].cpu(), want["token"]) and int(got["parent"].abs().max()) == 0
    assert torch.equal(lin_out.cpu()[:, :, 0], torch.zeros(n, W, dtype=torch.uint8)) and bool((lin_out.cpu()[:, :, 1:] == SENTINEL).all())


def test_beam_step_lineage_argument_errors():
    from gvl_amd import MultiScaleDeformableAttention as MSDA
    logits, score, fin = TB.step_inputs(2, 3, 41, 0)
    z = lambda dt: torch.zeros(2, 3, dtype=dt, device=DEV)           # noqa: E731
    lin = lambda P: torch.zeros(2, 3, P, dtype=torch.uint8, device=DEV)       # noqa: E731

    def call(lin_in, lin_out, t, score_in=None):
        MSDA.beam_step_lineage(logits.view(6, 41).to(DEV), score.to(DEV) if score_in is None else score_in, z(torch.uint8), lin_in,
                               lin_out, t, z(torch.float32), z(torch.uint8), z(torch.int32), z(torch.long), z(torch.float32),
                               torch.zeros(1, dtype=torch.int32, device=DEV))
    same = lin(8)
    with pytest.raises(RuntimeError, match="ping-pong"):
        call(same, same, 3)
    with pytest.raises(RuntimeError, match="0 <= t < P"):
        call(lin(8), lin(8), 8)
    with pytest.raises(RuntimeError, match="P <= 64"):
        call(lin(65), lin(65), 3)
    with pytest.raises(RuntimeError, match="beam width"):
        MSDA.beam_step_lineage(torch.zeros(18, 41, device=DEV), torch.zeros(2, 9, device=DEV), *[None] * 10)
    call(lin(8), lin(8), 7)                                          # the last position is served
    # the library refuses the same on its own (a caller of the C ABI)
    from gvl_amd import _lib
    L = _lib.lib()
    assert L.gvl_beam_step_lineage_f32(None, 44, 2, 3, 41, None, None, None, 65, 3, *[None] * 8) != 0 and b"P <= 64" in L.gvl_last_error()
    assert L.gvl_beam_step_lineage_f32(None, 44, 2, 9, 41, None, None, None, 8, 3, *[None] * 8) != 0 and b"1 <= W <= 8" in L.gvl_last_error()
    assert L.gvl_beam_step_lineage_f32(None, 44, 2, 3, 41, None, None, None, 8, 8, *[None] * 8) != 0 and b"0 <= t < P" in L.gvl_last_error()


# ---------------------------------------------------------------------------------------------------------------------------
# B. the cached attention step through a lineage
# ---------------------------------------------------------------------------------------------------------------------------
N_EVENTS, POSITIONS = 3, 64
ATTEND_T = [0, 1, 4, 5, 31, 32, 33, 63]


def attend_case(W, H, t, P=POSITIONS, D=64):
    C, rows = H * D, N_EVENTS * W
    g = torch.Generator().manual_seed(1000 * W + 10 * H + t)
    qkv = torch.randn(rows, 3 * C, generator=g)
    qkv[:, :C] *= 3.0                                                  # scores of a few units: a softmax that is not flat
    x = torch.randn(rows, C, generator=g)
    cache = torch.randn(2, rows, P, C, generator=g)
    lin = BR.random_lineage(N_EVENTS, W, P, seed=100 * W + t)
    if W > 1:                                                           # what random_lineage promises
        groups = lin[:, :, :P // 4 * 4].view(N_EVENTS, W, P // 4, 4)
        mixed = (groups != groups[..., :1]).any(-1)
        mixed[0, 0] = True
        assert bool(mixed.all()) and bool((lin[0, 0] == 1).all())
    cache[:, :, t:] = float("nan")                                     # nothing at or behind t may be read ...
    cache[:, ~BR.named_positions(lin, t)] = float("nan")               # ... nor a (slot, position) that no lineage names
    w, b = torch.rand(C, generator=g) + 0.5, 0.1 * torch.randn(C, generator=g)
    return qkv, x, cache, lin, w, b


def run_attend_beam(W, H, t, P=POSITIONS, D=64):
    from gvl_amd.CaptioningHead.Transformer_DSA import attend_step_beam
    qkv, x, cache, lin, w, b = attend_case(W, H, t, P, D)
    C = H * D
    refs = {dt: BR.lineage_attention_step(qkv.to(dt), x.to(dt), cache.to(dt).clone(), lin, t, H, w.to(dt), b.to(dt), 1e-5)
            for dt in (torch.float64, torch.float32)}
    dq, dx, dc, dw, db = (a.to(DEV) for a in (qkv, x, cache, w, b))
    dl = odd_table(N_EVENTS, W, P, values=lin)
    keep = (dq.clone(), dx.clone(), dl.clone())
    (y, am), tags = path_census(lambda: attend_step_beam(dq, dx, dc, dl, t, H, dw, db, 1e-5, want_amax=True))
    assert torch.equal(dq, keep[0]) and torch.equal(dx, keep[1]) and torch.equal(dl, keep[2]), "an input was written"
    name = f"attend_beam/W{W}_H{H}_D{D}_P{P}_t{t}"
    hold(name, y, refs[torch.float64], refs[torch.float32])             # (asserts that the result is finite, too)
    assert torch.equal(am.cpu(), y.abs().amax(1).cpu()), name
    # exactly the rows' own position t was written, with k and v as they came: the whole cache, bit for bit (NaN included)
    want = cache.clone()
    want[0, :, t] = qkv[:, C:2 * C]
    want[1, :, t] = qkv[:, 2 * C:]
    assert torch.equal(dc.cpu().view(torch.int32), want.view(torch.int32)), name
    # a second run on the same inputs: the same bits
    dc2 = cache.to(DEV)
    y2, am2 = attend_step_beam(dq, dx, dc2, dl, t, H, dw, db, 1e-5, want_amax=True)
    assert torch.equal(y2, y) and torch.equal(am2, am) and torch.equal(dc2.view(torch.int32), dc.view(torch.int32)), name
    return tags


@pytest.mark.parametrize("t", ATTEND_T)
@pytest.mark.parametrize("W", [1, 3, 8])
@pytest.mark.parametrize("H", [1, 2, 8])
def test_attend_step_beam_kernel(H, W, t):
    tags = run_attend_beam(W, H, t)
    assert tags["capt_attend_beam"] == 1 and sum(tags.values()) == 1, tags


def test_attend_step_beam_short_cache():
    """fewer positions than the kernel's limit, at the last one: the row stride of the cache and of the table is P"""
    tags = run_attend_beam(3, 2, 6, P=7)
    assert tags["capt_attend_beam"] == 1, tags


@pytest.mark.parametrize("t", [0, 5, 33])
def test_attend_step_beam_fallback_outside_the_kernels_domain(t):
    """D = 32: the PyTorch formulation of the same step on the same cache, same bound, no launch of either attention kernel"""
    tags = run_attend_beam(3, 4, t, D=32)
    assert tags["capt_attend_beam"] == 0 and tags["capt_attend"] == 0, tags


@pytest.mark.parametrize("t", [0, 5, 33, 63])
@pytest.mark.parametrize("H", [1, 2, 8])
def test_one_beam_and_a_zero_table_is_the_plain_step_bit_for_bit(H, t):
    from gvl_amd.CaptioningHead.Transformer_DSA import attend_step, attend_step_beam
    n, C = 5, 64 * H
    g = torch.Generator().manual_seed(31 * H + t)
    qkv, x = torch.randn(n, 3 * C, generator=g).to(DEV), torch.randn(n, C, generator=g).to(DEV)
    cache = torch.randn(2, n, POSITIONS, C, generator=g)
    cache[:, :, t:] = float("nan")
    w, b = (torch.rand(C, generator=g) + 0.5).to(DEV), (0.1 * torch.randn(C, generator=g)).to(DEV)
    ca, cb = cache.to(DEV), cache.to(DEV)
    (ya, ama), tags_a = path_census(lambda: attend_step(qkv, x, ca, t, H, w, b, 1e-5, want_amax=True))
    zero = torch.zeros(n, 1, POSITIONS, dtype=torch.uint8, device=DEV)
    (yb, amb), tags_b = path_census(lambda: attend_step_beam(qkv, x, cb, zero, t, H, w, b, 1e-5, want_amax=True))
    assert tags_a["capt_attend"] == 1 and tags_b["capt_attend_beam"] == 1 and tags_b["capt_attend"] == 0
    assert torch.isfinite(ya).all()
    assert torch.equal(ya.view(torch.int32), yb.view(torch.int32)) and torch.equal(ama.view(torch.int32), amb.view(torch.int32))
    assert torch.equal(ca.view(torch.int32), cb.view(torch.int32))


def test_attend_beam_refusals():
    from gvl_amd import _lib
    L = _lib.lib()
    assert L.gvl_capt_attend_beam_applicable(8, 64, 64, 8) == 1 and L.gvl_capt_attend_beam_applicable(8, 64, 64, 9) == 0
    assert L.gvl_capt_attend_beam_applicable(8, 64, 64, 0) == 0 and L.gvl_capt_attend_beam_applicable(9, 64, 64, 3) == 0
    assert L.gvl_capt_attend_beam_applicable(8, 32, 64, 3) == 0 and L.gvl_capt_attend_beam_applicable(8, 64, 65, 3) == 0
    rc = L.gvl_capt_attend_beam_f32(None, 192, None, 64, None, None, 4, 3, 8, 8, 1, None, None, 1e-5, None, None, None)
    assert rc != 0 and b"0 <= t < positions" in L.gvl_last_error()
    rc = L.gvl_capt_attend_beam_f32(None, 192, None, 64, None, None, 4, 9, 8, 3, 1, None, None, 1e-5, None, None, None)
    assert rc != 0 and b"1 <= W <= 8" in L.gvl_last_error()
    rc = L.gvl_capt_attend_beam_f32(None, 192, None, 64, None, None, 4, 3, 8, 3, 1, None, None, 1e-5, None, None, None)
    assert rc != 0 and b"null pointer" in L.gvl_last_error()

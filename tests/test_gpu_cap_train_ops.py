"""The captioner's four training kernels (gvl_amd/csrc/gvl_cap_train.hip: k_cap_train_fwd / _bwd, k_lstm_train_fwd / _bwd), each held
as a separate op against an fp64 restatement of the same operation evaluated with vectorised torch on the CPU, at the edges the
teacher-forced loop of tests/test_gpu_model.py never visits: clipped level ends, a level of length 1, the row clamp at the slab's
end, the compact row form with padded rows, centre-only reference points in the two-component layout, fewer than sixteen samples,
foreign leading dimensions, overwrite / accumulate semantics, contended scatters, the running gate sum, null operands, the second
pass of the cell's capped grid and saturated activations.

Inputs are drawn in fp32 from fixed seeds and widened, so both sides see the same numbers.  tests/test_cap_train_ref_cpu.py checks,
without a GPU, what the comparisons rest on: the restatements against oracle.torch_ref.captioner_step and gradcheck, and for every
seeded attend case that no sample sits within EDGE of a cell edge (an fp32 sample on the other side of an edge than its fp64 twin
has a legitimately different gradient) and that the clipping cases clip a quarter to three quarters of their samples at both ends.

Tolerance: every output is compared with the fp64 result (pre-filled accumulators included) and held to
    max(FACTOR * err32, 16 * 2**-23 * scale),   FACTOR = 8,
err32 being the deviation of the SAME restatement evaluated in fp32 torch on the CPU and scale the largest magnitude of the fp64
result (grad_alpha_b, a sum that is zero in exact arithmetic: scale = sum |d e_k|).  The kernels replace division and tanh by
v_rcp_f32 and __expf at a few ulp each and reorder sums over lanes, wavefronts and atomics: an honest fp32 evaluation of another
association, expected within a small multiple of the first.

Every test prints its figures as "RATIO <case>/<output> <kernel error / bound>" before it asserts (pytest -s).
Measured on the MI355X, the largest over the tests that run the case:

    attend case                    att     alpha   g_att_h     g_off    g_slab     g_ref g_alpha_w g_alpha_b
    grouped                      0.118     0.125     0.113     0.085     0.125     0.070     0.117     0.005
    rd1                          0.123     0.128     0.212     0.144     0.091     0.141     0.116     0.008
    compact                      0.143     0.116     0.160     0.143     0.171     0.320     0.131     0.008
    contention                   0.066     0.091     0.157     0.192     0.052     0.034     0.094     0.011
    few_2x4                      0.087     0.142     0.141     0.164     0.065     0.164     0.122     0.021
    few_1x1                      0.075     0.000     0.000     0.020     0.057     0.028     0.000     0.000
    few_3x5                      0.097     0.123     0.195     0.239     0.094     0.042     0.101     0.043
    few_4x3                      0.094     0.068     0.131     0.125     0.125     0.084     0.126     0.014
    leading_dims                 0.143     0.116     0.160     0.143     0.174     0.320     0.131     0.008
    semantics                    0.118     0.125     0.113     0.085     0.132     0.066     0.123     0.005
    saturation                   0.130     0.125     0.456     0.575     0.103     0.882     0.050     0.064

    cell case                      act         h        c2   d_gates       d_c gates_sum
    cell_3x5                     0.069     0.062     0.055     0.067     0.056         -
    cell_48x512                  0.118     0.115     0.064     0.128     0.096         -
    cell_2049x512                0.131     0.183     0.052     0.155     0.092         -
    cell_3x5_null                    -         -         -     0.135     0.072         -
    cell_48x512_null                 -         -         -     0.141     0.106         -
    cell_2049x512_null               -         -         -     0.144     0.141         -
    cell_3x5_sum                     -         -         -         -         -     0.062
    cell_48x512_sum                  -         -         -         -         -     0.132
    cell_2049x512_sum                -         -         -         -         -     0.120
    cell_3x5_saturated           0.040     0.068     0.045     0.063     0.100         -
    cell_48x512_saturated        0.110     0.123     0.038     0.099     0.115         -

Above one half: saturation g_off 0.575 and g_ref 0.882 (g_att_h 0.456), all at FACTOR = 8, which stays.  In that case e_k lies
100 and more apart inside a row, so the surviving alpha_k are __expf(e_k - m) at arguments of -10 .. -80: __expf is exp2 of the
argument times log2(e) rounded to fp32, a relative error of |argument| * 2**-24 (up to 5e-6) where torch's expf stays within an
ulp, and the 512-term fp32 sum behind e_k enters alpha_k the same way.  k_cap_train_bwd takes d e_k, d x_k and from them grad_off
and grad_ref from that saved alpha (grad_ref multiplied by T_l = 16 and by slab differences of +-60); the excess is 1.7e-6 of
grad_ref's largest entry (14 ulp).  The same outputs sit at 0.03 .. 0.32 in every case with ordinary e_k.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
C = 512
FACTOR = 8.0               # kernel error allowed per fp32-restatement error (module docstring)
FLOOR = 16 * 2.0 ** -23    # ... and never less than 16 ulp of the tensor's largest entry
EDGE = 1e-3                # every seeded sample keeps this distance from a cell edge / a clipping bound, in pixels
SENTINEL = -7.25e11        # fills what a call must not write


# ---------------------------------------------------------------------------------------------------------------------------
# restatements (any floating type; the reference is their fp64 evaluation)
# ---------------------------------------------------------------------------------------------------------------------------
def attend_restatement(slab, lens, ref, off_hs, off_h, att_h, alpha_w, alpha_b, row_video, P):
    """slab (B, S, 2C) = [value | ctx2att(value)], lens the level lengths, ref (n, L, RD), off_hs / off_h (n, L P), att_h (n, C),
    alpha_w (C), alpha_b (1), row_video (n) int64 (negative: padded row) -> att (n, C), alpha (n, L P), e (n, L P) and the
    sampling geometry x (unclamped pixel coordinate), lo / hi (clipped at the level's start / end)"""
    dt = slab.dtype
    n, L, RD = ref.shape
    Cv = slab.shape[-1] // 2
    T = torch.tensor(lens, dtype=dt).repeat_interleave(P)                       # (K) level length of every sample
    start = torch.tensor([sum(lens[:l_]) for l_ in range(L)]).repeat_interleave(P)
    off = off_hs + off_h
    ref0 = ref[:, :, 0].repeat_interleave(P, 1)
    loc = ref0 + off / T
    if RD == 2:
        ref1 = ref[:, :, 1].repeat_interleave(P, 1)
        loc = torch.where(ref1 >= 0, ref0 + off / P * ref1 * 0.5, loc)        # a negative length: centre-only reference point
    x = loc * T - 0.5
    lo = ~(x > 0)
    hi = (x >= T - 1) & ~lo
    # constants on the clipped branches (torch.where on the open interval, not clamp: no gradient at or beyond a bound)
    xc = torch.where(lo, torch.zeros_like(x), torch.where(hi, (T - 1).expand_as(x), x))
    x0 = xc.detach().floor()
    a = (xc - x0).unsqueeze(-1)
    i0 = x0.long()
    i1 = torch.minimum(i0 + 1, (T - 1).long().expand_as(i0))
    valid = row_video >= 0
    b = row_video.clamp(min=0)[:, None]
    clip = (1 - a) * slab[b, start + i0] + a * slab[b, start + i1]             # (n, K, 2C)
    e = (torch.tanh(clip[..., Cv:] + att_h[:, None, :]) * alpha_w).sum(-1) + alpha_b
    alpha = torch.softmax(e, -1) * valid[:, None]
    att = (alpha[..., None] * clip[..., :Cv]).sum(1)
    return att, alpha, e, dict(x=x.detach(), lo=lo, hi=hi, valid=valid)


def cell_restatement(ga, gb, gc, c):
    """gates = ga + gb + gc in the order i, f, g, o -> (act (n, 4H), h', c', gates)"""
    gates = ga + gb + gc
    i, f, g, o = gates.chunk(4, 1)
    act = torch.cat([torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)], 1)
    si, sf, tg, so = act.chunk(4, 1)
    c2 = sf * c + si * tg
    return act, so * torch.tanh(c2), c2, gates


# ---------------------------------------------------------------------------------------------------------------------------
# seeded attend inputs.  The seeds are the ones for which tests/test_cap_train_ref_cpu.py finds the EDGE margin kept (and the
# clipped share / mixed reference forms where the case is about them); no sample is ever excluded to get there.
# ---------------------------------------------------------------------------------------------------------------------------
LEVELS = (16, 8, 4, 2)
ODD_LEVELS = (13, 7, 3, 1)
ATTEND_CASES = {
    # centre range, offset scale: centres in [-0.2, 1.2] put ~40 % of the samples beyond a level's ends, three times wider offsets more
    "grouped": dict(B=2, Q=3, lens=LEVELS, P=4, RD=2, off=1.0, clipping=True),
    "rd1": dict(B=2, Q=3, lens=LEVELS, P=4, RD=1, off=3.0, clipping=True),
    # n = 7 rows over 3 videos, video 1 unused, first and last row padded, every other row a centre-only reference point
    "compact": dict(B=3, n=7, lens=ODD_LEVELS, P=4, RD=2, off=1.0, clipping=True, mixed=True),
    # S = 5: 64 rows scatter into the same five slab rows, and the last level's row pair clamps to S - 1
    "contention": dict(B=1, Q=64, lens=(2, 1, 1, 1), P=4, RD=2, off=1.0),
    "few_2x4": dict(B=2, Q=2, lens=ODD_LEVELS[:2], P=4, RD=2, off=1.0),
    "few_1x1": dict(B=2, Q=2, lens=ODD_LEVELS[:1], P=1, RD=1, off=3.0),
    "few_3x5": dict(B=2, Q=2, lens=ODD_LEVELS[:3], P=5, RD=2, off=1.0),
    "few_4x3": dict(B=2, Q=2, lens=ODD_LEVELS, P=3, RD=1, off=3.0),
    "saturation": dict(B=2, Q=3, lens=LEVELS, P=4, RD=2, off=1.0, saturated=True),
}
FEW = ("few_2x4", "few_1x1", "few_3x5", "few_4x3")
ATTEND_SEEDS = dict({k: 1 for k in ATTEND_CASES}, compact=2, contention=7)


@functools.lru_cache(maxsize=None)
def attend_inputs(name, seed=None):
    """fp32 CPU tensors of a case (never modified): slab, ref (n, L, RD), off_hs, off_h, att_h, alpha_w, alpha_b, row_video, g
    (the gradient of att) and the prefill of the four accumulated outputs"""
    cfg = ATTEND_CASES[name]
    g = torch.Generator().manual_seed(ATTEND_SEEDS[name] if seed is None else seed)
    lens, P, RD, B = cfg["lens"], cfg["P"], cfg["RD"], cfg["B"]
    L, S = len(lens), sum(lens)
    K = L * P
    if "n" in cfg:                                                  # compact form
        n = cfg["n"]
        mid = torch.tensor([2, 0, 2, 0, 0])[torch.randperm(n - 2, generator=g)]
        row_video = torch.cat([torch.tensor([-1]), mid, torch.tensor([-1])])
    else:
        n = B * cfg["Q"]
        row_video = torch.arange(n) // cfg["Q"]
    rnd = lambda *shape: torch.randn(*shape, generator=g)                   # noqa: E731
    uni = lambda lo, hi, *shape: lo + (hi - lo) * torch.rand(*shape, generator=g)   # noqa: E731
    slab = rnd(B, S, 2 * C)
    ref = uni(-0.2, 1.2, n, L, RD)
    if RD == 2:
        ref[..., 1] = uni(0.05, 0.5, n, L)
        if cfg.get("mixed"):
            ref[1::2, :, 1] = -1.0                                  # rows 1, 3, 5: centre only
    off_hs, off_h = cfg["off"] * 0.8 * rnd(n, K), cfg["off"] * 0.6 * rnd(n, K)      # (sum: normal with deviation cfg["off"])
    att_h, alpha_w, alpha_b = rnd(n, C), 0.1 * rnd(C), rnd(1)
    if cfg.get("saturated"):
        # pre-activations of +-30: every slab row's ctx2att half is +-30 by channel; alpha_w wide enough that e spans more than
        # 100 inside a row; whole (row, level) groups pushed 1e6 beyond either end
        slab[..., C:] = 30.0 * (2.0 * (torch.rand(B, S, C, generator=g) < 0.5) - 1.0)
        alpha_w = 4.0 * rnd(C)
        far = torch.rand(n, L, generator=g) < 0.5
        far[0, 0], far[0, 1] = True, False
        sign = 2.0 * (torch.rand(n, K, generator=g) < 0.5) - 1.0
        off_h = torch.where(far.repeat_interleave(P, 1), 1e6 * sign, off_h)
    out = dict(slab=slab, lens=lens, ref=ref, off_hs=off_hs, off_h=off_h, att_h=att_h, alpha_w=alpha_w, alpha_b=alpha_b,
               row_video=row_video, P=P, g=rnd(n, C), grouped=None if "n" in cfg else (B, cfg["Q"]))
    out["prefill"] = dict(g_slab=0.1 * rnd(B, S, 2 * C), g_ref=0.1 * rnd(n, L, RD), g_alpha_w=0.1 * rnd(C), g_alpha_b=0.1 * rnd(1))
    if cfg.get("saturated"):
        out["far"] = far
    return out


def _attend_eval(inp, dt):
    leaf = {k: inp[k].to(dt, copy=True).requires_grad_() for k in ("slab", "ref", "off_h", "att_h", "alpha_w", "alpha_b")}
    att, alpha, e, geo = attend_restatement(leaf["slab"], inp["lens"], leaf["ref"], inp["off_hs"].to(dt), leaf["off_h"],
                                            leaf["att_h"], leaf["alpha_w"], leaf["alpha_b"], inp["row_video"], inp["P"])
    grads = torch.autograd.grad((att * inp["g"].to(dt)).sum(), list(leaf.values()) + [e])
    res = dict(zip(("g_slab", "g_ref", "g_off", "g_att_h", "g_alpha_w", "g_alpha_b", "de"), grads))
    K = alpha.shape[1]
    res.update(att=att.detach(), alpha=F.pad(alpha.detach(), (0, 16 - K)), g_off=F.pad(res["g_off"], (0, 16 - K)),
               e=e.detach(), de_abs=float(res["de"].double().abs().sum()), **geo)
    return res


@functools.lru_cache(maxsize=None)
def attend_reference(name):
    """the case's restatement evaluated in fp64 (the reference) and in fp32 (the measure of what fp32 can give): never modified"""
    inp = attend_inputs(name)
    return _attend_eval(inp, torch.float64), _attend_eval(inp, torch.float32)


# ---------------------------------------------------------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------------------------------------------------------
def ratio(label, got, want64, want32, scale=None):
    """kernel error / bound of one output, printed; want32 is the fp32 evaluation of the same restatement"""
    got, want64, want32 = got.detach().cpu().double(), want64.double(), want32.double()
    assert got.shape == want64.shape, (label, got.shape, want64.shape)
    assert bool(torch.isfinite(got).all()), label + ": not finite"
    err32 = float((want32 - want64).abs().max())
    scale = float(want64.abs().max()) if scale is None else scale
    bound = max(FACTOR * err32, FLOOR * scale)
    err = float((got - want64).abs().max())
    r = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
    print("RATIO %-40s %.3f   (error %.3g, fp32 restatement %.3g, scale %.3g)" % (label, r, err, err32, scale))
    return r


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------------------
# attend: running the kernels
# ---------------------------------------------------------------------------------------------------------------------------
def attend_device(inp):
    lens = inp["lens"]
    d = {k: inp[k].to(DEV) for k in ("slab", "off_hs", "off_h", "att_h", "alpha_w", "alpha_b", "g")}
    d["shapes"] = torch.tensor([[1, T] for T in lens], dtype=torch.long, device=DEV)
    d["lsi"] = torch.tensor([sum(lens[:l_]) for l_ in range(len(lens))], dtype=torch.long, device=DEV)
    if inp["grouped"]:
        d["ref"], d["row_video"] = inp["ref"].view(*inp["grouped"], *inp["ref"].shape[1:]).to(DEV), None
    else:
        d["ref"], d["row_video"] = inp["ref"].to(DEV), inp["row_video"].to(DEV)
    d["L"], d["P"], d["n"] = len(lens), inp["P"], inp["ref"].shape[0]
    return d


def attend_forward(d, att_res=None, alpha_out=None):
    from gvl_amd import MultiScaleDeformableAttention as MSDA
    out = MSDA.cap_attend_train_forward(d["slab"], d["shapes"], d["lsi"], d["ref"], d["off_hs"], d["off_h"], d["att_h"],
                                        d["alpha_w"], d["alpha_b"], d["L"], d["P"], att_res=att_res, alpha_out=alpha_out,
                                        row_video=d["row_video"])
    torch.cuda.synchronize()
    return out


def attend_accumulators(d, inp, prefill):
    if prefill:
        acc = {k: v.to(DEV, copy=True) for k, v in inp["prefill"].items()}
        acc["g_ref"] = acc["g_ref"].view(d["ref"].shape).contiguous()
        return acc
    return dict(g_slab=torch.zeros_like(d["slab"]), g_ref=torch.zeros_like(d["ref"]), g_alpha_w=torch.zeros(C, device=DEV),
                g_alpha_b=torch.zeros(1, device=DEV))


def attend_backward(d, alpha, acc, g_att_h=None, g_off=None, g=None):
    from gvl_amd import MultiScaleDeformableAttention as MSDA
    g_att_h = torch.full((d["n"], C), float("nan"), device=DEV) if g_att_h is None else g_att_h
    g_off = torch.full((d["n"], 16), float("nan"), device=DEV) if g_off is None else g_off
    MSDA.cap_attend_train_backward(d["slab"], d["shapes"], d["lsi"], d["ref"], d["off_hs"], d["off_h"], d["att_h"], d["alpha_w"],
                                   alpha, d["g"] if g is None else g, d["L"], d["P"], acc["g_slab"], g_att_h, g_off, acc["g_ref"],
                                   acc["g_alpha_w"], acc["g_alpha_b"], row_video=d["row_video"])
    torch.cuda.synchronize()
    return g_att_h, g_off


def check_attend(name, prefill=False, label=None, d=None, bufs=None):
    """forward + backward of a case against its reference; the overwritten outputs start as NaN, the accumulated ones at zero
    or at the case's seeded prefill.  bufs: caller-owned views for att_h-side operands (leading-dimension case).
    -> everything the kernels returned"""
    inp = attend_inputs(name)
    w64, w32 = attend_reference(name)
    d = d or attend_device(inp)
    label = label or name
    n = d["n"]
    att, alpha = attend_forward(d, torch.full((n, C), float("nan"), device=DEV), torch.full((n, 16), float("nan"), device=DEV))
    acc = attend_accumulators(d, inp, prefill)
    g_att_h, g_off = attend_backward(d, alpha, acc, **(bufs or {}))
    got = dict(att=att, alpha=alpha, g_att_h=g_att_h, g_off=g_off, **acc)
    rs = {}
    for k in ("att", "alpha", "g_att_h", "g_off"):
        rs[k] = ratio(f"{label}/{k}", got[k], w64[k], w32[k])
    for k in ("g_slab", "g_ref", "g_alpha_w", "g_alpha_b"):
        pre = inp["prefill"][k] if prefill else torch.zeros_like(inp["prefill"][k])
        scale = None
        if k == "g_alpha_b":                                        # zero in exact arithmetic: measured against sum |d e_k|
            scale = w64["de_abs"]
        rs[k] = ratio(f"{label}/{k}", got[k].view(pre.shape), pre.double() + w64[k], pre + w32[k], scale)
    assert max(rs.values()) <= 1.0, {k: round(v, 3) for k, v in rs.items() if v > 1.0}
    K = d["L"] * d["P"]
    assert float(got["alpha"][:, K:].abs().sum()) == 0.0 and float(got["g_off"][:, K:].abs().sum()) == 0.0
    return got


# ---------------------------------------------------------------------------------------------------------------------------
# attend: the cases
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["grouped", "rd1"])
def test_attend_grouped_rows_both_reference_forms(name):
    """(B, Q) row layout, levels (16, 8, 4, 2), reference points with a length and without; a quarter to three quarters of the
    samples clipped at both ends, where the gradient of the offsets and reference points is exactly zero"""
    got = check_attend(name)
    w64 = attend_reference(name)[0]
    clipped = F.pad(w64["lo"] | w64["hi"], (0, 16 - w64["lo"].shape[1]))
    assert float(got["g_off"].cpu()[clipped].abs().sum()) == 0.0


def test_attend_compact_rows_padding_and_mixed_reference_forms():
    """row_video form: 7 rows over 3 videos (one unused), first and last row padded, alternating rows centre-only reference points
    in the two-component layout, levels (13, 7, 3, 1)"""
    name = "compact"
    inp = attend_inputs(name)
    got = check_attend(name, prefill=True)
    pad = (inp["row_video"] < 0).to(DEV)
    assert int(pad.sum()) == 2 and bool(pad[0]) and bool(pad[-1])
    for k in ("att", "alpha", "g_att_h", "g_off"):                  # exactly zero, not small
        assert float(got[k][pad].abs().sum()) == 0.0, k
    pre = {k: v.to(DEV) for k, v in inp["prefill"].items()}
    assert bits_equal(got["g_ref"][pad], pre["g_ref"][pad])         # accumulated outputs: untouched by the padded rows
    assert bits_equal(got["g_slab"][1], pre["g_slab"][1])           # ... and the unused video's slab gradient by everyone
    centre_only = (inp["ref"][:, 0, 1] < 0).to(DEV)
    assert bits_equal(got["g_ref"][centre_only][..., 1], pre["g_ref"][centre_only][..., 1])     # a length that is no length


def test_attend_contention_and_the_slabs_last_row():
    """64 rows of one video scatter into the same five slab rows (levels 2, 1, 1, 1: the last level's upper row clamps to S - 1),
    on top of non-zero accumulator contents"""
    check_attend("contention", prefill=True)


@pytest.mark.parametrize("name", FEW)
def test_attend_fewer_than_sixteen_samples(name):
    """L P in {8, 1, 15, 12}: columns K..15 of alpha and of grad_off are exactly zero (asserted by check_attend)"""
    check_attend(name)


def test_attend_leading_dimensions_and_sentinels():
    """column blocks of (n, 512 + 2048 + 16) matrices exactly as TeacherForcedLoop passes them -- TWO matrices, as there: off_h and
    att_h are blocks of the step's product over h (an input), grad_off and grad_att_h blocks of the step's gradient matrix (an
    output) -- and grad_att_res with a padded row stride: same results, and the columns outside the blocks keep their bits"""
    name = "compact"
    inp = attend_inputs(name)
    d = attend_device(inp)
    n, W = d["n"], C + 2048 + 16
    g_h, dg, gbuf = (torch.full((n, W), SENTINEL, device=DEV), torch.full((n, W), SENTINEL, device=DEV),
                     torch.full((n, C + 8), SENTINEL, device=DEV))
    g_h[:, :C], g_h[:, W - 16:], gbuf[:, :C] = d["att_h"], d["off_h"], d["g"]
    before = g_h.clone()
    d.update(att_h=g_h[:, :C], off_h=g_h[:, W - 16:], g=gbuf[:, :C])
    assert not d["att_h"].is_contiguous() and d["g"].stride(0) == C + 8
    check_attend(name, prefill=True, label="leading_dims", d=d, bufs=dict(g_att_h=dg[:, :C], g_off=dg[:, W - 16:]))
    assert bits_equal(g_h, before)
    assert bits_equal(dg[:, C:W - 16], torch.full((n, 2048), SENTINEL, device=DEV))
    assert bits_equal(gbuf[:, C:], torch.full((n, 8), SENTINEL, device=DEV))


def test_attend_output_semantics():
    """overwritten outputs start as NaN and come back finite and right (check_attend always does that); accumulated outputs
    start at seeded values and come back as prefill + reference"""
    check_attend("grouped", prefill=True, label="semantics")


def test_attend_saturation():
    """pre-activations of +-30 into the tanh, e spanning more than 100 (most alpha underflow), offsets of +-1e6: finite and equal to
    the restatement; the far-clipped samples have exactly zero grad_off and add exactly nothing to grad_ref"""
    name = "saturation"
    inp = attend_inputs(name)
    got = check_attend(name, prefill=True)
    far = inp["far"]
    assert bool(far.any()) and not bool(far.all())
    assert float(got["g_off"].cpu()[far.repeat_interleave(inp["P"], 1)].abs().sum()) == 0.0
    assert bits_equal(got["g_ref"].cpu().view(inp["ref"].shape)[far], inp["prefill"]["g_ref"][far])


def test_attend_repeatability():
    """the forward and the backward's overwritten outputs are pure functions of their inputs, bit for bit (the atomically
    accumulated outputs are not required to be)"""
    inp = attend_inputs("compact")
    d = attend_device(inp)
    a1, a2 = attend_forward(d), attend_forward(d)
    assert bits_equal(a1[0], a2[0]) and bits_equal(a1[1], a2[1])
    b1 = attend_backward(d, a1[1], attend_accumulators(d, inp, True))
    b2 = attend_backward(d, a1[1], attend_accumulators(d, inp, False))
    assert bits_equal(b1[0], b2[0]) and bits_equal(b1[1], b2[1])


def _refusal_cases():
    """(label, message, mutation of the device arguments / output buffers)"""
    def c_500(d, o):
        d["slab"] = d["slab"][..., :1000].contiguous()
        d["att_h"], d["g"] = d["att_h"][:, :500].contiguous(), d["g"][:, :500].contiguous()
        d["alpha_w"] = d["alpha_w"][:500].contiguous()
        o.update(att=o["att"][:, :500].contiguous(), g_att_h=o["g_att_h"][:, :500].contiguous(),
                 g_slab=o["g_slab"][..., :1000].contiguous(), g_alpha_w=o["g_alpha_w"][:500].contiguous())

    def lp_20(d, o):
        d["P"] = 5
        d["off_hs"], d["off_h"] = torch.zeros(d["n"], 20, device=DEV), torch.zeros(d["n"], 20, device=DEV)

    def stride(d, o):
        wide = torch.zeros(d["n"], C + 2, device=DEV)
        wide[:, :C] = d["att_h"]
        d["att_h"] = wide[:, :C]

    def narrow(d, o):
        # sixteen columns at a row stride of twelve floats: passes the wrapper, so the refusal is the library's own
        o["g_off"] = torch.empty(d["n"] * 12 + 4, device=DEV).as_strided((d["n"], 16), (12, 1))

    def unaligned(d, o):
        wide = torch.zeros(d["n"], C + 4, device=DEV)
        wide[:, 1:C + 1] = d["att_h"]
        d["att_h"] = wide[:, 1:C + 1]

    return [("C=500", "unsupported shape", c_500), ("LP=20", "unsupported shape", lp_20),
            ("att_h stride", "leading dimensions", stride), ("grad_off narrow", "leading dimensions", narrow),
            ("att_h alignment", "16-byte aligned", unaligned)]


@pytest.mark.parametrize("case", range(5), ids=[c[0].replace(" ", "_") for c in _refusal_cases()])
def test_attend_refusals_write_nothing(case):
    """outside the kernels' domain the library's error is raised, by the forward and by the backward, and no output is written"""
    label, message, mutate = _refusal_cases()[case]
    inp = attend_inputs("grouped")
    d = attend_device(inp)
    n = d["n"]
    alpha = torch.full((n, 16), 1.0 / 16, device=DEV)
    o = dict(att=torch.empty(n, C, device=DEV), alpha=torch.empty(n, 16, device=DEV), g_att_h=torch.empty(n, C, device=DEV),
             g_off=torch.empty(n, 16, device=DEV), g_slab=torch.empty_like(d["slab"]), g_ref=torch.empty_like(d["ref"]),
             g_alpha_w=torch.empty(C, device=DEV), g_alpha_b=torch.empty(1, device=DEV))
    mutate(d, o)
    whole = lambda v: v if v._base is None else v._base                    # noqa: E731  (the overlapping view: its buffer)
    for v in o.values():
        whole(v).fill_(SENTINEL)
    if label != "grad_off narrow":                                  # (the forward has no grad_off)
        with pytest.raises(RuntimeError, match=message):
            attend_forward(d, o["att"], o["alpha"])
    with pytest.raises(RuntimeError, match=message):
        attend_backward(d, alpha, o, g_att_h=o["g_att_h"], g_off=o["g_off"])
    torch.cuda.synchronize()
    for k, v in o.items():
        assert bits_equal(whole(v), torch.full_like(whole(v), SENTINEL)), k


# ---------------------------------------------------------------------------------------------------------------------------
# LSTM cell
# ---------------------------------------------------------------------------------------------------------------------------
CELL_SIZES = [(3, 5), (48, 512), (2049, 512)]       # 2049 x 512: the smallest round size above the 4096 x 256 elements one pass of the
CELL_STEPS = 3                                      # capped grid covers -- its second pass runs nowhere else


@functools.lru_cache(maxsize=None)
def cell_inputs(n, H, saturated=False):
    g = torch.Generator().manual_seed(100 + n + (7 if saturated else 0))
    rnd = lambda *shape: torch.randn(*shape, generator=g)                   # noqa: E731
    inp = dict(ga=rnd(n, 4 * H), gb=rnd(n, 4 * H), gc=rnd(n, 4 * H), c=rnd(n, H),
               dh_a=[rnd(n, H) for _ in range(CELL_STEPS)], dh_b=[rnd(n, H) for _ in range(CELL_STEPS)],
               dc=[rnd(n, H) for _ in range(CELL_STEPS)])
    if saturated:                                                   # half of the pre-activations at +-40 (a few at +-120)
        sat = torch.rand(n, 4 * H, generator=g) < 0.5
        sign = 2.0 * (torch.rand(n, 4 * H, generator=g) < 0.5) - 1.0
        three = torch.rand(n, 4 * H, generator=g) < 0.1
        inp["ga"] = torch.where(sat, 40.0 * sign, inp["ga"])
        inp["gb"] = torch.where(sat, torch.where(three, 40.0 * sign, torch.zeros(())), inp["gb"])
        inp["gc"] = torch.where(sat, torch.where(three, 40.0 * sign, torch.zeros(())), inp["gc"])
    return inp


def _cell_eval(inp, dt, step, use):
    """forward and the gradients for the step's (dh_a, dh_b, dc), each taken only if named in `use`"""
    gsum = (inp["ga"].to(dt) + inp["gb"].to(dt) + inp["gc"].to(dt)).requires_grad_()        # (fp32: added as the kernel adds them)
    c = inp["c"].to(dt, copy=True).requires_grad_()
    act, h, c2, _ = cell_restatement(gsum, torch.zeros((), dtype=dt), torch.zeros((), dtype=dt), c)
    dh = sum([inp[k][step].to(dt) for k in ("dh_a", "dh_b") if k in use], torch.zeros_like(h))
    dc = inp["dc"][step].to(dt) if "dc" in use else torch.zeros_like(h)
    d_gates, d_c = torch.autograd.grad((h * dh).sum() + (c2 * dc).sum(), [gsum, c])
    return dict(act=act.detach(), h=h.detach(), c2=c2.detach(), d_gates=d_gates, d_c=d_c)


@functools.lru_cache(maxsize=None)
def cell_reference(n, H, saturated=False, step=0, use=("dh_a", "dh_b", "dc")):
    """(fp64, fp32) evaluations of the cell restatement and its gradients: never modified"""
    inp = cell_inputs(n, H, saturated)
    return _cell_eval(inp, torch.float64, step, use), _cell_eval(inp, torch.float32, step, use)


def cell_forward(inp):
    """the three gate operands as column blocks of matrices of different widths"""
    from gvl_amd import MultiScaleDeformableAttention as MSDA
    n, H = inp["c"].shape
    H4 = 4 * H
    wa, wb, wc = (torch.full((n, H4 + w), SENTINEL, device=DEV) for w in (7, 16, 0))
    wa[:, 3:3 + H4], wb[:, :H4], wc[:] = inp["ga"], inp["gb"], inp["gc"]
    c = inp["c"].to(DEV)
    act, h, c2 = (torch.full((n, w), float("nan"), device=DEV) for w in (H4, H, H))
    MSDA.lstm_cell_train_forward(wa[:, 3:3 + H4], wb[:, :H4], wc, c, act, h, c2)
    torch.cuda.synchronize()
    return dict(act=act, h=h, c2=c2, c=c)


def cell_backward(inp, fwd, step, use, gates_sum=None, first=False):
    """grad_gates as a column block with sentinels on its neighbours (checked here)"""
    from gvl_amd import MultiScaleDeformableAttention as MSDA
    n, H = inp["c"].shape
    H4 = 4 * H
    wide = torch.full((n, H4 + 24), SENTINEL, device=DEV)
    d_c = torch.full((n, H), float("nan"), device=DEV)
    arg = lambda k: inp[k][step].to(DEV) if k in use else None              # noqa: E731
    MSDA.lstm_cell_train_backward(arg("dh_a"), arg("dh_b"), arg("dc"), fwd["act"], fwd["c"], fwd["c2"], wide[:, 8:8 + H4], d_c,
                                  gates_sum=gates_sum, first=first)
    torch.cuda.synchronize()
    assert bits_equal(wide[:, :8], torch.full((n, 8), SENTINEL, device=DEV))
    assert bits_equal(wide[:, 8 + H4:], torch.full((n, 16), SENTINEL, device=DEV))
    return dict(d_gates=wide[:, 8:8 + H4], d_c=d_c)


def check_cell(n, H, saturated=False, label=None):
    label = label or f"cell_{n}x{H}"
    inp = cell_inputs(n, H, saturated)
    w64, w32 = cell_reference(n, H, saturated)
    fwd = cell_forward(inp)
    got = dict(fwd, **cell_backward(inp, fwd, 0, ("dh_a", "dh_b", "dc")))
    rs = {k: ratio(f"{label}/{k}", got[k], w64[k], w32[k]) for k in ("act", "h", "c2", "d_gates", "d_c")}
    assert max(rs.values()) <= 1.0, {k: round(v, 3) for k, v in rs.items() if v > 1.0}


@pytest.mark.parametrize("n,H", CELL_SIZES)
def test_cell_forward_and_backward(n, H):
    check_cell(n, H)


@pytest.mark.parametrize("n,H", CELL_SIZES)
@pytest.mark.parametrize("use", [("dh_a", "dc"), ("dh_a", "dh_b"), ("dh_a",), ("dh_b", "dc")], ids=lambda u: "+".join(u))
def test_cell_backward_null_operands(n, H, use):
    """dh_b = None, dc = None, both None (and dh_a = None): an absent operand is a zero"""
    inp = cell_inputs(n, H)
    w64, w32 = cell_reference(n, H, False, 1, use)
    got = cell_backward(inp, cell_forward(inp), 1, use)
    rs = {k: ratio(f"cell_{n}x{H}_null/{k}", got[k], w64[k], w32[k]) for k in ("d_gates", "d_c")}
    assert max(rs.values()) <= 1.0, rs


@pytest.mark.parametrize("n,H", CELL_SIZES)
def test_cell_backward_running_gate_sum(n, H):
    """gates_sum over three calls: first=True overwrites a NaN-filled buffer, the next two accumulate -> the sum of the three
    gate gradients"""
    inp = cell_inputs(n, H)
    fwd = cell_forward(inp)
    acc = torch.full((n, 4 * H), float("nan"), device=DEV)
    want64, want32 = torch.zeros(n, 4 * H, dtype=torch.float64), torch.zeros(n, 4 * H)
    for step in range(CELL_STEPS):
        got = cell_backward(inp, fwd, step, ("dh_a", "dh_b", "dc"), gates_sum=acc, first=step == 0)
        w64, w32 = cell_reference(n, H, False, step)
        want64, want32 = want64 + w64["d_gates"], want32 + w32["d_gates"]
        if step == 0:
            assert not bool(torch.isnan(acc).any())
            assert bits_equal(acc, got["d_gates"])
    assert ratio(f"cell_{n}x{H}_sum/gates_sum", acc, want64, want32) <= 1.0


@pytest.mark.parametrize("n,H", CELL_SIZES[:2])
def test_cell_saturation(n, H):
    """half of the gate pre-activations at +-40 (some at +-120): finite, equal to the restatement"""
    check_cell(n, H, saturated=True, label=f"cell_{n}x{H}_saturated")


def test_cell_no_rows_touches_nothing():
    from gvl_amd import MultiScaleDeformableAttention as MSDA
    H = 5
    full = lambda *shape: torch.full(shape, SENTINEL, device=DEV)           # noqa: E731
    empty = torch.empty(0, H, device=DEV)
    act, h, c2, dg, dcp, acc = full(3, 4 * H), full(3, H), full(3, H), full(3, 4 * H), full(3, H), full(0, 4 * H)
    gates = torch.empty(0, 4 * H, device=DEV)
    MSDA.lstm_cell_train_forward(gates, gates, gates, empty, act, h, c2)
    MSDA.lstm_cell_train_backward(None, None, None, act, empty, empty, dg[:0], dcp, gates_sum=acc, first=True)
    torch.cuda.synchronize()
    for v in (act, h, c2, dg, dcp):
        assert bits_equal(v, torch.full_like(v, SENTINEL))

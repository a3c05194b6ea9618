"""The attention core of the decoder's self-attention in training (gvl_amd/csrc/gvl_mha_train.hip: k_mha_fwd, k_mha_bwd_kv, k_mha_bwd_q,
k_mha_delta) called ALONE -- tests/test_gpu_train_mha.py runs it between its two projections at H = 8, Q >= 64 and never reads lse
or the row maxima it leaves -- against the fp64 evaluation of its restatement in tests/mha_ref.py, at the edges of its tiling
(Q = 1 .. 321 around the 32 columns of a wavefront and the 160 of a workgroup), H = 1 and H = 3, key masks that empty a leading,
a middle and all but one key of the last tile, a video without a valid key beside two others, dropout up to the limit p = 0.9375
under the recomputed mask (a row that loses every weight; a kept weight of 16 on a probability of exactly 1), saturated and equal
scores, operands 2^10 and 2^12 apart, loose row bounds, a foreign leading dimension with NaN in the pad columns, NULL outputs,
the three by-product row maxima, repeatability and the refusals.

The core is reached through train_mha._Core.apply for a dense qkv and through the C entry points with the test's own buffers
where the case needs a leading dimension above 3 H 64, a NULL lse / amax_out or pre-filled outputs.  am is computed here as the
exact row maxima of the q | k and of the v columns.  tests/test_mha_train_ref_cpu.py checks, without a GPU, what the comparisons
rest on.

Tolerance: out, lse, dq, dk, dv are held to
    max(FACTOR * err32, 16 * 2**-23 * scale),   FACTOR = 8,
err32 being the deviation of the SAME restatement evaluated in fp32 torch on the CPU and scale the largest magnitude of the fp64
result (the bound of tests/test_gpu_cap_train_ops.py).  Two refinements, both narrower or forced: at Q = 1 dq and dk are zero in
exact arithmetic (dS = P (dP - delta) with a single key: dP = delta), both evaluations return exactly 0 and the kernel the
rounding of the two cancelling terms -- scale is then the magnitude of those terms, sum |P dP| |k| / 8 (as grad_alpha_b there);
and range_video is held video by video (the kernels scale their operands per video, so the small video must be right on its own
scale, not on the large one's).

Every test prints its figures as "RATIO <case>/<output> <kernel error / bound>" before it asserts (pytest -s).
Measured on the MI355X:

    case                         out     lse      dq      dk      dv
    edge_Q1_H1_p0              0.041   0.088   0.193   0.169   0.041
    edge_Q1_H1_p25             0.148   0.106   0.108   0.108   0.068
    edge_Q1_H3_p0              0.047   0.066   0.146   0.146   0.038
    edge_Q1_H3_p25             0.109   0.076   0.079   0.057   0.068
    edge_Q31_H1_p0             0.093   0.056   0.204   0.173   0.174
    edge_Q31_H1_p25            0.149   0.056   0.167   0.138   0.109
    edge_Q31_H3_p0             0.098   0.062   0.214   0.245   0.226
    edge_Q31_H3_p25            0.078   0.058   0.175   0.106   0.132
    edge_Q32_H1_p0             0.096   0.053   0.130   0.135   0.141
    edge_Q32_H1_p25            0.179   0.046   0.142   0.111   0.132
    edge_Q32_H3_p0             0.087   0.074   0.165   0.176   0.098
    edge_Q32_H3_p25            0.152   0.050   0.103   0.109   0.229
    edge_Q33_H1_p0             0.136   0.060   0.146   0.138   0.169
    edge_Q33_H1_p25            0.125   0.045   0.209   0.178   0.197
    edge_Q33_H3_p0             0.193   0.049   0.140   0.090   0.128
    edge_Q33_H3_p25            0.114   0.059   0.122   0.167   0.209
    edge_Q160_H1_p0            0.080   0.068   0.086   0.080   0.142
    edge_Q160_H1_p25           0.107   0.085   0.106   0.099   0.088
    edge_Q160_H3_p0            0.055   0.074   0.131   0.113   0.078
    edge_Q160_H3_p25           0.074   0.074   0.109   0.078   0.099
    edge_Q161_H1_p0            0.054   0.058   0.133   0.096   0.113
    edge_Q161_H1_p25           0.119   0.066   0.183   0.091   0.106
    edge_Q161_H3_p0            0.139   0.067   0.177   0.071   0.108
    edge_Q161_H3_p25           0.097   0.071   0.111   0.103   0.093
    edge_Q321_H1_p0            0.099   0.070   0.123   0.106   0.127
    edge_Q321_H1_p25           0.152   0.065   0.135   0.109   0.103
    edge_Q321_H3_p0            0.115   0.071   0.143   0.149   0.151
    edge_Q321_H3_p25           0.061   0.073   0.142   0.138   0.130
    mask_suffix                0.101   0.061   0.288   0.083   0.126
    mask_lead                  0.088   0.058   0.078   0.147   0.098
    mask_middle                0.103   0.066   0.138   0.099   0.123
    mask_single                0.064   0.060   0.413   0.515   0.056
    mask_null                  0.084   0.073   0.110   0.099   0.122
    isolation_open             0.091   0.065   0.210   0.131   0.106
    drop_p125                  0.067   0.065   0.263   0.186   0.171
    drop_p5                    0.118   0.068   0.161   0.150   0.217
    drop_p9375                 0.115   0.063   0.069   0.105   0.209
    drop_lost_row              0.056   0.044   0.138   0.125   0.104
    drop_p9375_single          0.051   0.091   0.227   0.655   0.035
    saturation                 0.077   0.135   0.102   0.169   0.331
    saturation_p25             0.144   0.094   0.071   0.186   0.260
    range_k_small              0.060   0.056   0.097   0.100   0.096
    range_row                  0.100   0.075   0.160   0.123   0.122
    range_row_k                0.088   0.071   0.188   0.125   0.097
    range_video[0]             0.086   0.030   0.109   0.098   0.145
    range_video[1]             0.099   0.070   0.133   0.156   0.237
    range_zero_v               0.000   0.057   0.000   0.000   0.114
    range_loose_am             0.122   0.072   0.119   0.056   0.086
    ld                         0.102   0.060   0.204   0.164   0.089

Above one half: mask_single dk 0.515 (dq 0.413) and drop_p9375_single dk 0.655, at FACTOR = 8, which stays.  In both, video 1 has a
single valid key: every query of it has P = 1, so dS = P (dP - delta) is zero in exact arithmetic, and the fp32 restatement
returns it as an exact 0 (softmax gives 1.0, the softmax backward 1 (dP - 1 dP)) -- its err32 comes from the other video alone.
The kernels take dP from the three-MFMA product of dO and v (22-bit operands, the lo.lo term dropped) and delta from
k_mha_delta's fp32 dot of dO with the stored out: two roundings of the same sum that differ by 2^-22 of sum_c |dO_c| |v_c|, and
that difference times q / 8, summed over the video's 70 (33) queries, lands in dk of the one key: 2.2e-6 of a largest entry of
1.15, i.e. 16 ulp.  At p = 0.9375 the kept weights are 16, dP and delta 16 times as large, the sum over a sixteenth as many
queries: 1.3e-5 on 6.85.  The same outputs sit at 0.06 .. 0.29 in every case whose rows have more than one valid key.

Narrowed: "one row at 2^10 times the others" is two cases here, the row's q and v columns (range_row) and its k and v columns
(range_row_k).  With the WHOLE row scaled its score with its own key is 2^20 times the ordinary ones (2000 and more): measured
at this bound, dk 136 (6.5e-4 of a largest entry of 1.6: that key carries the query with P = 1, dP - delta is the rounding
described above on terms 2^10 larger, and it is multiplied by a q row at 2^10 where the fp32 restatement has an exact 0) and, with
another seed, dv 3.5 (1.4e-5 of its largest entry: the backward recomputes P = exp(score - lse) from two fp32 numbers of
magnitude 2000, a relative error of |score| 2^-23).  Neither is an operand-range error; include/gvl_msda.h now names both.

Seeded errors (each applied alone to a scratch copy of gvl_mha_train.hip, values only; the tests of this file that then fail):
  1 mfma3 without its (al, bh) MFMA: 48 of 61 -- every test that compares values
  2 drop_factor(.., k, q) in k_mha_bwd_kv only: 21 -- every test with p > 0 and more than one key
  3 no corr = 1 under the `none` guard: 4 -- test_key_masks[mask_lead, mask_single], test_inference_form[mask_lead],
    test_dropout_at_the_limit_on_a_probability_of_one (leading tiles without a valid key: NaN)
  4 amax_out from t = 0 only: 48 -- every test that reads the by-products, test_inference_form included
  5 0.1249f in k_mha_bwd_q's output scale: 46 -- every test that compares a dq that is not zero (not range_zero_v, not Q = 1 with its key dropped)
  6 lse without its m term: 48 -- every test that compares lse
"""
import functools

import pytest
import torch

import mha_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FACTOR = 8.0               # kernel error allowed per fp32-restatement error (module docstring)
FLOOR = 16 * 2.0 ** -23    # ... and never less than 16 ulp of the tensor's largest entry
SENTINEL = -7.25e11        # fills what a call must write (or must not touch)
OUTPUTS = ("out", "lse", "dq", "dk", "dv")


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
    print("RATIO %-32s %.3f   (error %.3g, fp32 restatement %.3g, scale %.3g)" % (label, r, err, err32, scale))
    return r


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def parts(got, B, Q, H):
    """the five compared outputs in the restatement's shapes"""
    C = H * R.D
    d = got["dqkv"][:, :3 * C].reshape(B, Q, 3 * C)
    return dict(out=got["out"].reshape(B, Q, C), lse=got["lse"], dq=d[..., :C], dk=d[..., C:2 * C], dv=d[..., 2 * C:])


def check_values(name, got, label=None, per_video=False):
    i = R.inputs(name)
    w64, w32 = R.reference(name)
    label = label or name
    have = parts(got, i["B"], i["Q"], i["H"])
    rs = {}
    for k in OUTPUTS:
        if per_video:
            for b in range(i["B"]):
                rs[f"{k}[{b}]"] = ratio(f"{label}/{k}[{b}]", have[k][b], w64[k][b], w32[k][b])
            continue
        scale = None
        if i["Q"] == 1 and k in ("dq", "dk"):                       # zero in exact arithmetic (module docstring)
            assert float(w64[k].abs().max()) == 0.0
            scale = w64["cancel"][k]
        rs[k] = ratio(f"{label}/{k}", have[k], w64[k], w32[k], scale)
    assert max(rs.values()) <= 1.0, {k: round(v, 3) for k, v in rs.items() if v > 1.0}


def check_byproducts(got, H, rows=None):
    """the three row maxima are taken from the registers and roundings the kernels store: exactly the maxima of what they stored"""
    C = H * R.D
    rows = slice(None) if rows is None else rows
    out, d = got["out"][rows], got["dqkv"][rows]
    assert torch.equal(got["am_out"][rows], out.abs().amax(1))
    assert torch.equal(got["am_dqk"][rows], d[:, :2 * C].abs().amax(1))
    assert torch.equal(got["am_dv"][rows], d[:, 2 * C:3 * C].abs().amax(1))


# ---------------------------------------------------------------------------------------------------------------------------
# running the kernels
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def device_inputs(name):
    """never modified: qkv (B Q, 3 H 64), g (B Q, H 64), keep (B, Q) uint8 or None, am (2, B Q) the exact row maxima of the
    q | k and of the v columns (times the case's am_factor)"""
    i = R.inputs(name)
    B, Q, H = i["B"], i["Q"], i["H"]
    C = H * R.D
    qkv = i["qkv"].reshape(B * Q, 3 * C).to(DEV)
    am = torch.stack([qkv[:, :2 * C].abs().amax(1), qkv[:, 2 * C:].abs().amax(1)]) * i["am_factor"]
    keep = None if i["keep"] is None else i["keep"].to(DEV).contiguous().view(torch.uint8)
    return dict(qkv=qkv, g=i["g"].reshape(B * Q, C).to(DEV), keep=keep, am=am.contiguous())


def run_core(name):
    """forward and backward through train_mha._Core (dense qkv) -> out, lse, dqkv and the three by-products"""
    from gvl_amd import train_layers as TL
    from gvl_amd import train_mha as TM
    i, d = R.inputs(name), device_inputs(name)
    step = None
    if i["p"] > 0:                                                  # _Core draws its masks at the step counter's value
        step = TL.step_counter(DEV)
        step.fill_(i["step"])
        TL.arena(DEV).snap = None
    qkv = d["qkv"].clone().requires_grad_()
    out, am_out = TM._Core.apply(qkv, d["am"], d["keep"], i["B"], i["Q"], i["H"], i["p"], i["seed"], step)
    lse = out.grad_fn.saved_tensors[4]
    dqkv, = torch.autograd.grad(out, qkv, d["g"])
    left = getattr(dqkv, "_gvl_amax_qk_v", None)                    # (what the in-projection's backward picks up)
    assert left is not None and left[1] == dqkv._version
    torch.cuda.synchronize()
    assert bits_equal(qkv.detach(), d["qkv"])
    return dict(out=out.detach(), lse=lse, dqkv=dqkv, am_out=am_out, am_dqk=left[0][0], am_dv=left[0][1])


def _ptr(t):
    return None if t is None else t.data_ptr()


def run_c(name, ld=None, with_lse=True, with_amax=True, backward=True):
    """the same through the C entry points on this function's own buffers: qkv and dqkv at leading dimension ld with NaN / the
    sentinel in the pad columns, out, lse and dqkv pre-filled with the sentinel, the by-product vectors zero as their contract
    asks"""
    from gvl_amd import _lib
    i, d = R.inputs(name), device_inputs(name)
    B, Q, H, p = i["B"], i["Q"], i["H"], i["p"]
    C, n = H * R.D, B * Q
    W = 3 * C
    ld = ld or W
    qkv = torch.full((n, ld), float("nan"), device=DEV)
    qkv[:, :W] = d["qkv"]
    before = qkv.clone()
    full = lambda *shape: torch.full(shape, SENTINEL, device=DEV)           # noqa: E731
    zeros = lambda m: torch.zeros(m, device=DEV)                            # noqa: E731
    out, lse, dqkv = full(n, C), full(B, H, Q), full(n, ld)
    am_out, am_dqk, am_dv = zeros(n), zeros(n), zeros(n)
    step = torch.tensor([i["step"]], dtype=torch.int64, device=DEV) if p > 0 else None
    delta, am_g = torch.empty(B, H, Q, device=DEV), torch.empty(n, device=DEV)
    lib = _lib.lib()
    with torch.cuda.device(DEV):
        stream = torch.cuda.current_stream().cuda_stream
        rc = lib.gvl_mha_train_forward_f32(qkv.data_ptr(), ld, _ptr(d["keep"]), d["am"][0].data_ptr(), d["am"][1].data_ptr(), B, Q, H,
                                           p, i["seed"], _ptr(step), out.data_ptr(), lse.data_ptr() if with_lse else None,
                                           am_out.data_ptr() if with_amax else None, stream)
        _lib.check(rc, "mha_train_forward")
        if backward:
            assert with_lse
            rc = lib.gvl_mha_train_backward_amax_f32(qkv.data_ptr(), ld, _ptr(d["keep"]), d["am"][0].data_ptr(), d["am"][1].data_ptr(),
                                                     B, Q, H, p, i["seed"], _ptr(step), out.data_ptr(), lse.data_ptr(),
                                                     d["g"].data_ptr(), delta.data_ptr(), am_g.data_ptr(), dqkv.data_ptr(),
                                                     am_dqk.data_ptr(), am_dv.data_ptr(), stream)
            _lib.check(rc, "mha_train_backward")
    torch.cuda.synchronize()
    assert bits_equal(qkv, before)
    return dict(out=out, lse=lse, dqkv=dqkv, am_out=am_out, am_dqk=am_dqk, am_dv=am_dv)


def check_case(name, **kw):
    i = R.inputs(name)
    got = run_core(name)
    check_values(name, got, **kw)
    check_byproducts(got, i["H"])
    return got


# ---------------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.25], ids=["p0", "p25"])
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("Q", R.EDGE_QS)
def test_tile_and_workgroup_edges(Q, H, p):
    """Q around the 32 columns of a wavefront and the 160 of a workgroup (161, 321: a workgroup with one live column and four idle
    wavefronts); H = 3 makes k_mha_delta's loop over C / 4 float4s ragged; video 1 with a ragged key suffix"""
    check_case("edge_Q%d_H%d_p%s" % (Q, H, "25" if p else "0"))


@pytest.mark.parametrize("name", ["mask_suffix", "mask_lead", "mask_middle", "mask_single", "mask_null"])
def test_key_masks(name):
    """a ragged suffix per video; a leading 32-key tile without a valid key, then valid keys (the online softmax starts at -inf);
    an excluded tile in the middle; a single valid key in the last, partial tile; keep = NULL"""
    check_case(name)


def test_a_video_without_a_valid_key_leaves_the_others_alone():
    """video 1 of three has every key excluded (its own values are NaN by contract and not compared): the other two videos' out,
    lse and gradients are bit for bit those of the same call with video 1 open, which is held to the reference"""
    i = R.inputs("isolation")
    B, Q, H = i["B"], i["Q"], i["H"]
    assert bits_equal(i["qkv"], R.inputs("isolation_open")["qkv"]) and i["seed"] == R.inputs("isolation_open")["seed"]
    shut, opened = run_core("isolation"), check_case("isolation_open")
    a, b = parts(shut, B, Q, H), parts(opened, B, Q, H)
    for k in OUTPUTS:
        for v in (0, 2):
            assert bits_equal(a[k][v], b[k][v]), (k, v)
            assert bool(torch.isfinite(a[k][v]).all()), (k, v)
    rows = torch.cat([torch.arange(0, Q), torch.arange(2 * Q, 3 * Q)]).to(DEV)
    check_byproducts(shut, H, rows)


@pytest.mark.parametrize("name", ["drop_p125", "drop_p5", "drop_p9375"])
def test_dropout_under_the_recomputed_mask(name):
    check_case(name)


def test_a_row_that_loses_every_weight_is_exactly_zero():
    """p = 0.5, Q = 33, video 1 with three valid keys on both sides of a tile edge, the seed found by search on the CPU: a row whose
    three weights are all dropped gives out = 0 and dq = 0 exactly, not small"""
    name = "drop_lost_row"
    i = R.inputs(name)
    got = check_case(name)
    have = parts(got, i["B"], i["Q"], i["H"])
    lost = R.lost_rows(i["drop"], i["keep"])
    assert bool(lost.any())
    for b, h, q in lost.nonzero().tolist():
        cols = slice(h * R.D, (h + 1) * R.D)
        assert float(have["out"][b, q, cols].abs().max()) == 0.0 and float(have["dq"][b, q, cols].abs().max()) == 0.0, (b, h, q)


def test_dropout_at_the_limit_on_a_probability_of_one():
    """p = 0.9375 (kept weights are 16) and a video with a single valid key, whose probability is exactly 1: the fp16 operand
    2^11 * 16 = 2^15 is finite (check_values asserts finiteness) and the results are within bound"""
    name = "drop_p9375_single"
    i = R.inputs(name)
    got = check_case(name)
    k = int(i["keep"][1].nonzero())
    kept = i["drop"][1, :, :, k]                                     # (H, Q): rows of video 1 that keep their one weight
    assert bool(kept.any()) and not bool(kept.all())
    out = parts(got, i["B"], i["Q"], i["H"])["out"][1].reshape(i["Q"], i["H"], R.D).transpose(0, 1)
    v = device_inputs(name)["qkv"].reshape(i["B"], i["Q"], 3, i["H"], R.D)[1, k, 2]        # (H, 64)
    assert float(out[~kept.to(DEV)].abs().max()) == 0.0
    want = (16.0 * v.double())[:, None, :].expand(-1, i["Q"], -1)[kept.to(DEV)]
    assert float((out[kept.to(DEV)].double() - want).abs().max()) <= 2.0 ** -21 * float(want.abs().max())


@pytest.mark.parametrize("name", ["saturation", "saturation_p25"])
def test_saturated_and_equal_scores(name):
    """scores within a row +-60 apart (one key carries the row) and one query whose scores are all equal"""
    check_case(name)


@pytest.mark.parametrize("name", ["range_k_small", "range_row", "range_row_k", "range_video", "range_zero_v", "range_loose_am"])
def test_operand_range(name):
    """k at 2^-10 of q inside one video (they share amax_qk); one row whose q and v (k and v) columns are 2^10 times the others;
    one video at 2^12 times the other (held video by video); v = 0; am given as 4 times the true maxima -- all inside what
    include/gvl_msda.h promises (an element 2^-k below the video's largest keeps max(2^-23, 2^(k - 36)) of itself), so all at the
    same bound"""
    got = check_case(name, per_video=name == "range_video")
    if name == "range_zero_v":
        i = R.inputs(name)
        have = parts(got, i["B"], i["Q"], i["H"])
        assert all(float(have[k].abs().max()) == 0.0 for k in ("out", "dq", "dk"))


def test_leading_dimension_pads_and_prefilled_outputs():
    """ld = 3 H 64 + 8 through the C entry points, NaN in the pad columns of qkv, out / lse / dqkv pre-filled with a sentinel: every
    element of out, lse and of the columns [0, 3 H 64) of dqkv is written (and right), the pad columns of dqkv keep the sentinel"""
    name = "ld"
    i = R.inputs(name)
    W = 3 * i["H"] * R.D
    got = run_c(name, ld=W + 8)
    for k in ("out", "lse"):
        assert not bool((got[k] == SENTINEL).any()), k
    assert not bool((got["dqkv"][:, :W] == SENTINEL).any())
    assert bits_equal(got["dqkv"][:, W:], torch.full((i["B"] * i["Q"], 8), SENTINEL, device=DEV))
    check_values(name, got)
    check_byproducts(got, i["H"])
    dense = run_core(name)                                          # ... and the dense call gives the same bits
    for k in ("out", "lse", "am_out", "am_dqk", "am_dv"):
        assert bits_equal(got[k], dense[k]), k
    assert bits_equal(got["dqkv"][:, :W], dense["dqkv"])


@pytest.mark.parametrize("name", ["mask_lead", "edge_Q161_H3_p0"])
def test_inference_form_null_lse_and_amax_out(name):
    """lse = NULL and amax_out = NULL (gvl_amd/layers.py calls the forward so at p = 0): out is bit for bit the out of the call
    that passes both"""
    both = run_c(name, backward=False)
    assert torch.equal(both["am_out"], both["out"].abs().amax(1))
    for kw in (dict(with_lse=False, with_amax=False), dict(with_lse=False), dict(with_amax=False)):
        one = run_c(name, backward=False, **kw)
        assert bits_equal(one["out"], both["out"]), kw
        if not kw.get("with_lse", True):
            assert bits_equal(one["lse"], torch.full_like(one["lse"], SENTINEL))
        if not kw.get("with_amax", True):
            assert float(one["am_out"].abs().max()) == 0.0


@pytest.mark.parametrize("name", ["isolation_open", "edge_Q321_H3_p25"])
def test_repeatability(name):
    """the same call twice: out, lse and dqkv bit for bit (no atomics in the sums; the row maxima are atomic maxima, order-free)"""
    a, b = run_core(name), run_core(name)
    for k in ("out", "lse", "dqkv", "am_out", "am_dqk", "am_dv"):
        assert bits_equal(a[k], b[k]), k


# ---------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------
_ABOVE = float(torch.nextafter(torch.tensor(0.9375), torch.tensor(1.0)))          # the fp32 number after the limit
REFUSALS = {
    "p_negative": (dict(p=-0.125), "dropout probability"),
    "p_above_the_limit": (dict(p=0.95), "dropout probability"),
    "p_next_after_the_limit": (dict(p=_ABOVE), "dropout probability"),
    "p_one": (dict(p=1.0), "dropout probability"),
    "ld_below_3H64": (dict(ld=188), "ld >= 3 H 64"),
    "ld_not_a_multiple_of_4": (dict(ld=194), "ld >= 3 H 64"),
    # sizes only: check() precedes any access, the buffers are those of the tiny shape
    "BHQQ_at_2_to_32": (dict(B=1, H=1, Q=65536), r"below 2\^32"),
    "amax_dqk_without_amax_dv": (dict(pair=False), "come together"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals_launch_nothing(case):
    """outside the entry points' domain the library's error comes back through _lib.check, from the forward and from the backward,
    and no output is written"""
    from gvl_amd import _lib
    kw, message = REFUSALS[case]
    B, Q, H = kw.get("B", 1), kw.get("Q", 4), kw.get("H", 1)
    ld, p = kw.get("ld", 192), kw.get("p", 0.25)
    n = 4                                                             # rows of the buffers, whatever the sizes passed say
    qkv = torch.randn(n, 200, device=DEV)
    am = torch.full((2, n), 8.0, device=DEV)
    full = lambda *shape: torch.full(shape, SENTINEL, device=DEV)           # noqa: E731
    out, lse, dqkv, delta, am_g = full(n, 64), full(n), full(n, 200), full(n), full(n)
    am_out, am_dqk, am_dv = full(n), full(n), full(n)
    g = torch.randn(n, 64, device=DEV)
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    lib = _lib.lib()
    with torch.cuda.device(DEV):
        stream = torch.cuda.current_stream().cuda_stream
        if "pair" not in kw:                                            # (the forward has no such pair)
            rc = lib.gvl_mha_train_forward_f32(qkv.data_ptr(), ld, None, am[0].data_ptr(), am[1].data_ptr(), B, Q, H, p, 1,
                                               step.data_ptr(), out.data_ptr(), lse.data_ptr(), am_out.data_ptr(), stream)
            assert rc != 0
            with pytest.raises(RuntimeError, match=message):
                _lib.check(rc, "mha_train_forward")
        rc = lib.gvl_mha_train_backward_amax_f32(qkv.data_ptr(), ld, None, am[0].data_ptr(), am[1].data_ptr(), B, Q, H, p, 1,
                                                 step.data_ptr(), out.data_ptr(), lse.data_ptr(), g.data_ptr(), delta.data_ptr(),
                                                 am_g.data_ptr(), dqkv.data_ptr(), am_dqk.data_ptr(),
                                                 am_dv.data_ptr() if kw.get("pair", True) else None, stream)
        assert rc != 0
        with pytest.raises(RuntimeError, match=message):
            _lib.check(rc, "mha_train_backward")
    torch.cuda.synchronize()
    for name, t in dict(out=out, lse=lse, dqkv=dqkv, delta=delta, am_g=am_g, am_out=am_out, am_dqk=am_dqk, am_dv=am_dv).items():
        assert bits_equal(t, torch.full_like(t, SENTINEL)), name


def test_the_limit_itself_is_accepted_and_the_module_agrees():
    """p = 0.9375 passes check() (test_dropout_at_the_limit_on_a_probability_of_one runs it); train_mha.eligible draws the same
    line, so a module with a larger dropout takes torch's path in training instead of raising"""
    from gvl_amd import train_mha as TM
    B, Q, C, H = 4, 300, 512, 8
    tgt = torch.zeros(B, Q, C, device=DEV)
    pos = torch.zeros(Q, C, device=DEV).unsqueeze(0).expand(B, -1, -1)
    at_limit = torch.nn.MultiheadAttention(C, H, dropout=0.9375).to(DEV).train()
    above = torch.nn.MultiheadAttention(C, H, dropout=0.97).to(DEV).train()
    assert TM.MAX_DROPOUT == 0.9375 and TM.eligible(at_limit, tgt, pos)
    assert not TM.eligible(above, tgt, pos)
    assert TM.eligible(above.eval(), tgt, pos)                       # (no dropout outside training)

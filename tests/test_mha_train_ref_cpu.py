"""CPU side of tests/test_gpu_mha_train_ops.py: what its comparisons rest on.  The fp64 restatement of the attention core
(tests/mha_ref.py) against nn.MultiheadAttention in fp64 (values and the gradient of qkv, the agreement of two fp64 evaluations);
gradcheck of the restatement under a fixed dropout mask; and for every case of the table that each query has a valid key (but in
the isolation case), that the dropout probabilities have an exact threshold and the drawn masks the share they should, that the
searched seed loses a row, and that the dynamic-range cases have the ratios they claim.  Also: what _Core refuses before any
launch."""
import pytest
import torch

import mha_ref as R


def _mha_identity(C, H):
    """nn.MultiheadAttention in fp64 whose projections are the identity: its input triple IS [q | k | v]"""
    mha = torch.nn.MultiheadAttention(C, H, dropout=0.0, bias=True).double().eval()
    with torch.no_grad():
        mha.in_proj_weight.copy_(torch.eye(C, dtype=torch.float64).repeat(3, 1))
        mha.in_proj_bias.zero_()
        mha.out_proj.weight.copy_(torch.eye(C, dtype=torch.float64))
        mha.out_proj.bias.zero_()
    return mha


@pytest.mark.parametrize("name", ["mask_null", "mask_suffix", "mask_lead", "edge_Q33_H1_p0"])
def test_restatement_equals_multihead_attention_in_fp64(name):
    """p = 0, with and without a key mask, H = 3 and H = 1: out and the gradient of qkv at 1e-10 of each tensor's largest entry"""
    i = R.inputs(name)
    C = i["H"] * R.D
    w64 = R.reference(name)[0]
    qkv = i["qkv"].double().requires_grad_()
    q, k, v = (qkv[..., j * C:(j + 1) * C].transpose(0, 1) for j in range(3))
    mha = _mha_identity(C, i["H"])
    out = mha(q, k, v, key_padding_mask=None if i["keep"] is None else ~i["keep"], need_weights=False)[0].transpose(0, 1)
    dqkv, = torch.autograd.grad((out * i["g"].double()).sum(), qkv)
    pairs = [("out", w64["out"], out.detach()), ("dq", w64["dq"], dqkv[..., :C]), ("dk", w64["dk"], dqkv[..., C:2 * C]),
             ("dv", w64["dv"], dqkv[..., 2 * C:])]
    for n, a, b in pairs:
        assert float((a - b).abs().max()) <= 1e-10 * float(b.abs().max()), n
    # lse: log sum exp of the scores, the softmax's own normaliser
    s = R.scores(i["qkv"].double(), i["keep"])
    assert float((w64["lse"] - s.exp().sum(-1).log()).abs().max()) <= 1e-10 * float(w64["lse"].abs().max())


def test_restatement_passes_gradcheck_under_a_fixed_dropout_mask():
    B, Q, H, p = 2, 5, 1, 0.25
    gen = torch.Generator().manual_seed(0)
    qkv = torch.randn(B, Q, 3 * H * R.D, generator=gen, dtype=torch.float64, requires_grad=True)
    keep = torch.ones(B, Q, dtype=torch.bool)
    keep[1, 3:] = False
    drop = R._keep_mask(B, H, Q, p, 11, 3, "cpu")
    assert bool(drop.any()) and not bool(drop.all())
    assert torch.autograd.gradcheck(lambda x: R.core_restatement(x, keep, drop, p), (qkv,), eps=1e-6, atol=1e-7, rtol=1e-5)


def test_dropout_scale_is_the_fp32_quotient():
    assert [R.drop_scale(p) for p in (0.125, 0.25, 0.5, 0.9375)] == [float(torch.tensor(8.0 / 7.0, dtype=torch.float32)),
                                                                     float(torch.tensor(4.0 / 3.0, dtype=torch.float32)), 2.0, 16.0]


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_case_table(name):
    i = R.inputs(name)
    B, Q, H, p = i["B"], i["Q"], i["H"], i["p"]
    assert B <= 3 and H in (1, 3) and Q <= 321 and i["qkv"].dtype == torch.float32 and i["qkv"].shape == (B, Q, 3 * H * R.D)
    valid = torch.ones(B, Q, dtype=torch.bool) if i["keep"] is None else i["keep"]
    if name == "isolation":
        assert valid.any(-1).tolist() == [True, False, True]
    else:
        assert bool(valid.any(-1).all())                            # every query of every video has a valid key
    if p > 0:
        assert p in R.DROP_PS
        thr = float(torch.tensor(p, dtype=torch.float32)) * 4294967296.0
        assert thr == p * 2.0 ** 32 and thr == int(thr)             # no rounding question in the threshold
        n = i["drop"].numel()
        dev = abs(float(i["drop"].double().mean()) - (1.0 - p))
        assert dev <= 4.0 * (p * (1.0 - p) / n) ** 0.5, (dev, n)      # within four binomial standard deviations
    else:
        assert i["drop"] is None
    w64, w32 = R.reference(name)
    live = valid.any(-1)
    for k in ("out", "lse", "dq", "dk", "dv"):                      # (the videos with a valid key)
        assert bool(torch.isfinite(w64[k][live]).all()) and bool(torch.isfinite(w32[k][live]).all()), k


def test_mask_cases_exclude_what_they_name():
    keep = R.inputs("mask_lead")["keep"]
    assert not bool(keep[0, :32].any()) and bool(keep[0, 32:].all()) and bool(keep[1, :32].all())
    keep = R.inputs("mask_middle")["keep"]
    assert bool(keep[0, :32].all()) and not bool(keep[0, 32:64].any()) and bool(keep[0, 64:].all())
    for name, Q in (("mask_single", 70), ("drop_p9375_single", 33)):
        keep = R.inputs(name)["keep"]
        k = int(keep[1].nonzero())
        assert int(keep[1].sum()) == 1 and k >= 32 * ((Q - 1) // 32) and Q % 32 != 0          # inside the last, partial tile
        a = torch.softmax(R.scores(R.inputs(name)["qkv"].double(), keep), -1)
        assert bool((a[1, :, :, k] == 1.0).all())                   # its probability is exactly 1
    keep = R.inputs("mask_suffix")["keep"]
    tails = [int(Q_) for Q_ in keep.sum(-1)]
    assert tails[0] == 70 and len(set(tails)) == 3                  # ragged: a different suffix per video
    assert R.inputs("mask_null")["keep"] is None


def test_the_searched_seed_loses_a_row():
    assert R.find_lost_row_seed() == R.DROP_LOST_SEED
    i = R.inputs("drop_lost_row")
    lost = R.lost_rows(i["drop"], i["keep"])
    assert bool(lost.any()) and not bool(lost[1].all()) and not bool(lost[0].any())
    w64 = R.reference("drop_lost_row")[0]
    b, h, q = (int(x) for x in lost.nonzero()[0])
    assert float(w64["out"][b, q, h * R.D:(h + 1) * R.D].abs().max()) == 0.0
    assert float(w64["dq"][b, q, h * R.D:(h + 1) * R.D].abs().max()) == 0.0


def test_dynamic_range_cases_have_the_ratio_they_claim():
    amax = lambda t: float(t.abs().max())                              # noqa: E731
    # saturation: scores within a row +-60 apart, one key carries the row; one row with all scores equal
    for name in ("saturation", "saturation_p25"):
        i = R.inputs(name)
        s = R.scores(i["qkv"].double(), i["keep"])
        fin = torch.where(torch.isinf(s), torch.full_like(s, float("nan")), s)
        spread = torch.nan_to_num(fin, nan=-1e30).amax(-1) - torch.nan_to_num(fin, nan=1e30).amin(-1)
        b, q = R.EQUAL_ROW
        assert float(spread[b, :, q].abs().max()) == 0.0
        spread[b, :, q] = float("nan")
        rest = spread[~torch.isnan(spread)]
        assert float(rest.median()) >= 120.0 and float(rest.min()) >= 60.0, (float(rest.median()), float(rest.min()))
        top = torch.softmax(s, -1).amax(-1)
        top[b, :, q] = 1.0
        assert float((top > 0.99).double().mean()) >= 0.6              # one key carries two rows in three (the others: two close keys)
    C = 3 * R.D
    x = R.inputs("range_k_small")["qkv"]
    assert amax(x[0, :, :C]) / amax(x[0, :, C:2 * C]) == pytest.approx(2.0 ** 10, rel=0.35)
    assert amax(x[1, :, :C]) / amax(x[1, :, C:2 * C]) == pytest.approx(1.0, rel=0.35)
    b, r = R.OUTLIER_ROW
    for name, cols in (("range_row", "qv"), ("range_row_k", "kv")):
        i = R.inputs(name)
        x = i["qkv"]
        others = torch.cat([x[b, :r], x[b, r + 1:]])
        for j, c in enumerate("qkv"):
            want = 2.0 ** 10 if c in cols else 1.0
            got = x[b, r, j * C:(j + 1) * C].abs().mean() / others[:, j * C:(j + 1) * C].abs().mean()
            assert got.item() == pytest.approx(want, rel=0.15), (name, c)
        # the scores stay ordinary (a whole row at 2^10 would score 2^20 with itself: include/gvl_msda.h)
        s = R.scores(x.double(), i["keep"])[b]
        assert float(s[torch.isfinite(s)].abs().max()) < 8.0 and float(torch.softmax(s, -1).max()) < 0.5
    x = R.inputs("range_video")["qkv"]
    assert (x[1].abs().mean() / x[0].abs().mean()).item() == pytest.approx(2.0 ** 12, rel=0.05)
    x = R.inputs("range_zero_v")["qkv"]
    assert amax(x[..., 2 * C:]) == 0.0 and amax(x[..., :2 * C]) > 1.0
    assert R.inputs("range_loose_am")["am_factor"] == 4.0


def test_core_refuses_a_padded_qkv_before_any_launch():
    """a column slice of a wider buffer: the backward's dense dqkv would not have its leading dimension"""
    from gvl_amd import train_mha as TM
    B, Q, H = 1, 4, 1
    wide = torch.zeros(B * Q, 3 * H * 64 + 8)
    am = torch.ones(2, B * Q)
    with pytest.raises(ValueError, match="qkv"):
        TM._Core.apply(wide[:, :3 * H * 64], am, None, B, Q, H, 0.0, 0, None)
    with pytest.raises(ValueError, match="qkv"):
        TM._Core.apply(torch.zeros(3 * H * 64, B * Q).t(), am, None, B, Q, H, 0.0, 0, None)
    with pytest.raises(ValueError, match="qkv"):
        TM._Core.apply(torch.zeros(B, Q, 3 * H * 64), am, None, B, Q, H, 0.0, 0, None)
    assert TM.MAX_DROPOUT == 0.9375

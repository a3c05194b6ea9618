"""CPU side of tests/test_gpu_criterion_ops.py: what its comparisons rest on.  The fp64 restatements of tests/criterion_ref.py against
the project's PyTorch formulation in fp64 -- SetCriterion.get_loss on hand-made matchings, HungarianMatcher.cost_matrix,
F.log_softmax(...).gather -- at 1e-10 of each tensor's largest entry, values and gradients; gradcheck of the criterion restatement
where nothing ties; and for every case of the table that it has the property it is named for, and that the only non-finite
reference value anywhere is loss_self_iou in the cases listed for it."""
import argparse

import pytest
import torch
import torch.nn.functional as F

import criterion_ref as R

CRIT = sorted(n for n, c in R.CASES.items() if c["kind"] == "crit")
COST = sorted(n for n, c in R.CASES.items() if c["kind"] == "cost")
CE = sorted(n for n, c in R.CASES.items() if c["kind"] == "ce")


def close(a, b, what):
    a, b = a.double(), b.double()
    assert a.shape == b.shape, what
    nan = torch.isnan(b)
    assert torch.equal(torch.isnan(a), nan), what
    if bool((~nan).any()):
        err = float((a - b)[~nan].abs().max())
        assert err <= 1e-10 * float(b[~nan].abs().max()), (what, err)


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement is the project's PyTorch formulation
# ---------------------------------------------------------------------------------------------------------------------------
def project_criterion(i, dt=torch.float64):
    """SetCriterion.get_loss (the un-fused formulation) layer by layer on the case's hand-made matching -> the entries of
    R.evaluate_criterion"""
    from gvl_amd.criterion import SetCriterion
    from gvl_amd.matcher import HungarianMatcher
    opt = argparse.Namespace(lloss_gau_mask=i["gau"], lloss_beta=i["beta"], set_cost_caption=0)
    crit = SetCriterion(i["NC"], HungarianMatcher(opt=opt), {}, ['labels', 'boxes', 'cardinality'], focal_alpha=i["alpha"],
                        focal_gamma=i["gamma"], opt=opt)
    crit.fused = False
    crit.counter_class_rate = i["ccr"].to(dt)
    crit._tgt_cat = (i["tlabels"], i["tboxes"].to(dt))
    crit._gt_counts = i["gt_counts"]
    leaves = [i[k].to(dt, copy=True).requires_grad_() for k in ("logits", "counts", "boxes")]
    targets = [{"labels": torch.zeros(n, dtype=torch.int64)} for n in i["sizes"]]
    rows = []
    for l in range(i["nl"]):
        crit._state = {}
        out = {"pred_logits": leaves[0][l], "pred_count": leaves[1][l], "pred_boxes": leaves[2][l]}
        es = i["ent_start"]
        indices = ([(i["mq"][l, es[v]:es[v + 1]], i["mt"][l, es[v]:es[v + 1]]) for v in range(i["B"])], None)
        got = {}
        for loss in ('labels', 'boxes', 'cardinality'):
            got.update(crit.get_loss(loss, out, targets, indices, i["num_boxes"]))
        rows.append([got[k].to(dt) for k in R.LOSS_KEYS])
    gl = i["gl"]
    total = sum(rows[l][k] * float(gl[l, k]) for l in range(i["nl"]) for k in range(5) if float(gl[l, k]) != 0.0)
    grads = torch.autograd.grad(total, leaves)
    out = {k: torch.stack([r[j].detach() for r in rows]) for j, k in enumerate(R.LOSS_KEYS)}
    out.update(d_logits=grads[0], d_counts=grads[1], d_boxes=grads[2])
    return out


@pytest.mark.parametrize("name", ["crit_layers3", "crit_g15_aneg_b05", "crit_g1_gau0", "crit_g1_b2_wd2", "crit_aneg_gau0_wd2",
                                  "crit_clamp_wd11", "crit_card_ties", "crit_ties", "crit_single_match", "crit_zero_match"])
def test_criterion_restatement_equals_get_loss_in_fp64(name):
    """the default hyper-parameters, gamma = 1.5 / alpha = -1 / beta = 0.5, gamma = 1 / gau_mask = 0 and more; ties, the count clamp
    and videos below two matches included"""
    i = R.inputs(name)
    want, got = project_criterion(i), R.reference(name)[0]
    assert sorted(want) == sorted(got)
    for k in want:
        if k == "cardinality_error":                      # (a logging figure the project computes in fp32 whatever the inputs' type)
            assert torch.equal(got[k].float(), want[k].float())
            continue
        close(got[k], want[k], (name, k))


@pytest.mark.parametrize("name", ["cost_nc3", "cost_nc1_bbox_g1", "cost_noclass_bbox_g15", "cost_g15", "cost_range30"])
def test_cost_restatement_equals_cost_matrix_in_fp64(name):
    from gvl_amd.matcher import HungarianMatcher
    i = R.inputs(name)
    w = i["w"]
    m = HungarianMatcher(cost_class=w[0], cost_bbox=w[1], cost_giou=w[2], cost_alpha=i["alpha"], cost_gamma=i["gamma"])
    got, ok = R.reference(name)[0]["cost"], R.reference(name)[0]["ok"]
    gotp = R.reference(name)[0]["cost_padded"]
    for l in range(i["nl"]):
        out = {"pred_logits": i["logits"][l].double(), "pred_boxes": i["boxes"][l].double()}
        C, flag = m.cost_matrix(out, None, tgt_cat=(i["tlabels"], i["tboxes"].double()), with_flag=True)
        close(got[l], C, (name, l))
        assert bool(flag) and ok
        # the padded form: the video's own block, 0 beyond the count
        for b in range(i["B"]):
            n = min(int(i["pcounts"][b]), i["slots"])
            one = {"pred_logits": i["logits"][l, b:b + 1].double(), "pred_boxes": i["boxes"][l, b:b + 1].double()}
            if n < i["slots"]:
                assert float(gotp[l, b, :, n:].abs().max()) == 0.0
            if n:
                C = m.cost_matrix(one, None, tgt_cat=(i["plabels"][b, :n], i["pboxes"][b, :n].double()))
                close(gotp[l, b, :, :n], C[0], (name, l, b))


@pytest.mark.parametrize("name", ["ce_V37_pad0", "ce_V257_pad3", "ce_V1_pad0"])
def test_ce_rows_restatement_equals_log_softmax_gather_in_fp64(name):
    i = R.inputs(name)
    got = R.reference(name)[0]
    live = i["weight"] != 0
    x = i["x"][live].double().requires_grad_()
    logp = F.log_softmax(x, -1)
    out = logp.gather(1, i["target"][live][:, None]).squeeze(1) * i["weight"][live].double()
    dx, = torch.autograd.grad((out * i["g"][live].double()).sum(), x)
    close(got["out"][live], out.detach(), "out")
    close(got["dx"][live], dx, "dx")
    close(got["lse"][live], torch.logsumexp(x.detach(), -1), "lse")
    for k in ("out", "lse", "dx"):
        assert float(got[k][~live].abs().max()) == 0.0, k


def test_criterion_restatement_passes_gradcheck_where_nothing_ties():
    i = R.inputs("crit_layers1")
    assert not _has_tie(i)
    gl = i["gl"].double()

    def f(logits, counts, boxes):
        t = R.criterion(logits, counts, boxes, R.matches_of(i), (i["tlabels"], i["tboxes"]), i["gt_counts"], i["ccr"], i["num_boxes"],
                        i["alpha"], i["gamma"], i["beta"], i["gau"])
        return (t[:, :5] * gl[:, :5]).sum()
    leaves = tuple(i[k].double().requires_grad_() for k in ("logits", "counts", "boxes"))
    assert torch.autograd.gradcheck(f, leaves, eps=1e-6, atol=1e-8, rtol=1e-5)


# ---------------------------------------------------------------------------------------------------------------------------
# every case has the property it is named for
# ---------------------------------------------------------------------------------------------------------------------------
def _pairs(i, l):
    """fp32 ends of the matched predictions and of their targets in layer l, per pair"""
    src = i["boxes"][l][i["vid"], i["mq"][l]]
    dst = i["tboxes"][i["tbase"] + i["mt"][l]]
    return R.ends(src), R.ends(dst)


def _has_tie(i):
    for l in range(i["nl"]):
        (s0, s1), (t0, t1) = _pairs(i, l)
        same = i["vid"][:, None] == i["vid"][None, :]
        off = same & ~torch.eye(len(s0), dtype=torch.bool)
        if bool(((s0 == t0) | (s1 == t1) | (s1 == t0) | (s0 == t1)).any()):
            return True
        for a in (s0, s1):
            for b in (s0, s1):
                if bool(((a[:, None] == b[None, :]) & off).any()):
                    return True
    return False


def _exact(box):
    """c -+ l / 2 has no rounding in fp32"""
    a32, a64 = R.ends(box), R.ends(box.double())
    return bool((a32[0].double() == a64[0]).all()) and bool((a32[1].double() == a64[1]).all())


def test_tie_case_ties_exactly_in_fp32():
    i = R.inputs("crit_ties")
    assert _exact(i["boxes"]) and _exact(i["tboxes"])
    assert (i["boxes"][..., 0] * 64 == (i["boxes"][..., 0] * 64).round()).all() and (i["boxes"][..., 1] * 32 == (i["boxes"][..., 1] * 32).round()).all()
    assert min(i["sizes"]) >= 2 and torch.bincount(i["vid"], minlength=i["B"]).min() >= 2       # a defined self-IoU in every video
    r = i["roles"]
    assert sorted(r) == sorted(R.TIE_PAIRS)
    for l in range(i["nl"]):
        (s0, s1), (t0, t1) = _pairs(i, l)
        d = torch.minimum(s1, t1) - torch.maximum(s0, t0)
        hull = torch.maximum(s1, t1) - torch.minimum(s0, t0)
        e = r["equal"]
        assert s0[e] == t0[e] and s1[e] == t1[e]
        k = r["identical"]
        assert s0[k] == s0[e] and s1[k] == s1[e] and i["vid"][k] == i["vid"][e] and i["mq"][l, k] != i["mq"][l, e]
        k = r["touching"]
        assert d[k] == 0 and s1[k] == t0[k] and s1[k] > s0[k]                        # rb - lt == 0
        assert s1[k] == s0[e]                                                        # ... and with the two predictions above
        k = r["disjoint"]
        assert d[k] < 0 and d[k].clamp(min=0) == 0 and hull[k] > 0                   # inter == 0 < area
        k = r["containing"]
        assert s0[k] < t0[k] and t1[k] < s1[k]
        k = r["contained"]
        assert t0[k] < s0[k] and s1[k] < t1[k]
        k = r["zero_length"]
        assert s0[k] == s1[k] and t0[k] < s0[k] < t1[k] and d[k] == 0
        assert s0[k] == s0[r["containing"]] and i["vid"][k] == i["vid"][r["containing"]]       # a min / max tie inside the self-IoU
    # the fp32 evaluation of the reference sees the same ties: its box gradient is the fp64 one to rounding, not half a term off
    w64, w32 = R.reference("crit_ties")
    assert float((w64["d_boxes"] - w32["d_boxes"].double()).abs().max()) <= 1e-5 * float(w64["d_boxes"].abs().max())
    row = w64["d_boxes"][0, i["vid"][r["equal"]], i["mq"][0, r["equal"]]]
    assert bool((row != 0).any())                                                    # equal to its target, identical to another: not trivial


def test_card_case_ties_on_the_argmax():
    i = R.inputs("crit_card_ties")
    x = i["logits"][:, 0]
    assert i["NC"] == 3
    for q, row in R.CARD_ROWS.items():
        assert x[0, q].tolist() == list(row)
    top = x.amax(-1, keepdim=True)
    tied = (x == top).sum(-1)
    assert sorted(tied[0, :5].tolist()) == [1, 2, 2, 2, 3]
    assert bool(((x[0, :5, 2] == top[0, :5, 0]) & (tied[0, :5] > 1)).any())         # a tie that includes the last class
    assert x[0, :5].argmax(-1).tolist() == [0, 1, 0, 0, 2]                           # the first maximal index wins


@pytest.mark.parametrize("name", CRIT)
def test_criterion_case_table(name):
    i = R.inputs(name)
    B, Q, NC, Wd = i["B"], i["Q"], i["NC"], i["Wd"]
    assert i["logits"].dtype == torch.float32 and float(i["logits"].abs().max()) <= 6.0
    assert B * Q <= 24576
    cnt = torch.bincount(i["vid"], minlength=B)
    assert cnt.tolist() == [min(Q, n) for n in i["sizes"]] and i["ent_start"].tolist() == [0] + cnt.cumsum(0).tolist()
    for l in range(i["nl"]):                              # a matching: distinct queries and distinct targets per video
        for v in range(B):
            a, b = int(i["ent_start"][v]), int(i["ent_start"][v + 1])
            assert len(set(i["mq"][l, a:b].tolist())) == b - a and len(set(i["mt"][l, a:b].tolist())) == b - a
            assert b == a or (0 <= int(i["mt"][l, a:b].min()) and int(i["mt"][l, a:b].max()) < i["sizes"][v])
    if i["nl"] > 1 and name != "crit_ties" and len(i["vid"]):
        assert not torch.equal(i["mq"][0], i["mq"][1])    # different matches per layer
    assert len(set(i["gl"][:, :4].flatten().tolist())) == 4 * i["nl"]
    single, zero = R.SINGLE_MATCH.get(name, []), R.ZERO_MATCH.get(name, [])
    assert [v for v in range(B) if cnt[v] == 1] == single and [v for v in range(B) if cnt[v] == 0] == zero
    assert (name in R.SELF_IOU_NAN) == bool(single or zero)
    assert (name in R.CLAMP) == bool((i["gt_counts"] >= Wd).any())
    if name == "crit_clamp_wd11":
        assert i["gt_counts"].tolist() == [0, Wd - 1, Wd + 1]
    if name.startswith("crit_threads_"):
        assert B * Q * NC == int(name.rsplit("_", 1)[1])
    if name == "crit_lds_limit":
        assert B * Q == 24576
    # the only non-finite reference value anywhere is loss_self_iou, in the cases listed for it
    for w in R.reference(name):
        for k, t in w.items():
            if k == "loss_self_iou" and name in R.SELF_IOU_NAN:
                assert bool(torch.isnan(t).all()), k
            else:
                assert bool(torch.isfinite(t).all()), k
    if name in R.SELF_IOU_NAN:
        assert float(i["gl"][:, 4].abs().max()) == 0.0
        unmatched = torch.ones(i["nl"], B, Q, dtype=torch.bool)
        for l in range(i["nl"]):
            unmatched[l, i["vid"], i["mq"][l]] = False
        if bool(unmatched.any()):                         # unmatched queries get exactly 0
            assert float(R.reference(name)[0]["d_boxes"][unmatched].abs().max()) == 0.0
    if name in R.PADDED:
        p = R.padded_layout(i, max(i["sizes"]) + 1)
        assert bool((p["pair_count"] < p["ent_start"][1:] - p["ent_start"][:-1]).all())         # unused pair slots in every video
        assert 0 <= int(p["mq"].min()) and int(p["mq"].max()) < Q and 0 <= int(p["mt"].min()) and int(p["mt"].max()) <= max(i["sizes"])


def test_a_padded_case_has_a_video_whose_slots_are_all_empty():
    assert "crit_zero_match" in R.PADDED
    i = R.inputs("crit_zero_match")
    assert R.padded_layout(i, 4)["pair_count"].tolist() == [2, 0, 3]


@pytest.mark.parametrize("name", COST)
def test_cost_case_table(name):
    i = R.inputs(name)
    assert float(i["logits"].abs().max()) <= i["amp"] and (i["amp"] == 6.0 or float(i["logits"].abs().max()) == 30.0)
    assert sorted(set(i["tlabels"].tolist())) == list(range(i["NC"]))                # labels over all classes
    n = i["nl"] * i["B"] * i["Q"]
    if name == "cost_stride":
        assert n * i["G"] > 4096 * 256 and n * i["slots"] > 4096 * 256                 # the stride loop runs twice
        assert n * i["G"] <= 2 * 4096 * 256
    c, S = i["pcounts"].tolist(), i["slots"]
    assert 0 in c and S in c and max(c) > S                                          # counts of 0, of `slots`, and above
    (s0, s1), (t0, t1) = R.ends(i["boxes"][0, 0]), R.ends(i["tboxes"][0])
    d = torch.minimum(s1, t1) - torch.maximum(s0, t0)
    assert s0[0] == t0 and s1[0] == t1 and d[1] == 0 and d[2] < 0 and s0[3] == s1[3]   # identical, touching, disjoint, zero length
    for w in R.reference(name):
        assert w["ok"] and w["ok_padded"]
        assert bool(torch.isfinite(w["cost"]).all()) and bool(torch.isfinite(w["cost_padded"]).all())


def test_the_flag_falls_for_a_negative_length_and_a_nan_box_only():
    i = R.inputs("cost_nc3")
    w = i["w"]
    for what, value, ok in (("prediction", -0.25, False), ("target", -0.125, False), ("prediction", float("nan"), False),
                            ("prediction", 0.0, True)):
        boxes, tboxes = i["boxes"].clone(), i["tboxes"].clone()
        if what == "prediction":
            boxes[1, 2, 5, 1] = value
        else:
            tboxes[3, 1] = value
        assert R.match_cost(i["logits"], boxes, i["tlabels"], tboxes, w[0], w[1], w[2], i["alpha"], i["gamma"])[1] == ok, (what, value)


@pytest.mark.parametrize("name", CE)
def test_ce_case_table(name):
    i = R.inputs(name)
    V, x, t = i["V"], i["x"], i["target"]
    assert int(t.min()) >= 0 and int(t.max()) < V
    for r, kind in enumerate(R.CE_ROWS):
        live = float(i["weight"][r]) != 0.0
        assert live == (not kind.startswith("masked"))
        if live:
            assert bool(torch.isfinite(x[r]).all())
        if kind == "constant":
            assert float(x[r].max()) == float(x[r].min())
        elif kind == "target_max":
            assert float(x[r, t[r]]) == float(x[r].max())
        elif kind == "target_min":
            assert float(x[r, t[r]]) == float(x[r].min())
        elif kind.startswith("peak") and V > 1:
            top = x[r].topk(2).values
            assert float(top[0] - top[1]) >= 80.0 and (kind != "peak_target" or float(x[r, t[r]]) == float(top[0]))
        elif kind == "masked_nan":
            assert bool(torch.isnan(x[r]).all())
        elif kind == "masked_inf":
            assert bool(torch.isinf(x[r]).all())
    for w in R.reference(name):
        for k in ("out", "lse", "dx"):
            assert bool(torch.isfinite(w[k]).all()), k

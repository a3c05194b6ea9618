"""The Transformer-DSA caption head (gvl_amd/CaptioningHead/Transformer_DSA.py) and the model around it on the GPU, against the
fixtures the imported reference produced under CUDA-op semantics (tests/golden/transformer_cap_{a6,a34,b}.npz,
pdvc_transformer_cap.npz; generator: tests/golden/make_golden_transformer_cap.py).  Tolerances are those tests/test_gpu_model.py
applies: 5e-4 on log-probs, 1e-3 on loss terms, 2e-3 (relative to max(1, scale)) on gradients.

Greedy tokens are compared exactly on STRICT rows -- rows whose smallest top-2 log-prob margin in the reference's decode is at
least 10 x the log-prob tolerance; a row that is not strict is compared up to its first step below that margin."""
import ast
import copy

import numpy as np
import pytest
import torch

import transformer_cap_ref as R
from helpers import load, maxerr, path_census, pdvc_dt, pdvc_state, synth_state_dict, t

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
_HEADS = {}


def gpu_head(case):
    """the head of a fixture's case with the fixture's weights (built once per case; tests that change it take a deepcopy)"""
    if case not in _HEADS:
        from gvl_amd.CaptioningHead import build_captioner
        f = load("transformer_cap_" + case)
        head = build_captioner(R.head_opt(case))
        shapes = {str(n): ast.literal_eval(str(s)) for n, s in zip(f["param_names"], f["param_shapes"])}
        sd = {k: t(v) for k, v in synth_state_dict(shapes, int(f["seed"])).items()}
        sd["pos_table"] = t(f["pos_table"])
        sd["logits.weight"] = sd["logits.weight"] * float(f["logit_scale"])
        head.load_state_dict(sd, strict=True)
        _HEADS[case] = (f, head.to(DEV).eval())
    return _HEADS[case]


def gpu_inputs(case, seed=1):
    from gvl_amd.deformable_transformer import make_level_tensors
    inp = R.head_inputs(case, seed)
    tshapes, lsi = make_level_tensors(inp["lens"], DEV)
    o = inp["others"]
    others = {"memory": o["memory"].to(DEV), "spatial_shapes": tshapes, "level_start_index": lsi,
              "mask_flatten": o["mask_flatten"].to(DEV), "valid_ratios": o["valid_ratios"].to(DEV)}
    return dict(hs=inp["hs"].to(DEV), reference=inp["reference"].to(DEV), others=others, seq=inp["seq"].to(DEV),
                cap_mask=inp["cap_mask"].to(DEV), gout=inp["gout"].to(DEV))


def hold_grad(name, got, want):
    want = np.asarray(want)
    bound = R.GRAD_TOL * max(1.0, float(np.abs(want).max()))
    err = maxerr(got, want)
    print(f"GRAD {name} error {err:.3e} bound {bound:.3e}")
    assert err <= bound, (name, err, bound)


def compare_decode(name, seq, lp, want_seq, want_lp, margins):
    """strict rows: tokens exactly, log-probs within LOGPROB_TOL, over every returned step; the others up to their first near tie"""
    want_seq, want_lp = np.asarray(want_seq), np.asarray(want_lp)
    keep = want_seq.shape[1]
    strict, first = R.strict_rows(margins, keep)
    assert strict.sum() * 3 >= 2 * len(strict), name
    if strict.all():
        assert isinstance(seq, torch.Tensor) and seq.shape == want_seq.shape, (name, getattr(seq, "shape", None), want_seq.shape)
    seq, lp = seq.cpu().numpy(), lp.cpu().numpy()
    for r in range(len(strict)):
        k = keep if strict[r] else min(int(first[r]), seq.shape[1])
        assert np.array_equal(seq[r, :k], want_seq[r, :k]), (name, r, seq[r], want_seq[r])
        err = float(np.abs(lp[r, :k] - want_lp[r, :k]).max()) if k else 0.0
        print(f"DECODE {name} row {r} strict {bool(strict[r])} steps {k} log-prob error {err:.3e}")
        assert err < R.LOGPROB_TOL, (name, r, err)
    return strict


# ---- teacher forcing ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(R.HEAD_CASES))
def test_teacher_forcing_matches_reference(case):
    f, head = gpu_head(case)
    inp = gpu_inputs(case)
    hs = inp["hs"].clone().requires_grad_()
    others = dict(inp["others"])
    others["memory"] = inp["others"]["memory"].clone().requires_grad_()
    head.zero_grad()
    logp = head(hs, inp["reference"], others, inp["seq"])
    err = maxerr(logp, f["logp"])
    print(f"LOGP {case} error {err:.3e}")
    assert err < R.LOGPROB_TOL
    rows = head.build_loss(logp, inp["seq"][:, 1:], inp["cap_mask"][:, 1:])
    assert maxerr(rows, f["loss_rows"]) < R.LOSS_TOL
    (logp * inp["gout"]).sum().backward()
    params = dict(head.named_parameters())
    names = [str(n) for n in f["grad_names"]]
    assert sorted(n for n, p_ in params.items() if p_.grad is not None) == names
    for n, want in zip(names, f["grad_norms"]):
        got = float(params[n].grad.double().norm())
        assert abs(got - float(want)) <= R.GRAD_TOL * max(1.0, float(want)), (n, got, float(want))
        hold_grad(f"{case}/{n}", R.grad_sample(params[n].grad), f["grad." + n])
    hold_grad(f"{case}/hs", hs.grad, f["grad_hs"])
    hold_grad(f"{case}/memory", others["memory"].grad, f["grad_memory"])
    head.zero_grad()


def test_steps_shortens_the_positions_not_the_loss():
    """`steps` (PDVC.caption_prediction: 1 + the longest caption) computes positions [0, steps] only; loss and gradients unchanged"""
    f, head = gpu_head("a6")
    inp = gpu_inputs("a6")
    seq, mask = inp["seq"].clone(), inp["cap_mask"].clone()
    seq[:, 4:] = 0                                                  # at most 3 words: the loss reads positions 0..3
    mask[:, 5:] = 0
    res = []
    for steps in (None, 4):
        head.zero_grad()
        hs = inp["hs"].clone().requires_grad_()
        logp = head(hs, inp["reference"], inp["others"], seq, steps=steps)
        assert logp.shape[1] == (seq.shape[1] if steps is None else steps + 1)
        rows = head.build_loss(logp, seq[:, 1:], mask[:, 1:])
        rows.sum().backward()
        res.append((rows.detach(), hs.grad, {n: p_.grad.clone() for n, p_ in head.named_parameters() if p_.grad is not None}))
    assert maxerr(res[0][0], res[1][0]) <= 1e-5 * max(1.0, float(res[0][0].abs().max())) and maxerr(res[0][1], res[1][1]) <= 1e-4 * max(1.0, float(res[0][1].abs().max()))
    assert sorted(res[0][2]) == sorted(res[1][2])
    for n, g in res[0][2].items():
        assert maxerr(g, res[1][2][n]) <= 1e-4 * max(1.0, float(g.abs().max())), n
    head.zero_grad()


# ---- greedy decoding ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(R.HEAD_CASES))
def test_greedy_decode_matches_reference(case):
    f, head = gpu_head(case)
    inp = gpu_inputs(case)
    seq, lp = head.sample(inp["hs"], inp["reference"], inp["others"])
    strict = compare_decode(case, seq, lp, f["sample_seq"], f["sample_lp"], f["margins"])
    want = f["sample_seq"]
    full = (want != 0).all(1) & (want.shape[1] == R.HEAD_CASES[case]["T"])
    assert (strict & full).any() and (strict & (want == 0).any(1)).any()          # what the generator promised


def test_decode_equals_the_uncached_forward_at_T34():
    """every emitted position's log-prob equals the head's own uncached forward on the decoded sequence (35 cached positions: a
    cache indexed one off, or a position read past a 32-position boundary, shows here)"""
    f, head = gpu_head("a34")
    inp = gpu_inputs("a34")
    seq, lp = head.sample(inp["hs"], inp["reference"], inp["others"])
    assert seq.shape[1] == 34
    inputs = torch.cat([torch.zeros_like(seq[:, :1]), seq[:, :-1]], 1)
    with torch.no_grad():
        logp = head(inp["hs"], inp["reference"], inp["others"], inputs)
    top, arg = logp.max(-1)
    ends = []
    for r in range(seq.shape[0]):
        zero = (seq[r] == 0).nonzero()
        e = int(zero[0]) if len(zero) else seq.shape[1] - 1            # the row's last fed position: its end token, or the last step
        ends.append(e)
        assert torch.equal(arg[r, :e + 1], seq[r, :e + 1]), r
        err = maxerr(top[r, :e + 1], lp[r, :e + 1])
        print(f"SELF row {r} end {e} error {err:.3e}")
        assert err < R.LOGPROB_TOL, (r, err)
        assert not seq[r, e + 1:].any()                                  # zero behind the end token
    assert len(set(ends)) > 1                                            # rows end at different steps


def _keep_of(head, inp):
    seq, _ = head.sample(inp["hs"], inp["reference"], inp["others"])
    return (seq.shape[1] if isinstance(seq, torch.Tensor) else 0), seq


def test_termination_by_the_end_tokens_bias():
    """logits.bias[0] decides when rows end.  The step a row ends at never grows with the bias, so the number of returned columns is
    monotone in it: the smallest bias (to 2^-20 of the bracket) that returns at most 2 columns is bisected -- over a few input seeds:
    with these weights the end token loses ground from step to step in most rows, and the bias that ends EVERY row by token 2 then
    ends them all at once; the third seed has a row that goes the other way -- and the output there is trimmed to exactly 2 columns.
    A bias that makes every first token <end> returns ([], [])."""
    _, base = gpu_head("b")
    head = copy.deepcopy(base)
    found = None
    for seed in range(1, 9):
        inp = gpu_inputs("b", seed)
        lo, hi = -200.0, 200.0                                            # keep(lo) = T presumably, keep(hi) = 0
        for _ in range(24):
            mid = 0.5 * (lo + hi)
            with torch.no_grad():
                head.logits.bias[0] = mid
            keep, _ = _keep_of(head, inp)
            lo, hi = (mid, hi) if keep > 2 else (lo, mid)
        with torch.no_grad():
            head.logits.bias[0] = hi
        keep, seq = _keep_of(head, inp)
        if keep == 2:
            found = (seed, hi, seq)
            break
    assert found is not None
    seq = found[2]
    assert seq.shape == (10, 2) and bool(seq[:, 1].any()) and bool((seq[:, 0] != 0).any())
    with torch.no_grad():
        head.logits.bias[0] = 1e4
    assert _keep_of(head, gpu_inputs("b")) == (0, [])
    seq, lp = head.sample(inp["hs"], inp["reference"], inp["others"])
    assert seq == [] and lp == []


@pytest.mark.parametrize("case", ["a6", "b"])
def test_graph_decode(case):
    """graph_decode: the replay is bitwise the eager decode, also for other inputs of the same shape; a parameter update re-captures"""
    _, base = gpu_head(case)
    head = copy.deepcopy(base)
    a, b = gpu_inputs(case, 1), gpu_inputs(case, 2)
    eager = [head.sample(i_["hs"], i_["reference"], i_["others"]) for i_ in (a, b)]
    head.graph_decode = True
    for i_, (seq_e, lp_e) in zip((a, b, a), eager + eager[:1]):
        seq_g, lp_g = head.sample(i_["hs"], i_["reference"], i_["others"])
        assert torch.equal(seq_g, seq_e) and torch.equal(lp_g, lp_e)
    assert len(head._decode_graphs) == 1
    key0 = next(iter(head._decode_graphs))
    with torch.no_grad():
        head.logits.bias.add_(torch.linspace(-1.0, 1.0, head.logits.bias.numel(), device=DEV))
    seq_g, lp_g = head.sample(a["hs"], a["reference"], a["others"])
    key1 = next(iter(head._decode_graphs))
    assert len(head._decode_graphs) == 1 and key1 != key0 and key1[:-1] == key0[:-1]
    head.graph_decode = False
    seq_e, lp_e = head.sample(a["hs"], a["reference"], a["others"])
    assert torch.equal(seq_g, seq_e) and torch.equal(lp_g, lp_e)
    assert not torch.equal(lp_e, eager[0][1])                              # the update was seen


def test_decode_under_autocast_is_the_fp32_decode():
    _, head = gpu_head("b")
    inp = gpu_inputs("b")
    want = head.sample(inp["hs"], inp["reference"], inp["others"])
    with torch.autocast("cuda", dtype=torch.bfloat16):
        got = head.sample(inp["hs"].bfloat16().float(), inp["reference"], inp["others"])
        same = head.sample(inp["hs"], inp["reference"], inp["others"])
    assert torch.equal(same[0], want[0]) and torch.equal(same[1], want[1]) and got[1].dtype == torch.float32


def test_path_census_at_real_width(monkeypatch):
    """C = 512, H = 8, V = 8517: per token and layer exactly one k_capt_attend and one deformable-attention forward launch, one
    argmax product per token, no log_softmax / cat inside sample, value_proj(memory) once per decode and layer"""
    from gvl_amd import layers as L
    from gvl_amd.CaptioningHead import build_captioner
    from gvl_amd.deformable_transformer import make_level_tensors
    B, Q, T, C, nl = 2, 10, 4, 512, 2
    torch.manual_seed(3)
    head = build_captioner(R.head_opt(dict(C=C, H=8, layers=nl, V=8517, T=T))).to(DEV).eval()
    lens = R.level_lengths(R.FRAMES)
    S = sum(lens)
    tshapes, lsi = make_level_tensors(lens, DEV)
    g = torch.Generator().manual_seed(4)
    others = {"memory": torch.randn(B, S, C, generator=g).to(DEV), "spatial_shapes": tshapes, "level_start_index": lsi,
              "mask_flatten": torch.zeros(B, S, dtype=torch.bool, device=DEV), "valid_ratios": torch.ones(B, 4, device=DEV)}
    hs, ref = torch.randn(B, Q, C, generator=g).to(DEV), (torch.rand(B, Q, 2, generator=g) * 0.5 + 0.25).to(DEV)
    head.defer_trim = True                               # the full loop whatever the random head emits
    head.sample(hs, ref, others)                          # weight planes are built once per parameter version: not part of a decode
    memory_rows = []
    real_linear = L.linear

    def counting_linear(a, w, segs, a2=None, flags=0):
        memory_rows.append(a.shape[0])
        return real_linear(a, w, segs, a2=a2, flags=flags)

    def forbidden(*a, **k):
        raise AssertionError("torch.log_softmax / torch.cat inside sample")
    monkeypatch.setattr(L, "linear", counting_linear)
    monkeypatch.setattr(torch, "log_softmax", forbidden)
    monkeypatch.setattr(torch, "cat", forbidden)
    (seq, lp), tags = path_census(lambda: head.sample(hs, ref, others))
    monkeypatch.undo()
    assert seq.shape == (B * Q, T) and torch.isfinite(lp).all()
    print("CENSUS", dict(tags))
    assert tags["capt_attend"] == T * nl and tags["capt_embed"] == T
    assert tags["fwd_t1d_d64"] == T * nl
    assert tags["gemm_f16x3"] == T
    assert memory_rows.count(B * S) == nl                 # value_proj(memory): once per decode and layer, not per token
    assert len(memory_rows) == 2 * nl + T * nl * 6        # per token and layer: q|k|v, dim_project, offsets|weights, output_proj, FFN x 2


# ---- the model ----------------------------------------------------------------------------------------------------------------------
def to_dev(dt):
    out = dict(dt)
    for k in ("video_tensor", "video_mask", "video_length"):
        out[k] = dt[k].to(DEV)
    out["video_target"] = [{k: v.to(DEV) for k, v in tg.items()} for tg in dt["video_target"]]
    return out


def build_model(f, train=False):
    from gvl_amd.config import make_opt
    from gvl_amd.pdvc import build
    over = dict(transformer_dropout_prob=0.0, drop_prob=0.0) if train else {}
    opt = make_opt(num_queries=5, feature_dim=64, vocab_size=60, max_caption_len=6, device="cuda",
                   caption_decoder_type="transformer", cap_nheads=8, **over)
    model, criterion, _, post = build(opt)
    own = model.state_dict()
    assert sorted(own) == [str(n) for n in f["param_names"]]
    sd = pdvc_state(f, int(f["seed"]))                              # (resolves the names of tied tensors as load_state_dict does)
    for k in sd:
        if k.endswith("pos_table"):
            sd[k] = own[k]                                          # a buffer the constructor computes
        if k.endswith("logits.weight"):
            sd[k] = sd[k] * float(f["logit_scale"])
    model.load_state_dict(sd, strict=True)
    return opt, model.to(DEV), criterion, post


@pytest.fixture(scope="module")
def model_eval():
    f = load("pdvc_transformer_cap")
    opt, model, criterion, post = build_model(f)
    return f, opt, model.eval(), criterion, post


def test_model_eval_matches_reference(model_eval):
    from test_gpu_pipeline import LOADER
    f, opt, model, criterion, post = model_eval
    dt = to_dev(pdvc_dt(f))
    with torch.no_grad():
        out, loss = model(dt, criterion, None, "queries", eval_mode=True)
    assert maxerr(out["pred_logits"], f["pred_logits"]) < 5e-4
    assert maxerr(out["pred_boxes"], f["pred_boxes"]) < 1e-4
    assert maxerr(out["pred_count"], f["pred_count"]) < 5e-4
    Bv, Qn, keep = f["seq"].shape
    strict = compare_decode("model", out["seq"].reshape(Bv * Qn, -1), out["caption_probs"]["cap_prob_eval"].reshape(Bv * Qn, -1),
                            f["seq"].reshape(Bv * Qn, keep), f["cap_prob_eval"].reshape(Bv * Qn, keep), f["margins"])
    for k in [k for k in f if k.startswith("loss.")]:
        assert maxerr(loss[k[5:]].reshape(()), f[k].reshape(())) < 5e-4 or (f[k] != f[k]).all(), k
    res = post["bbox"](out, dt["video_length"][:, 1], LOADER)
    for i, r in enumerate(res):
        assert maxerr(torch.as_tensor(r["scores"]), f[f"post.{i}.scores"]) < 5e-4
        assert maxerr(torch.as_tensor(r["boxes"]), f[f"post.{i}.boxes"]) < 2e-2        # seconds: 1e-4 of a box x the duration
        qid = torch.as_tensor(r["query_id"]).cpu().numpy()
        assert np.array_equal(qid, f[f"post.{i}.query_id"])
        assert np.array_equal(torch.as_tensor(r["raw_idx"]).cpu().numpy(), f[f"post.{i}.raw_idx"])
        assert torch.equal(torch.as_tensor(r["labels"]).cpu(), t(f[f"post.{i}.labels"]))
        assert int(r["pred_seq_len"]) == int(f[f"post.{i}.pred_seq_len"])              # (the predicted number of events)
        rows = strict[i * Qn + qid]
        assert [c for c, s_ in zip(r["captions"], rows) if s_] == [str(c) for c, s_ in zip(f[f"post.{i}.captions"], rows) if s_]
        got_cs = np.asarray(r["caption_scores"], np.float64)[rows]
        assert np.abs(got_cs - f[f"post.{i}.caption_scores"][rows]).max() < 5e-4 * keep


def test_graphed_eval_forward_equals_eager(model_eval):
    from gvl_amd.parallel import GraphedEvalForward
    f, opt, model, criterion, post = model_eval
    dt = to_dev(pdvc_dt(f))
    with torch.no_grad():
        out_e, loss_e = model(dt, criterion, None, "queries", eval_mode=True)
    graphed = GraphedEvalForward(model, criterion)
    for _ in range(2):
        out_g, loss_g = graphed(dt)
        assert torch.equal(out_g["seq"], out_e["seq"])
        assert maxerr(out_g["caption_probs"]["cap_prob_eval"], out_e["caption_probs"]["cap_prob_eval"]) < 1e-5
        assert maxerr(out_g["pred_boxes"], out_e["pred_boxes"]) < 1e-5 and maxerr(out_g["pred_logits"], out_e["pred_logits"]) < 1e-5
    assert graphed.captures == 1


def train_batch(f):
    dt = to_dev(pdvc_dt(f))
    dt.update(cap_tensor=t(f["cap_tensor"]).to(DEV), cap_mask=t(f["cap_mask"]).to(DEV),
              gt_boxes_mask=torch.tensor([[1, 1, 1], [1, 1, 0]], dtype=torch.bool, device=DEV))
    return dt


def test_model_train_step_matches_reference():
    f = load("pdvc_transformer_cap")
    opt, model, criterion, _ = build_model(f, train=True)
    model.train()
    dt = train_batch(f)
    out, loss = model(dt, criterion, None, "queries")
    wd = criterion.weight_dict
    final = sum(loss[k] * wd[k] for k in loss.keys() if k in wd)
    final.backward()
    for k in [k for k in f if k.startswith("train_loss.")]:
        assert maxerr(loss[k[11:]].reshape(()), f[k].reshape(())) < R.LOSS_TOL, k
    assert abs(float(final) - float(f["final_loss"])) < 2e-3
    for i, (a, b) in enumerate(out["matched_indices"][0]):
        assert torch.equal(torch.stack([a, b]).cpu(), t(f[f"match_{i}"]))
    params = dict(model.named_parameters())
    names = [str(n) for n in f["grad_names"]]
    assert sorted(n for n, p_ in params.items() if p_.grad is not None) == names
    assert any(n.startswith("caption_head.") and "self_attention" in n for n in names)
    for n, want in zip(names, f["grad_norms"]):
        got = float(params[n].grad.double().norm())
        assert abs(got - float(want)) <= R.GRAD_TOL * max(1.0, float(want)), (n, got, float(want))
        hold_grad("model/" + n, R.grad_sample(params[n].grad)[::4], f["grad." + n])


def test_train_step_updates_the_head_and_padded_capture_refuses():
    from gvl_amd.parallel import GraphedTrainStep, TrainStep
    f = load("pdvc_transformer_cap")
    opt, model, criterion, _ = build_model(f, train=True)
    model.train()
    head = {n: p_.detach().clone() for n, p_ in model.named_parameters() if n.startswith("caption_head.")}
    assert len(head) > 20
    final, loss = TrainStep(model, criterion, opt)(train_batch(f))
    assert torch.isfinite(final) and "loss_caption" in loss and "loss_caption_0" in loss
    params = dict(model.named_parameters())
    for n, before in head.items():
        assert not torch.equal(params[n].detach(), before), n
    assert not model.supports_padded_targets(criterion, False)
    with pytest.raises(RuntimeError, match="padded=True"):
        GraphedTrainStep(model, criterion, opt, padded=True)(train_batch(f))

"""Beam-search decoding of the Transformer-DSA caption head over its KV cache (TransformerDSACaptioner.beam_search; DESIGN.md
sections 4.3 and 10) against an UNCACHED search: per token the head's own teacher-forced `forward` (pinned to the reference by
tests/test_gpu_transformer_cap.py::test_teacher_forcing_matches_reference) runs on every beam's full prefix, the last position's
log-probs go through the fp64 selection restatement of tests/test_gpu_beam.py, and the prefixes are re-ordered on the host.  The
oracle shares no cache, no lineage table and no selection kernel with the code under test.

Tolerances are the head's own (tests/transformer_cap_ref.py): LOGPROB_TOL on token log-probs, LOGPROB_TOL x emitted tokens on the
summed scores; a row is STRICT when the smallest gap between consecutive candidates among its top W + 1, over all steps of the
oracle's search, is at least STRICT_MARGIN = 10 x LOGPROB_TOL.  At most one eighth of the rows (rounded up) may be non-strict, and
of those only the best score is compared, within 4 x LOGPROB_TOL x emitted tokens.

The input seed and the amount logits.bias[0] is raised by (so that beams end at mixed lengths) are chosen per case such that the
ORACLE alone satisfies that cap and the preconditions below: CHOICE."""
import copy
import functools
import math

import pytest
import torch

import transformer_cap_ref as R
from helpers import maxerr, path_census
from test_gpu_beam import NEG, oracle_rank, step_restatement
from test_gpu_transformer_cap import gpu_head, gpu_inputs

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# case -> (beams, input seed of head_inputs, raise of logits.bias[0]).  Seed 1 (the fixtures' own inputs) and a raise of 1.0 in every
# case: a scan of seeds 1 .. 4 x raises 0.5 .. 4 through `uncached_search` and `preconditions` (the oracle alone) shows every
# precondition met there, with 0 of 6 (a6), 1 of 10 (b; cap 2) and 0 of 6 (a34) non-strict rows.  Raises from 1.5 (a6) and 3.0 (b)
# on no longer let the penalty change a best beam; a34 from 3.0 on keeps every best beam in one slot.
CHOICE = {"a6": (3, 1, 1.0), "b": (3, 1, 1.0), "a34": (2, 1, 1.0)}


class raised_end_bias:
    """logits.bias[0] raised for a scope"""

    def __init__(self, head, by):
        self.head, self.by = head, by

    def __enter__(self):
        with torch.no_grad():
            self.head.logits.bias[0] += self.by

    def __exit__(self, *exc):
        with torch.no_grad():
            self.head.logits.bias[0] -= self.by


def uncached_search(case, W, seed, bias0):
    """section 4.3 over head.forward on full prefixes -> per-step records (T, n, W) parent / token / logp / fin, final score (n, W),
    the smallest step gap of every row"""
    _, head = gpu_head(case)
    inp = gpu_inputs(case, seed)
    T = R.HEAD_CASES[case]["T"]
    B, Q, _ = inp["hs"].shape
    n = B * Q
    hs, ref = inp["hs"].repeat_interleave(W, 1), inp["reference"].repeat_interleave(W, 1)
    prefix = torch.zeros(n, W, 1, dtype=torch.long)                         # <bos>
    score = torch.full((n, W), NEG, dtype=torch.float64)
    score[:, 0] = 0.0
    fin = torch.zeros(n, W, dtype=torch.bool)
    rec = dict(parent=[], token=[], logp=[], fin=[])
    margin = torch.full((n,), float("inf"), dtype=torch.float64)
    with torch.no_grad(), raised_end_bias(head, bias0):
        for _ in range(T):
            logp = head(hs, ref, inp["others"], prefix.view(n * W, -1).to(DEV))[:, -1].cpu()
            st = step_restatement(logp.view(n, W, -1), score, fin)
            finite = torch.isfinite(st["score"]).all(1, keepdim=True) & torch.isfinite(st["gap"])
            margin = torch.minimum(margin, torch.where(finite, st["gap"], torch.full_like(st["gap"], float("inf"))).min(1).values)
            prefix = torch.cat([prefix.gather(1, st["parent"][:, :, None].expand(-1, -1, prefix.shape[2])), st["token"][:, :, None]], 2)
            score, fin = st["score"], st["fin"]
            for k in rec:
                rec[k].append(st[k])
    return {k: torch.stack(v) for k, v in rec.items()}, score, margin


@functools.lru_cache(maxsize=None)
def oracle(case):
    W, seed, bias0 = CHOICE[case]
    return uncached_search(case, W, seed, bias0)


def slots_of(rec, row, beam):
    """the slot of every position of a final beam's prefix: the chain of parents, last position first"""
    cur, slots = beam, []
    for step in range(rec["parent"].shape[0] - 1, -1, -1):
        cur = int(rec["parent"][step][row, cur])
        slots.append(cur)
    return slots


def preconditions(rec, score, margin, with_penalty):
    """what the oracle alone must show for a comparison against it to mean something -> dict of bools"""
    T, n, W = rec["parent"].shape
    plain = oracle_rank(rec, score, 0.0)
    best = plain["order"][:, 0]
    ident = torch.arange(W)[None].expand(n, W)
    ends = (plain["tokens"] == 0).any(2)
    out = {"cap": int((margin < R.STRICT_MARGIN).sum()) <= math.ceil(n / 8),
           "best beam visits two slots": any(len(set(slots_of(rec, r, int(best[r])))) >= 2 for r in range(n)),
           "re-ordered at t >= 2": any(bool((rec["parent"][step] != ident).any()) for step in range(2, T)),
           "mixed lengths in a row": any(len(set(plain["lengths"][r].tolist())) > 1 and bool(ends[r].any()) for r in range(n))}
    if with_penalty:
        out["penalty changes a best beam"] = bool((oracle_rank(rec, score, 1.0)["order"][:, 0] != best).any())
    return out


def device_search(case, length_penalty, head=None):
    W, seed, bias0 = CHOICE[case]
    head = gpu_head(case)[1] if head is None else head
    inp = gpu_inputs(case, seed)
    with torch.no_grad(), raised_end_bias(head, bias0):
        res = head.beam_search(inp["hs"], inp["reference"], inp["others"], W, length_penalty)
        return {k: v.cpu() for k, v in res.items()}


@pytest.mark.parametrize("case,length_penalty", [("a6", 0.0), ("a6", 1.0), ("b", 0.0), ("b", 1.0), ("a34", 0.0)])
def test_beam_search_equals_the_uncached_search(case, length_penalty):
    W = CHOICE[case][0]
    T = R.HEAD_CASES[case]["T"]
    rec, score, margin = oracle(case)
    n = score.shape[0]
    pre = preconditions(rec, score, margin, with_penalty=case != "a34")
    assert all(pre.values()), pre                                    # of the oracle, not of the code under test
    want = oracle_rank(rec, score, length_penalty)
    got = device_search(case, length_penalty)
    assert got["tokens"].shape == (n, W, T) and got["alive"].shape == (T,)
    strict = margin >= R.STRICT_MARGIN
    emitted = (want["lengths"] + 1).clamp(max=T).double()
    for r in range(n):
        err = abs(float(got["scores"][r, 0]) - float(want["scores"][r, 0]))
        print(f"BEAM {case} penalty {length_penalty} row {r} strict {bool(strict[r])} margin {float(margin[r]):.3e} best-score error {err:.3e}")
        if not strict[r]:
            assert err <= 4 * R.LOGPROB_TOL * float(emitted[r, 0]), (r, float(got["scores"][r, 0]), float(want["scores"][r, 0]))
            continue
        same = torch.equal(got["tokens"][r], want["tokens"][r]) and torch.equal(got["lengths"][r], want["lengths"][r])
        assert same, (r, float(margin[r]), got["scores"][r].tolist(), want["scores"][r].tolist(), got["tokens"][r].tolist(),
                      want["tokens"][r].tolist())
        assert maxerr(got["logprobs"][r], want["logprobs"][r]) <= R.LOGPROB_TOL
        assert bool(((got["scores"][r].double() - want["scores"][r]).abs() <= R.LOGPROB_TOL * emitted[r]).all()), r
    if bool(strict.all()):
        live = ~rec["fin"].view(T, -1).all(1)                       # some beam of some row still live after token t
        assert got["alive"].tolist() == live.tolist()


def test_beam_of_one_is_greedy():
    _, head = gpu_head("a6")
    inp = gpu_inputs("a6")
    with torch.no_grad():
        seq, lp = head.sample(inp["hs"], inp["reference"], inp["others"])
        res = head.beam_search(inp["hs"], inp["reference"], inp["others"], 1)
    keep = seq.shape[1]
    assert keep == int(res["lengths"].max()) >= 1
    assert torch.equal(res["tokens"][:, 0, :keep], seq)
    # greedy keeps booking log-probs behind a row's end token, the search books zeros there: compare up to the end token
    upto = (torch.arange(keep, device=DEV)[None] <= res["lengths"][:, :1]).float()
    assert maxerr(res["logprobs"][:, 0, :keep] * upto, lp * upto) <= R.LOGPROB_TOL


@pytest.mark.parametrize("case,length_penalty", [("a6", 0.0), ("b", 1.0)])
def test_sample_returns_the_best_beam_in_the_greedy_form(case, length_penalty):
    W, seed, bias0 = CHOICE[case]
    _, head = gpu_head(case)
    inp = gpu_inputs(case, seed)
    res = device_search(case, length_penalty)
    with raised_end_bias(head, bias0):
        seq, lp = head.sample(inp["hs"], inp["reference"], inp["others"], {"beam_size": W, "length_penalty": length_penalty})
    keep = int(res["lengths"][:, 0].max())
    if keep == 0:                                                    # every best caption is empty
        assert isinstance(seq, list) and isinstance(lp, list) and seq == [] and lp == []
        return
    n = res["tokens"].shape[0]
    assert tuple(seq.shape) == (n, keep) == tuple(lp.shape)
    assert torch.equal(seq.cpu(), res["tokens"][:, 0, :keep]) and torch.equal(lp.cpu(), res["logprobs"][:, 0, :keep])


def test_every_caption_empty_returns_empty_lists():
    _, base = gpu_head("b")
    head = copy.deepcopy(base)
    inp = gpu_inputs("b")
    with torch.no_grad():
        head.logits.bias[0] = 1e4
        res = head.beam_search(inp["hs"], inp["reference"], inp["others"], 3)
    assert int(res["lengths"][:, 0].max()) == 0                      # (the other beams of a row are its second and third first words)
    seq, lp = head.sample(inp["hs"], inp["reference"], inp["others"], {"beam_size": 3})
    assert isinstance(seq, list) and isinstance(lp, list) and seq == [] and lp == []


def test_graph_replayed_beam_search_equals_eager_bit_for_bit():
    W, _, bias0 = CHOICE["a6"]
    _, base = gpu_head("a6")
    head = copy.deepcopy(base)
    inputs = [gpu_inputs("a6", s_) for s_ in (1, 2, 3)]
    with torch.no_grad(), raised_end_bias(head, bias0):
        eager = [{k: v.clone() for k, v in head.beam_search(i_["hs"], i_["reference"], i_["others"], W, 1.0).items()} for i_ in inputs]
        greedy = head.sample(inputs[0]["hs"], inputs[0]["reference"], inputs[0]["others"])
        head.graph_decode = True
        for i_, want in zip(inputs, eager):                          # a capture, then two replays on other inputs
            got = head.beam_search(i_["hs"], i_["reference"], i_["others"], W, 1.0)
            for k in want:
                assert torch.equal(got[k], want[k]), k
        assert len(head._decode_graphs) == 1
        # the beam pair is part of the key: a greedy graph beside it, and another penalty is another graph
        seq_g, lp_g = head.sample(inputs[0]["hs"], inputs[0]["reference"], inputs[0]["others"])
        assert len(head._decode_graphs) == 2 and torch.equal(seq_g, greedy[0]) and torch.equal(lp_g, greedy[1])
        got = head.beam_search(inputs[0]["hs"], inputs[0]["reference"], inputs[0]["others"], W, 1.0)
        assert len(head._decode_graphs) == 2 and all(torch.equal(got[k], eager[0][k]) for k in eager[0])
        head.beam_search(inputs[0]["hs"], inputs[0]["reference"], inputs[0]["others"], W, 0.0)
        assert len(head._decode_graphs) == 3
    assert not torch.equal(eager[0]["tokens"], eager[1]["tokens"])


def test_beam_options_that_raise():
    _, base = gpu_head("a6")
    head = copy.deepcopy(base)
    inp = gpu_inputs("a6")
    args = (inp["hs"], inp["reference"], inp["others"])
    with torch.no_grad():
        for bad in (0, 9):
            with pytest.raises(ValueError, match="beam_size"):
                head.beam_search(*args, bad)
        with pytest.raises(ValueError, match="beam_size"):
            head.sample(*args, {"beam_size": 9})
        with pytest.raises(ValueError, match="sample_max"):
            head.sample(*args, {"beam_size": 3, "sample_max": 0})
        with torch.autocast("cuda", dtype=torch.bfloat16), pytest.raises(NotImplementedError, match="autocast"):
            head.beam_search(*args, 3)
    with pytest.raises(RuntimeError, match="no_grad"):
        head.beam_search(*args, 3)
    head.defer_trim = True
    with pytest.raises(NotImplementedError, match="defer_trim"):
        head.sample(*args, {"beam_size": 3})


def test_path_census_at_real_width(monkeypatch):
    """C = 512, H = 8, one layer, V = 8517, T = 6, W = 3: one selection launch per token, one lineage attention launch per token and
    layer and NO plain cached-attention launch, the inference layers of the greedy decode's census, the logits written by the plain
    split product (no fused argmax), no ATen topk / log_softmax / cat"""
    from gvl_amd import layers as L
    from gvl_amd.CaptioningHead import build_captioner
    from gvl_amd.deformable_transformer import make_level_tensors
    B, Q, T, C, nl, W = 2, 10, 6, 512, 1, 3
    torch.manual_seed(3)
    head = build_captioner(R.head_opt(dict(C=C, H=8, layers=nl, V=8517, T=T))).to(DEV).eval()
    lens = R.level_lengths(R.FRAMES)
    S = sum(lens)
    tshapes, lsi = make_level_tensors(lens, DEV)
    g = torch.Generator().manual_seed(4)
    others = {"memory": torch.randn(B, S, C, generator=g).to(DEV), "spatial_shapes": tshapes, "level_start_index": lsi,
              "mask_flatten": torch.zeros(B, S, dtype=torch.bool, device=DEV), "valid_ratios": torch.ones(B, 4, device=DEV)}
    hs, ref = torch.randn(B, Q, C, generator=g).to(DEV), (torch.rand(B, Q, 2, generator=g) * 0.5 + 0.25).to(DEV)
    rows = []
    real_linear = L.linear

    def counting_linear(a, w, segs, a2=None, flags=0):
        rows.append(a.shape[0])
        return real_linear(a, w, segs, a2=a2, flags=flags)

    def refuse(name):
        def fn(*a, **k):
            raise AssertionError(f"ATen {name} called inside the beam search")
        return fn

    with torch.no_grad():
        head.beam_search(hs, ref, others, W)                 # weight planes are built once per parameter version: not part of a search
        monkeypatch.setattr(L, "linear", counting_linear)
        for mod, name in ((torch, "topk"), (torch.Tensor, "topk"), (torch, "log_softmax"), (torch.Tensor, "log_softmax"),
                          (torch.nn.functional, "log_softmax"), (torch, "cat")):
            monkeypatch.setattr(mod, name, refuse(name))
        res, tags = path_census(lambda: head.beam_search(hs, ref, others, W))
        monkeypatch.undo()
    assert res["tokens"].shape == (B * Q, W, T) and torch.isfinite(res["scores"]).all()
    print("CENSUS", dict(tags))
    assert tags["beam_step_lineage"] == T and tags["beam_finish"] == 1 and tags["beam_step"] == 0
    assert tags["capt_attend_beam"] == T * nl and tags["capt_attend"] == 0 and tags["capt_embed"] == T
    assert tags["fwd_t1d_d64"] == T * nl
    assert tags["gemm_f16x3"] == T and tags["row_argmax_lse"] == 0
    assert rows.count(B * S) == nl                        # value_proj(memory): once per search and layer, per video
    assert rows.count(B * Q) == nl                        # the event-feature half of dim_project: per EVENT, not per beam
    assert len(rows) == 2 * nl + T * nl * 6               # per token and layer: q|k|v, dim_project, offsets|weights, output_proj, FFN x 2
    assert rows.count(B * Q * W) == T * nl * 6


def test_eval_forward_with_beam_size_feeds_postprocess():
    """PDVC.forward in eval mode with caption_decoder_type='transformer' and opt.beam_size = 3: seq / caption_probs in the form
    PostProcess turns into records; the whole-forward graph refuses the option"""
    from synth import synth_samples
    from gvl_amd.config import make_opt
    from gvl_amd.eval_utils import batch_result_json
    from gvl_amd.parallel import GraphedEvalForward
    from gvl_amd.pdvc import build
    from gvl_amd.video_dataset import collate_fn
    from test_gpu_pipeline import LOADER, to_device
    opt = make_opt(num_queries=10, feature_dim=16, vocab_size=60, max_caption_len=7, frame_embedding_num=64, device="cuda",
                   caption_decoder_type="transformer", cap_nheads=8)
    torch.manual_seed(0)
    model, criterion, _, post = build(opt)
    model = model.to(DEV).eval()
    dt = to_device(collate_fn(synth_samples()), DEV)
    with torch.no_grad():
        model.opt.beam_size, model.opt.beam_length_penalty = 3, 0.0
        (out, _), tags = path_census(lambda: model(dt, criterion, None, "queries", eval_mode=True))
        with pytest.raises(NotImplementedError, match="beam"):
            GraphedEvalForward(model, criterion)(dt)
    assert tags["beam_step_lineage"] == 7 * tags["beam_finish"] >= 7 and tags["capt_attend"] == 0 and tags["capt_attend_beam"] >= 7
    seq, lp = out["seq"], out["caption_probs"]["cap_prob_eval"]
    assert seq.dim() == 3 and seq.shape[:2] == (3, 10) and seq.shape == lp.shape and seq.shape[2] <= 7
    results = post["bbox"](out, dt["video_length"][:, 1], LOADER)
    records = batch_result_json(results, dt["video_key"], score_threshold=0)
    assert sorted(records) == ["v_000", "v_001", "v_002"]
    for events in records.values():
        assert len(events) == 10 and all(isinstance(e["sentence"], str) for e in events)

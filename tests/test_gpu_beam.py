"""Beam-search decoding of the LSTM-DSA captioner (gvl_amd/csrc/gvl_beam.hip, Captioner.beam_search).

The reference reads `beam_size` and drops it, so there is no reference output: the specification is restated here twice, in
fp64 on the CPU -- `step_restatement` for one token of the search fed the kernel's own logits, `oracle_beam_search` for the whole
search over the oracle's token step (oracle.torch_ref.captioner_step) -- and the device path is held against both.
tests/test_beam_cpu.py checks the preconditions of these comparisons (margins, mixed lengths) without a GPU."""
import functools

import pytest
import torch

from helpers import load, maxerr, path_census, pdvc_state, t

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PRE = "caption_head.1."
NEG = float("-inf")

# ---------------------------------------------------------------------------------------------------------------------------
# A. one token of the search
# ---------------------------------------------------------------------------------------------------------------------------
STEP_SHAPES = [(7, 1, 41), (7, 3, 41), (5, 2, 8518), (3, 5, 8518), (2, 8, 8518)]        # (event rows, beams, vocabulary + 1)
STEP_GAP = 1e-4            # the restatement's own gap between consecutive candidates among its top W + 1, every row
STEP_TOL = 1e-5            # scores and log-probs: fp32 log-sum-exp over 8518 terms at |score| <= 8 (ulp 1e-6)


def step_restatement(logits, score, fin):
    """section 4.3, one step, fp64: logits (n, W, V), score (n, W), fin (n, W) bool -> dict with the new beams in descending
    order of score (equal scores: the smaller flat index b V + v) and `gap`, the smallest difference between consecutive
    candidates among the top W + 1 of every row"""
    n, W, V = logits.shape
    logp = torch.log_softmax(logits.double(), -1)
    cand = score.double()[:, :, None] + logp
    ended = torch.full_like(cand, NEG)
    ended[:, :, 0] = score.double()
    cand = torch.where(fin[:, :, None], ended, cand)
    tok_lp = torch.where(fin[:, :, None], torch.zeros_like(logp), logp)
    val, idx = torch.sort(cand.view(n, W * V), dim=1, descending=True, stable=True)       # stable: ties keep the smaller index first
    top = val[:, :W + 1]
    gap = (top[:, :-1] - top[:, 1:])
    idx = idx[:, :W]
    parent, token = idx // V, idx % V
    new_fin = fin.gather(1, parent) | (token == 0)
    return dict(score=val[:, :W], parent=parent, token=token, logp=tok_lp.view(n, W * V).gather(1, idx), fin=new_fin,
                alive=bool((~new_fin).any()), gap=gap)


def step_inputs(n, W, V, seed, start=False):
    """random logits, random finite scores, about a third of the beams finished (start: the first step's 0, -inf, ...)"""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(n, W, V, generator=g) * 2.0
    if start:
        score = torch.full((n, W), NEG)
        score[:, 0] = 0.0
        fin = torch.zeros(n, W, dtype=torch.bool)
    else:
        score = -8.0 * torch.rand(n, W, generator=g)
        fin = torch.rand(n, W, generator=g) < 1.0 / 3.0
    return logits, score, fin


# one seed per shape for which the restatement's margin holds (checked on the CPU: tests/test_beam_cpu.py)
STEP_SEEDS = {(7, 1, 41): 1, (7, 3, 41): 2, (5, 2, 8518): 1, (3, 5, 8518): 2, (2, 8, 8518): 5}
START_CASE = (5, 3, 8518, 1)


def run_step(logits, score, fin, H, padded, seed=0):
    from gvl_amd import MultiScaleDeformableAttention as MSDA
    n, W, V = logits.shape
    ld = (V + 3) // 4 * 4 if padded else V
    buf = torch.full((n * W, ld), 1e30, device=DEV)                  # (the padding must never be read: it would win every arg-max)
    dev_logits = buf[:, :V]
    dev_logits.copy_(logits.view(n * W, V))
    g = torch.Generator().manual_seed(1000 + seed)
    h, c = torch.randn(n * W, H, generator=g).to(DEV), torch.randn(n * W, H, generator=g).to(DEV)
    out = dict(score=torch.empty(n, W, device=DEV), fin=torch.empty(n, W, dtype=torch.uint8, device=DEV),
               parent=torch.empty(n, W, dtype=torch.int32, device=DEV), token=torch.empty(n, W, dtype=torch.long, device=DEV),
               logp=torch.empty(n, W, device=DEV), alive=torch.zeros(1, dtype=torch.int32, device=DEV),
               h=torch.empty_like(h), c=torch.empty_like(c))
    MSDA.beam_step(dev_logits, score.to(DEV), fin.to(torch.uint8).to(DEV), h, c, out["score"], out["fin"], out["parent"],
                   out["token"], out["logp"], out["alive"], out["h"], out["c"])
    torch.cuda.synchronize()
    return out, h, c


def check_step(logits, score, fin, H, padded, need_gap=True):
    want = step_restatement(logits, score, fin)
    if need_gap:
        assert float(want["gap"].min()) >= STEP_GAP, float(want["gap"].min())             # precondition, not a property of the kernel
    got, h, c = run_step(logits, score, fin, H, padded)
    n, W, _ = logits.shape
    assert torch.equal(got["parent"].cpu().long(), want["parent"])
    assert torch.equal(got["token"].cpu(), want["token"])
    assert torch.equal(got["fin"].cpu().bool(), want["fin"])
    assert bool(got["alive"].item()) == want["alive"]
    print("beam step: score err %.3g, log-prob err %.3g" % (maxerr(got["score"], want["score"]), maxerr(got["logp"], want["logp"])))
    assert maxerr(got["score"], want["score"]) <= STEP_TOL
    assert maxerr(got["logp"], want["logp"]) <= STEP_TOL
    src = (torch.arange(n)[:, None] * W + want["parent"]).view(-1).to(DEV)
    assert torch.equal(got["h"], h[src]) and torch.equal(got["c"], c[src])                 # bit for bit


@pytest.mark.parametrize("H", [64, 512])
@pytest.mark.parametrize("padded", [True, False])
@pytest.mark.parametrize("shape", STEP_SHAPES)
def test_beam_step_equals_the_fp64_restatement(shape, padded, H):
    check_step(*step_inputs(*shape, STEP_SEEDS[shape]), H, padded)


@pytest.mark.parametrize("padded", [True, False])
def test_beam_step_from_the_start_scores(padded):
    """scores (0, -inf, ...): the W new beams are W distinct continuations of beam 0"""
    n, W, V, seed = START_CASE
    logits, score, fin = step_inputs(n, W, V, seed, start=True)
    check_step(logits, score, fin, 64, padded)
    assert int(step_restatement(logits, score, fin)["parent"].abs().max()) == 0


def tie_inputs():
    """beams 0 and 1 with identical scores and identical logit rows: every candidate of one ties with the other's"""
    logits, score, fin = step_inputs(4, 3, 8518, 11)
    fin[:] = False
    logits[:, 1] = logits[:, 0]
    score[:, 1] = score[:, 0]
    score[:, 2] = score[:, 0] - 30.0                                  # out of the running
    return logits, score, fin


@pytest.mark.parametrize("padded", [True, False])
def test_beam_step_exact_ties_go_to_the_smaller_flat_index(padded):
    logits, score, fin = tie_inputs()
    want = step_restatement(logits, score, fin)
    # the tie cuts through the selection: (0, best), (1, best), (0, second) are in, (1, second) -- equal to the last -- is out
    assert want["parent"].tolist() == [[0, 1, 0]] * 4 and bool((want["token"][:, 0] == want["token"][:, 1]).all())
    assert float(want["gap"][:, 1].min()) >= STEP_GAP and float(want["gap"][:, 0].max()) == 0.0 == float(want["gap"][:, 2].max())
    check_step(logits, score, fin, 64, padded, need_gap=False)


def test_beam_step_argument_errors():
    from gvl_amd import MultiScaleDeformableAttention as MSDA
    logits, score, fin = step_inputs(2, 3, 41, 0)
    with pytest.raises(RuntimeError, match="beam width"):
        MSDA.beam_step(torch.zeros(18, 41, device=DEV), torch.zeros(2, 9, device=DEV), *[None] * 11)
    h = torch.zeros(6, 64, device=DEV)
    z = lambda dt: torch.zeros(2, 3, dtype=dt, device=DEV)           # noqa: E731
    with pytest.raises(RuntimeError, match="ping-pong"):
        MSDA.beam_step(logits.view(6, 41).to(DEV), score.to(DEV), z(torch.uint8), h, h.clone(), z(torch.float32), z(torch.uint8),
                       z(torch.int32), z(torch.long), z(torch.float32), torch.zeros(1, dtype=torch.int32, device=DEV), h, h.clone())


# ---------------------------------------------------------------------------------------------------------------------------
# B. the whole search against a CPU beam search over the oracle's token step
# ---------------------------------------------------------------------------------------------------------------------------
E2E_W = 3
E2E_TOL = 5e-4             # scores / log-probs: the tolerance tests/test_gpu_sampling.py uses on this fixture
E2E_DELTA = 1e-3           # rows whose smallest step margin is below it may flip a beam: only their best score is compared ...
E2E_LOOSE = 2e-3           # ... within this
E2E_MAX_LOOSE = 2          # and there may be at most this many of the 16


def cpu_inputs(dtype=torch.float64):
    f, c = load("pdvc_eval"), load("captioner_step")
    sd = {k: v.to(dtype) for k, v in pdvc_state(f).items() if k.startswith(PRE)}
    hs, reference = t(c["hs"]), t(c["ref_in"])[:, :, 0].contiguous()
    vr = torch.ones(hs.shape[0], 4)
    ref_in = reference[:, :, None] * torch.stack([vr] * 2, -1)[:, None]
    return dict(sd=sd, hs=hs.to(dtype), ref_in=ref_in.to(dtype), memory=t(c["memory"]).to(dtype), mask=t(c["mask"]),
                tshapes=torch.tensor(c["tshapes"].tolist()), reference=reference, vr=vr)


def oracle_search(cpu, W, T, bias0):
    """the search of section 4.3 over oracle.torch_ref.captioner_step with logit.bias[0] raised by bias0, in cpu['sd']'s type:
    -> per-step records (T, n, W) parent / token / logp, final score (n, W), and the smallest step margin of every row"""
    from oracle import torch_ref as R
    sd = dict(cpu["sd"])
    sd[PRE + "logit.bias"] = sd[PRE + "logit.bias"].clone()
    sd[PRE + "logit.bias"][0] += bias0
    B, Q, C = cpu["hs"].shape
    n = B * Q
    hs, ref_in = cpu["hs"].repeat_interleave(W, 1), cpu["ref_in"].repeat_interleave(W, 1)
    state = (hs.new_zeros(n * W, C), hs.new_zeros(n * W, C))
    it = torch.zeros(n * W, dtype=torch.long)
    score = hs.new_full((n, W), NEG)
    score[:, 0] = 0.0
    fin = torch.zeros(n, W, dtype=torch.bool)
    rec = dict(parent=[], token=[], logp=[], fin=[])
    margin = hs.new_full((n,), float("inf"))
    for _ in range(T):
        logp, state = R.captioner_step(sd, PRE, it, state, hs, ref_in, cpu["memory"], cpu["tshapes"], cpu["mask"])
        # (the step's log-probs are a log_softmax already: applying it again in the restatement changes nothing)
        st = step_restatement(logp.view(n, W, -1), score, fin)
        finite = torch.isfinite(st["score"]).all(1, keepdim=True) & torch.isfinite(st["gap"])
        margin = torch.minimum(margin, torch.where(finite, st["gap"], torch.full_like(st["gap"], float("inf"))).min(1).values.to(margin.dtype))
        src = (torch.arange(n)[:, None] * W + st["parent"]).view(-1)
        state = (state[0][src], state[1][src])
        score, fin, it = st["score"].to(hs.dtype), st["fin"], st["token"].view(-1)
        for k in rec:
            rec[k].append(st[k])
    return {k: torch.stack(v) for k, v in rec.items()}, score, margin


def oracle_rank(rec, score, length_penalty):
    """final ranking and back-trace -> tokens (n, W, T), logprobs (n, W, T), scores (n, W), lengths (n, W), rank gap (n,)"""
    T, n, W = rec["parent"].shape
    tokens, logps = torch.zeros(n, W, T, dtype=torch.long), torch.zeros(n, W, T, dtype=score.dtype)
    cur = torch.arange(W)[None].expand(n, W)
    for step in range(T - 1, -1, -1):
        tokens[:, :, step] = rec["token"][step].gather(1, cur)
        logps[:, :, step] = rec["logp"][step].gather(1, cur).to(score.dtype)
        cur = rec["parent"][step].gather(1, cur)
    words = (tokens != 0).sum(2)
    length = (words + 1).clamp(max=T)
    value = score / length.to(score.dtype) ** length_penalty
    sval, order = torch.sort(value, dim=1, descending=True, stable=True)
    gap = (sval[:, 0] - sval[:, 1]) if W > 1 else torch.full((n,), float("inf"))
    pick = lambda x: x.gather(1, order[(...,) + (None,) * (x.dim() - 2)].expand(-1, -1, *x.shape[2:]))   # noqa: E731
    return dict(tokens=pick(tokens), logprobs=pick(logps), scores=pick(score), lengths=pick(words), order=order, gap=gap)


@functools.lru_cache(maxsize=None)
def oracle(bias0, W=E2E_W, T=6):
    return oracle_search(cpu_inputs(), W, T, bias0)


@pytest.fixture(scope="module")
def cap_setup():
    """the captioner of tests/test_gpu_sampling.py: cap_setup (B = 2, Q = 8, vocabulary 40, T = 6), a fresh model"""
    from gvl_amd.config import make_opt
    from gvl_amd.deformable_transformer import make_level_tensors
    from gvl_amd.pdvc import build
    f = load("pdvc_eval")
    opt = make_opt(num_queries=8, feature_dim=64, vocab_size=40, max_caption_len=6, device="cuda")
    model, _, _, _ = build(opt)
    model.load_state_dict(pdvc_state(f), strict=True)
    cap = model.to(DEV).eval().caption_head[-1]
    cpu = cpu_inputs(torch.float32)
    ts, ls = make_level_tensors(cpu["tshapes"].tolist(), DEV)
    others = {"memory": cpu["memory"].to(DEV), "mask_flatten": cpu["mask"].to(DEV), "spatial_shapes": ts, "level_start_index": ls,
              "valid_ratios": cpu["vr"].to(DEV)}
    return cap, cpu["hs"].to(DEV), cpu["reference"].to(DEV), others


class raised_end_bias:
    """logit.bias[0] raised for a scope, so that beams end at mixed lengths"""

    def __init__(self, cap, by):
        self.cap, self.by = cap, by

    def __enter__(self):
        with torch.no_grad():
            self.cap.logit.bias[0] += self.by

    def __exit__(self, *exc):
        with torch.no_grad():
            self.cap.logit.bias[0] -= self.by


def device_search(cap_setup, bias0, W, length_penalty):
    cap, hs, reference, others = cap_setup
    with torch.no_grad(), raised_end_bias(cap, bias0):
        res = cap.beam_search(hs, reference, others, W, length_penalty)
        return {k: v.cpu() for k, v in res.items()}


@pytest.mark.parametrize("bias0,length_penalty", [(0.75, 0.0), (0.75, 1.0), (0.25, 0.0)])
def test_beam_search_equals_the_oracle_search(cap_setup, bias0, length_penalty):
    rec, score, margin = oracle(bias0)
    want = oracle_rank(rec, score, length_penalty)
    if length_penalty:                                              # precondition: the penalty is exercised
        assert int((want["order"][:, 0] != oracle_rank(rec, score, 0.0)["order"][:, 0]).sum()) >= 1
    got = device_search(cap_setup, bias0, E2E_W, length_penalty)
    assert got["tokens"].shape == (16, E2E_W, 6) and got["alive"].shape == (6,)
    strict = margin >= E2E_DELTA
    assert int((~strict).sum()) <= E2E_MAX_LOOSE, margin
    for r in range(16):
        err = abs(float(got["scores"][r, 0]) - float(want["scores"][r, 0]))
        if not strict[r]:
            assert err <= E2E_LOOSE, (r, float(got["scores"][r, 0]), float(want["scores"][r, 0]))
            continue
        same = torch.equal(got["tokens"][r], want["tokens"][r]) and torch.equal(got["lengths"][r], want["lengths"][r])
        assert same, (r, float(margin[r]), got["scores"][r].tolist(), want["scores"][r].tolist(), got["tokens"][r].tolist(),
                      want["tokens"][r].tolist())
        assert maxerr(got["scores"][r], want["scores"][r]) <= E2E_TOL and maxerr(got["logprobs"][r], want["logprobs"][r]) <= E2E_TOL
    if bool(strict.all()):
        live = ~rec["fin"].view(6, -1).all(1)                       # some beam of some row still live after token t
        assert got["alive"].tolist() == live.tolist()


# ---------------------------------------------------------------------------------------------------------------------------
# C. interface
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias0,length_penalty", [(0.75, 0.0), (0.75, 1.0), (0.25, 0.0)])
def test_sample_returns_the_best_beam_in_the_greedy_form(cap_setup, bias0, length_penalty):
    cap, hs, reference, others = cap_setup
    res = device_search(cap_setup, bias0, E2E_W, length_penalty)
    with torch.no_grad(), raised_end_bias(cap, bias0):
        seq, lp = cap.sample(hs, reference, others, {"beam_size": E2E_W, "length_penalty": length_penalty})
    keep = int(res["lengths"][:, 0].max())
    assert (keep == 0) == ((bias0, length_penalty) == (0.75, 0.0))  # there every best caption is empty (as the oracle's)
    if keep == 0:
        assert isinstance(seq, list) and isinstance(lp, list) and seq == [] and lp == []
        return
    assert tuple(seq.shape) == (16, keep) == tuple(lp.shape)
    assert torch.equal(seq.cpu(), res["tokens"][:, 0, :keep]) and torch.equal(lp.cpu(), res["logprobs"][:, 0, :keep])


def test_beam_of_one_is_greedy(cap_setup):
    cap, hs, reference, others = cap_setup
    with torch.no_grad(), raised_end_bias(cap, 0.25):
        seq, lp = cap.sample(hs, reference, others, {"sample_max": 1})
        res = cap.beam_search(hs, reference, others, 1)
    keep = seq.shape[1]
    assert keep == int(res["lengths"].max()) >= 1
    assert torch.equal(res["tokens"][:, 0, :keep], seq)
    # greedy keeps booking log-probs behind a row's end token, the search books zeros there: compare up to the end token
    upto = (torch.arange(keep, device=DEV)[None] <= res["lengths"][:, :1]).float()
    assert maxerr(res["logprobs"][:, 0, :keep] * upto, lp * upto) <= E2E_TOL


def test_graph_replayed_beam_search_equals_eager_bit_for_bit(cap_setup):
    cap, hs, reference, others = cap_setup
    inputs = [(hs, reference), (hs.flip(1).contiguous(), reference.flip(1).contiguous()), (hs * 0.5, reference)]
    with torch.no_grad(), raised_end_bias(cap, 0.25):
        eager = [{k: v.clone() for k, v in cap.beam_search(h_, r_, others, E2E_W, 1.0).items()} for h_, r_ in inputs]
        cap.graph_decode = True
        try:
            for (h_, r_), want in zip(inputs, eager):               # a capture, then two replays on other inputs
                got = cap.beam_search(h_, r_, others, E2E_W, 1.0)
                for k in want:
                    assert torch.equal(got[k], want[k]), k
        finally:
            cap.graph_decode = False
    assert not torch.equal(eager[0]["tokens"], eager[1]["tokens"])


def test_beam_options_that_raise(cap_setup):
    cap, hs, reference, others = cap_setup
    with torch.no_grad():
        with pytest.raises(ValueError, match="beam_size"):
            cap.beam_search(hs, reference, others, 9)
        with pytest.raises(ValueError, match="beam_size"):
            cap.sample(hs, reference, others, {"beam_size": 9})
        with pytest.raises(ValueError, match="sample_max"):
            cap.sample(hs, reference, others, {"beam_size": 3, "sample_max": 0})
        with torch.autocast("cuda", dtype=torch.bfloat16), pytest.raises(NotImplementedError, match="autocast"):
            cap.sample(hs, reference, others, {"beam_size": 3})


def test_eval_forward_with_beam_size_feeds_postprocess():
    """PDVC.forward in eval mode with opt.beam_size = 3: seq / caption_probs in the form PostProcess turns into records; the
    whole-forward graph refuses the option"""
    from synth import synth_samples
    from gvl_amd.config import make_opt
    from gvl_amd.eval_utils import batch_result_json
    from gvl_amd.parallel import GraphedEvalForward
    from gvl_amd.pdvc import build
    from gvl_amd.video_dataset import collate_fn
    from test_gpu_pipeline import LOADER, to_device
    opt = make_opt(num_queries=10, feature_dim=16, vocab_size=60, max_caption_len=7, frame_embedding_num=64, device="cuda")
    torch.manual_seed(0)
    model, criterion, _, post = build(opt)
    model = model.to(DEV).eval()
    dt = to_device(collate_fn(synth_samples()), DEV)
    with torch.no_grad():
        model.opt.beam_size, model.opt.beam_length_penalty = 3, 0.0
        out, _ = model(dt, criterion, None, "queries", eval_mode=True)
        with pytest.raises(NotImplementedError, match="beam"):
            GraphedEvalForward(model, criterion)(dt)
    seq, lp = out["seq"], out["caption_probs"]["cap_prob_eval"]
    assert seq.dim() == 3 and seq.shape[:2] == (3, 10) and seq.shape == lp.shape and seq.shape[2] <= 7
    results = post["bbox"](out, dt["video_length"][:, 1], LOADER)
    records = batch_result_json(results, dt["video_key"], score_threshold=0)
    assert sorted(records) == ["v_000", "v_001", "v_002"]
    for events in records.values():
        assert len(events) == 10 and all(isinstance(e["sentence"], str) for e in events)


# ---------------------------------------------------------------------------------------------------------------------------
# D. which kernels served it
# ---------------------------------------------------------------------------------------------------------------------------
TOKEN_STEP_TAGS = ("gemm_f16x3", "cap_attend", "lstm_cell", "split_rows", "layer_gemm", "proj")


def test_path_census_at_the_real_dimensions(monkeypatch):
    """B = 2, Q = 10, hidden 512, vocabulary 8517, W = 3, 4 tokens: the token step of the search is served by the kernels that
    serve a greedy decode of the same inputs (with the fp32 h written, as the search needs it), the beam kernel runs once per
    token, and no ATen topk / log_softmax is called"""
    from gvl_amd.CaptioningHead import build_captioner
    from gvl_amd.config import make_opt
    from gvl_amd.deformable_transformer import make_level_tensors
    T = 4
    opt = make_opt("anet_tsp_ssvg", num_queries=10, max_caption_len=T, device="cuda")
    assert (opt.hidden_dim, opt.vocab_size) == (512, 8517)
    torch.manual_seed(3)
    cap = build_captioner(opt).to(DEV).eval()
    B, Q = 2, 10
    lengths = [100, 50, 25, 13]
    ts, ls = make_level_tensors(lengths, DEV)
    g = torch.Generator().manual_seed(4)
    hs = torch.randn(B, Q, 512, generator=g).to(DEV)
    reference = torch.stack([0.2 + 0.6 * torch.rand(B, Q, generator=g), 0.1 + 0.3 * torch.rand(B, Q, generator=g)], -1).to(DEV)
    others = {"memory": torch.randn(B, sum(lengths), 512, generator=g).to(DEV),
              "mask_flatten": torch.zeros(B, sum(lengths), dtype=torch.bool, device=DEV), "spatial_shapes": ts,
              "level_start_index": ls, "valid_ratios": torch.ones(B, 4, device=DEV)}

    def greedy():
        memory, tshapes, lsi, mask = cap._level_inputs(others)
        real = cap.core.prepare

        def prepare(*a):                                             # (h_planes_only off: the fp32 h is written, as in the search)
            const = real(*a)
            const["h_planes_only"] = False
            return const
        monkeypatch.setattr(cap.core, "prepare", prepare)
        try:
            return cap._decode_device(hs, reference, memory, mask, others["valid_ratios"], tshapes, lsi, 1, 1.0)
        finally:
            monkeypatch.setattr(cap.core, "prepare", real)

    def refuse(name):
        def fn(*a, **k):
            raise AssertionError(f"ATen {name} called inside the beam search")
        return fn

    with torch.no_grad():
        _, tags_g = path_census(greedy)
        for mod, name in ((torch, "topk"), (torch.Tensor, "topk"), (torch, "log_softmax"), (torch.Tensor, "log_softmax"),
                          (torch.nn.functional, "log_softmax")):
            monkeypatch.setattr(mod, name, refuse(name))
        res, tags_b = path_census(lambda: cap.beam_search(hs, reference, others, 3))
    assert res["tokens"].shape == (B * Q, 3, T)
    assert tags_b["beam_step"] == T and tags_b["beam_finish"] == 1 and "beam_step" not in tags_g
    step_g = {k for k in TOKEN_STEP_TAGS if tags_g[k]}
    assert step_g == {k for k in TOKEN_STEP_TAGS if tags_b[k]} and {"gemm_f16x3", "cap_attend"} <= step_g, (tags_g, tags_b)
    assert tags_b["row_argmax_lse"] == 0

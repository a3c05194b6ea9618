"""The three kernels of the contrastive branch (gvl_amd/csrc/gvl_contrastive.hip: k_cl_logits, k_cl_loss_fwd, k_cl_loss_bwd) through
their wrappers (gvl_amd.criterion.ContrastiveCriterion.logits_layers / loss_layers / forward), against the fp64 evaluation of
tests/contrastive_ref.py on the CPU.  Inputs are drawn in fp32 from fixed seeds and widened, so both sides see the same numbers.

Tolerance (the convention of tests/test_gpu_cap_train_ops.py): every output is held to
    max(FACTOR * err32, 16 * 2**-23 * scale),   FACTOR = 8,
err32 being the deviation of the SAME restatement evaluated in fp32 torch on the CPU and scale the largest magnitude of the fp64
result.  Rows whose norm is clamped (all-zero rows) have gradients 1e12 times the others'; they are compared as a group of their
own so that their scale does not hide the ordinary rows.  Every comparison prints "RATIO <case>/<output> <error / bound>" before it
asserts (pytest -s).
"""
import collections

import pytest
import torch

import contrastive_ref as R
from helpers import path_census

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FACTOR, FLOOR = 8.0, 16 * 2.0 ** -23
TAGS = ("cl_logits", "cl_loss_fwd", "cl_loss_bwd")       # GVL_PROF_CL_* (include/gvl_msda.h) as profile_collect names them
MODES = {"default": (True, False, False), "e2t": (True, True, False), "e2t_bg": (True, True, True), "pervideo": (False, False, False)}


def split_counts(G, B, Q):
    """G sentences over B videos, none with more than Q"""
    base, extra = divmod(G, B)
    n = [base + (i < extra) for i in range(B)]
    assert max(n) <= Q
    return n


def make_case(G, B, Q, D, L=1, per_layer_text=False, seed=0, n_gt=None):
    g = torch.Generator().manual_seed(1000 + seed)
    n_gt = split_counts(G, B, Q) if n_gt is None else n_gt
    text = torch.randn(L if per_layer_text else 1, G, D, generator=g)
    event = torch.randn(L, B * Q, D, generator=g)
    bg = torch.randn(1, D, generator=g)
    pq, pt, pv = [], [], []
    for _ in range(L):
        q, c, base = [], [], 0
        for i, n in enumerate(n_gt):
            q.append(torch.randperm(Q, generator=g)[:n])
            c.append(torch.randperm(n, generator=g) + base)
            base += n
        pq.append(torch.cat(q)); pt.append(torch.cat(c))
    pv = torch.cat([torch.full((n,), i, dtype=torch.long) for i, n in enumerate(n_gt)])
    w = torch.rand(L, generator=g) + 0.5                               # d total / d loss_l
    return dict(text=text, event=event, bg=bg, pq=torch.stack(pq), pt=torch.stack(pt), pv=pv, w=w, B=B, Q=Q, n_gt=n_gt)


def restate(case, mode, dtype, tau=0.1):
    """the restatement in `dtype` on the CPU -> dict of outputs (cosine tables, losses, gradients)"""
    cross, e2t, bgall = MODES[mode]
    text, event, bg = (case[k].to(dtype).clone().requires_grad_() for k in ("text", "event", "bg"))
    L, B, Q = event.shape[0], case["B"], case["Q"]
    losses, tables = [], []
    for l in range(L):
        tl = text[l if text.shape[0] > 1 else 0]
        tables.append(R.cosines(tl, event[l], bg if e2t else None).t().detach())
        pe = case["pv"] * Q + case["pq"][l]
        losses.append(R.contrastive_loss(tl, event[l], case["pt"][l], pe, case["pv"], B, Q, tau, cross, e2t, bgall, bg)[0])
    losses = torch.stack(losses)
    (losses * case["w"].to(dtype)).sum().backward()
    out = dict(table=torch.stack(tables), loss=losses.detach(), g_text=text.grad, g_event=event.grad)
    if e2t:
        out["g_bg"] = bg.grad
    return out


def run_gpu(case, mode, tau=0.1):
    from gvl_amd.criterion import ContrastiveCriterion
    cross, e2t, bgall = MODES[mode]
    crit = ContrastiveCriterion(tau, cross, e2t, bgall)
    text, event, bg = (case[k].to(DEV).requires_grad_() for k in ("text", "event", "bg"))
    keep = [x.detach().clone() for x in (text, event, bg)]
    # what the caching allocator hands out next is NaN, not zeros: blocks of its small pool (< 1 MB) and of its large pool
    poison = [torch.full((n,), float("nan"), device=DEV) for n in (128, 1024, 8192, 65536, 1 << 18, 1 << 22) for _ in range(12)]
    del poison
    rec = crit.logits_layers(text, event, bg if e2t else None)
    losses = crit.loss_layers(rec, case["pq"].to(DEV), case["pt"].to(DEV), case["pv"].to(DEV), None, case["B"], case["Q"])
    (losses * case["w"].to(DEV)).sum().backward()
    for a, b in zip(keep, (text, event, bg)):
        assert torch.equal(a, b.detach()), "an input was written"
    out = dict(table=rec.out, loss=losses.detach(), g_text=text.grad, g_event=event.grad)
    if e2t:
        out["g_bg"] = bg.grad
    return {k: v.detach().cpu() for k, v in out.items()}


def hold(name, got, ref64, ref32, mask=None):
    got, ref64, ref32 = got.double(), ref64.double(), ref32.double()
    assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
    if mask is not None:
        got, ref64, ref32 = got[mask], ref64[mask], ref32[mask]
    if got.numel() == 0:
        return
    nan = torch.isnan(ref64)
    assert torch.equal(torch.isnan(got), nan), f"{name}: NaN pattern differs"
    got, ref64, ref32 = got[~nan], ref64[~nan], ref32[~nan]
    if got.numel() == 0:
        print(f"RATIO {name} nan")
        return
    err32 = float((ref32 - ref64).abs().max())
    bound = max(FACTOR * err32, FLOOR * float(ref64.abs().max()))
    err = float((got - ref64).abs().max())
    print(f"RATIO {name} {err / bound if bound else 0.0:.3f}   (error {err:.3e}, err32 {err32:.3e}, bound {bound:.3e})")
    assert err <= bound, (name, err, bound)


def check(name, case, mode, tau=0.1):
    got = run_gpu(case, mode, tau)
    r64, r32 = restate(case, mode, torch.float64, tau), restate(case, mode, torch.float32, tau)
    zt = (case["text"] == 0).all(-1)
    ze = (case["event"] == 0).all(-1)
    for k in r64:
        if k == "g_text" and zt.any():
            hold(f"{name}/{k}", got[k], r64[k], r32[k], ~zt)
            hold(f"{name}/{k}[zero rows]", got[k], r64[k], r32[k], zt)
        elif k == "g_event" and ze.any():
            hold(f"{name}/{k}", got[k], r64[k], r32[k], ~ze)
            hold(f"{name}/{k}[zero rows]", got[k], r64[k], r32[k], ze)
        else:
            hold(f"{name}/{k}", got[k], r64[k], r32[k])
    return got


SHAPES = {"1x1x1x1": dict(G=1, B=1, Q=1, D=1), "5x2x8x16": dict(G=5, B=2, Q=8, D=16), "67x3x37x33": dict(G=67, B=3, Q=37, D=33),
          "7x2x8x128_shared": dict(G=7, B=2, Q=8, D=128, L=2), "7x2x8x128_layers": dict(G=7, B=2, Q=8, D=128, L=2, per_layer_text=True)}


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_against_restatement(shape, mode):
    check(f"{shape}.{mode}", make_case(seed=len(shape) + len(mode), **SHAPES[shape]), mode)


def test_config_size_once():
    check("160x16x300x128.e2t_bg", make_case(160, 16, 300, 128, L=2, seed=3), "e2t_bg")


@pytest.mark.parametrize("mode", ["e2t", "e2t_bg", "pervideo"])
def test_zero_rows_take_the_clamped_norm(mode):
    case = make_case(5, 2, 8, 16, L=2, seed=11)
    case["text"][0, 1] = 0
    case["event"][:, 3] = 0
    case["event"][1, int(case["pq"][1][0])] = 0                      # a MATCHED event of video 0, too
    check(f"zero_rows.{mode}", case, mode)


@pytest.mark.parametrize("mode", ["e2t_bg", "pervideo"])
def test_largest_logits(mode):
    """tau = 0.1 and cosines of +-1: logits of +-10 in every row"""
    case = make_case(6, 2, 8, 16, seed=12)
    for p in range(6):
        e = int(case["pv"][p]) * 8 + int(case["pq"][0][p])
        case["event"][0, e] = case["text"][0, int(case["pt"][0][p])] * (2.5 if p % 2 == 0 else -0.5)
    check(f"largest_logits.{mode}", case, mode)


def test_long_rows_do_not_overflow():
    """4800 events at 1 / tau = 10 with every cosine near 1: the sums of exponentials are taken online"""
    case = make_case(8, 16, 300, 32, seed=13)
    case["event"][:] = case["text"][0, 0] + 0.01 * case["event"]
    case["text"][:] = case["text"][0, 0] + 0.01 * case["text"]
    got = check("long_rows.e2t_bg", case, "e2t_bg")
    assert torch.isfinite(got["loss"]).all()


@pytest.mark.parametrize("mode", sorted(MODES))
def test_video_without_sentence_and_unmatched_events(mode):
    """video 1 has no sentence (per-video mode: the mean of an empty set, NaN, as the reference's op sequence gives); most events
    are matched in no pair, with and without enable_bg_for_cl"""
    case = make_case(3, 3, 8, 16, L=2, seed=14, n_gt=[2, 0, 1])
    got = check(f"empty_video.{mode}", case, mode)
    assert bool(torch.isnan(got["loss"]).all()) == (mode == "pervideo")
    assert torch.isfinite(got["g_event"]).all() and torch.isfinite(got["g_text"]).all()


def test_no_sentences_at_all():
    """G = 0 launches nothing and returns what the op sequence returns: a NaN mean, an empty table with the background column"""
    from gvl_amd.criterion import ContrastiveCriterion
    event = torch.randn(2, 4, 16, device=DEV)
    text = [torch.zeros(0, 16, device=DEV), torch.zeros(0, 16, device=DEV)]
    bg = torch.randn(1, 16, device=DEV)
    empty = [(torch.zeros(0, dtype=torch.long), torch.zeros(0, dtype=torch.long))] * 2
    for mode, (cross, e2t, bgall) in MODES.items():
        crit = ContrastiveCriterion(0.1, cross, e2t, bgall)
        (loss, raw), tags = path_census(lambda: crit(text, event, empty, return_logits=True, bg_embed=bg))
        assert torch.isnan(loss) and raw.shape == (0, 8), mode
        table, tags2 = path_census(lambda: crit.forward_logits(torch.cat(text), event.reshape(-1, 16), bg))
        assert table.shape == (1, 8) and not any(tags[t_] + tags2[t_] for t_ in TAGS)
        ref = R.cosines(torch.cat(text).cpu().double(), event.reshape(-1, 16).cpu().double(), bg.cpu().double())
        assert (table.cpu().double() - ref).abs().max() < 1e-6


@pytest.mark.parametrize("per_layer_text", [False, True])
def test_outputs_are_written_not_accumulated(per_layer_text):
    """the three entry points' outputs in caller-owned buffers pre-filled with NaN come out fully written and equal to a run into
    zero-filled buffers, bit for bit (nothing is added to what a buffer held); a second backward doubles .grad exactly"""
    import ctypes
    from gvl_amd import _lib
    from gvl_amd.criterion import ContrastiveCriterion
    case = make_case(67, 3, 37, 33, L=2, per_layer_text=per_layer_text, seed=21)
    text, event, bg = (case[k].to(DEV).contiguous() for k in ("text", "event", "bg"))
    pq, pt, pv = (case[k].to(DEV).contiguous() for k in ("pq", "pt", "pv"))
    L, E, D = event.shape
    G, B, Q = text.shape[1], case["B"], case["Q"]
    lib, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
    stride = G * D if per_layer_text else 0
    results = []
    for fill in (float("nan"), 0.0):
        f = lambda *shape: torch.full(shape, fill, device=DEV)                      # noqa: E731
        i_ = lambda *shape: torch.full(shape, -77, dtype=torch.int32, device=DEV)   # noqa: E731
        out, inv_e, inv_t, inv_bg = f(L, E, G + 1), f(L, E), f(L, G), f(1)
        _lib.check(lib.gvl_cl_logits_f32(event.data_ptr(), text.data_ptr(), stride, bg.data_ptr(), L, E, G, D, out.data_ptr(),
                                         inv_e.data_ptr(), inv_t.data_ptr(), inv_bg.data_ptr(), st), "logits")
        loss, saved = f(L, 3), [f(L, G), f(L, E), i_(L, G), i_(L, E), i_(L, G), f(L, G), f(L, E)]
        nbytes = lib.gvl_cl_loss_workspace_bytes(L, E, G)
        ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
        ws[:16].zero_()
        _lib.check(lib.gvl_cl_loss_forward_f32(out.data_ptr(), pq.data_ptr(), pt.data_ptr(), pv.data_ptr(), None, L, E, G, 1,
                                               pq.shape[1], B, Q, 0.1, 1, 1, 1, loss.data_ptr(), *[s_.data_ptr() for s_ in saved],
                                               ws.data_ptr(), nbytes, st), "loss_forward")
        gl = torch.tensor([0.75, 1.25], device=DEV)
        g_event, g_text, g_bg = f(L, E, D), f(text.shape[0], G, D), f(1, D)
        _lib.check(lib.gvl_cl_loss_backward_f32(gl.data_ptr(), out.data_ptr(), saved[0].data_ptr(), saved[1].data_ptr(),
                                                saved[2].data_ptr(), saved[3].data_ptr(), saved[4].data_ptr(), saved[5].data_ptr(),
                                                saved[6].data_ptr(), event.data_ptr(), text.data_ptr(), stride, bg.data_ptr(),
                                                inv_e.data_ptr(), inv_t.data_ptr(), inv_bg.data_ptr(), L, E, G, D, Q, 0.1,
                                                g_event.data_ptr(), g_text.data_ptr(), g_bg.data_ptr(), st), "loss_backward")
        torch.cuda.synchronize()
        results.append([out, inv_e, inv_t, inv_bg, loss, *saved, g_event, g_text, g_bg])
    for a, b in zip(*results):
        assert not torch.isnan(a.float()).any() and torch.equal(a, b)
    assert all(int((s_ == -77).sum()) == 0 for s_ in results[0][7:10])
    # through autograd: the node returns fresh gradients, which autograd adds to .grad -- twice the step, twice the gradient
    crit = ContrastiveCriterion(0.1, True, True, True)
    tx, ev, b_ = (x.clone().requires_grad_() for x in (text, event, bg))
    for _ in range(2):
        rec = crit.logits_layers(tx, ev, b_)
        crit.loss_layers(rec, pq, pt, pv, None, B, Q).sum().backward()
        if _ == 0:
            once = [x.grad.clone() for x in (tx, ev, b_)]
    for x, g1 in zip((tx, ev, b_), once):
        assert torch.equal(x.grad, g1 + g1)


def test_bitwise_repeatable():
    case = make_case(67, 3, 37, 33, L=2, seed=15)
    a, b = run_gpu(case, "e2t_bg"), run_gpu(case, "e2t_bg")
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_reference_api_on_the_kernels():
    """ContrastiveCriterion.forward / forward_logits with the reference's arguments run the kernels and agree with the restatement"""
    from gvl_amd.criterion import ContrastiveCriterion
    case = make_case(5, 2, 8, 16, seed=16)
    n_gt, Q = case["n_gt"], 8
    text = [x.to(DEV).requires_grad_() for x in case["text"][0].split(n_gt)]
    event, bg = case["event"][0].view(2, 8, 16).to(DEV).requires_grad_(), case["bg"].to(DEV).requires_grad_()
    idx, base = [], 0
    for i, n in enumerate(n_gt):
        sel = case["pv"] == i
        idx.append((case["pq"][0][sel], case["pt"][0][sel] - base))
        base += n
    crit = ContrastiveCriterion(0.1, True, True, True)
    (loss, raw), tags = path_census(lambda: crit(text, event, idx, return_logits=True, bg_embed=bg))
    assert [tags[t_] for t_ in TAGS] == [1, 1, 0]
    r64 = restate(case, "e2t_bg", torch.float64)
    assert abs(float(loss) - float(r64["loss"][0])) < 1e-5
    assert (raw.detach().cpu().double() - r64["table"][0].t()[case["pt"][0]]).abs().max() < 1e-6
    with torch.no_grad():
        table, tags = path_census(lambda: crit.forward_logits(torch.cat(text), event.reshape(-1, 16), bg))
    assert tags[TAGS[0]] == 1 and (table.cpu().double() - r64["table"][0].t()).abs().max() < 1e-6


def test_refusals():
    from gvl_amd.criterion import ContrastiveCriterion
    crit = ContrastiveCriterion(0.1, True, False, False)
    # D = 513: outside the kernels' range -> the PyTorch formulation, no launch of ours
    g = torch.Generator().manual_seed(3)
    text, event = torch.randn(4, 513, generator=g), torch.randn(2, 5, 513, generator=g)
    idx = [(torch.tensor([1, 3]), torch.tensor([1, 0])), (torch.tensor([0, 4]), torch.tensor([0, 1]))]
    loss, tags = path_census(lambda: crit(list(text.to(DEV).split(2)), event.to(DEV), idx))
    assert not any(tags[t_] for t_ in TAGS)
    pe = torch.tensor([1, 3, 5, 9])
    ref = R.contrastive_loss(text.double(), event.double().reshape(-1, 513), torch.tensor([1, 0, 2, 3]), pe,
                             torch.tensor([0, 0, 1, 1]), 2, 5, 0.1)[0]
    assert abs(float(loss) - float(ref)) < 1e-5
    with pytest.raises(ValueError, match="dtype and device"):
        crit.forward_logits(torch.randn(4, 16, device=DEV, dtype=torch.float64), torch.randn(6, 16, device=DEV))
    with pytest.raises(ValueError, match="dtype and device"):
        crit.forward_logits(torch.randn(4, 16), torch.randn(6, 16, device=DEV))
    # fp64 on the GPU: the PyTorch formulation
    t64, e64 = torch.randn(4, 16, device=DEV, dtype=torch.float64), torch.randn(6, 16, device=DEV, dtype=torch.float64)
    table, tags = path_census(lambda: crit.forward_logits(t64, e64))
    assert table.dtype == torch.float64 and not tags[TAGS[0]]


def test_launch_census_of_a_two_layer_step():
    """one logits launch, one loss-forward launch, one loss-backward launch for two decoder layers, and neither log_softmax nor
    normalize among the ATen calls"""
    from torch.utils._python_dispatch import TorchDispatchMode
    from gvl_amd.criterion import ContrastiveCriterion
    seen = collections.Counter()

    class Record(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            seen[str(func)] += 1
            return func(*args, **(kwargs or {}))

    case = make_case(7, 2, 8, 128, L=2, seed=17)
    crit = ContrastiveCriterion(0.1, True, True, True)
    text, event, bg = (case[k].to(DEV).requires_grad_() for k in ("text", "event", "bg"))
    pq, pt, pv = (case[k].to(DEV) for k in ("pq", "pt", "pv"))

    def step():
        with Record():
            rec = crit.logits_layers(text, event, bg)
            crit.loss_layers(rec, pq, pt, pv, None, 2, 8).sum().backward()

    _, tags = path_census(step)
    assert [tags[t_] for t_ in TAGS] == [1, 1, 1], tags
    bad = [k for k in seen if any(w in k for w in ("log_softmax", "normalize", "vector_norm", "cross_entropy", "nll_loss", "mm"))]
    assert not bad, bad

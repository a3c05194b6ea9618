"""Clip + Adam / AdamW over several parameter groups with the hyper-parameters in device memory (gvl_clip_adam_groups_step_f32,
gvl_amd.optim.ClipAdam.sync): against torch's clip_grad_norm_ + optimizer.step() with the learning rate changed between steps,
inside a captured hipGraph whose replays follow a scheduler, and in the whole captured train step (AdamW with the task heads' own
lr: train.py:272-292; only_ft_captioner: train.py:248-249,407)."""
import warnings

import pytest
import torch

from helpers import load, pdvc_state
from bench import synth_batch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SHAPES = [(512, 512), (2048, 512), (512,), (1,), (3, 7), (8518, 512), (33,), (2, 4097)]
CLIP_SHAPES = [(640, 8), (5, 3)]


def _params(flat, shapes, off):
    ps = []
    for i, s in enumerate(shapes):
        n = torch.Size(s).numel()
        src = flat[off:off + n]                          # (odd offsets: views that are NOT 16-byte aligned)
        ps.append(torch.nn.Parameter(src.view(s).clone() if i % 2 == 0 else src.view(s).detach().clone()))
        off += n
    return ps


def _groups(ps, kind, variant):
    g0 = {"params": ps[0::2], "lr": 5e-3, "weight_decay": 1e-2 if kind == "adamw" else 1e-4}
    g1 = {"params": ps[1::2], "lr": 2e-3, "weight_decay": 0.05 if kind == "adamw" else 0.0}
    if variant:
        g1.update(betas=(0.8, 0.99), eps=1e-6)
    return [g0, g1]


def _make(kind, groups, **kw):
    return (torch.optim.AdamW if kind == "adamw" else torch.optim.Adam)(groups, capturable=True, fused=True, **kw)


def _close_state(oa, ob, p, q, ctx):
    sa, sb = oa.state[p], ob.state[q]
    assert float(sa["step"]) == float(sb["step"]), ctx
    assert float((sa["exp_avg"] - sb["exp_avg"]).abs().max()) <= 1e-6 * max(1e-3, float(sb["exp_avg"].abs().max())), ctx
    assert float((sa["exp_avg_sq"] - sb["exp_avg_sq"]).abs().max()) <= 1e-6 * max(1e-6, float(sb["exp_avg_sq"].abs().max())), ctx


def _close_param(p, q, ctx):
    assert float((p.detach() - q.detach()).abs().max()) <= 2e-6 * max(1.0, float(q.detach().abs().max())), ctx


@pytest.mark.parametrize("kind,variant", [("adam", False), ("adamw", False), ("adamw", True), ("adam", True)])
def test_groups_and_clip_only_equal_torch(kind, variant):
    """two groups (different lr and weight decay; `variant`: different betas / eps too), lr halved after step 2 and group 1's
    set to 0 after step 4, tensors that sit a step out, clip-only tensors in the norm -- against clip_grad_norm_ over ALL the
    tensors + optimizer.step() on clones"""
    from gvl_amd.optim import ClipAdam
    g = torch.Generator(device=DEV).manual_seed(5)
    total = sum(torch.Size(s).numel() for s in SHAPES + CLIP_SHAPES) + 3
    flat = torch.randn(total, device=DEV, generator=g)
    n_main = sum(torch.Size(s).numel() for s in SHAPES)
    pa, pb = _params(flat, SHAPES, 1), _params(flat, SHAPES, 1)
    ca_, cb_ = _params(flat, CLIP_SHAPES, 1 + n_main), _params(flat, CLIP_SHAPES, 1 + n_main)
    clip_start = [c.detach().clone() for c in ca_]
    oa, ob = _make(kind, _groups(pa, kind, variant)), _make(kind, _groups(pb, kind, variant))
    clip = ClipAdam(oa, 0.5)
    used = []
    for step in range(7):
        if step == 3:
            for o in (oa, ob):
                for grp in o.param_groups:
                    grp["lr"] *= 0.5
        if step == 5:
            oa.param_groups[1]["lr"] = ob.param_groups[1]["lr"] = 0.0
        grads = [torch.randn(p.shape, device=DEV, generator=g) * (10.0 if step in (2, 3) else 0.05) for p in pa + ca_]
        for p, q, gr in zip(pa + ca_, pb + cb_, grads):
            p.grad, q.grad = gr.clone(), gr.clone()
        if step == 2:
            for i in (1, 4, 5):
                pa[i].grad = pb[i].grad = None
        act_a, act_b = [p for p in pa if p.grad is not None], [q for q in pb if q.grad is not None]
        frozen = [p.detach().clone() for p in pa] if step >= 5 else None
        used.append(clip.step(act_a, ca_))
        if not used[-1]:                                      # (first step: torch creates the state)
            torch.nn.utils.clip_grad_norm_(act_a + ca_, 0.5)
            oa.step()
        norm = torch.nn.utils.clip_grad_norm_(act_b + cb_, 0.5)
        ob.step()
        if used[-1]:
            assert abs(float(clip.last[0]) - float(norm)) <= 1e-5 * float(norm), step
        for i, (p, q) in enumerate(zip(pa, pb)):
            ctx = (kind, variant, step, i)
            if p.grad is None:
                assert q.grad is None
                continue
            assert float((p.grad - q.grad).abs().max()) <= 1e-6 * max(1e-6, float(q.grad.abs().max())), ctx
            _close_param(p, q, ctx)
            _close_state(oa, ob, p, q, ctx)
            if frozen is not None and i % 2 == 1:            # group 1 at lr = 0: not one bit moves
                assert torch.equal(p.detach(), frozen[i]), ctx
        for c, d, c0 in zip(ca_, cb_, clip_start):
            assert float((c.grad - d.grad).abs().max()) <= 1e-6 * max(1e-6, float(d.grad.abs().max()))
            assert torch.equal(c.detach(), c0) and c not in oa.state           # clipped, never stepped, no state
    assert used == [False] + [True] * 6


@pytest.mark.parametrize("kind", ["adam", "adamw"])
@pytest.mark.parametrize("strategy", ["multi_step", "warmup_linear"])
def test_captured_update_follows_the_scheduler(kind, strategy):
    """ClipAdam.step captured once in a torch.cuda.CUDAGraph; between the replays a scheduler (build_scheduler: MultiStepLR or
    the warm-up LambdaLR) changes both groups' lr and ClipAdam.sync() writes them -- every replay equals torch's eager
    optimizer fed the same gradients at the lr in force"""
    from gvl_amd.config import make_opt
    from gvl_amd.optim import ClipAdam, build_scheduler
    g = torch.Generator(device=DEV).manual_seed(9)
    shapes = SHAPES[:5]
    flat = torch.randn(sum(torch.Size(s).numel() for s in shapes) + 3, device=DEV, generator=g)
    pa, pb = _params(flat, shapes, 1), _params(flat, shapes, 1)
    oa = _make(kind, _groups(pa, kind, True))
    ob = (torch.optim.AdamW if kind == "adamw" else torch.optim.Adam)(_groups(pb, kind, True))     # torch's eager default
    clip = ClipAdam(oa, 1.0)
    static = [torch.zeros_like(p) for p in pa]

    def grads(scale):
        gs = [torch.randn(p.shape, device=DEV, generator=g) * scale for p in pa]
        for p, q, s, gr in zip(pa, pb, static, gs):
            s.copy_(gr)
            p.grad, q.grad = s, gr.clone()

    def reference():
        torch.nn.utils.clip_grad_norm_(pb, 1.0)
        ob.step()
    for it in range(2):                                      # eager: torch creates the state, then the table is built
        grads(0.3)
        if not clip.step(pa):
            torch.nn.utils.clip_grad_norm_(pa, 1.0)
            oa.step()
        reference()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        assert clip.step(pa)
    torch.cuda.current_stream().wait_stream(side)
    opt = make_opt(learning_strategy=strategy, warm_up_ratio=0.25, learning_rate_decay_start=1, learning_rate_decay_every=2,
                   epoch=8)
    sa, sb = build_scheduler(opt, oa, 8), build_scheduler(opt, ob, 8)
    seen = set()
    for it in range(8):
        grads(0.3 if it % 2 else 3.0)
        seen.add(tuple(grp["lr"] for grp in oa.param_groups))
        clip.sync()
        graph.replay()
        reference()
        for i, (p, q) in enumerate(zip(pa, pb)):
            ctx = (kind, strategy, it, i)
            assert float((p.grad - q.grad).abs().max()) <= 1e-6 * max(1e-6, float(q.grad.abs().max())), ctx
            _close_param(p, q, ctx)
            _close_state(oa, ob, p, q, ctx)
        sa.step()
        sb.step()
    assert len(seen) >= 3                                    # (the lr did change between the replays)


# ---- the whole captured train step ---------------------------------------------------------------------------------------------
def toy(**over):
    from gvl_amd.config import make_opt
    from gvl_amd.pdvc import build
    f = load("pdvc_eval")
    kw = dict(num_queries=8, feature_dim=64, vocab_size=40, max_caption_len=6, device="cuda",
              transformer_dropout_prob=0.0, drop_prob=0.0, lr=1e-3, weight_decay=1e-2)
    kw.update(over)
    opt = make_opt(**kw)
    model, criterion, _, _ = build(opt)
    model.load_state_dict(pdvc_state(f), strict=True)
    return opt, model.to(DEV).train(), criterion, int(f["meta_T"])


def batches(T, n=6):
    lay = [([3, 2], (2, 3)), ([1, 5], (1, 4)), ([4, 1], (3, 3)), ([2, 2], (2, 2)), ([4, 4], (1, 3)), ([2, 3], (2, 4))]
    return [synth_batch(2, T, 64, 40, ns, DEV, seed=40 + i, cap_words=cw) for i, (ns, cw) in enumerate(lay[:n])]


def _no_scheduler_warning(caught):
    msgs = [str(w.message) for w in caught if "lr_scheduler.step()" in str(w.message)]
    assert not msgs, msgs


def test_graphed_step_adamw_task_heads_lr_follows_scheduler():
    """optimizer_type='adamw' + task_heads_different_lr: after the capture a scheduler moves the other group's lr every step and
    sets the heads' lr to exactly 0 -- the replays then leave every head parameter bit-identical while the rest moves, one
    replay equals torch's AdamW recomputed from the snapshot before it and the clipped gradient it left, and nothing is
    captured again"""
    from gvl_amd.parallel import GraphedTrainStep
    opt, model, crit, T = toy(optimizer_type="adamw", task_heads_different_lr=True, task_heads_lr=2e-3)
    step = GraphedTrainStep(model, crit, opt, max_gt=8, max_cap_len=8, cap_len_policy="grow")
    o = step.optimizer
    assert type(o) is torch.optim.AdamW and len(o.param_groups) == 2
    heads_ids = {id(p) for p in model.caption_head.parameters()} | {id(p) for p in model.bbox_head.parameters()}
    assert {id(p) for p in o.param_groups[0]["params"]} == heads_ids
    heads, others = o.param_groups[0]["params"], o.param_groups[1]["params"]
    sched = torch.optim.lr_scheduler.LambdaLR(o, [lambda e: 1.0 if e < 2 else 0.0, lambda e: 1.0 / (1 + e)])
    bs = batches(T)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        step(bs[0])
        sched.step()
        assert step.captures == 1
        # one replay against torch's AdamW from a snapshot (both groups' lr != 0 here; the other group's is already halved)
        live = [p for p in heads + others]
        snap = {p: (p.detach().clone(), {k: v.clone() for k, v in o.state[p].items()}) for p in live}
        lrs = [grp["lr"] for grp in o.param_groups]
        assert lrs == [2e-3, 0.5e-3]
        step(bs[1])
        sched.step()
        stepped = [p for p in live if p.grad is not None]
        assert len(stepped) > len(live) // 2
        clones = {p: snap[p][0].clone().requires_grad_() for p in stepped}
        ref = torch.optim.AdamW([{"params": [clones[p] for p in heads if p in clones], "lr": lrs[0]},
                                 {"params": [clones[p] for p in others if p in clones], "lr": lrs[1]}],
                                weight_decay=opt.weight_decay, capturable=True, fused=True)
        for p in stepped:
            c = clones[p]
            c.grad = p.grad.detach().clone()
            ref.state[c] = {k: v.clone() for k, v in snap[p][1].items()}
        ref.step()
        for p in stepped:
            c = clones[p]
            assert float(o.state[p]["step"]) == float(ref.state[c]["step"]) == float(snap[p][1]["step"]) + 1
            _close_param(p, c, tuple(p.shape))
            _close_state(o, ref, p, c, tuple(p.shape))
        # the heads' lr is now exactly 0
        assert [grp["lr"] for grp in o.param_groups][0] == 0.0
        for dt in bs[2:]:
            before = [p.detach().clone() for p in heads + others]
            step(dt)
            sched.step()
            after = heads + others
            assert all(torch.equal(a.detach(), b) for a, b in zip(after[:len(heads)], before[:len(heads)]))
            moved = sum(not torch.equal(a.detach(), b) for a, b in zip(after[len(heads):], before[len(heads):]))
            assert moved > len(others) // 2, moved
    _no_scheduler_warning(caught)
    assert step.captures == 1 and step.replays == len(bs) and len(step.graphs) == 1


def test_graphed_step_only_ft_captioner():
    """only_ft_captioner: the optimizer holds the captioner's parameters; the captured step still clips every gradient by the norm
    over all of them (train.py:407: clip_grad_norm_(model.parameters())) and leaves everything else bit-identical, without
    optimizer state"""
    from gvl_amd.criterion import weighted_loss_sum
    from gvl_amd.linear import deferred_wgrads
    from gvl_amd.parallel import GraphedTrainStep
    opt, model, crit, T = toy(only_ft_captioner=True, grad_clip=0.01)
    _, model_b, crit_b, _ = toy(only_ft_captioner=True, grad_clip=0.01)
    step = GraphedTrainStep(model, crit, opt, max_gt=8, max_cap_len=8, cap_len_policy="grow")
    cap_ids = {id(p) for p in model.captioner_parameters()}
    assert {id(p) for grp in step.optimizer.param_groups for p in grp["params"]} == cap_ids
    rest = [(n, p) for n, p in model.named_parameters() if id(p) not in cap_ids]
    start = {n: p.detach().clone() for n, p in rest}
    bs = batches(T)
    step(bs[0])
    # the reference's loop on an identical model: backward, then clip_grad_norm_ over model.parameters()
    out, loss = model_b(bs[0], crit_b, None, opt.transformer_input_type)
    final = weighted_loss_sum(loss, crit_b.weight_dict, {})
    with deferred_wgrads():
        final.backward()
    total = float(torch.nn.utils.clip_grad_norm_(model_b.parameters(), opt.grad_clip))
    assert total > 2 * opt.grad_clip                                     # (the clip is active)
    assert abs(float(step.clip_adam.last[0]) - total) <= 1e-4 * total
    # every gradient, the captioner's and the rest's, scaled by the one coefficient of the norm over all of them
    for part in (True, False):
        pairs = [(pa.grad, pb.grad) for pa, pb in zip(model.parameters(), model_b.parameters())
                 if (id(pa) in cap_ids) == part and pb.grad is not None]
        assert len(pairs) > 10
        diff = sum(float(((a - b) ** 2).sum()) for a, b in pairs) ** 0.5
        ref = sum(float((b ** 2).sum()) for _, b in pairs) ** 0.5
        assert diff <= 1e-3 * ref, (part, diff, ref)
    for dt in bs[1:4]:
        step(dt)
    for n, p in rest:
        assert torch.equal(p.detach(), start[n]), n
        assert p not in step.optimizer.state, n
    assert all(float(step.optimizer.state[p]["step"]) == 4.0 for p in model.captioner_parameters() if p.grad is not None)
    assert step.captures == 1


def test_graphed_step_refuses_a_stale_frozen_lr():
    """where the captured update is torch's own (here forced: ClipAdam declines), the learning rate is frozen into the graph; a
    change after the capture raises instead of being replayed silently as the old value"""
    from gvl_amd.parallel import GraphedTrainStep
    opt, model, crit, T = toy()
    step = GraphedTrainStep(model, crit, opt, max_gt=8, max_cap_len=8, cap_len_policy="grow")
    step.clip_adam.step = lambda params, clip_only=(): False
    bs = batches(T, 2)
    step(bs[0])
    step(bs[1])                                                          # same lr: replays
    step.optimizer.param_groups[0]["lr"] *= 0.5
    with pytest.raises(RuntimeError, match="hyper-parameters of the capture"):
        step(bs[0])
    assert step.captures == 1

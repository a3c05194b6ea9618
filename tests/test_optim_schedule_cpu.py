"""CPU: the reference trainer's optimizer and learning-rate schedule as gvl_amd.optim restates them (train.py:35-54,243-292) --
build_scheduler against the closed forms (and transformers' own warm-up schedules where transformers is installed),
build_optimizer's parameter groups for each switch, and TrainStep's optimizer under the defaults."""
import math
import warnings

import pytest
import torch

from gvl_amd.config import make_opt
from gvl_amd.optim import build_optimizer, build_scheduler


def _sgd_free_optimizer(lrs=(1e-4, 5e-5)):
    ps = [torch.nn.Parameter(torch.zeros(3)) for _ in lrs]
    return torch.optim.Adam([{"params": [p], "lr": lr} for p, lr in zip(ps, lrs)])


def _lrs(opt_, optimizer, sched, n):
    """the groups' lr in force at each of n steps (optimizer.step() first, as train.py:409-411 orders them)"""
    seen = []
    with warnings.catch_warnings():
        warnings.simplefilter("error")                   # (no "scheduler stepped before the optimizer" warning either)
        for _ in range(n):
            seen.append([g["lr"] for g in optimizer.param_groups])
            optimizer.step()
            sched.step()
    return seen


@pytest.mark.parametrize("strategy", ["warmup_linear", "warmup_cosine"])
@pytest.mark.parametrize("total,ratio", [(50, 0.1), (37, 0.25), (9, 0.05), (20, 0.0)])
def test_warmup_schedules_closed_form(strategy, total, ratio):
    opt = make_opt(learning_strategy=strategy, warm_up_ratio=ratio)
    optimizer = _sgd_free_optimizer()
    sched = build_scheduler(opt, optimizer, total)
    assert isinstance(sched, torch.optim.lr_scheduler.LambdaLR)
    warm = ratio * total                                 # a float, as train.py:39 passes it
    for step, lrs in enumerate(_lrs(opt, optimizer, sched, total + 3)):
        if step < warm:
            f = step / max(1, warm)
        elif strategy == "warmup_linear":
            f = max(0.0, (total - step) / max(1, total - warm))
        else:
            f = max(0.0, 0.5 * (1.0 + math.cos(math.pi * 0.5 * 2.0 * (step - warm) / max(1, total - warm))))
        for lr, base in zip(lrs, (1e-4, 5e-5)):
            assert lr == pytest.approx(base * f, rel=1e-12, abs=1e-20), (step, lr, base * f)


@pytest.mark.parametrize("strategy", ["warmup_linear", "warmup_cosine"])
def test_warmup_schedules_equal_transformers(strategy):
    tf = pytest.importorskip("transformers")
    make = tf.get_linear_schedule_with_warmup if strategy == "warmup_linear" else tf.get_cosine_schedule_with_warmup
    for total, ratio in [(50, 0.1), (37, 0.25), (9, 0.05)]:
        opt = make_opt(learning_strategy=strategy, warm_up_ratio=ratio)
        oa, ob = _sgd_free_optimizer(), _sgd_free_optimizer()
        sa = build_scheduler(opt, oa, total)
        sb = make(ob, num_warmup_steps=ratio * total, num_training_steps=total)
        assert _lrs(opt, oa, sa, total + 3) == _lrs(opt, ob, sb, total + 3)


@pytest.mark.parametrize("over", [{}, {"epoch": 20, "learning_rate_decay_start": 4, "learning_rate_decay_every": 5,
                                       "learning_rate_decay_rate": 0.1}])
def test_multi_step_schedule(over):
    opt = make_opt(**over)
    assert opt.learning_strategy == "multi_step"
    optimizer = _sgd_free_optimizer()
    sched = build_scheduler(opt, optimizer, 1000)
    assert isinstance(sched, torch.optim.lr_scheduler.MultiStepLR)
    start, every, rate = opt.learning_rate_decay_start, opt.learning_rate_decay_every, opt.learning_rate_decay_rate
    milestones = [start + every * k for k in range(int((opt.epoch - start) / every))]
    if not over:
        assert milestones == [8, 11, 14, 17, 20, 23, 26]
    for epoch, lrs in enumerate(_lrs(opt, optimizer, sched, opt.epoch)):     # stepped once per epoch (train.py:584)
        f = rate ** sum(1 for m in milestones if m <= epoch)
        for lr, base in zip(lrs, (1e-4, 5e-5)):
            assert lr == pytest.approx(base * f, rel=1e-12)


def test_unknown_strategy_raises():
    with pytest.raises(NotImplementedError):
        build_scheduler(make_opt(learning_strategy="cyclic"), _sgd_free_optimizer(), 10)


@pytest.fixture(scope="module")
def cpu_model():
    from gvl_amd.pdvc import build
    opt = make_opt(num_queries=8, feature_dim=64, vocab_size=40, max_caption_len=6, device="cpu")
    model, criterion, _, _ = build(opt)
    return model, criterion


def _ids(ps):
    return {id(p) for p in ps}


@pytest.mark.parametrize("kind", ["adam", "adamw"])
@pytest.mark.parametrize("heads", [False, True])
@pytest.mark.parametrize("captioner_only", [False, True])
def test_build_optimizer_groups_as_train_py(cpu_model, kind, heads, captioner_only):
    """train.py:243-292: every switch, the groups' members (by the reference's name rules: pdvc.py captioner_parameters /
    bbox_head_parameters), their lr, the weight decay and the optimizer class"""
    model, _ = cpu_model
    opt = make_opt(optimizer_type=kind, task_heads_different_lr=heads, only_ft_captioner=captioner_only, lr=1e-4,
                   task_heads_lr=3e-5, weight_decay=1e-3, device="cpu")
    named = list(model.named_parameters())
    cap = [p for n, p in named if "caption_head" in n]
    box = [p for n, p in named if "bbox_head" in n]
    everything = cap if captioner_only else [p for _, p in named]
    o = build_optimizer(model, opt)
    assert type(o) is {"adam": torch.optim.Adam, "adamw": torch.optim.AdamW}[kind]
    if heads:
        expect = [(cap + box, 3e-5), ([p for p in everything if id(p) not in _ids(cap + box)], 1e-4)]
    else:
        expect = [(everything, 1e-4)]
    assert len(o.param_groups) == len(expect)
    for g, (ps, lr) in zip(o.param_groups, expect):
        assert _ids(g["params"]) == _ids(ps) and len(g["params"]) == len(ps)
        assert g["lr"] == lr and g["weight_decay"] == 1e-3 and g["betas"] == (0.9, 0.999) and g["eps"] == 1e-8
        assert g["decoupled_weight_decay"] == (kind == "adamw")


def test_train_step_defaults_adam_one_group(cpu_model):
    """make_opt() without the new keys' overrides (and a Namespace without them at all) still gives TrainStep the optimizer it
    always built: torch.optim.Adam over every trainable parameter, one group at opt.lr"""
    import argparse
    from gvl_amd.parallel import TrainStep
    model, criterion = cpu_model
    opt = make_opt(device="cpu")
    new_keys = ("optimizer_type", "learning_strategy", "warm_up_ratio", "learning_rate_decay_start", "learning_rate_decay_every",
                "learning_rate_decay_rate", "epoch", "task_heads_different_lr", "task_heads_lr", "only_ft_captioner")
    assert (opt.optimizer_type, opt.task_heads_different_lr, opt.only_ft_captioner) == ("adam", False, False)
    old = argparse.Namespace(**{k: v for k, v in vars(opt).items() if k not in new_keys})
    trainable = [p for p in model.parameters() if p.requires_grad]
    for o in (opt, old):
        ts = TrainStep(model, criterion, o)
        assert type(ts.optimizer) is torch.optim.Adam and len(ts.optimizer.param_groups) == 1
        g = ts.optimizer.param_groups[0]
        assert [id(p) for p in g["params"]] == [id(p) for p in trainable]
        assert g["lr"] == opt.lr and g["weight_decay"] == opt.weight_decay and not g["decoupled_weight_decay"]
        assert not g["fused"] and not g["capturable"]
    assert isinstance(build_scheduler(old, ts.optimizer, 100), torch.optim.lr_scheduler.MultiStepLR)

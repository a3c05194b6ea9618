"""The update of the training step -- ``clip_grad_norm_(params, max_norm); optimizer.step()`` of train.py:405-409 with a
``torch.optim.Adam`` or ``AdamW`` -- on gvl_clip_adam_groups_step_f32 (gvl_optim.hip): three launches over a table of (parameter,
gradient, moments) instead of torch's ~10 multi-tensor launches that pass over the gradients three times.  The optimizer object, its
hyper-parameters and its STATE stay torch's (``state_dict`` / checkpoints unchanged): this only replaces what one clip + step
computes.  Each parameter group's hyper-parameters reach the kernels through a small device table (``ClipAdam.sync``), so a
captured step replays the learning rate a scheduler set, not the one in force at capture time.
Anything this path does not cover (amsgrad, maximize, a tensor lr, non-fp32 or non-contiguous tensors, state not yet created)
falls back to torch's own launches -- same numbers either way, to fp32 rounding (tests/test_gpu_optim.py,
tests/test_gpu_optim_groups.py).

``build_optimizer`` / ``build_scheduler`` restate the reference trainer's optimizer and learning-rate schedule (train.py:243-292,
35-54) without importing transformers."""
import ctypes
import math

import numpy as np
import torch

from . import _lib

class _Desc(ctypes.Structure):                      # include/gvl_msda.h: gvl_adam_desc
    _fields_ = [("p", ctypes.c_void_p), ("g", ctypes.c_void_p), ("m", ctypes.c_void_p), ("v", ctypes.c_void_p),
                ("step", ctypes.c_void_p), ("n", ctypes.c_int64), ("vec", ctypes.c_int), ("group", ctypes.c_int)]


def bump_versions(tensors):
    """The kernels of this file -- and every hipGraph replay of a captured update -- write parameters through raw pointers, so
    torch's version counters do not move by themselves.  Every weight-derived cache of the package (split-fp16 planes, the
    captioner's stacked matrices, captured eval / decode graphs, reference-point tables) is keyed on (data_ptr, _version): without
    this bump an evaluation after training would run on the planes of the weights it saw first.  No launch, no
    synchronisation: the counter is host-side metadata, as torch's own in-place update would have moved it."""
    torch.autograd.graph.increment_version(tensors)


_HYPER_COLS = 8                                     # include/gvl_msda.h: GVL_ADAM_HYPER_COLS
_CLIP_ONLY = -1                                     # gvl_adam_desc.group of a tensor that is clipped but not updated


class ClipAdam:
    def __init__(self, optimizer, max_norm):
        # max_norm reaches clip_grad_norm_'s formula unchanged (0 zeroes the gradients, as torch's own call with 0 does)
        self.opt, self.max_norm = optimizer, float(max_norm)
        self.tables = {}
        self.last = None                                     # scal tensor of the last step: [total norm, clip coefficient, ...]
        self.hyper_dev = None                                # device table: one row of _HYPER_COLS doubles per parameter group
        self.written = None                                  # the rows last copied into it

    def hyper(self):
        """((lr, weight_decay, beta1, beta2, eps, mode), ...) per parameter group as the kernels take them (mode 1 = AdamW's
        decoupled decay), or None when the optimizer is not one this path covers"""
        if not isinstance(self.opt, torch.optim.Adam):       # (AdamW is an Adam with decoupled_weight_decay=True)
            return None
        rows = []
        for g in self.opt.param_groups:
            if g.get("amsgrad") or g.get("maximize") or g.get("differentiable") or isinstance(g["lr"], torch.Tensor):
                return None
            b1, b2 = g["betas"]
            rows.append((float(g["lr"]), float(g["weight_decay"]), float(b1), float(b2), float(g["eps"]),
                         1.0 if g.get("decoupled_weight_decay") else 0.0))
        return tuple(rows)

    def sync(self):
        """copy the groups' current hyper-parameters into the device table, only when they changed since the last copy: one
        small host -> device copy on the current stream, ordered before the launches (or the graph replay) that follow.  Must
        run outside a capture.  -> False when the optimizer is not one this path covers."""
        rows = self.hyper()
        if rows is None:
            return False
        if rows == self.written:
            return True
        for lr, wd, b1, b2, eps, _ in rows:
            if not (lr >= 0.0 and wd >= 0.0 and eps >= 0.0 and 0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
                raise ValueError(f"ClipAdam: lr, weight_decay, eps >= 0 and betas in [0, 1) (got {rows})")
        if self.hyper_dev is None:
            # sized once (room for groups added later): captured graphs keep this address
            dev = self.opt.param_groups[0]["params"][0].device
            self.hyper_dev = torch.zeros((max(16, len(rows)), _HYPER_COLS), dtype=torch.float64, device=dev)
        if len(rows) > self.hyper_dev.shape[0]:
            raise RuntimeError(f"ClipAdam: {len(rows)} parameter groups, the device table holds {self.hyper_dev.shape[0]}")
        # a FRESH pinned buffer per copy: the caching host allocator hands it out again only after this copy has run
        host = torch.zeros((len(rows), _HYPER_COLS), dtype=torch.float64)
        host[:, :6] = torch.tensor(rows, dtype=torch.float64)
        self.hyper_dev[:len(rows)].copy_(host.pin_memory(), non_blocking=True)
        self.written = rows
        return True

    def _state(self, params):
        """[(p, grad, exp_avg, exp_avg_sq, step)] or None when something is not what the kernels take"""
        rows = []
        for p in params:
            st = self.opt.state.get(p)
            if not st or "exp_avg" not in st:
                return None
            g, m, v, t = p.grad, st["exp_avg"], st["exp_avg_sq"], st["step"]
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32):
                return None
            for x in (p, g, m, v):
                if not _kernel_tensor(x, p):
                    return None
            rows.append((p, g, m, v, t))
        return rows

    def _build(self, rows, clip_rows, vec_grads):
        chunk = _lib.lib().gvl_adam_chunk_elems()
        dev = (rows or clip_rows)[0][0].device
        group_of = {id(p): i for i, g in enumerate(self.opt.param_groups) for p in g["params"]}
        descs, cmap = [], []
        for p, g, m, v, t in rows + clip_rows:
            i, n = len(descs), p.numel()
            if m is None:                                     # clip-only: only the gradient is read and written
                vec = int(vec_grads and n % 4 == 0)
                descs.append(_Desc(p.data_ptr(), None, None, None, None, n, vec, _CLIP_ONLY))
            else:
                vec = int(vec_grads and n % 4 == 0 and all(x.data_ptr() % 16 == 0 for x in (p, m, v)))
                descs.append(_Desc(p.data_ptr(), None, m.data_ptr(), v.data_ptr(), t.data_ptr(), n, vec, group_of[id(p)]))
            cmap.extend((i, c) for c in range((n + chunk - 1) // chunk))
        arr = (_Desc * len(descs))(*descs)
        raw = np.frombuffer(ctypes.string_at(ctypes.addressof(arr), ctypes.sizeof(arr)), dtype=np.uint8).copy()
        return {"descs": torch.from_numpy(raw).to(dev), "cmap": torch.tensor(cmap, dtype=torch.int32, device=dev).contiguous(),
                "partial": torch.empty(len(cmap), dtype=torch.float32, device=dev),
                "scal": torch.zeros(4, dtype=torch.float32, device=dev),
                "corr": torch.zeros(2 * len(descs), dtype=torch.float32, device=dev), "n_chunks": len(cmap),
                "ptrs": _ptrs(rows, clip_rows), "steps": [r[4] for r in rows], "n": len(descs)}

    def step(self, params, clip_only=()):
        """clip over `params` + `clip_only`, Adam / AdamW over `params` (those that have a gradient and belong to the optimizer;
        `clip_only`: tensors with a gradient outside it, which count in the norm and have their gradient scaled, nothing else:
        train.py's only_ft_captioner clips model.parameters() and steps the captioner's) -> True, or False when torch's own
        path must run"""
        params, clip_only = list(params), list(clip_only)
        if not (params or clip_only) or not (params or clip_only)[0].is_cuda:
            return False
        capturing = torch.cuda.is_current_stream_capturing()
        # outside a capture the table is brought up to date here; a captured step reads it at replay time, after the sync the
        # caller runs before every replay (GraphedTrainStep)
        if capturing:
            if self.hyper() is None or self.hyper_dev is None:
                return False
        elif not self.sync():
            return False
        rows = self._state(params)
        if rows is None or not all(p.grad is not None and _kernel_tensor(p.grad, p) and _kernel_tensor(p, p) for p in clip_only):
            return False
        clip_rows = [(p, p.grad, None, None, None) for p in clip_only]
        # gradients 16-byte aligned (fresh tensors: always; views of a flat buffer: not all): the table's `vec` flags count on it
        vec_grads = all(r[1].data_ptr() % 16 == 0 for r in rows + clip_rows)
        key = (tuple(id(p) for p in params), tuple(id(p) for p in clip_only), vec_grads)
        tab = self.tables.get(key)
        if tab is None or tab["ptrs"] != _ptrs(rows, clip_rows):
            if capturing:                                         # (the table is built with host -> device copies)
                return False
            tab = self.tables[key] = self._build(rows, clip_rows, vec_grads)
        # the gradients' addresses change (a step without a flat buffer gets fresh tensors from autograd; a captured step's live
        # in the graph's pool): they reach the table through the arguments of a launch
        dev = (params or clip_only)[0].device
        gp = (ctypes.c_void_p * tab["n"])(*[r[1].data_ptr() for r in rows + clip_rows])
        with torch.cuda.device(dev):
            rc = _lib.lib().gvl_adam_set_grads(tab["descs"].data_ptr(), tab["n"], gp, torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "adam_set_grads")
        if tab["steps"]:
            torch._foreach_add_(tab["steps"], 1.0)
        with torch.cuda.device(dev):
            rc = _lib.lib().gvl_clip_adam_groups_step_f32(tab["descs"].data_ptr(), tab["n"], tab["cmap"].data_ptr(),
                                                          tab["n_chunks"], tab["partial"].data_ptr(), tab["scal"].data_ptr(),
                                                          tab["corr"].data_ptr(), self.hyper_dev.data_ptr(),
                                                          self.hyper_dev.shape[0], self.max_norm,
                                                          torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "clip_adam_groups_step")
        # parameters updated, gradients clipped in place
        bump_versions([r[0] for r in rows] + [r[1] for r in rows + clip_rows])
        self.opt._opt_called = True          # (what torch's LRScheduler checks: its optimizer.step() wrapper was bypassed)
        self.last = tab["scal"]
        return True


def _kernel_tensor(x, p):
    return (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.device == p.device and x.numel() == p.numel()
            and x.data_ptr() % 4 == 0)


def _ptrs(rows, clip_rows):
    return (tuple(x.data_ptr() for r in rows for x in (r[0], r[2], r[3], r[4])) + tuple(r[0].data_ptr() for r in clip_rows))


# ---- the reference trainer's optimizer and schedule ------------------------------------------------------------------------------
def build_optimizer(model, opt, params=None, **torch_kwargs):
    """train.py:243-292: Adam or AdamW (opt.optimizer_type) over one group at opt.lr, or -- task_heads_different_lr -- the
    captioner and box heads at opt.task_heads_lr and everything else at opt.lr; only_ft_captioner keeps only the captioner's
    parameters (the rest still has gradients, which the step clips with them: train.py:407).  `params` (default: the model's
    parameters) is what "everything" means; options missing from `opt` take the reference's defaults (opts.py), so an older
    Namespace still gives Adam with one group.  torch_kwargs (capturable, fused, ...) go to the torch optimizer.  The
    frozen text encoder of a contrastive model is left out (train.py:242-246); the word-level pool, the contrastive projections
    and the background embedding are ordinary parameters of "everything".  ft_captioner_from_scratch and only_ft_class_head are
    out of scope."""
    other = [p for p in (model.parameters() if params is None else params)]
    if getattr(model, "text_encoder", None) is not None:
        frozen = {id(p) for p in model.text_encoder.parameters()}
        other = [p for p in other if id(p) not in frozen]
    if getattr(opt, "only_ft_captioner", False):
        other = model.captioner_parameters()
    if getattr(opt, "task_heads_different_lr", False):
        heads = model.captioner_parameters() + model.bbox_head_parameters()
        head_ids = {id(p) for p in model.caption_head.parameters()} | {id(p) for p in model.bbox_head.parameters()}
        groups = [{"params": heads, "lr": getattr(opt, "task_heads_lr", 5e-5)},
                  {"params": [p for p in other if id(p) not in head_ids], "lr": opt.lr}]
    else:
        groups = [{"params": other, "lr": opt.lr}]
    kind = getattr(opt, "optimizer_type", "adam")
    cls = {"adam": torch.optim.Adam, "adamw": torch.optim.AdamW}.get(kind)
    if cls is None:
        raise ValueError(f"optimizer_type {kind!r}: have 'adam', 'adamw'")
    return cls(groups, weight_decay=opt.weight_decay, **torch_kwargs)


def _warmup_linear(warmup, total):
    # transformers.get_linear_schedule_with_warmup's factor (num_warmup_steps may be a float: train.py:39)
    def f(step):
        if step < warmup:
            return float(step) / float(max(1, warmup))
        return max(0.0, float(total - step) / float(max(1, total - warmup)))
    return f


def _warmup_cosine(warmup, total, cycles=0.5):
    # transformers.get_cosine_schedule_with_warmup's factor
    def f(step):
        if step < warmup:
            return float(step) / float(max(1, warmup))
        progress = float(step - warmup) / float(max(1, total - warmup))
        return max(0.0, 0.5 * (1.0 + math.cos(math.pi * float(cycles) * 2.0 * progress)))
    return f


def build_scheduler(opt, optimizer, total_steps):
    """train.py:35-54.  warmup_linear / warmup_cosine: a LambdaLR stepped once per batch (train.py:410-411) with
    num_warmup_steps = warm_up_ratio * total_steps; multi_step: MultiStepLR at epochs learning_rate_decay_start + k *
    learning_rate_decay_every, stepped once per epoch (train.py:584).  Options missing from `opt` take opts.py's defaults."""
    strategy = getattr(opt, "learning_strategy", "multi_step")
    if strategy in ("warmup_linear", "warmup_cosine"):
        warmup = getattr(opt, "warm_up_ratio", 0.1) * total_steps
        f = (_warmup_linear if strategy == "warmup_linear" else _warmup_cosine)(warmup, total_steps)
        return torch.optim.lr_scheduler.LambdaLR(optimizer, f)
    if strategy == "multi_step":
        start = getattr(opt, "learning_rate_decay_start", 8)
        every = getattr(opt, "learning_rate_decay_every", 3)
        milestones = [start + every * k for k in range(int((getattr(opt, "epoch", 30) - start) / every))]
        return torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones, gamma=getattr(opt, "learning_rate_decay_rate", 0.5))
    raise NotImplementedError(f"learning_strategy {strategy!r}")


def contrastive_weight(opt, epoch):
    """the weight of the contrastive losses in force at `epoch` (train.py:304-311,363-368): cl_schedule_val[i] from epoch
    cl_schedule_time[i] on"""
    times, vals = list(opt.cl_schedule_time), list(opt.cl_schedule_val)
    weight = 0.0
    for t_, v in zip(times, vals):
        if epoch >= t_:
            weight = v
    return weight


def apply_contrastive_schedule(criterion, opt, epoch):
    """train.py:343-346,363-368: every contrastive_loss* weight of the set criterion, and the matcher's cost_cl -- 0 while the weight is 0"""
    weight = contrastive_weight(opt, epoch)
    for key in criterion.weight_dict:
        if 'contrastive_loss' in key:
            criterion.weight_dict[key] = weight
    criterion.matcher.cost_cl = 0 if weight == 0 else opt.set_cost_cl
    return weight

"""What every hipGraph capture of the package shares (gvl_amd.parallel's captured train / eval steps, the captioner's
captured greedy loop): the bounded graph cache and its keys, the two static batch forms a captured step reads its
inputs from, the grow-only capacities of the padded form, and the warm-up / capture stream discipline."""
import contextlib
from collections import OrderedDict
from dataclasses import dataclass
from typing import Any, NamedTuple

import torch

from .targets import PaddedTargets, needed_capacity, round_up_pow2, total_events


class _LRU(OrderedDict):
    """captured graphs, least recently used first; each entry pins a private memory pool, so the cache is bounded"""

    def __init__(self, limit):
        super().__init__()
        self.limit = max(1, int(limit))

    def lookup(self, key):
        entry = self.get(key)
        if entry is not None:
            self.move_to_end(key)
        return entry

    def store(self, key, entry):
        self[key] = entry
        self.move_to_end(key)
        while len(self) > self.limit:
            self.popitem(last=False)


class _GraphKey(NamedTuple):
    """what a captured step depends on.  form "padded": `shapes` of the three feature tensors + the capacities of the
    padded layout (`slots` per video, caption width `cap_len`, caption `rows`; the eval forward has no caption buffers:
    0, 0).  form "layout": `shapes` of every tensor of the batch, `slots` = the events of each video (a tuple),
    `cap_len` = the teacher-forcing length (train).  `epoch`: the parameter version an eval graph was captured at."""
    form: str
    shapes: tuple
    slots: Any = 0
    cap_len: int = 0
    rows: int = 0
    epoch: int = 0


@dataclass
class _Entry:
    """one cached capture: the graphs in replay order, the static batch they read, their static outputs (+ the eval
    forward's loss dict and the `alive` flags of its decode segments)"""
    graphs: tuple
    batch: Any
    outs: Any
    loss: Any = None
    flags: Any = None


def _shape_sig(dt, keys=None):
    """(name, shape, dtype) of dt's tensors (`keys`: of these only)"""
    if keys is None:
        keys = [k for k, v in dt.items() if isinstance(v, torch.Tensor)]
    return tuple((k, tuple(dt[k].shape), str(dt[k].dtype)) for k in keys)


def _drop_superseded(graphs, key, keep_width_buckets=False):
    """grow-only capacities never shrink, so a padded graph of the same tensor shapes with a smaller one is never
    replayed again.  With cap_len_policy="bucket" the caption width is not a grow-only capacity: graphs that differ
    only in it stay.  (Keys may be plain tuples in _GraphKey's field order.)"""
    def named(k):
        return k if isinstance(k, _GraphKey) else _GraphKey(*k)

    def grow_part(k):
        return (k.slots, k.rows) if keep_width_buckets else (k.slots, k.cap_len, k.rows)
    key = named(key)
    for k in [k for k in graphs if named(k).form == "padded" and named(k).shapes == key.shapes
              and grow_part(named(k)) != grow_part(key)]:
        del graphs[k]


_STATIC_KEYS = ("video_tensor", "video_mask", "video_length")


class _PaddedBatch:
    """static device buffers of one captured step: the three feature tensors of pdvc.py:250-258 + PaddedTargets"""

    def __init__(self, dt, slots, cap_len, pair_rows=0):
        dev = dt["video_tensor"].device
        self.dt = {k: dt[k].clone() for k in _STATIC_KEYS}
        self.targets = PaddedTargets(dt["video_tensor"].shape[0], slots, cap_len, dev, pair_rows)
        self.dt["_gvl_targets"] = self.targets
        # paths that still want the reference's list (LayerMatch.host(), PostProcess) are served from the host counts
        self.dt["video_target"] = None

    def load(self, dt, num_boxes=None):
        for k in _STATIC_KEYS:
            self.dt[k].copy_(dt[k], non_blocking=True)
        self.targets.load(dt, num_boxes)
        for k, v in dt.items():                               # non-tensor bookkeeping travels along (video_key, cap_raw ...)
            if k not in self.dt and not isinstance(v, torch.Tensor):
                self.dt[k] = v
        self.dt["video_target"] = dt["video_target"]


class _LayoutBatch:
    """static copy of a whole batch, for the fallback form (one graph per batch layout): every tensor of dt, those
    inside `video_target` included, at an address of its own.  `load` copies the next batch of the same layout in
    place; non-tensor entries travel along as they are.  A captured step reads non-tensor entries only while it is
    being recorded, so carrying them cannot change a replay."""

    def __init__(self, dt):
        def copy(d):
            return {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in d.items()}
        self.dt = copy(dt)
        self.dt["video_target"] = [copy(t_) for t_ in dt.get("video_target") or []]

    def load(self, dt):
        def refresh(dst, src):
            for k, v in src.items():
                if isinstance(v, torch.Tensor):
                    dst[k].copy_(v, non_blocking=True)
                elif k != "video_target":
                    dst[k] = v
        refresh(self.dt, dt)
        for a, b in zip(self.dt["video_target"], dt.get("video_target") or []):
            refresh(a, b)


class _Capacity:
    """Grow-only capacities of the padded layout: slots per video = next power of two >= the largest event count seen
    (>= 4), caption width = next multiple of 4 >= the widest caption tensor seen, caption rows (matched pairs of a
    whole batch, train only) = next multiple of 32 >= the largest event total seen.  A batch that does not fit raises
    the capacity and the step is captured again; in a steady run that happens a handful of times, then never."""

    def __init__(self, slots=0, cap_len=0, pair_rows=0, cap_len_policy="grow", cap_len_step=4):
        self.slots, self.cap_len, self.pair_rows = int(slots or 0), int(cap_len or 0), int(pair_rows or 0)
        self.cap_len_policy, self.cap_len_step = cap_len_policy, max(1, int(cap_len_step))

    def fit(self, dt, with_captions):
        n_gt, cap_len = needed_capacity(dt)
        self.slots = max(self.slots, round_up_pow2(n_gt, 4))
        if not with_captions:
            return self.slots, 0
        step = self.cap_len_step
        bucket = step * ((max(cap_len, 2) + step - 1) // step)
        self.cap_len = max(self.cap_len, bucket)
        self.pair_rows = max(self.pair_rows, 32 * ((max(total_events(dt), 1) + 31) // 32))
        # "bucket": the step runs at THIS batch's caption-width bucket (one graph per bucket of cap_len_step tokens)
        # instead of at the widest caption tensor seen so far -- the teacher-forced loop is serial in
        # the caption length, so a batch of 10-word captions then pays 11 steps, not the 23 a 22-word batch once needed
        return self.slots, (bucket if self.cap_len_policy == "bucket" else self.cap_len)


def _padded_eligible(model, criterion, capacity, dt, eval_mode, num_queries, required=None):
    """can this batch run on the padded form?  The model / criterion pair must have a padded-target path at the slots
    the batch needs (`required`: name of a step whose caller insisted on one -- its absence is then an error), and
    those slots must not exceed 64 or the number of queries."""
    if criterion is None:
        return False
    slots = max(capacity.slots, round_up_pow2(needed_capacity(dt)[0], 4))
    ok = model.supports_padded_targets(criterion, eval_mode=eval_mode, batch=dt["video_tensor"].shape[0], slots=slots)
    if not ok and required:
        raise RuntimeError(f"{required}(padded=True): this model / criterion has no padded-target path")
    return ok and slots <= min(64, num_queries)


@contextlib.contextmanager
def side_stream(device=None):
    """run the body on a fresh side stream ordered after the current stream, then make the current stream wait for it
    -> the side stream.  This is where a capture's eager warm-up runs: >= 1 real run must precede a capture (autograd's
    gradient accumulators, hipBLASLt workspaces and lazily built constants have to exist before a stream is capturing)."""
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        yield side
    torch.cuda.current_stream().wait_stream(side)


@contextlib.contextmanager
def capture_on(side, pool=None):
    """capture the body into a new graph (-> the graph), optionally into the memory pool of an earlier one, ON the
    stream the warm-up ran on (`side_stream`): autograd's AccumulateGrad nodes were created there and keep running
    there; captured from another stream they become a parallel branch of the graph that the optimizer kernels do not
    wait for (seen as NaN parameters after a few replays of the bf16 step)"""
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, pool=pool, stream=side):
        yield graph

"""What tests/test_gpu_mha_train_ops.py compares the attention core of gvl_amd/csrc/gvl_mha_train.hip with, and the seeded cases it
runs (no tests here; tests/test_mha_train_ref_cpu.py checks this file without a GPU):

    core_restatement   the core in vectorised torch for any floating type: the reference is its fp64 evaluation, the gradients are
                       autograd's on that evaluation, and its fp32 evaluation measures what fp32 can give
    _hash32, _keep_mask  the dropout mask rule of include/gvl_msda.h, recomputed
    CASES / inputs / reference  the case table: inputs drawn in fp32 from a fixed seed and widened, so both sides see the same numbers
"""
import functools
import zlib

import torch

D = 64                                      # head dimension
DROP_PS = (0.125, 0.25, 0.5, 0.9375)        # p 2^32 is an integer in fp32: the threshold of the mask rule has no rounding question


# ---------------------------------------------------------------------------------------------------------------------------
# the dropout mask rule
# ---------------------------------------------------------------------------------------------------------------------------
def _hash32(x):
    m = 0xFFFFFFFF
    x = x & m
    x = x ^ (x >> 16); x = (x * 0x7feb352d) & m
    x = x ^ (x >> 15); x = (x * 0x846ca68b) & m
    return x ^ (x >> 16)


def _keep_mask(B, H, Q, p, seed, step, device="cuda:0"):
    """weight (b, h, q, k) is kept iff hash32(((b H + h) Q + q) Q + k ^ hash32(seed + step 0x9E3779B9)) >= p 2^32"""
    key = _hash32(torch.tensor((seed + step * 0x9E3779B9) & 0xFFFFFFFF, dtype=torch.int64, device=device))
    idx = torch.arange(B * H * Q * Q, dtype=torch.int64, device=device)
    # (the kernel receives p as a C float: 0.1f 2^32 is 7 above 0.1 2^32 -- one mask element in 6e8 would differ, which fails
    #  this test at about one (seed, step) pair in fifty)
    thr = min(int(float(torch.tensor(p, dtype=torch.float32)) * 4294967296.0), 0xFFFFFFFF)
    return (_hash32(idx ^ key) >= thr).view(B, H, Q, Q)


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------
def drop_scale(p):
    """1 / (1 - p) as the kernels compute it: in fp32"""
    one = torch.ones((), dtype=torch.float32)
    return float(one / (one - torch.tensor(p, dtype=torch.float32)))


def _heads(t, H):
    B, Q, _ = t.shape
    return t.reshape(B, Q, H, D).transpose(1, 2)                     # (B, H, Q, 64)


def scores(qkv, key_keep):
    """(B, H, Q, Q) scores q . k / 8 with the excluded keys at -inf"""
    C = qkv.shape[-1] // 3
    H = C // D
    s = _heads(qkv[..., :C], H) @ _heads(qkv[..., C:2 * C], H).transpose(-1, -2) * 0.125
    if key_keep is not None:
        s = s.masked_fill(~key_keep[:, None, None, :], float("-inf"))
    return s


def core_restatement(qkv, key_keep, drop_keep, p):
    """qkv (B, Q, 3 H 64) = [q | k | v], key_keep (B, Q) bool or None, drop_keep (B, H, Q, Q) or None, p
    -> out (B, Q, H 64) = dropout(softmax_k(q . k / 8 over the kept keys)) v per head, lse (B, H, Q) = log sum_k exp(score)"""
    B, Q, W = qkv.shape
    C = W // 3
    H = C // D
    s = scores(qkv, key_keep)
    lse = torch.logsumexp(s, -1)
    a = torch.softmax(s, -1)
    if drop_keep is not None:
        a = a * drop_keep.to(qkv.dtype) * torch.tensor(drop_scale(p), dtype=torch.float32).to(qkv.dtype)
    out = (a @ _heads(qkv[..., 2 * C:], H)).transpose(1, 2).reshape(B, Q, C)
    return out, lse


def evaluate(qkv32, key_keep, drop_keep, p, g32, dt):
    """the restatement and its gradients under the output gradient g, in type dt
    -> dict(out (B, Q, H 64), lse (B, H, Q), dq, dk, dv (B, Q, H 64 each))"""
    qkv = qkv32.to(dt, copy=True).requires_grad_()
    out, lse = core_restatement(qkv, key_keep, drop_keep, p)
    dqkv, = torch.autograd.grad((out * g32.to(dt)).sum(), qkv)
    C = out.shape[-1]
    return dict(out=out.detach(), lse=lse.detach(), dq=dqkv[..., :C], dk=dqkv[..., C:2 * C], dv=dqkv[..., 2 * C:])


def cancelling_terms(qkv32, key_keep, drop_keep, p, g32):
    """fp64: max over the entries of sum_k |P dP| |k| / 8 (dq) and sum_q |P dP| |q| / 8 (dk), the terms whose difference
    P (dP - delta) the two gradients are made of: the scale of dq and dk where that difference is zero in exact arithmetic (a
    single key: Q = 1)"""
    qkv, g = qkv32.double(), g32.double()
    C = qkv.shape[-1] // 3
    H = C // D
    a = torch.softmax(scores(qkv, key_keep), -1)
    f = 1.0 if drop_keep is None else drop_keep.double() * drop_scale(p)
    t = (a * f * (_heads(g, H) @ _heads(qkv[..., 2 * C:], H).transpose(-1, -2))).abs()
    dq = float((t @ _heads(qkv[..., C:2 * C], H).abs()).max()) * 0.125
    dk = float((t.transpose(-1, -2) @ _heads(qkv[..., :C], H).abs()).max()) * 0.125
    return dict(dq=dq, dk=dk)


# ---------------------------------------------------------------------------------------------------------------------------
# the cases.  B <= 3, H in {1, 3}, Q <= 321; `mask` names the key mask (below), `kind` the way the inputs are shaped
# ---------------------------------------------------------------------------------------------------------------------------
EDGE_QS = (1, 31, 32, 33, 160, 161, 321)     # one wavefront owns 32 columns, one workgroup 160: 161 and 321 leave a workgroup
                                             # with a single live column and four idle wavefronts
CASES = {}
for _Q in EDGE_QS:
    for _H in (1, 3):
        for _p in (0.0, 0.25):
            CASES["edge_Q%d_H%d_p%s" % (_Q, _H, "25" if _p else "0")] = dict(B=2, Q=_Q, H=_H, p=_p, mask="suffix")
CASES.update({
    # key masks (Q = 70: two whole 32-key tiles and a partial one of 6)
    "mask_suffix": dict(B=3, Q=70, H=3, p=0.0, mask="suffix"),
    "mask_lead": dict(B=3, Q=70, H=3, p=0.0, mask="lead"),            # keys 0 .. 31 excluded: a leading tile without a valid key
    "mask_middle": dict(B=3, Q=70, H=3, p=0.0, mask="middle"),        # keys 32 .. 63 excluded
    "mask_single": dict(B=3, Q=70, H=3, p=0.0, mask="single"),        # one valid key, in the last, partial tile
    "mask_null": dict(B=3, Q=70, H=3, p=0.0, mask=None),
    # one video of three with every key excluded, and the same call with that video open
    "isolation": dict(B=3, Q=70, H=3, p=0.25, mask="isolation"),
    "isolation_open": dict(B=3, Q=70, H=3, p=0.25, mask="isolation_open", seed_of="isolation"),
    # dropout
    "drop_p125": dict(B=2, Q=70, H=3, p=0.125, mask="suffix"),
    "drop_p5": dict(B=2, Q=70, H=3, p=0.5, mask="suffix"),
    "drop_p9375": dict(B=2, Q=70, H=3, p=0.9375, mask="suffix"),
    # p = 0.5, Q = 33, video 1 with three valid keys (30, 31, 32: both sides of a tile edge): DROP_LOST_SEED is the first seed for
    # which some (b, h, q) row loses every weight (find_lost_row_seed)
    "drop_lost_row": dict(B=2, Q=33, H=3, p=0.5, mask="three", seed_drop="lost"),
    # p at the limit and a video whose single valid key has probability exactly 1: kept weights are 16, the operand 2^15
    "drop_p9375_single": dict(B=2, Q=33, H=3, p=0.9375, mask="single"),
    # saturation: scores within a row +-60 apart (one key carries the row), and one query whose scores are all equal
    "saturation": dict(B=2, Q=70, H=1, p=0.0, mask="suffix", kind="saturation"),
    "saturation_p25": dict(B=2, Q=70, H=3, p=0.25, mask="suffix", kind="saturation"),
    # operand range (include/gvl_msda.h: an element 2^-k below the video's largest keeps max(2^-23, 2^(k - 36)) of itself)
    "range_k_small": dict(B=2, Q=70, H=3, p=0.0, mask="suffix", kind="k_small"),        # k at 2^-10 of q: they share amax_qk
    # one row at 2^10 times the others: its q and v columns (range_row), its k and v columns (range_row_k), so that the scores stay
    # ordinary.  (The WHOLE row is outside what include/gvl_msda.h holds to fp32 level -- its score with its own key is 2^20 times
    # the others' -- and is no case: the figures measured for it are in the header and in tests/test_gpu_mha_train_ops.py.)
    "range_row": dict(B=2, Q=70, H=3, p=0.0, mask="suffix", kind="row", cols="qv"),
    "range_row_k": dict(B=2, Q=70, H=3, p=0.0, mask="suffix", kind="row", cols="kv"),
    "range_video": dict(B=2, Q=70, H=3, p=0.0, mask="suffix", kind="video"),            # one video at 2^12 times the other
    "range_zero_v": dict(B=2, Q=70, H=3, p=0.0, mask="suffix", kind="zero_v"),
    "range_loose_am": dict(B=2, Q=70, H=3, p=0.25, mask="suffix", kind="plain", am_factor=4.0),
    # leading dimension 3 H 64 + 8 through the C entry points
    "ld": dict(B=2, Q=33, H=3, p=0.25, mask="suffix"),
})
STEP = 5                      # the step counter's value in every dropout case
DROP_LOST_SEED = 0            # (tests/test_mha_train_ref_cpu.py: equals find_lost_row_seed())
OUTLIER_ROW = (0, 7)          # range_row: (video, row)
EQUAL_ROW = (0, 3)            # saturation: the query whose scores are all equal


def _case_seed(name):
    return zlib.crc32(CASES[name].get("seed_of", name).encode())         # (fixed per name: adding a case moves no other)


def key_mask(kind, B, Q):
    """(B, Q) bool (True = attend) or None"""
    if kind is None:
        return None
    keep = torch.ones(B, Q, dtype=torch.bool)
    tail = lambda b: Q - (Q // 3 if b % 2 else Q // 7)                # noqa: E731  (ragged: a different suffix per video)
    if kind == "suffix":
        for b in range(1, B):                                         # video 0 unmasked
            keep[b, tail(b):] = False
    elif kind == "lead":
        keep[::2, :32] = False
        keep[1, tail(1):] = False
    elif kind == "middle":
        keep[::2, 32:64] = False
    elif kind == "single":                                            # video 1: one valid key, inside the last, partial tile
        keep[1] = False
        keep[1, Q - 1 - (Q % 32 > 1)] = True                          # (Q = 70: key 68 of 64 .. 69; Q = 33: key 32)
    elif kind == "three":                                             # video 1: keys 30, 31, 32 (both sides of a tile edge)
        keep[1] = False
        keep[1, 30:33] = True
    elif kind in ("isolation", "isolation_open"):
        keep[2, tail(2):] = False
        if kind == "isolation":
            keep[1] = False
    else:
        raise KeyError(kind)
    return keep


def find_lost_row_seed(limit=64):
    """the first dropout seed for which, in the case drop_lost_row, some (b, h, q) row with valid keys keeps none of them"""
    cfg = CASES["drop_lost_row"]
    keep = key_mask(cfg["mask"], cfg["B"], cfg["Q"])
    for seed in range(limit):
        if bool(lost_rows(_keep_mask(cfg["B"], cfg["H"], cfg["Q"], cfg["p"], seed, STEP, "cpu"), keep).any()):
            return seed
    raise AssertionError("no such seed")


def lost_rows(drop_keep, key_keep):
    """(B, H, Q) bool: rows whose every valid key is dropped"""
    valid = drop_keep if key_keep is None else drop_keep & key_keep[:, None, None, :]
    return ~valid.any(-1)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """fp32 CPU tensors of a case (never modified): qkv (B, Q, 3 H 64), g (B, Q, H 64) the gradient of out, keep (B, Q) bool or
    None, drop (B, H, Q, Q) bool or None, and B, Q, H, p, seed (of the dropout), step, am_factor"""
    cfg = CASES[name]
    B, Q, H, p = cfg["B"], cfg["Q"], cfg["H"], cfg["p"]
    C = H * D
    gen = torch.Generator().manual_seed(_case_seed(name))
    rnd = lambda *shape: torch.randn(*shape, generator=gen)          # noqa: E731
    qkv, g = rnd(B, Q, 3 * C), rnd(B, Q, C)
    kind = cfg.get("kind", "plain")
    if kind == "saturation":
        qkv[..., :2 * C] *= 30.0 ** 0.5                               # scores: deviation 30 (q . k over 64 channels / 8)
        qkv[EQUAL_ROW[0], EQUAL_ROW[1], :C] = 0.0                     # this query's scores are all 0
    elif kind == "k_small":
        qkv[0, :, :C] *= 2.0 ** 5
        qkv[0, :, C:2 * C] *= 2.0 ** -5
    elif kind == "row":
        qkv[0] *= 2.0 ** -5
        for j, c in enumerate("qkv"):
            if c in cfg["cols"]:
                qkv[OUTLIER_ROW[0], OUTLIER_ROW[1], j * C:(j + 1) * C] *= 2.0 ** 10
    elif kind == "video":
        qkv[0] *= 2.0 ** -11
        qkv[1] *= 2.0
    elif kind == "zero_v":
        qkv[..., 2 * C:] = 0.0
    keep = key_mask(cfg["mask"], B, Q)
    seed = DROP_LOST_SEED if cfg.get("seed_drop") == "lost" else (_case_seed(name) * 2654435761) & 0xFFFFFFFF
    drop = _keep_mask(B, H, Q, p, seed, STEP, "cpu") if p > 0 else None
    return dict(qkv=qkv, g=g, keep=keep, drop=drop, B=B, Q=Q, H=H, p=p, seed=seed, step=STEP, am_factor=cfg.get("am_factor", 1.0))


@functools.lru_cache(maxsize=None)
def reference(name):
    """(fp64, fp32) evaluations of the case's restatement and gradients: never modified.  The fp64 one also carries `cancel`
    (cancelling_terms)"""
    i = inputs(name)
    w64 = evaluate(i["qkv"], i["keep"], i["drop"], i["p"], i["g"], torch.float64)
    w64["cancel"] = cancelling_terms(i["qkv"], i["keep"], i["drop"], i["p"], i["g"])
    return w64, evaluate(i["qkv"], i["keep"], i["drop"], i["p"], i["g"], torch.float32)

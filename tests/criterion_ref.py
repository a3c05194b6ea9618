"""What tests/test_gpu_criterion_ops.py compares the kernels of gvl_amd/csrc/gvl_criterion.hip with (k_match_cost, k_match_cost_padded,
k_criterion_fwd / _bwd, k_ce_rows_fwd / _bwd), and the seeded cases it runs (no tests here; tests/test_criterion_ref_cpu.py checks
this file without a GPU):

    match_cost, match_cost_padded   the matcher's cost tensor of all decoder layers and the degenerate-box flag
    criterion                       the (layers, 6) loss table from EXPLICIT matches (no solver)
    ce_rows                         weight (x[target] - logsumexp x) and the logsumexp, per row
    CASES / inputs / reference      the case table: inputs drawn in fp32 from a fixed seed and widened, so both sides see the same numbers

Every function is plain torch for any floating type: the reference is its fp64 evaluation, the gradients are autograd's on that
evaluation (so the subgradients at ties are PyTorch's: minimum / maximum split a tie in half, clamp passes the gradient at its
boundary, abs has slope 0 at 0), and its fp32 evaluation on the CPU measures what fp32 can give.

Box coordinates of every tie case are dyadic rationals (centres multiples of 2^-6, lengths multiples of 2^-5): c +- l / 2 is then
exact in fp32 and a tie is a tie on both sides."""
import functools
import zlib

import torch
import torch.nn.functional as F

LOSS_KEYS = ('loss_ce', 'loss_counter', 'loss_bbox', 'loss_giou', 'loss_self_iou', 'cardinality_error')
EPS = 1e-5                                  # in the denominators of IoU and GIoU


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------
def ends(box):
    """(centre, length) -> (x0, x1)"""
    c, l = box.unbind(-1)
    return c - 0.5 * l, c + 0.5 * l


def iou_giou(a0, a1, b0, b1):
    """1-D IoU and generalised IoU of segments (a0, a1) and (b0, b1), broadcast"""
    inter = (torch.minimum(a1, b1) - torch.maximum(a0, b0)).clamp(min=0)
    union = (a1 - a0) + (b1 - b0) - inter
    hull = (torch.maximum(a1, b1) - torch.minimum(a0, b0)).clamp(min=0)
    iou = inter / (union + EPS)
    return iou, iou - (hull - union) / (hull + EPS)


def _pair_cost(logits, boxes, labels, tboxes, w_class, w_bbox, w_giou, alpha, gamma):
    """logits (..., Q, NC), boxes (..., Q, 2) against labels (G), tboxes (G, 2) -> (..., Q, G)"""
    p = logits.sigmoid()
    neg = (1 - alpha) * p ** gamma * (-(1 - p + 1e-8).log())
    pos = alpha * (1 - p) ** gamma * (-(p + 1e-8).log())
    cost_class = (pos - neg)[..., labels]
    l1 = (boxes[..., None, :] - tboxes).abs().sum(-1)
    x0, x1 = ends(boxes)
    t0, t1 = ends(tboxes)
    giou = iou_giou(x0[..., None], x1[..., None], t0, t1)[1]
    return w_bbox * l1 + w_class * cost_class + w_giou * (-giou)


def _proper(box):
    x0, x1 = ends(box)
    return bool((x1 >= x0).all())                                     # (False for a NaN as well)


def match_cost(logits, boxes, tgt_labels, tgt_boxes, w_class, w_bbox, w_giou, alpha, gamma):
    """logits (nl, B, Q, NC), boxes (nl, B, Q, 2), tgt_labels (G), tgt_boxes (G, 2) -> cost (nl, B, Q, G): every query priced against
    every target of the batch, and ok: no box with x1 < x0"""
    C = _pair_cost(logits, boxes, tgt_labels, tgt_boxes.to(logits.dtype), w_class, w_bbox, w_giou, alpha, gamma)
    return C, _proper(boxes) and _proper(tgt_boxes)


def match_cost_padded(logits, boxes, tgt_labels, tgt_boxes, gt_counts, w_class, w_bbox, w_giou, alpha, gamma):
    """tgt_labels (B, S), tgt_boxes (B, S, 2): every video owns S slots of which the first gt_counts[b] are real -> cost (nl, B, Q, S),
    the video's own block, 0 in the slots beyond the count; ok looks at the real slots and at the predictions of the videos that
    have one"""
    nl, B, Q, _ = logits.shape
    S = tgt_labels.shape[1]
    C = torch.zeros(nl, B, Q, S, dtype=logits.dtype)
    ok = True
    for b in range(B):
        n = min(int(gt_counts[b]), S)
        if n == 0:
            continue
        tb = tgt_boxes[b, :n].to(logits.dtype)
        C[:, b, :, :n] = _pair_cost(logits[:, b], boxes[:, b], tgt_labels[b, :n], tb, w_class, w_bbox, w_giou, alpha, gamma)
        ok = ok and _proper(boxes[:, b]) and _proper(tb)
    return C, ok


def criterion(logits, counts, boxes, matches, targets, gt_counts, ccr, num_boxes, alpha, gamma, beta, gau_mask, terms=False):
    """logits (nl, B, Q, NC), counts (nl, B, Wd), boxes (nl, B, Q, 2); matches: per layer (video, query, target row) int64 vectors of
    its matched pairs; targets: (labels (G), boxes (G, 2)); gt_counts (B) int64; ccr (Wd) the counter's class rate
    -> (nl, 6) in LOSS_KEYS order; terms=True: the same as nl lists of six scalars (a sum over SOME of them then leaves the others
    out of the graph, where a zero weight on the stacked table would send 0 * inf through the 0 / 0 of loss_self_iou)"""
    nl, B, Q, NC = logits.shape
    Wd = counts.shape[-1]
    dt = logits.dtype
    labels, tboxes = targets[0], targets[1].to(dt)
    rows = []
    for l in range(nl):
        vid, q, tg = matches[l]
        # focal loss on the one-hot of the matched targets' classes, "no object" elsewhere
        onehot = torch.zeros(B, Q, NC, dtype=dt)
        onehot[vid, q, labels[tg]] = 1
        x = logits[l]
        p = x.sigmoid()
        ce = F.binary_cross_entropy_with_logits(x, onehot, reduction="none")
        p_t = p * onehot + (1 - p) * (1 - onehot)
        focal = ce * (1 - p_t) ** gamma
        if alpha >= 0:
            focal = (alpha * onehot + (1 - alpha) * (1 - onehot)) * focal
        loss_ce = focal.sum() / num_boxes
        # counter: BCE on the one-hot of min(count, Wd - 1), the other bins damped by a gaussian (sigma = 2) around it
        tgt = gt_counts.clamp(max=Wd - 1)
        hot = F.one_hot(tgt, Wd).to(dt)
        coef = torch.ones(B, Wd, dtype=dt)
        if gau_mask:
            # (the damping is a constant fp32 table in the formulation this restates, whatever the type of the logits)
            bins = torch.arange(Wd, dtype=torch.float32)
            gauss = torch.exp(-(bins[None, :] - tgt[:, None].float()) ** 2 / 8)
            coef = hot + ((1 - gauss) ** beta).to(dt) * (1 - hot)
        bce = F.binary_cross_entropy_with_logits(counts[l], hot, reduction="none")
        loss_counter = (bce * (1 - ccr.to(dt)) * coef).mean()
        # matched boxes
        src, dst = boxes[l][vid, q], tboxes[tg]
        loss_bbox = (src - dst).abs().sum() / num_boxes
        s0, s1 = ends(src)
        d0, d1 = ends(dst)
        loss_giou = (1 - iou_giou(s0, s1, d0, d1)[1]).sum() / num_boxes
        # IoU among the matched predictions of one video: mean over its pairs (0 / 0 below two matches), summed over the videos
        iou = iou_giou(s0[:, None], s1[:, None], s0[None, :], s1[None, :])[0]
        n = vid.numel()
        upper = torch.ones(n, n, dtype=torch.bool).triu(1) & (vid[:, None] == vid[None, :])
        per_video = torch.zeros(B, dtype=dt).index_add(0, vid, (iou * upper).sum(1))
        cnt = torch.bincount(vid, minlength=B).to(dt)
        loss_self = (per_video / (0.5 * cnt * (cnt - 1))).sum()
        # cardinality: queries whose first maximal class is not the last one, against the count
        with torch.no_grad():
            card = ((x.argmax(-1) != NC - 1).sum(1).to(dt) - gt_counts.to(dt)).abs().mean()
        rows.append([loss_ce, loss_counter, loss_bbox, loss_giou, loss_self, card])
    return rows if terms else torch.stack([torch.stack(r) for r in rows])


def ce_rows(logits, target, weight):
    """logits (R, V), target (R) int64, weight (R) -> (weight (x[target] - logsumexp x), logsumexp x); a row of weight 0 is not
    read: both are 0 there whatever the row holds"""
    live = weight != 0
    x = torch.where(live[:, None], logits, torch.zeros_like(logits))
    lse = torch.logsumexp(x, -1)
    out = weight * (x.gather(1, target[:, None]).squeeze(1) - lse)
    return torch.where(live, out, torch.zeros_like(out)), torch.where(live, lse, torch.zeros_like(lse))


# ---------------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------------
def _crit(B, Q, NC, sizes, nl=2, Wd=11, alpha=0.25, gamma=2.0, beta=1.0, gau=1, plant=None):
    assert len(sizes) == B
    return dict(kind="crit", B=B, Q=Q, NC=NC, sizes=list(sizes), nl=nl, Wd=Wd, alpha=alpha, gamma=gamma, beta=beta, gau=gau, plant=plant)


def _cost(B, Q, NC, G, nl=2, w=(2.0, 0.0, 4.0), alpha=0.25, gamma=2.0, slots=4, counts=(0, 4, 6), amp=6.0, plant=True):
    return dict(kind="cost", B=B, Q=Q, NC=NC, G=G, nl=nl, w=w, alpha=alpha, gamma=gamma, slots=slots, counts=list(counts), amp=amp,
                plant=plant)


CASES = {
    # B Q NC around the 1024 threads of the one workgroup per layer; one thread with work
    "crit_threads_1023": _crit(1, 341, 3, [5], nl=1),
    "crit_threads_1024": _crit(1, 1024, 1, [4], nl=1),
    "crit_threads_1025": _crit(1, 205, 5, [3], nl=1),
    "crit_starved": _crit(1, 1, 1, [1], nl=1),                                # one pair: a single-match video
    "crit_lds_limit": _crit(16, 1536, 1, [2, 3] * 8, nl=1),                   # B Q = 24576: the whole on-chip class map
    # layer count, different matches per layer; the hyper-parameters
    "crit_layers1": _crit(3, 9, 3, [3, 2, 4], nl=1),
    "crit_layers3": _crit(3, 9, 3, [3, 2, 4], nl=3),
    "crit_g15_aneg_b05": _crit(3, 9, 3, [3, 2, 4], alpha=-1.0, gamma=1.5, beta=0.5),
    "crit_g1_gau0": _crit(3, 9, 3, [3, 2, 4], gamma=1.0, gau=0),
    "crit_g1_b2_wd2": _crit(3, 9, 3, [3, 2, 4], gamma=1.0, beta=2.0, Wd=2),   # every count >= Wd
    "crit_aneg_gau0_wd2": _crit(3, 9, 3, [3, 2, 4], alpha=-1.0, gau=0, Wd=2),
    "crit_g15_b2": _crit(3, 9, 3, [3, 2, 4], gamma=1.5, beta=2.0),
    # counter clamp: counts of 0, of Wd - 1 and above it (the video without an event has no match either)
    "crit_clamp_wd11": _crit(3, 13, 1, [0, 10, 12]),
    # cardinality: exact argmax ties, with the last class among them
    "crit_card_ties": _crit(2, 9, 3, [2, 3], plant="card"),
    # the tie subgradients, all in one batch, every video with >= 2 matches
    "crit_ties": _crit(3, 9, 3, [4, 3, 2], plant="ties"),
    # videos below two matches
    "crit_single_match": _crit(3, 9, 3, [2, 1, 3]),
    "crit_zero_match": _crit(3, 9, 3, [2, 0, 3]),
    "crit_no_pairs": _crit(2, 9, 3, [0, 0]),
    # matcher cost
    "cost_stride": _cost(8, 300, 1, 150, nl=3, slots=150, counts=(150, 0, 97, 151, 1, 150, 33, 400)),   # 1 080 000 entries, both forms
    "cost_nc3": _cost(3, 7, 3, 5),
    "cost_nc1_bbox_g1": _cost(3, 7, 1, 5, w=(2.0, 1.5, 4.0), gamma=1.0),
    "cost_noclass": _cost(3, 7, 3, 5, w=(0.0, 0.0, 4.0)),
    "cost_noclass_bbox_g15": _cost(3, 7, 3, 5, w=(0.0, 1.5, 4.0), gamma=1.5),
    "cost_g15": _cost(3, 7, 3, 5, gamma=1.5),
    "cost_g1": _cost(3, 7, 3, 5, gamma=1.0),
    "cost_range30": _cost(3, 7, 3, 5, amp=30.0),          # (1 - p) + 1e-8 is ill-conditioned in fp32: held to its own err32 alone
}
CE_VS = (1, 37, 255, 256, 257, 1000)                      # around the 256 threads of a row's workgroup
CE_PADS = (0, 3, 256)                                     # ld - V
for _V in CE_VS:
    for _pad in CE_PADS:
        CASES["ce_V%d_pad%d" % (_V, _pad)] = dict(kind="ce", V=_V, pad=_pad)

# the cases with a video below two matches: loss_self_iou is NaN there (0 / 0), on both sides, and nothing else is
SELF_IOU_NAN = ("crit_starved", "crit_clamp_wd11", "crit_single_match", "crit_zero_match", "crit_no_pairs")
SINGLE_MATCH = {"crit_starved": [0], "crit_single_match": [1]}             # case -> its videos with exactly one match
ZERO_MATCH = {"crit_clamp_wd11": [0], "crit_zero_match": [1], "crit_no_pairs": [0, 1]}
CLAMP = ("crit_g1_b2_wd2", "crit_aneg_gau0_wd2", "crit_clamp_wd11")        # a count >= Wd
PADDED = ("crit_layers3", "crit_g15_aneg_b05", "crit_ties", "crit_single_match", "crit_zero_match", "crit_clamp_wd11")

# crit_ties: (centre, length) of the matched predictions and their targets, pair by pair.  Ends: c -+ l / 2.
TIE_PAIRS = {
    # video 0
    "equal": ((0.5, 0.25), (0.5, 0.25)),                  # [0.375, 0.625] on itself
    "identical": ((0.5, 0.25), (0.75, 0.125)),            # the same prediction again (its own target lies apart)
    "touching": ((0.25, 0.25), (0.5, 0.25)),              # [0.125, 0.375] | [0.375, 0.625]: rb - lt == 0 (and it touches the two above)
    "disjoint": ((0.875, 0.125), (0.25, 0.125)),          # [0.8125, 0.9375] and [0.1875, 0.3125]
    # video 1
    "containing": ((0.5, 0.5), (0.5, 0.25)),              # [0.25, 0.75] around [0.375, 0.625]
    "contained": ((0.515625, 0.125), (0.5, 0.5)),         # [0.453125, 0.578125] inside [0.25, 0.75]
    "zero_length": ((0.25, 0.0), (0.25, 0.25)),           # a point inside its target, on the left end of `containing`
}
TIE_VIDEOS = (("equal", "identical", "touching", "disjoint"), ("containing", "contained", "zero_length"))
CARD_ROWS = {                                             # crit_card_ties: logits planted at (video 0, query i) of every layer
    0: (1.5, 1.5, -0.5),                                  # classes 0 and 1 tie: 0 wins, counted
    1: (-0.5, 1.5, 1.5),                                  # class 1 ties with the last class: 1 wins, counted
    2: (0.75, 0.75, 0.75),                                # all three: 0 wins, counted
    3: (1.5, -0.5, 1.5),                                  # class 0 ties with the last class: 0 wins, counted
    4: (-0.5, -0.5, 1.5),                                 # the last class alone: not counted
}


def _seed(name):
    return zlib.crc32(name.encode())                      # (fixed per name: adding a case moves no other)


def _dyadic(gen, shape, bits, lo, hi):
    """multiples of 2^-bits in [lo, hi)"""
    k = torch.randint(int(lo * 2 ** bits), int(hi * 2 ** bits), shape, generator=gen)
    return k.float() / 2 ** bits


def _crit_inputs(name, cfg):
    B, Q, NC, nl, Wd, sizes = cfg["B"], cfg["Q"], cfg["NC"], cfg["nl"], cfg["Wd"], cfg["sizes"]
    gen = torch.Generator().manual_seed(_seed(name))
    G = sum(sizes)
    logits = (torch.randn(nl, B, Q, NC, generator=gen) * 2).clamp(-6, 6)
    counts = torch.randn(nl, B, Wd, generator=gen)
    ties = cfg["plant"] == "ties"
    if ties:
        boxes = torch.stack([_dyadic(gen, (nl, B, Q), 6, 0.125, 0.875), _dyadic(gen, (nl, B, Q), 5, 0.0625, 0.5)], -1)
        tboxes = torch.stack([_dyadic(gen, (G,), 6, 0.25, 0.75), _dyadic(gen, (G,), 5, 0.125, 0.375)], -1)
    else:
        boxes = torch.stack([torch.rand(nl, B, Q, generator=gen), torch.rand(nl, B, Q, generator=gen) * 0.5 + 0.01], -1)
        tboxes = torch.stack([torch.rand(G, generator=gen) * 0.5 + 0.25, torch.rand(G, generator=gen) * 0.3 + 0.1], -1)
    tlabels = torch.randint(0, NC, (G,), generator=gen)
    n1 = [min(Q, n) for n in sizes]                       # matches of a video: as many as it has events
    T1 = sum(n1)
    vid = torch.tensor([v for v, n in enumerate(n1) for _ in range(n)], dtype=torch.int64)
    base = [sum(sizes[:v]) for v in range(B)]
    tbase = torch.tensor([base[v] for v, n in enumerate(n1) for _ in range(n)], dtype=torch.int64)
    ent_start = torch.tensor([sum(n1[:v]) for v in range(B + 1)], dtype=torch.int64)
    mq = torch.zeros(nl, T1, dtype=torch.int64)
    mt = torch.zeros(nl, T1, dtype=torch.int64)
    for l in range(nl):                                   # a matching of its own per layer: distinct queries, a permutation of the targets
        for v in range(B):
            a, n = int(ent_start[v]), n1[v]
            if ties and l > 0:                            # (the planted targets are shared by the layers: one matching for all)
                mq[l, a:a + n], mt[l, a:a + n] = mq[0, a:a + n], mt[0, a:a + n]
                continue
            mq[l, a:a + n] = torch.randperm(Q, generator=gen)[:n]
            mt[l, a:a + n] = torch.randperm(sizes[v], generator=gen)[:n]
    roles = {}
    if ties:
        for v, names in enumerate(TIE_VIDEOS):
            for j, role in enumerate(names):
                e = int(ent_start[v]) + j
                roles[role] = e
                tboxes[int(tbase[e] + mt[0, e])] = torch.tensor(TIE_PAIRS[role][1])
                for l in range(nl):
                    boxes[l, v, mq[l, e]] = torch.tensor(TIE_PAIRS[role][0])
    if cfg["plant"] == "card":
        for q, row in CARD_ROWS.items():
            logits[:, 0, q] = torch.tensor(row)
    ccr = torch.rand(Wd, generator=gen) * 0.5
    gl = 0.5 + 0.125 * torch.arange(nl * 6, dtype=torch.float32).view(nl, 6)         # a distinct weight per (layer, term)
    if name in SELF_IOU_NAN:
        gl[:, 4] = 0.0                                    # selected away, as the train step does for an unweighted term
    return dict(kind="crit", logits=logits, counts=counts, boxes=boxes, tlabels=tlabels, tboxes=tboxes, mq=mq, mt=mt, vid=vid,
                tbase=tbase, ent_start=ent_start, gt_counts=torch.tensor(sizes, dtype=torch.int64), ccr=ccr, gl=gl,
                num_boxes=float(max(G, 1)), roles=roles, **{k: cfg[k] for k in ("B", "Q", "NC", "nl", "Wd", "sizes", "alpha", "gamma",
                                                                               "beta", "gau")})


def padded_layout(i, slots):
    """the problem of a criterion case laid out in `slots` target slots and G1 = min(Q, slots) pair slots per video: the unused
    target slots hold other labels and boxes, the unused pair slots in-range but wrong indices -> the arguments of the padded form"""
    B, Q, nl, sizes = i["B"], i["Q"], i["nl"], i["sizes"]
    assert slots >= max(sizes)
    gen = torch.Generator().manual_seed(_seed("padded") + slots)
    G1 = min(Q, slots)
    tlabels = torch.randint(0, i["NC"], (B, slots), generator=gen)
    tboxes = torch.stack([torch.rand(B, slots, generator=gen), torch.rand(B, slots, generator=gen) * 0.5], -1)
    mq = torch.randint(0, Q, (nl, B, G1), generator=gen)
    mt = torch.randint(0, slots, (nl, B, G1), generator=gen)
    for v, n in enumerate(sizes):
        a, first = int(i["ent_start"][v]), sum(sizes[:v])
        tlabels[v, :n], tboxes[v, :n] = i["tlabels"][first:first + n], i["tboxes"][first:first + n]
        m = min(Q, n)
        mq[:, v, :m], mt[:, v, :m] = i["mq"][:, a:a + m], i["mt"][:, a:a + m]
    vid = torch.arange(B, dtype=torch.int64).repeat_interleave(G1)
    return dict(tlabels=tlabels.reshape(-1), tboxes=tboxes.reshape(-1, 2), mq=mq.reshape(nl, B * G1), mt=mt.reshape(nl, B * G1),
                vid=vid, tbase=vid * slots, ent_start=torch.arange(B + 1, dtype=torch.int64) * G1,
                pair_count=torch.tensor([min(Q, n) for n in sizes], dtype=torch.int64),
                num_boxes_dev=torch.tensor([i["num_boxes"]], dtype=torch.float32))


COST_BOXES = {                                            # planted at (video 0, query i) of every layer, against target 0 = (0.5, 0.25)
    0: (0.5, 0.25),                                       # identical
    1: (0.25, 0.25),                                      # touching
    2: (0.875, 0.125),                                    # disjoint
    3: (0.5, 0.0),                                        # zero length
}


def _cost_inputs(name, cfg):
    B, Q, NC, G, nl, S = cfg["B"], cfg["Q"], cfg["NC"], cfg["G"], cfg["nl"], cfg["slots"]
    gen = torch.Generator().manual_seed(_seed(name))
    amp = cfg["amp"]
    logits = (torch.randn(nl, B, Q, NC, generator=gen) * (amp / 3)).clamp(-amp, amp)
    if amp > 6:
        logits[0, 0, 0, 0], logits[0, 0, 1, 0] = amp, -amp
    boxes = torch.stack([torch.rand(nl, B, Q, generator=gen), torch.rand(nl, B, Q, generator=gen) * 0.5 + 0.01], -1)
    tboxes = torch.stack([torch.rand(G, generator=gen) * 0.5 + 0.25, torch.rand(G, generator=gen) * 0.3 + 0.1], -1)
    tlabels = torch.arange(G, dtype=torch.int64) % NC     # labels over all classes
    tlabels = tlabels[torch.randperm(G, generator=gen)]
    plabels = torch.randint(0, NC, (B, S), generator=gen)
    plabels[1, :min(S, NC)] = torch.arange(min(S, NC))
    pboxes = torch.stack([torch.rand(B, S, generator=gen) * 0.5 + 0.25, torch.rand(B, S, generator=gen) * 0.3 + 0.1], -1)
    if cfg["plant"] and Q >= len(COST_BOXES):
        tboxes[0] = torch.tensor(COST_BOXES[0])
        pboxes[:, 0] = torch.tensor(COST_BOXES[0])
        for q, b in COST_BOXES.items():
            boxes[:, :, q] = torch.tensor(b)
    return dict(kind="cost", logits=logits, boxes=boxes, tlabels=tlabels, tboxes=tboxes, plabels=plabels, pboxes=pboxes,
                pcounts=torch.tensor(cfg["counts"], dtype=torch.int64), **{k: cfg[k] for k in ("B", "Q", "NC", "G", "nl", "w", "alpha",
                                                                                             "gamma", "slots", "amp")})


CE_ROWS = ("plain", "plain", "plain", "constant", "target_max", "target_min", "peak", "peak_target", "masked_nan", "masked_inf",
           "plain", "masked_plain")
CE_GROUPS = {"plain": ("plain", "constant", "target_max", "target_min"), "peak": ("peak", "peak_target")}


def _ce_inputs(name, cfg):
    V = cfg["V"]
    gen = torch.Generator().manual_seed(_seed("ce_V%d" % V))          # the same rows at every leading dimension
    R = len(CE_ROWS)
    x = torch.randn(R, V, generator=gen) * 3
    target = torch.randint(0, V, (R,), generator=gen)
    weight = torch.rand(R, generator=gen) + 0.5
    for r, kind in enumerate(CE_ROWS):
        if kind == "constant":
            x[r] = 1.25
        elif kind == "target_max":
            target[r] = int(x[r].argmax())
        elif kind == "target_min":
            target[r] = int(x[r].argmin())
        elif kind.startswith("peak"):                     # one logit 80 above the rest
            k = int(torch.randint(0, V, (1,), generator=gen))
            x[r, k] = x[r].max() + 80.0
            if kind == "peak_target":
                target[r] = k
        elif kind.startswith("masked"):
            weight[r] = 0.0
            if kind == "masked_nan":
                x[r] = float("nan")
            elif kind == "masked_inf":
                x[r, ::2], x[r, 1::2] = float("inf"), float("-inf")
    g = torch.randn(R, generator=gen)
    return dict(kind="ce", x=x, target=target, weight=weight, g=g, V=V, pad=cfg["pad"], R=R)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """fp32 / int64 CPU tensors of a case: never modified"""
    cfg = CASES[name]
    return {"crit": _crit_inputs, "cost": _cost_inputs, "ce": _ce_inputs}[cfg["kind"]](name, cfg)


def matches_of(i):
    return [(i["vid"], i["mq"][l], i["tbase"] + i["mt"][l]) for l in range(i["nl"])]


def evaluate_criterion(i, dt, gl=None):
    """the table and the gradients of sum(gl * table) in type dt; the terms whose weight is exactly 0 are LEFT OUT of the sum (never
    multiplied by 0: loss_self_iou is 0 / 0 below two matches), and so is the cardinality error, which has no gradient"""
    gl = i["gl"] if gl is None else gl
    leaves = [i[k].to(dt, copy=True).requires_grad_() for k in ("logits", "counts", "boxes")]
    rows = criterion(*leaves, matches_of(i), (i["tlabels"], i["tboxes"]), i["gt_counts"], i["ccr"], i["num_boxes"], i["alpha"],
                     i["gamma"], i["beta"], i["gau"], terms=True)
    total = sum(rows[l][k] * float(gl[l, k]) for l in range(i["nl"]) for k in range(5) if float(gl[l, k]) != 0.0)
    grads = torch.autograd.grad(total, leaves)
    out = {k: torch.stack([r[j].detach() for r in rows]) for j, k in enumerate(LOSS_KEYS)}
    out.update(d_logits=grads[0], d_counts=grads[1], d_boxes=grads[2])
    return out


def evaluate_cost(i, dt, padded=False):
    w = i["w"]
    lg, bx = i["logits"].to(dt), i["boxes"].to(dt)
    if padded:
        return match_cost_padded(lg, bx, i["plabels"], i["pboxes"], i["pcounts"], w[0], w[1], w[2], i["alpha"], i["gamma"])
    return match_cost(lg, bx, i["tlabels"], i["tboxes"], w[0], w[1], w[2], i["alpha"], i["gamma"])


def evaluate_ce(i, dt):
    x = i["x"].to(dt, copy=True).requires_grad_()
    out, lse = ce_rows(x, i["target"], i["weight"].to(dt))
    dx, = torch.autograd.grad((out * i["g"].to(dt)).sum(), x)
    return dict(out=out.detach(), lse=lse.detach(), dx=dx)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(fp64, fp32) evaluations of the case's restatement: never modified.  crit: the six loss columns and d_logits, d_counts,
    d_boxes; cost: cost, ok, cost_padded, ok_padded; ce: out, lse, dx"""
    i = inputs(name)
    both = []
    for dt in (torch.float64, torch.float32):
        if i["kind"] == "crit":
            both.append(evaluate_criterion(i, dt))
        elif i["kind"] == "cost":
            c, ok = evaluate_cost(i, dt)
            cp, okp = evaluate_cost(i, dt, padded=True)
            both.append(dict(cost=c, ok=ok, cost_padded=cp, ok_padded=okp))
        else:
            both.append(evaluate_ce(i, dt))
    return tuple(both)

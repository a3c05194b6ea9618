"""The matcher-cost, set-criterion and vocabulary-loss kernels of gvl_amd/csrc/gvl_criterion.hip (k_match_cost, k_match_cost_padded,
k_criterion_fwd, k_criterion_bwd, k_ce_rows_fwd, k_ce_rows_bwd) called ALONE -- tests/test_gpu_criterion.py compares them with the
fp32 PyTorch op sequence at one shape family and on whatever matching the solver returns -- against the fp64 evaluation of their
restatement in tests/criterion_ref.py, on hand-made matchings, at the edges of their launch shapes and of their arithmetic.

The entry points are the kernels' own: gvl_set_criterion_forward_f32 / _backward_f32 through _lib.lib() on the test's buffers (every
output pre-filled with NaN, so an element left unwritten is seen; null pointers for an empty match or target array) and, bit for
bit the same, through SetCriterionFunction.apply; gvl_match_cost_f32 and gvl_match_cost_padded_f32; gvl_ce_rows_forward_f32 /
_backward_f32 on a buffer with its own leading dimension and, bit for bit the same, through MSDA.ce_rows_forward / ce_rows_backward_.
The matches are built by hand (mq, mt, vid, tbase, ent_start; pair_count and num_boxes_dev in the padded form) and grad_losses is a
distinct value per (layer, term), so a mixed-up layer or term shows.  tests/test_criterion_ref_cpu.py checks, without a GPU, what
the comparisons rest on: that the restatement is the project's PyTorch formulation in fp64, and that every case has the property
it is named for.

Tolerance, per case and output (each loss term is an output of its own):
    max(FACTOR * err32, 16 * 2**-23 * scale),   FACTOR = 8,
err32 being the deviation of the SAME restatement evaluated in fp32 torch on the CPU and scale the largest magnitude of the fp64
result (the bound of tests/test_gpu_cap_train_ops.py and tests/test_gpu_mha_train_ops.py).  NaN counts as equal only for
loss_self_iou in the cases of criterion_ref.SELF_IOU_NAN (a video below two matches: 0 / 0 on both sides); nothing else is excluded.
The vocabulary rows are held in two groups, `plain` and `peak` (a logit 80 above the rest), each on its own scale: one row with a
logsumexp of 90 would otherwise loosen the floor of all the others.  k_ce_rows_* meets this bound as it stands, fast exp / log
intrinsics included: no extra term is taken.

Every comparison prints "RATIO <case>/<output> <kernel error / bound>" before it asserts (pytest -s).  Measured on the MI355X
(nan: loss_self_iou where it is NaN on both sides):

    case                               ce  counter     bbox     giou self_iou     card d_logits d_counts  d_boxes
    crit_aneg_gau0_wd2              0.018    0.022    0.011    0.019    0.124    0.011    0.065    0.033    0.125
    crit_card_ties                  0.021    0.029    0.015    0.038    0.082    0.000    0.091    0.041    0.071
    crit_clamp_wd11                 0.001    0.017    0.028    0.039      nan    0.011    0.068    0.074    0.131
    crit_g15_aneg_b05               0.039    0.047    0.005    0.025    0.079    0.007    0.086    0.051    0.132
    crit_g15_b2                     0.031    0.032    0.036    0.026    0.033    0.000    0.125    0.046    0.101
    crit_g1_b2_wd2                  0.012    0.031    0.013    0.044    0.093    0.010    0.076    0.064    0.108
    crit_g1_gau0                    0.046    0.008    0.018    0.011    0.015    0.014    0.071    0.056    0.085
    crit_layers1                    0.034    0.012    0.038    0.030    0.033    0.018    0.100    0.037    0.024
    crit_layers3                    0.022    0.017    0.042    0.042    0.083    0.011    0.104    0.037    0.056
    crit_lds_limit                  0.003    0.028    0.021    0.032    0.007    0.000    0.110    0.050    0.077
    crit_no_pairs                   0.013    0.009    0.000    0.000      nan    0.000    0.074    0.030    0.000
    crit_single_match               0.050    0.033    0.013    0.027      nan    0.008    0.081    0.063    0.027
    crit_starved                    0.088    0.053    0.000    0.007      nan    0.000    0.065    0.038    0.021
    crit_threads_1023               0.020    0.014    0.022    0.009    0.009    0.000    0.125    0.038    0.053
    crit_threads_1024               0.055    0.006    0.022    0.006    0.125    0.000    0.126    0.042    0.056
    crit_threads_1025               0.049    0.000    0.004    0.024    0.125    0.000    0.158    0.043    0.098
    crit_ties                       0.043    0.024    0.024    0.028    0.028    0.000    0.125    0.053    0.068
    crit_zero_match                 0.029    0.013    0.018    0.043      nan    0.016    0.119    0.046    0.038
    crit_layers3[padded]            0.022    0.017    0.042    0.042    0.083    0.011    0.104    0.037    0.056
    crit_g15_aneg_b05[padded]       0.039    0.047    0.005    0.025    0.079    0.007    0.086    0.051    0.132
    crit_ties[padded]               0.043    0.024    0.024    0.028    0.028    0.000    0.125    0.053    0.068
    crit_single_match[padded]       0.050    0.033    0.013    0.027      nan    0.008    0.081    0.063    0.027
    crit_zero_match[padded]         0.029    0.013    0.018    0.043      nan    0.016    0.119    0.046    0.038
    crit_clamp_wd11[padded]         0.001    0.017    0.028    0.039      nan    0.011    0.068    0.074    0.131

    case                             list   padded
    cost_g1                         0.125    0.125
    cost_g15                        0.142    0.141
    cost_nc1_bbox_g1                0.125    0.125
    cost_nc3                        0.129    0.129
    cost_noclass                    0.071    0.049
    cost_noclass_bbox_g15           0.110    0.082
    cost_range30                    0.125    0.125
    cost_stride                     0.125    0.125
      its first row                 0.075    0.101
      its last row                  0.125    0.118

    case (any pad)                out[plain]  lse[plain]   dx[plain]   out[peak]   lse[peak]    dx[peak]
    ce_V1000                           0.015       0.025       0.066       0.004       0.000       0.013
    ce_V1                              0.000       0.000       0.000       0.000       0.000       0.000
    ce_V255                            0.027       0.026       0.105       0.008       0.000       0.007
    ce_V256                            0.013       0.017       0.025       0.008       0.000       0.003
    ce_V257                            0.026       0.021       0.043       0.004       0.000       0.017
    ce_V37                             0.013       0.013       0.055       0.019       0.000       0.006

Nothing is above one half; the largest figure is 0.158 (crit_threads_1025 d_logits).  cost_range30 (logits up to +-30, where
(1 - p) + 1e-8 is ill-conditioned in fp32 for the formula itself) is held to its own err32 alone, 0.125 of 8 err32.

What the tests found.  The padded form did not return the bits of the compact one: k_criterion_fwd summed loss_bbox and loss_giou
pair by pair over the threads, and the padded layout puts the pairs on other lanes of the butterfly sum -- the two terms
differed by one or two ulp (up to 6e-8 on 1.1) in four of the six padded cases (crit_layers3, crit_g15_aneg_b05, crit_single_match, crit_clamp_wd11).  The kernel
now sums them video by video in pair order, thread v for video v in both layouts, as it already did for loss_self_iou; all six
are equal bit for bit.  Nothing else failed.

Seeded errors (each applied alone to a scratch copy of gvl_criterion.hip built into a scratch library, values only; the tests of
this file that then fail, and whether tests/test_gpu_criterion.py alone fails):
  1 tie weight 0.5 -> 1 in iou_grad: 2 -- test_criterion_forward_and_backward[crit_ties], test_padded_form[crit_ties]; old file: no
  2 d >= 0 -> d > 0 in iou_grad and the GIoU backward: the same 2; old file: no
  3 the d_u term dropped from g1 / g0: 27 -- every criterion test with a matched pair; old file: yes (6)
  4 counter_coef ignoring beta: 4 -- the cases with beta = 0.5 and beta = 2 under the gaussian mask (crit_g15_aneg_b05 in both
    forms, crit_g15_b2, crit_g1_b2_wd2); old file: no
  5 the sign of dmod in the gamma == 1 branch: 2 -- crit_g1_gau0, crit_g1_b2_wd2; old file: no
  6 the self-IoU normaliser without its 0.5 (forward and backward): 16 -- every criterion test whose videos all have two matches;
    old file: yes (4)
  7 alpha < 0 treated as alpha = 0: 3 -- crit_aneg_gau0_wd2, crit_g15_aneg_b05 in both forms; old file: no
  8 ce_block_max_sum merging without the rescale: 15 -- test_ce_rows at every V > 1; old file: yes (3)
  9 k_match_cost_padded reading tgt_boxes[g] for [b G + g]: 8 -- test_match_cost[*-padded] but cost_range30 (whose own bound, 8 err32,
    is 19 on a scale of 30), test_degenerate_box_flag[padded]; old file: no
"""
import functools

import pytest
import torch

import criterion_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FACTOR = 8.0               # kernel error allowed per fp32-restatement error (module docstring)
FLOOR = 16 * 2.0 ** -23    # ... and never less than 16 ulp of the tensor's largest entry
NAN = float("nan")
GRADS = ("d_logits", "d_counts", "d_boxes")

CRIT = sorted(n for n, c in R.CASES.items() if c["kind"] == "crit")
COST = sorted(n for n, c in R.CASES.items() if c["kind"] == "cost")
CE = sorted(n for n, c in R.CASES.items() if c["kind"] == "ce")


# ---------------------------------------------------------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------------------------------------------------------
def ratio(label, got, want64, want32):
    """kernel error / bound of one output, printed; want32 is the fp32 evaluation of the same restatement"""
    got, want64, want32 = got.detach().cpu().double(), want64.double(), want32.double()
    assert got.shape == want64.shape, (label, got.shape, want64.shape)
    assert bool(torch.isfinite(got).all()), label + ": not finite"
    err32 = float((want32 - want64).abs().max()) if got.numel() else 0.0
    scale = float(want64.abs().max()) if got.numel() else 0.0
    bound = max(FACTOR * err32, FLOOR * scale)
    err = float((got - want64).abs().max()) if got.numel() else 0.0
    r = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
    print("RATIO %-44s %.3f   (error %.3g, fp32 restatement %.3g, scale %.3g)" % (label, r, err, err32, scale))
    return r


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def nans(*shape):
    return torch.full(shape, NAN, device=DEV)


def _ptr(t):
    return None if t is None or t.numel() == 0 else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def device_inputs(name):
    """the case's tensors on the device: never modified"""
    return {k: v.to(DEV) for k, v in R.inputs(name).items() if isinstance(v, torch.Tensor)}


# ---------------------------------------------------------------------------------------------------------------------------
# criterion: running the kernels
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def match_args(name, padded):
    """mq, mt, vid, tbase, ent_start, tlabels, tboxes and, in the padded form, pair_count and num_boxes_dev, on the device"""
    i, d = R.inputs(name), device_inputs(name)
    if not padded:
        return dict({k: d[k] for k in ("mq", "mt", "vid", "tbase", "ent_start", "tlabels", "tboxes")}, pair_count=None,
                    num_boxes_dev=None, num_boxes=i["num_boxes"])
    p = R.padded_layout(i, max(i["sizes"]) + 1)
    return dict({k: v.to(DEV) for k, v in p.items()}, num_boxes=12345.0)          # (the scalar must not be read)


def _crit_call(fn, i, d, m, *rest):
    return fn(d["logits"].data_ptr(), d["counts"].data_ptr(), d["boxes"].data_ptr(), _ptr(m["mq"]), _ptr(m["mt"]), _ptr(m["vid"]),
              _ptr(m["tbase"]), m["ent_start"].data_ptr(), _ptr(m["tlabels"]), _ptr(m["tboxes"]), d["gt_counts"].data_ptr(),
              d["ccr"].data_ptr(), i["nl"], i["B"], i["Q"], i["NC"], i["Wd"], m["mq"].shape[1], m["tlabels"].shape[0], m["num_boxes"],
              i["alpha"], i["gamma"], i["beta"], i["gau"], _ptr(m["pair_count"]), _ptr(m["num_boxes_dev"]), *rest, _stream())


def run_c(name, padded=False):
    """forward and backward through the C entry points on this function's own buffers, every output pre-filled with NaN; an empty
    match or target array is passed as a null pointer"""
    from gvl_amd import _lib
    i, d, m = R.inputs(name), device_inputs(name), match_args(name, padded)
    gl = d["gl"].contiguous()
    table = nans(i["nl"], 6)
    grads = [nans(*d[k].shape) for k in ("logits", "counts", "boxes")]
    before = [d[k].clone() for k in ("logits", "counts", "boxes")]
    lib = _lib.lib()
    with torch.cuda.device(DEV):
        _lib.check(_crit_call(lib.gvl_set_criterion_forward_f32, i, d, m, table.data_ptr()), "set_criterion_forward")
        _lib.check(_crit_call(lib.gvl_set_criterion_backward_f32, i, d, m, gl.data_ptr(), *[g.data_ptr() for g in grads]),
                   "set_criterion_backward")
    torch.cuda.synchronize()
    for k, b in zip(("logits", "counts", "boxes"), before):
        assert bits_equal(d[k], b), k
    return dict(table=table, d_logits=grads[0], d_counts=grads[1], d_boxes=grads[2])


def run_fn(name, padded=False):
    """the same through SetCriterionFunction.apply and autograd"""
    from gvl_amd.criterion import SetCriterionFunction
    i, d, m = R.inputs(name), device_inputs(name), match_args(name, padded)
    leaves = [d[k].clone().requires_grad_() for k in ("logits", "counts", "boxes")]
    table = SetCriterionFunction.apply(*leaves, m["mq"], m["mt"], m["vid"], m["tbase"], m["ent_start"], m["tlabels"], m["tboxes"],
                                       d["gt_counts"], d["ccr"], m["num_boxes"], i["alpha"], i["gamma"], i["beta"], i["gau"],
                                       m["pair_count"], m["num_boxes_dev"])
    grads = torch.autograd.grad(table, leaves, d["gl"])
    torch.cuda.synchronize()
    return dict(table=table.detach(), d_logits=grads[0], d_counts=grads[1], d_boxes=grads[2])


def check_crit(name, got, label=None):
    """the six loss terms, each on its own scale, and the three gradients, against the fp64 reference"""
    i = R.inputs(name)
    w64, w32 = R.reference(name)
    label = label or name
    rs = {}
    for j, k in enumerate(R.LOSS_KEYS):
        col = got["table"][:, j]
        if k == "loss_self_iou" and name in R.SELF_IOU_NAN:              # 0 / 0 on both sides, the only NaN anywhere
            assert bool(torch.isnan(col).all()) and bool(torch.isnan(w64[k]).all()) and bool(torch.isnan(w32[k]).all()), label
            continue
        rs[k] = ratio(f"{label}/{k}", col, w64[k], w32[k])
    for k in GRADS:
        rs[k] = ratio(f"{label}/{k}", got[k], w64[k], w32[k])
    assert max(rs.values()) <= 1.0, {k: round(v, 3) for k, v in rs.items() if v > 1.0}
    unmatched = torch.ones(i["nl"], i["B"], i["Q"], dtype=torch.bool)
    for l in range(i["nl"]):
        unmatched[l, i["vid"], i["mq"][l]] = False
    if bool(unmatched.any()):                                          # unmatched queries get exactly 0
        assert float(got["d_boxes"].cpu()[unmatched].abs().max()) == 0.0, label


def same_bits(a, b, what):
    for k in ("table",) + GRADS:
        x, y = a[k], b[k]
        if k == "table":                                               # (NaN is not one bit pattern)
            assert torch.equal(torch.isnan(x), torch.isnan(y)), (what, k)
            x, y = torch.nan_to_num(x, nan=0.0), torch.nan_to_num(y, nan=0.0)
        assert bits_equal(x, y), (what, k)


# ---------------------------------------------------------------------------------------------------------------------------
# criterion: the cases
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CRIT)
def test_criterion_forward_and_backward(name):
    """every case of the table (tests/criterion_ref.py: thread-count edges, the whole on-chip class map, 1 and 3 layers with their own
    matches, the hyper-parameters, the counter clamp, argmax ties, the tie subgradients, videos with one and with no match, a batch
    without a pair and with null match pointers) through the C entry points, and bit for bit the same through
    SetCriterionFunction.apply"""
    got = run_c(name)
    check_crit(name, got)
    same_bits(run_fn(name), got, name)


@pytest.mark.parametrize("name", R.SELF_IOU_NAN)
def test_below_two_matches_only_loss_self_iou_is_nan(name):
    """loss_self_iou is NaN (checked against the reference in check_crit) and everything else finite: with grad_losses[:, 4] = 0
    the three gradients are the reference's gradient of the other terms, self-IoU left out of the sum -- not 0 * NaN"""
    got = run_c(name)
    assert float(R.inputs(name)["gl"][:, 4].abs().max()) == 0.0
    keep = [j for j in range(6) if j != 4]
    assert bool(torch.isfinite(got["table"][:, keep]).all()) and bool(torch.isnan(got["table"][:, 4]).all())
    for k in GRADS:
        assert bool(torch.isfinite(got[k]).all()), k
    check_crit(name, got)


@pytest.mark.parametrize("name", R.PADDED)
def test_padded_form(name):
    """the same problems laid out in slots (one more than the largest video needs, so every video has unused ones; crit_zero_match
    and crit_clamp_wd11 have a video whose slots are all empty), in-range but wrong indices in the unused pair slots, other labels
    and boxes in the unused target slots, num_boxes from device memory (the scalar argument is 12345): equal to the reference, and
    to the compact form of the same kernels bit for bit"""
    got = run_c(name, padded=True)
    check_crit(name, got, label=name + "[padded]")
    same_bits(got, run_c(name), name)
    same_bits(run_fn(name, padded=True), got, name)


@pytest.mark.parametrize("name", ["crit_layers3", "crit_ties", "crit_lds_limit"])
def test_criterion_repeatability(name):
    same_bits(run_c(name), run_c(name), name)


@pytest.mark.parametrize("entry", ["forward", "backward"])
def test_one_row_beyond_the_class_map_is_refused_without_a_launch(entry):
    """B Q = 24577: the library's error, nothing written (sizes only: the check precedes any access, the buffers are tiny)"""
    from gvl_amd import _lib
    name = "crit_starved"
    i, d, m = dict(R.inputs(name)), device_inputs(name), match_args(name, False)
    i["Q"] = 24577
    table, grads = nans(1, 6), [nans(4), nans(4), nans(4)]
    lib = _lib.lib()
    with torch.cuda.device(DEV):
        if entry == "forward":
            rc = _crit_call(lib.gvl_set_criterion_forward_f32, i, d, m, table.data_ptr())
        else:
            rc = _crit_call(lib.gvl_set_criterion_backward_f32, i, d, m, d["gl"].data_ptr(), *[g.data_ptr() for g in grads])
    assert rc != 0
    with pytest.raises(RuntimeError, match="exceeds the on-chip class map"):
        _lib.check(rc, "set_criterion_" + entry)
    torch.cuda.synchronize()
    for t in [table] + grads:
        assert bool(torch.isnan(t).all())


# ---------------------------------------------------------------------------------------------------------------------------
# matcher cost
# ---------------------------------------------------------------------------------------------------------------------------
def run_cost(name, padded, boxes=None, tboxes=None, sizes=None):
    """-> (cost, ok, rc): the cost buffer pre-filled with NaN, ok preset to 1.  boxes / tboxes replace the case's; sizes = (B, G) the
    sizes passed (the buffers stay the case's)"""
    from gvl_amd import _lib
    i, d = R.inputs(name), device_inputs(name)
    nl, B, Q, NC = i["nl"], i["B"], i["Q"], i["NC"]
    G = i["slots"] if padded else i["G"]
    cost = nans(nl, B, Q, G)
    ok = torch.ones(1, dtype=torch.int32, device=DEV)
    boxes = d["boxes"] if boxes is None else boxes.to(DEV)
    tb = (d["pboxes"] if padded else d["tboxes"]) if tboxes is None else tboxes.to(DEV)
    if sizes is not None:
        B, G = sizes
    w = i["w"]
    lib = _lib.lib()
    with torch.cuda.device(DEV):
        if padded:
            rc = lib.gvl_match_cost_padded_f32(d["logits"].data_ptr(), boxes.data_ptr(), d["plabels"].data_ptr(), tb.data_ptr(),
                                               d["pcounts"].data_ptr(), nl, B, Q, NC, G, w[0], w[1], w[2], i["alpha"], i["gamma"],
                                               cost.data_ptr(), ok.data_ptr(), _stream())
        else:
            rc = lib.gvl_match_cost_f32(d["logits"].data_ptr(), boxes.data_ptr(), d["tlabels"].data_ptr(), tb.data_ptr(), nl, B, Q, NC, G,
                                        w[0], w[1], w[2], i["alpha"], i["gamma"], cost.data_ptr(), ok.data_ptr(), _stream())
    torch.cuda.synchronize()
    return cost, int(ok), rc


@pytest.mark.parametrize("padded", [False, True], ids=["list", "padded"])
@pytest.mark.parametrize("name", COST)
def test_match_cost(name, padded):
    """cost_stride: 1 080 000 entries in both forms, the grid-stride loop runs a second time (its first and last rows also
    on their own); NC in {1, 3} with labels over all classes; w_bbox in {0, 1.5}; w_class = 0, where the GIoU and L1 terms meet the
    floor alone; gamma in {2, 1, 1.5}; identical, touching, disjoint and zero-length boxes; padded counts of 0, of `slots` and above;
    logits within +-6, and cost_range30 up to +-30"""
    i = R.inputs(name)
    w64, w32 = R.reference(name)
    key, label = ("cost_padded", name + "[padded]") if padded else ("cost", name)
    cost, ok, rc = run_cost(name, padded)
    assert rc == 0 and ok == 1 and w64["ok_padded" if padded else "ok"]
    rs = [ratio(f"{label}/cost", cost, w64[key], w32[key])]
    if name == "cost_stride":
        for part, sl in (("first", (0, 0, 0)), ("last", (-1, -1, -1))):
            rs.append(ratio(f"{label}/cost[{part}]", cost[sl], w64[key][sl], w32[key][sl]))
    assert max(rs) <= 1.0, rs
    if padded:                                                         # exactly 0 in the slots beyond the count
        for b, n in enumerate(i["pcounts"].tolist()):
            if n < i["slots"]:
                assert float(cost[:, b, :, n:].abs().max()) == 0.0, b


@pytest.mark.parametrize("padded", [False, True], ids=["list", "padded"])
def test_match_cost_of_an_empty_problem_writes_nothing(padded):
    for sizes in ((3, 0), (0, 4)):                                     # G = 0 (slots = 0), B = 0
        cost, ok, rc = run_cost("cost_nc3", padded, sizes=sizes)
        assert rc == 0 and ok == 1 and bool(torch.isnan(cost).all()), sizes


@pytest.mark.parametrize("padded", [False, True], ids=["list", "padded"])
def test_degenerate_box_flag(padded):
    """the flag falls for a negative length (of a prediction, of a target) and for a NaN box, and for nothing else: not for a zero
    length, and in the padded form not for a box in an unused target slot.  The entries that do not involve the planted box are bit
    for bit those of the untouched call."""
    name = "cost_nc3"
    i = R.inputs(name)
    clean, ok, _ = run_cost(name, padded)
    assert ok == 1
    l, b, q, g = 1, 2, 5, 3
    assert not padded or i["pcounts"][b] > g
    for what, value, want in (("prediction", -0.25, 0), ("target", -0.125, 0), ("prediction", NAN, 0), ("prediction", 0.0, 1),
                              ("target", 0.0, 1), ("unused", -0.125, 1)):
        boxes = i["boxes"].clone()
        tboxes = (i["pboxes"] if padded else i["tboxes"]).clone()
        if what == "prediction":
            boxes[l, b, q, 1] = value
        elif what == "target":
            tboxes[(b, g, 1) if padded else (g, 1)] = value
        elif padded:                                                   # a slot of video 0, which has no event
            assert i["pcounts"][0] == 0
            tboxes[0, 0, 1] = value
        else:
            continue
        cost, ok, rc = run_cost(name, padded, boxes=boxes, tboxes=tboxes)
        assert rc == 0 and ok == want, (what, value, ok)
        touched = torch.zeros_like(clean, dtype=torch.bool)
        if what == "unused":
            assert bits_equal(cost, clean)
            continue
        if what == "prediction":
            touched[l, b, q] = True
        elif padded:
            touched[:, b, :, g] = True
        else:
            touched[..., g] = True
        assert bits_equal(cost[~touched], clean[~touched]), (what, value)
        if value != value:
            assert bool(torch.isnan(cost[touched]).all())
        else:
            assert bool(torch.isfinite(cost[touched]).all())


# ---------------------------------------------------------------------------------------------------------------------------
# vocabulary loss rows
# ---------------------------------------------------------------------------------------------------------------------------
def run_ce(name, wrappers=False):
    """forward and backward on a (R, ld = V + pad) buffer whose pad columns hold NaN, out / lse / amax pre-filled with NaN
    -> out, lse, the buffer after the in-place backward, amax"""
    from gvl_amd import MultiScaleDeformableAttention as MSDA
    from gvl_amd import _lib
    i, d = R.inputs(name), device_inputs(name)
    Rn, V, ld = i["R"], i["V"], i["V"] + i["pad"]
    buf = nans(Rn, ld)
    buf[:, :V] = d["x"]
    amax = nans(Rn)
    if wrappers:
        out, lse = MSDA.ce_rows_forward(buf[:, :V], d["target"], d["weight"])
        MSDA.ce_rows_backward_(buf[:, :V], d["target"], d["weight"], d["g"], lse, amax=amax)
    else:
        out, lse = nans(Rn), nans(Rn)
        lib = _lib.lib()
        with torch.cuda.device(DEV):
            _lib.check(lib.gvl_ce_rows_forward_f32(buf.data_ptr(), ld, Rn, V, d["target"].data_ptr(), d["weight"].data_ptr(),
                                                   out.data_ptr(), lse.data_ptr(), _stream()), "ce_rows_forward")
            _lib.check(lib.gvl_ce_rows_backward_f32(buf.data_ptr(), ld, Rn, V, d["target"].data_ptr(), d["weight"].data_ptr(),
                                                    d["g"].data_ptr(), lse.data_ptr(), amax.data_ptr(), _stream()), "ce_rows_backward")
    torch.cuda.synchronize()
    return dict(out=out, lse=lse, buf=buf, amax=amax)


@pytest.mark.parametrize("name", CE)
def test_ce_rows(name):
    """V around the 256 threads of a row's workgroup, ld = V, V + 3 and V + 256 with NaN in the pad columns: the backward leaves the
    pad columns exactly 0, the forward is bit for bit that of ld = V; rows whose maximum stands 80 above the rest (held on their own
    scale: `peak`), a constant row, the target at the maximum and at the minimum; weight = 0 rows holding NaN and inf give
    out = lse = 0 and an all-zero gradient row; amax[row] == |g w|"""
    i, d = R.inputs(name), device_inputs(name)
    V = i["V"]
    w64, w32 = R.reference(name)
    got = run_ce(name)
    dx = got["buf"][:, :V]
    rs = {}
    for group, kinds in R.CE_GROUPS.items():
        rows = torch.tensor([r for r, k in enumerate(R.CE_ROWS) if k in kinds])
        for k, have in (("out", got["out"]), ("lse", got["lse"]), ("dx", dx)):
            rs[f"{k}[{group}]"] = ratio(f"{name}/{k}[{group}]", have[rows.to(DEV)], w64[k][rows], w32[k][rows])
    assert max(rs.values()) <= 1.0, {k: round(v, 3) for k, v in rs.items() if v > 1.0}
    masked = torch.tensor([k.startswith("masked") for k in R.CE_ROWS], device=DEV)
    assert bool(masked.any())
    for k in ("out", "lse"):
        assert float(got[k][masked].abs().max()) == 0.0, k
    assert float(dx[masked].abs().max()) == 0.0
    if i["pad"]:
        assert float(got["buf"][:, V:].abs().max()) == 0.0             # (NaN before the call)
        dense = run_ce("ce_V%d_pad0" % V)
        for k in ("out", "lse", "amax"):
            assert bits_equal(got[k], dense[k]), k
        assert bits_equal(dx, dense["buf"])
    assert bits_equal(got["amax"], (d["g"] * d["weight"]).abs())
    both = run_ce(name, wrappers=True)                                 # MSDA.ce_rows_forward / ce_rows_backward_ on a column slice
    for k in ("out", "lse", "buf", "amax"):
        assert bits_equal(torch.nan_to_num(got[k]), torch.nan_to_num(both[k])), k


def test_ce_rows_backward_refuses_more_pad_columns_than_threads():
    """ld - V = 257: the backward zeroes one pad column per thread; the forward has no such limit"""
    from gvl_amd import _lib
    name = "ce_V37_pad0"
    i, d = R.inputs(name), device_inputs(name)
    Rn, V = i["R"], i["V"]
    ld = V + 257
    buf = nans(Rn, ld)
    buf[:, :V] = d["x"]
    before = buf.clone()
    out, lse, amax = nans(Rn), nans(Rn), nans(Rn)
    lib = _lib.lib()
    with torch.cuda.device(DEV):
        _lib.check(lib.gvl_ce_rows_forward_f32(buf.data_ptr(), ld, Rn, V, d["target"].data_ptr(), d["weight"].data_ptr(), out.data_ptr(),
                                               lse.data_ptr(), _stream()), "ce_rows_forward")
        rc = lib.gvl_ce_rows_backward_f32(buf.data_ptr(), ld, Rn, V, d["target"].data_ptr(), d["weight"].data_ptr(), d["g"].data_ptr(),
                                          lse.data_ptr(), amax.data_ptr(), _stream())
    assert rc != 0
    with pytest.raises(RuntimeError, match="bad sizes"):
        _lib.check(rc, "ce_rows_backward")
    torch.cuda.synchronize()
    assert bits_equal(torch.nan_to_num(buf), torch.nan_to_num(before)) and bool(torch.isnan(amax).all())
    assert bits_equal(out, run_ce(name)["out"])

"""CPU side of tests/test_gpu_cap_train_ops.py: what its comparisons rest on.  The fp64 restatements of the attend and cell ops,
composed into one token step, against oracle.torch_ref.captioner_step in fp64 (values and gradients, the agreement of two fp64
evaluations); gradcheck of the attend restatement; and for every seeded attend case the distance of its samples from the cell
edges and clipping bounds, the clipped share of the clipping cases and the reference forms of the mixed case."""
import pytest
import torch
import torch.nn.functional as F

import test_gpu_cap_train_ops as G
from helpers import load, pdvc_state, t

PRE = "caption_head.1."


def _golden_step(dt=torch.float64):
    f, c = load("pdvc_eval"), load("captioner_step")
    sd = {k: v.to(dt) for k, v in pdvc_state(f).items() if k.startswith(PRE)}
    leaves = {k: t(c[k]).to(dt).requires_grad_() for k in ("memory", "ref_in", "h0")}
    return sd, c, leaves


def _restated_step(sd, c, memory, ref_in, h0, dt=torch.float64):
    """the token step as TeacherForcedLoop composes it: slab = [value | ctx2att(value)], the products over h, the attend op, the
    products over att, the cell"""
    hs, it, c0, mask = t(c["hs"]).to(dt), t(c["it"]), t(c["c0"]).to(dt), t(c["mask"])
    lens = tuple(int(x) for x in c["tshapes"])
    B, Q, H = hs.shape
    n = B * Q
    a = PRE + "core.deformable_att."
    value = F.linear(memory, sd[a + "value_proj.weight"], sd[a + "value_proj.bias"]).masked_fill(mask[..., None], 0.0)
    slab = torch.cat([value, F.linear(value, sd[PRE + "core.ctx2att.weight"], sd[PRE + "core.ctx2att.bias"])], -1)
    w_off, b_off = sd[a + "sampling_offsets.weight"], sd[a + "sampling_offsets.bias"]        # over [h | hs]
    off_h, off_hs = F.linear(h0, w_off[:, :H]), F.linear(hs.reshape(n, H), w_off[:, H:], b_off)
    att_h = F.linear(h0, sd[PRE + "core.h2att.weight"], sd[PRE + "core.h2att.bias"])
    att, _, _, _ = G.attend_restatement(slab, lens, ref_in.reshape(n, len(lens), -1), off_hs, off_h, att_h,
                                        sd[PRE + "core.alpha_net.weight"].reshape(-1), sd[PRE + "core.alpha_net.bias"],
                                        torch.arange(n) // Q, off_h.shape[1] // len(lens))
    w_ih, w_hh = sd[PRE + "core.rnn.weight_ih_l0"], sd[PRE + "core.rnn.weight_hh_l0"]
    xt = F.embedding(it, sd[PRE + "embed.weight"])
    E, Cv = xt.shape[1], att.shape[1]
    ga, gb = F.linear(att, w_ih[:, E:E + Cv]), F.linear(h0, w_hh)
    gc = F.linear(xt, w_ih[:, :E]) + F.linear(hs.reshape(n, H), w_ih[:, E + Cv:])
    _, h1, c1, _ = G.cell_restatement(ga, gb, gc, c0)
    return h1, c1


def test_restatements_compose_to_the_oracle_token_step():
    """h1, c1 and the gradients of (h1 r).sum() w.r.t. memory (through the slab derived from it), ref_in and h0 at 1e-10 of each
    tensor's largest entry"""
    from oracle import torch_ref as R
    sd, c, leaves = _golden_step()
    r = torch.randn(16, 512, generator=torch.Generator().manual_seed(0)).double()
    h1, c1 = _restated_step(sd, c, leaves["memory"], leaves["ref_in"], leaves["h0"])
    got = torch.autograd.grad((h1 * r).sum(), list(leaves.values()))
    _, (h1o, c1o) = R.captioner_step(sd, PRE, t(c["it"]), (leaves["h0"], t(c["c0"]).double()), t(c["hs"]).double(),
                                     leaves["ref_in"], leaves["memory"], t(c["tshapes"]), t(c["mask"]))
    want = torch.autograd.grad((h1o * r).sum(), list(leaves.values()))
    pairs = [("h1", h1, h1o), ("c1", c1, c1o)] + [("d " + k, g, w) for k, g, w in zip(leaves, got, want)]
    for name, g, w in pairs:
        scale = float(w.detach().abs().max())
        assert scale > 0, name
        err = float((g - w).detach().abs().max())
        assert err <= 1e-10 * scale, (name, err, scale)
    assert float(want[1][..., 1].abs().max()) > 0                   # the fixture's reference points carry a length, with a gradient


GRADCHECK_SEED = 1


def _gradcheck_inputs():
    g = torch.Generator().manual_seed(GRADCHECK_SEED)
    lens, P, n, Cv = (4, 3), 2, 3, 3
    rnd = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)          # noqa: E731
    ref = torch.stack([0.3 + 0.4 * torch.rand(n, 2, generator=g, dtype=torch.float64),
                       torch.tensor([0.3, -1.0, 0.2], dtype=torch.float64)[:, None].expand(n, 2)], -1)
    tensors = [rnd(2, sum(lens), 2 * Cv), ref, 0.3 * rnd(n, 4), rnd(n, Cv), rnd(Cv), rnd(1)]
    fn = lambda slab, ref, off_h, att_h, aw, ab: G.attend_restatement(      # noqa: E731
        slab, lens, ref, torch.zeros(n, 4, dtype=torch.float64), off_h, att_h, aw, ab, torch.tensor([1, 0, 1]), P)[0]
    return fn, tensors


def test_attend_restatement_passes_gradcheck_at_an_interior_case():
    """autograd of the restatement against finite differences: a restatement consistent with itself and nothing else would
    pass everything above.  Every sample is unclipped and 0.05 from a cell edge, so the finite differences stay inside a cell;
    both reference forms take part"""
    fn, tensors = _gradcheck_inputs()
    slab, ref, off_h, att_h, aw, ab = tensors
    geo = G.attend_restatement(slab, (4, 3), ref, torch.zeros(3, 4, dtype=torch.float64), off_h, att_h, aw, ab,
                               torch.tensor([1, 0, 1]), 2)[3]
    assert not bool((geo["lo"] | geo["hi"]).any())
    assert float((geo["x"] - geo["x"].round()).abs().min()) >= 0.05
    assert torch.autograd.gradcheck(fn, [x.requires_grad_() for x in tensors], eps=1e-6, atol=1e-7, rtol=1e-5)


def conditions(name, seed=None):
    """figures of a seeded attend case, from its fp64 restatement, every row and every sample included"""
    inp = G.attend_inputs(name, seed)
    w = G._attend_eval(inp, torch.float64)
    x, lo, hi = w["x"], w["lo"], w["hi"]
    clipped = lo | hi
    Tm1 = torch.tensor(inp["lens"], dtype=torch.float64).repeat_interleave(inp["P"]) - 1
    cell = (x - x.round()).abs()[~clipped]
    return dict(cell=float(cell.min()) if cell.numel() else float("inf"), unclipped=int((~clipped).sum()),
                bound=float(torch.minimum(x.abs(), (x - Tm1).abs()).min()),
                share=float(clipped.double().mean()), lo=int(lo.sum()), hi=int(hi.sum()), w=w, inp=inp)


@pytest.mark.parametrize("name", list(G.ATTEND_CASES))
def test_attend_seeds_keep_their_distance_from_the_edges(name):
    """no unclipped sample within EDGE of an integer pixel coordinate, no sample at all within EDGE of a clipping bound: three
    orders above fp32's error in x at these sizes, so the fp32 kernel samples the cells the fp64 restatement samples"""
    cnd = conditions(name)
    assert cnd["cell"] >= G.EDGE and cnd["bound"] >= G.EDGE, (cnd["cell"], cnd["bound"])
    assert cnd["lo"] + cnd["hi"] > 0 and cnd["unclipped"] > 0               # every case sees a clipped sample and an inner one
    w32 = G.attend_reference(name)[1]
    assert torch.equal(w32["lo"], cnd["w"]["lo"]) and torch.equal(w32["hi"], cnd["w"]["hi"])
    assert torch.equal(w32["x"].floor()[~w32["lo"] & ~w32["hi"]].double(), cnd["w"]["x"].floor()[~cnd["w"]["lo"] & ~cnd["w"]["hi"]])


@pytest.mark.parametrize("name", [k for k, v in G.ATTEND_CASES.items() if v.get("clipping")])
def test_attend_clipping_cases_clip_a_quarter_to_three_quarters(name):
    cnd = conditions(name)
    assert 0.25 <= cnd["share"] <= 0.75 and cnd["lo"] > 0 and cnd["hi"] > 0, cnd["share"]


def test_attend_case_shapes_are_what_they_claim():
    inp = G.attend_inputs("compact")
    rv, length = inp["row_video"], inp["ref"][:, 0, 1]
    assert rv.tolist()[0] == -1 == rv.tolist()[-1] and sorted(set(rv.tolist())) == [-1, 0, 2]
    valid = rv >= 0
    assert int((valid & (length >= 0)).sum()) >= 2 and int((valid & (length < 0)).sum()) >= 2       # both reference forms
    assert bool((inp["ref"][1::2, :, 1] == -1).all()) and bool((inp["ref"][0::2, :, 1] > 0).all())
    # contention: one video, five slab rows, a level-0 sample between its two rows in more than a few rows
    inp = G.attend_inputs("contention")
    assert inp["slab"].shape[:2] == (1, 5) and inp["ref"].shape[0] == 64 and conditions("contention")["unclipped"] >= 16
    assert [len(G.ATTEND_CASES[k]["lens"]) * G.ATTEND_CASES[k]["P"] for k in G.FEW] == [8, 1, 15, 12]
    # saturation: e spans more than 100 in every row, most alpha are below fp32's smallest normal number, +-30 into the tanh,
    # and whole (row, level) groups lie 1e6 beyond either end
    inp, w = G.attend_inputs("saturation"), G.attend_reference("saturation")[0]
    assert float((w["e"].max(1).values - w["e"].min(1).values).min()) > 100
    assert float((w["alpha"] < 2.0 ** -126).double().mean()) > 0.5
    assert float(inp["slab"][..., G.C:].abs().min()) == 30.0
    far = inp["far"].repeat_interleave(inp["P"], 1)
    assert bool((w["x"][far].abs() > 1e4).all()) and bool((w["x"][far] > 0).any()) and bool((w["x"][far] < 0).any())
    assert bool((w["lo"] | w["hi"])[far].all()) and float(w["g_off"][:, :16][far].abs().max()) == 0.0
    for side in G.attend_reference("saturation"):
        assert all(bool(torch.isfinite(v).all()) for v in side.values() if isinstance(v, torch.Tensor) and v.is_floating_point())


@pytest.mark.parametrize("n,H", G.CELL_SIZES)
def test_cell_sizes_reach_the_paths_they_name(n, H):
    assert (n * H > 4096 * 256) == (n == 2049)                     # only the last one runs the grid-stride loop's second pass
    if n == 2049:
        assert n * H - 4096 * 256 == 512
        return
    inp = G.cell_inputs(n, H, saturated=True)                       # (the saturated case runs at the two smaller sizes)
    s = (inp["ga"] + inp["gb"] + inp["gc"]).abs()
    assert float((s == 40).double().mean()) > 0.3 and bool((s == 120).any())
    w64, w32 = G.cell_reference(n, H, True)
    assert all(bool(torch.isfinite(v).all()) for v in list(w64.values()) + list(w32.values()))

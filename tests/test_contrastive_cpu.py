"""CPU: the contrastive branch's host side.  The restatement of the criterion (tests/contrastive_ref.py) and the product's PyTorch
formulation equal the reference's recorded loss, logits and gradients in fp64; the text-encoder interface, build()'s three routes,
the loss-weight schedule and the refusals behave as documented; the model fixtures' assignments do not hang on rounding."""
import glob
import os

import numpy as np
import pytest
import torch

import contrastive_ref as R
from contrastive_stub import unpack_fixture
from helpers import GOLDEN, load, t

CASES = {"default": (True, False, False), "e2t": (True, True, False), "e2t_bg": (True, True, True),
         "pervideo": (False, False, False)}


@pytest.fixture(scope="module")
def op():
    return load("contrastive_op")


def pairs_of(f):
    n_gt = [int(n) for n in f["n_gt"]]
    B, Q, D = (int(v) for v in f["dims"])
    pt, pe, pv, base = [], [], [], 0
    for i, n in enumerate(n_gt):
        q, c = t(f[f"match_{i}"])
        pt.append(c + base); pe.append(q + i * Q); pv.append(torch.full_like(q, i))
        base += n
    return torch.cat(pt), torch.cat(pe), torch.cat(pv), n_gt, B, Q, D


def match_lists(f):
    return [(t(f[f"match_{i}"])[0], t(f[f"match_{i}"])[1]) for i in range(len(f["n_gt"]))]


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_equals_the_reference(op, name):
    cross, e2t, bgall = CASES[name]
    pt, pe, pv, n_gt, B, Q, D = pairs_of(op)
    text, event, bg = (t(op[k]).clone().requires_grad_() for k in ("text", "event", "bg"))
    loss, _, _ = R.contrastive_loss(text, event.reshape(-1, D), pt, pe, pv, B, Q, 0.1, cross, e2t, bgall, bg)
    loss.backward()
    assert abs(float(loss) - float(op[f"{name}.loss"])) < 1e-10
    assert (R.cosines(text, event.reshape(-1, D))[pt] - t(op[f"{name}.raw_logits"])).abs().max() < 1e-10
    assert (R.cosines(text, event.reshape(-1, D), bg).t() - t(op[f"{name}.match_mat"])).abs().max() < 1e-10
    assert (text.grad - t(op[f"{name}.grad_text"])).abs().max() < 1e-10
    assert (event.grad - t(op[f"{name}.grad_event"])).abs().max() < 1e-10
    if e2t:
        assert (bg.grad - t(op[f"{name}.grad_bg"])).abs().max() < 1e-10


@pytest.mark.parametrize("name", sorted(CASES))
def test_product_formulation_equals_the_reference(op, name):
    from gvl_amd.criterion import ContrastiveCriterion
    cross, e2t, bgall = CASES[name]
    n_gt = [int(n) for n in op["n_gt"]]
    text = [x.clone().requires_grad_() for x in t(op["text"]).split(n_gt)]
    event, bg = t(op["event"]).clone().requires_grad_(), t(op["bg"]).clone().requires_grad_()
    crit = ContrastiveCriterion(0.1, cross, e2t, bgall)
    loss, raw = crit(text, event, match_lists(op), return_logits=True, bg_embed=bg)
    loss.backward()
    assert abs(float(loss) - float(op[f"{name}.loss"])) < 1e-10
    assert (raw - t(op[f"{name}.raw_logits"])).abs().max() < 1e-10
    assert (torch.cat([x.grad for x in text]) - t(op[f"{name}.grad_text"])).abs().max() < 1e-10
    assert (event.grad - t(op[f"{name}.grad_event"])).abs().max() < 1e-10
    mm = crit.forward_logits(torch.cat(text).detach(), event.detach().reshape(-1, event.shape[-1]), bg.detach()).t()
    assert (mm - t(op[f"{name}.match_mat"])).abs().max() < 1e-10


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_gradcheck(op, name):
    cross, e2t, bgall = CASES[name]
    pt, pe, pv, n_gt, B, Q, D = pairs_of(op)
    text, event, bg = (t(op[k]).clone().requires_grad_() for k in ("text", "event", "bg"))
    fn = lambda a, b, c: R.contrastive_loss(a, b.reshape(-1, D), pt, pe, pv, B, Q, 0.1, cross, e2t, bgall, c)[0]  # noqa: E731
    inputs = (text, event, bg) if e2t else (text, event, bg.detach())
    assert torch.autograd.gradcheck(fn, inputs, eps=1e-6, atol=1e-6)


def test_word_pool_restatement_equals_the_module():
    from gvl_amd.text import WordLevelContextModeling
    torch.manual_seed(0)
    m = WordLevelContextModeling(12).double()
    x = torch.randn(5, 7, 12, dtype=torch.float64)
    mask = (torch.arange(7)[None] < torch.tensor([7, 3, 1, 5, 2])[:, None]).long()
    ref = R.word_attention_pool(x, mask, m.w1.weight, m.w1.bias, m.w2.weight, m.w2.bias)
    assert (m(x, mask) - ref).abs().max() < 1e-12
    # padded words carry no weight: changing them changes nothing
    x2 = x.clone()
    x2[1, 3:] += 5.0
    assert (m(x2, mask)[1] - m(x, mask)[1]).abs().max() < 1e-12


def test_precomputed_text_encoder():
    from gvl_amd.text import PrecomputedTextEncoder
    enc = PrecomputedTextEncoder(48)
    assert enc.config.hidden_size == 48 and not list(enc.parameters())
    h, mask = torch.randn(4, 6, 48), torch.ones(4, 6)
    out = enc(**{"last_hidden_state": h, "attention_mask": mask})
    assert out.last_hidden_state is h and torch.equal(out["pooler_output"], h[:, 0])
    with pytest.raises(ValueError):
        enc(last_hidden_state=torch.randn(4, 6, 47), attention_mask=mask)


def small_opt(**over):
    from gvl_amd.config import make_opt
    kw = dict(num_queries=8, feature_dim=64, vocab_size=40, max_caption_len=6, device="cpu", enable_contrastive=True,
              contrastive_hidden_size=16, text_feature_dim=48)
    kw.update(over)
    return make_opt("anet_c3d_ssvg", **kw)


def test_build_routes():
    from contrastive_stub import StubTextEncoder
    from gvl_amd.criterion import ContrastiveCriterion
    from gvl_amd.pdvc import build
    from gvl_amd.text import PrecomputedTextEncoder
    enc = StubTextEncoder()
    model, crit, cc, post = build(small_opt(text_feature_dim=None), text_encoder=enc)
    assert model.text_encoder is enc and isinstance(cc, ContrastiveCriterion)
    assert all(not p.requires_grad for p in enc.parameters())
    assert "contrastive_loss" in crit.weight_dict and "contrastive_loss_0" in crit.weight_dict
    keys = set(model.state_dict())
    for k in ("text_encoder.embeddings.weight", "word_context_model.w1.weight", "word_context_model.w2.bias",
              "contrastive_projection_event.0.weight", "contrastive_projection_event.1.bias", "contrastive_projection_text.0.weight"):
        assert k in keys, k
    assert "background_embed" not in keys
    assert model.contrastive_projection_event[0] is model.contrastive_projection_event[1]          # shared, as the reference ties them
    model2, _, cc2, _ = build(small_opt(enable_e2t_cl=True, disable_cl_proj_layer_share_weight=True, enable_multilayer_projection=True))
    assert isinstance(model2.text_encoder, PrecomputedTextEncoder) and model2.text_encoder.config.hidden_size == 48
    assert model2.background_embed.shape == (1, 16) and cc2.enable_e2t_cl
    assert model2.contrastive_projection_event[0] is not model2.contrastive_projection_event[1]
    assert "contrastive_projection_text.0.layers.1.weight" in model2.state_dict()
    with pytest.raises(ValueError, match="text_encoder.*text_feature_dim"):
        build(small_opt(text_feature_dim=None))
    # the optimizer never sees the frozen encoder (train.py:242-246)
    from gvl_amd.optim import build_optimizer
    opt_ids = {id(p) for g in build_optimizer(model, small_opt()).param_groups for p in g["params"]}
    assert not opt_ids & {id(p) for p in enc.parameters()}
    assert id(model.word_context_model.w1.weight) in opt_ids and id(model.contrastive_projection_text[0].weight) in opt_ids


def test_refusals_name_their_switch():
    from gvl_amd.pdvc import build
    with pytest.raises(NotImplementedError, match="enable_sentence_context_modeling"):
        build(small_opt(enable_sentence_context_modeling=True))
    with pytest.raises(NotImplementedError, match="frozen"):
        build(small_opt(text_encoder_learning_strategy="warmup_linear"))
    with pytest.raises(NotImplementedError, match="enable_e2t_cl"):
        build(small_opt(enable_cross_video_cl=False, enable_e2t_cl=True))
    with pytest.raises(NotImplementedError, match="caption_loss_type"):
        build(small_opt(caption_loss_type="rl"))
    from gvl_amd.parallel import GraphedEvalForward, GraphedTrainStep
    model, crit, cc, _ = build(small_opt())
    assert not model.supports_padded_targets(crit, True)
    for cls in (GraphedTrainStep, GraphedEvalForward):
        with pytest.raises(NotImplementedError, match="contrastive branch: captured steps not built"):
            cls(model, crit, small_opt()) if cls is GraphedTrainStep else cls(model, crit)


def test_schedule():
    from gvl_amd import optim
    from gvl_amd.pdvc import build
    o = small_opt()
    _, crit, _, _ = build(o)
    assert [optim.contrastive_weight(o, e) for e in range(4)] == [0, 0, 0.1, 0.1]
    assert optim.apply_contrastive_schedule(crit, o, 0) == 0 and crit.matcher.cost_cl == 0
    assert all(v == 0 for k, v in crit.weight_dict.items() if "contrastive_loss" in k)
    assert optim.apply_contrastive_schedule(crit, o, 2) == 0.1 and crit.matcher.cost_cl == o.set_cost_cl
    assert {v for k, v in crit.weight_dict.items() if "contrastive_loss" in k} == {0.1}
    assert crit.weight_dict["loss_ce"] == o.cls_loss_coef
    for path in glob.glob(os.path.join(GOLDEN, "pdvc_contrastive_*.npz")):
        assert [optim.contrastive_weight(o, e) for e in range(4)] == list(unpack_fixture(path)["schedule"])


def test_make_opt_defaults_unchanged():
    from gvl_amd.config import make_opt
    from gvl_amd.pdvc import build
    o = make_opt()
    assert o.enable_contrastive is False and o.set_cost_cl == 2.0 and o.text_feature_dim == 768
    assert o.cl_schedule_time == [0, 2] and o.cl_schedule_val == [0, 0.1] and o.eval_enable_grounding is True
    model, crit, cc, _ = build(make_opt("anet_c3d_ssvg", num_queries=8, feature_dim=64, vocab_size=40, max_caption_len=6, device="cpu"))
    assert cc is None and not model.enable_contrastive and model.background_embed is None
    assert not any(k.startswith(("text_encoder", "contrastive", "word_context")) for k in model.state_dict())


def test_fixture_assignments_do_not_hang_on_rounding():
    """the seed condition of tests/golden/make_golden_contrastive.py: every stored cost matrix keeps its assignment under 32 seeded
    perturbations of +-1e-3, so comparing matched indices cannot turn on fp32 rounding"""
    from scipy.optimize import linear_sum_assignment
    paths = sorted(glob.glob(os.path.join(GOLDEN, "pdvc_contrastive_*.npz")))
    assert paths
    for path in paths:
        f = unpack_fixture(path)
        for key in [k for k in f if k.startswith("cost_")]:
            C = f[key].astype(np.float64)
            base = linear_sum_assignment(C)
            rs = np.random.RandomState(0)
            for _ in range(32):
                got = linear_sum_assignment(C + 1e-3 * rs.choice([-1.0, 1.0], size=C.shape))
                assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1]), (path, key)

#!/usr/bin/env python3
"""Generate the contrastive fixtures by running the *imported* reference on the CPU (build container only):

    python tests/golden/make_golden_contrastive.py [op] [model]          (from any directory; writes next to this file)

contrastive_op.npz: for each covered switch combination, in fp64, inputs of the reference's ContrastiveCriterion, its loss, raw
logits and the gradients of text, event and background.  pdvc_contrastive_*.npz: the reference PDVC built from
cfgs/anet_c3d_ssvg.yml at small dimensions with the stand-in text encoder of tests/contrastive_stub.py in place of
AutoModel.from_pretrained (nothing is downloaded): eval forward, grounding, a training forward / backward, the schedule's weights.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402  (installs the reference import shim)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from synth import synth_array, synth_state_dict  # noqa: E402
import contrastive_stub as stub  # noqa: E402

OP_CASES = {                      # name -> (cross_video, e2t, bg_for_cl)
    "default": (True, False, False), "e2t": (True, True, False), "e2t_bg": (True, True, True), "pervideo": (False, False, False)}


def make_op():
    from pdvc.criterion import ContrastiveCriterion
    B, Q, D, n_gt = 3, 7, 16, [3, 1, 2]
    rec = dict(n_gt=np.array(n_gt), dims=np.array([B, Q, D]), temperature=np.array(0.1))
    g = torch.Generator().manual_seed(5)
    match = []
    for i, n in enumerate(n_gt):
        match.append((torch.randperm(Q, generator=g)[:n], torch.randperm(n, generator=g)))
        rec[f"match_{i}"] = torch.stack(match[-1])
    for name, (cross, e2t, bgall) in OP_CASES.items():
        text = [torch.from_numpy(synth_array(f"cl.text{i}", (n, D), 7)).double().requires_grad_() for i, n in enumerate(n_gt)]
        event = torch.from_numpy(synth_array("cl.event", (B, Q, D), 7)).double().requires_grad_()
        bg = torch.from_numpy(synth_array("cl.bg", (1, D), 7)).double().requires_grad_()
        crit = ContrastiveCriterion(temperature=0.1, enable_cross_video_cl=cross, enable_e2t_cl=e2t, enable_bg_for_cl=bgall)
        loss, raw = crit(text, event, match, return_logits=True, bg_embed=bg)
        loss.backward()
        rec.update({f"{name}.loss": loss.detach(), f"{name}.raw_logits": raw.detach(), f"{name}.grad_event": event.grad,
                    f"{name}.grad_text": torch.cat([t_.grad for t_ in text])})
        if e2t:
            rec[f"{name}.grad_bg"] = bg.grad
        rec[f"{name}.match_mat"] = crit.forward_logits(torch.cat(text), event.reshape(-1, D), bg).t().detach()
    rec.update(text=torch.cat([t_.detach() for t_ in text]), event=event.detach(), bg=bg.detach())
    MG.save("contrastive_op", **rec)


MODEL_CASES = {
    "default": dict(),
    "e2t": dict(enable_e2t_cl=True),
    "e2t_bg": dict(enable_e2t_cl=True, enable_bg_for_cl=True),
    "pervideo": dict(enable_cross_video_cl=False),
    "layerdiff": dict(enable_layer_diff_text_feature=True, disable_cl_proj_layer_share_weight=True),
}
B, T, VALID, N_GT = 2, 24, [24, 17], [3, 2]


def text_input(n_gt):
    sents = stub.sentences(n_gt)
    return sents, stub.StubTokenizer()([s for v in sents for s in v])


def stable(C, trials=32, eps=1e-3):
    """is the assignment of this cost matrix unchanged under seeded perturbations of +-eps?"""
    from scipy.optimize import linear_sum_assignment
    base = linear_sum_assignment(C)
    rs = np.random.RandomState(0)
    for _ in range(trials):
        got = linear_sum_assignment(C + eps * rs.choice([-1.0, 1.0], size=C.shape))
        if not (np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1])):
            return False
    return True


def make_model(only=None):
    import pdvc.pdvc as P
    P.AutoModel.from_pretrained = staticmethod(lambda *a, **k: stub.StubTextEncoder())
    for name, over in MODEL_CASES.items():
        if only and name not in only:
            continue
        overrides = dict(MG.PDVC_OVERRIDES)
        overrides.update(enable_contrastive=True, contrastive_hidden_size=16, transformer_dropout_prob=0.0, drop_prob=0.0,
                         contrastive_loss_start_coef=0.1, eval_enable_matching_score=True)
        overrides.update(over)
        opt, model, criterion, cc = MG.build_pdvc("cfgs/anet_c3d_ssvg.yml", overrides)
        post = MG.post['bbox']
        shapes = {k: tuple(v.shape) for k, v in model.state_dict().items() if not k.startswith("text_encoder.")}
        sd = {k: torch.from_numpy(v) for k, v in synth_state_dict(shapes, seed=320).items()}
        sd.update({k: v for k, v in model.state_dict().items() if k.startswith("text_encoder.")})
        model.load_state_dict(sd, strict=True)
        loaded = model.state_dict()
        names = sorted(shapes)
        ties = [f"{a}={b}" for i, a in enumerate(names) for b in names[i + 1:] if loaded[a].data_ptr() == loaded[b].data_ptr()]
        sents, enc_in = text_input(N_GT)
        for seed in range(1, 40):                       # the data seed: every video's assignment must not hang on rounding
            dt = MG.synth_dt(B, T, opt.feature_dim, valid=VALID, n_gt=N_GT, seed=seed)
            dt.update(cap_raw=sents, text_encoder_input=enc_in)
            with MG.cuda_semantics(), torch.no_grad():
                out, loss = model.eval()(dt, criterion, cc, "queries", eval_mode=True)
                layers = [out] + list(out["aux_outputs"])
                Cs = [criterion.matcher(o, dt["video_target"], return_C=True)[2] for o in layers]
            if all(stable(c.double().numpy()) for cl in Cs for c in cl):
                break
        else:
            raise RuntimeError("no data seed with stable assignments")
        assert all(stable(c.double().numpy()) for cl in Cs for c in cl)
        rec = dict(meta_T=np.array(T), valid=np.array(VALID), n_gt=np.array(N_GT), data_seed=np.array(seed),
                   param_names=np.array(names), param_shapes=np.array([str(shapes[k]) for k in names]),
                   ties=np.array(ties if ties else ["-"]), out_keys=np.array(sorted(out.keys())),
                   aux_keys=np.array(sorted(out["aux_outputs"][0].keys())), loss_keys=np.array(sorted(loss.keys())))
        rec.update(pred_logits=out["pred_logits"], pred_boxes=out["pred_boxes"], pred_count=out["pred_count"],
                   aux_pred_logits=out["aux_outputs"][0]["pred_logits"], aux_pred_boxes=out["aux_outputs"][0]["pred_boxes"],
                   cl_match_mats=out["cl_match_mats"], aux_cl_match_mats=out["aux_outputs"][0]["cl_match_mats"],
                   cl_logits=out["cl_logits"], seq=out["seq"])
        for l, cl in enumerate(Cs):
            for i, c in enumerate(cl):
                rec[f"cost_{l}_{i}"] = c
        for i, (a, b) in enumerate(out["matched_indices"][0]):
            rec[f"match_{i}"] = torch.stack([a, b])
        for k, v in loss.items():
            rec[f"loss.{k}"] = torch.as_tensor(v).detach()
        # grounding (pdvc.py:938-1000)
        import copy
        tsz = dt["video_length"][:, 1]
        res, cl_scores = post.forward_grounding(out, tsz, copy.deepcopy(dt["video_target"]))
        spans = stub.grounding_spans(out["pred_boxes"], tsz)
        for i, r in enumerate(res):
            rec[f"ground_boxes_{i}"], rec[f"ground_confs_{i}"] = np.array(r["boxes"]), np.array(r["confs"])
            rec[f"ground_cl_{i}"] = np.array(r["cl_scores"])
            rec[f"ground_events_{i}"] = np.array(stub.events_of_boxes(r["boxes"], spans[i]))       # the chosen events
        # the same with eval_enable_maximum_matching_for_grounding
        opt.eval_enable_maximum_matching_for_grounding = True
        res_max, _ = post.forward_grounding(out, tsz, copy.deepcopy(dt["video_target"]))
        opt.eval_enable_maximum_matching_for_grounding = False
        for i, r in enumerate(res_max):
            rec[f"ground_max_events_{i}"] = np.array(stub.events_of_boxes(r["boxes"], spans[i]))
            rec[f"ground_max_cl_{i}"] = np.array(r["cl_scores"])
        # PostProcess.forward's cl_scores (pdvc.py:1059-1081) with the stand-in tokenizer
        with torch.no_grad():
            records = post(out, tsz, stub.StubLoader(), model, stub.StubTokenizer())
        rec["post_cl_scores"] = np.stack([np.asarray(r_["cl_scores"], dtype=np.float64) for r_ in records])
        rec["post_query_id"] = np.stack([np.asarray(r_["query_id"]) for r_ in records])
        assert np.abs(rec["post_cl_scores"]).max() > 0
        if isinstance(cl_scores, (list, tuple)):
            for i, c in enumerate(cl_scores):
                rec[f"ground_scores_{i}"] = c
        else:
            rec["ground_scores"] = cl_scores
        # a training forward / backward
        g = torch.Generator().manual_seed(11)
        caps = torch.randint(1, opt.vocab_size, (sum(N_GT), 7), generator=g)
        caps[:, 0] = 0
        caps[:, -1] = 0
        cap_mask = (torch.arange(7)[None] <= (caps != 0).sum(1)[:, None]).float()
        dt.update(cap_tensor=caps, cap_mask=cap_mask, gt_boxes_mask=torch.tensor([[1, 1, 1], [1, 1, 0]]).bool(),
                  gt_gather_idx=torch.tensor([0, 0, 0, 1, 1]))
        model.train()
        with MG.cuda_semantics():
            out_t, loss_t = model(dt, criterion, cc, "queries")
        wd = criterion.weight_dict
        final = sum(loss_t[k] * wd[k] for k in loss_t.keys() if k in wd)
        final.backward()
        params = dict(model.named_parameters())
        gn = sorted(n for n, p_ in params.items() if p_.grad is not None)
        rec.update(cap_tensor=caps, cap_mask=cap_mask, final_loss=final.detach(), grad_names=np.array(gn),
                   grad_norms=torch.stack([params[n].grad.double().norm() for n in gn]),
                   weight_keys=np.array(sorted(wd)), weight_vals=np.array([float(wd[k]) for k in sorted(wd)]))
        for k, v in loss_t.items():
            rec[f"train_loss.{k}"] = torch.as_tensor(v).detach()
        # the schedule (train.py:304-311,363-368) over epochs 0..3
        sched, w = [], 0.0
        for epoch in range(4):
            if epoch in opt.cl_schedule_time:
                w = opt.cl_schedule_val[opt.cl_schedule_time.index(epoch)]
            sched.append(w)
        rec["schedule"] = np.array(sched)
        MG.save("pdvc_contrastive_" + name, **stub.pack_fixture(rec))


if __name__ == "__main__":
    what = [a for a in sys.argv[1:] if not a.startswith("-")]
    if not what or "op" in what:
        make_op()
    if not what or "model" in what:
        make_model([a for a in what if a in MODEL_CASES] or None)

#!/usr/bin/env python3
"""Generate the Transformer-DSA caption head's fixtures by running the *imported* reference on the CPU (build container only):

    python tests/golden/make_golden_transformer_cap.py [head] [model]          (from any directory; writes next to this file)

transformer_cap_{a6,a34,b}.npz: the reference's TransformerDSACaptioner (pdvc/CaptioningHead/Transformer_DSA.py) on the seeded inputs
of tests/transformer_cap_ref.py, weights from synth_state_dict: teacher-forced log-probs, build_loss rows, gradients (norm and a
strided sample of every parameter's, hs's and memory's in full) for a seeded upstream gradient, the greedy decode and the top-2
log-prob margin of every decode step.  pdvc_transformer_cap.npz: the reference PDVC with caption_decoder_type='transformer': an eval
forward with its PostProcess records, and a dropout-0 training forward / backward.  Everything under CUDA-op semantics (MSDeformAttn
pads with zeros).  The fixtures hold outputs and name / shape lists only.

Near ties: greedy tokens are compared exactly on STRICT rows only (smallest margin over all steps >= 10 x the log-prob tolerance).
The weight seed and a scale on logits.weight are searched until at least two thirds of a case's rows are strict, one strict row
runs the full length and one ends early."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402  (installs the reference import shim)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from synth import synth_state_dict  # noqa: E402
import transformer_cap_ref as R  # noqa: E402

SCALES = (6.0, 8.0, 12.0, 16.0, 24.0)


def decode_with_margins(head, sample):
    """run `sample()` -> (its result, (steps, n) top-2 log-prob margins of the last position of every forward the decode made)"""
    rec, orig = [], head.forward

    def fwd(*a, **k):
        out = orig(*a, **k)
        top = out[:, -1].detach().topk(2, -1).values
        rec.append((top[:, 0] - top[:, 1]).clone())
        return out
    head.forward = fwd
    try:
        res = sample()
    finally:
        del head.forward
    return res, torch.stack(rec).numpy()


def acceptable(seq, margins, T):
    """the generator's three conditions on a decode"""
    if not isinstance(seq, torch.Tensor) or seq.numel() == 0:
        return False
    rows = seq.reshape(-1, seq.shape[-1])
    keep = rows.shape[1]
    strict, _ = R.strict_rows(margins, keep)
    full = (rows != 0).all(1).numpy() & (keep == T)
    early = (rows == 0).any(1).numpy()
    return strict.sum() * 3 >= 2 * len(strict) and bool((strict & full).any()) and bool((strict & early).any())


def make_head(only=None):
    from pdvc.CaptioningHead.Transformer_DSA import TransformerDSACaptioner
    for case, c in R.HEAD_CASES.items():
        if only and case not in only:
            continue
        inp = R.head_inputs(case)
        torch.manual_seed(0)
        head = TransformerDSACaptioner(R.head_opt(case)).eval()
        shapes = {k: tuple(v.shape) for k, v in head.state_dict().items()}
        pos_table = head.pos_table.clone()
        found = None
        for seed in range(300, 340):
            for scale in SCALES:
                sd = {k: torch.from_numpy(v) for k, v in synth_state_dict(shapes, seed).items()}
                sd["pos_table"] = pos_table                         # a buffer the constructor computes, not a weight
                sd["logits.weight"] = sd["logits.weight"] * scale
                head.load_state_dict(sd, strict=True)
                with MG.cuda_semantics(), torch.no_grad():
                    (seq, lp), margins = decode_with_margins(head, lambda: head.sample(inp["hs"], inp["reference"], inp["others"]))
                if acceptable(seq, margins, c["T"]):
                    found = (seed, scale)
                    break
            if found:
                break
        if not found:
            raise RuntimeError(f"{case}: no (seed, scale) meets the near-tie conditions")
        keep = seq.shape[1]
        strict, _ = R.strict_rows(margins, keep)
        print(f"{case}: seed {found[0]} scale {found[1]} keep {keep} strict {int(strict.sum())}/{len(strict)} "
              f"min margin {margins[:keep].min():.2e} median {np.median(margins[:keep]):.2f}")
        hs = inp["hs"].clone().requires_grad_()
        others = dict(inp["others"])
        others["memory"] = inp["others"]["memory"].clone().requires_grad_()
        head.zero_grad()
        with MG.cuda_semantics():
            logp = head(hs, inp["reference"], others, inp["seq"])
            loss_rows = head.build_loss(logp, inp["seq"][:, 1:], inp["cap_mask"][:, 1:])
            (logp * inp["gout"]).sum().backward()
        params = dict(head.named_parameters())
        gn = sorted(n for n, p_ in params.items() if p_.grad is not None)
        rec = dict(seed=np.array(found[0]), logit_scale=np.array(found[1]), param_names=np.array(sorted(shapes)),
                   param_shapes=np.array([str(shapes[k]) for k in sorted(shapes)]), pos_table=pos_table,
                   logp=logp.detach(), loss_rows=loss_rows.detach(), grad_names=np.array(gn),
                   grad_norms=torch.stack([params[n].grad.double().norm() for n in gn]),
                   grad_hs=hs.grad, grad_memory=others["memory"].grad, sample_seq=seq, sample_lp=lp, margins=margins[:keep])
        for n in gn:
            rec["grad." + n] = R.grad_sample(params[n].grad)
        MG.save("transformer_cap_" + case, **rec)


MODEL_OVER = dict(caption_decoder_type="transformer", cap_nheads=8, vocab_size=60, max_caption_len=6, num_queries=5)
B, T, VALID, N_GT = 2, 24, [24, 17], [3, 2]


def make_model():
    over = dict(MG.PDVC_OVERRIDES)
    over.update(MODEL_OVER)
    opt, model, criterion, cc = MG.build_pdvc(overrides=over)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    names = sorted(shapes)
    buffers = {k: v.clone() for k, v in model.state_dict().items() if k.endswith("pos_table")}
    dt = MG.synth_dt(B, T, opt.feature_dim, valid=VALID, n_gt=N_GT)
    head = model.caption_head[-1]
    found = None
    for seed in range(300, 330):
        for scale in SCALES:
            sd = {k: torch.from_numpy(v) for k, v in synth_state_dict(shapes, seed).items()}
            sd.update(buffers)
            for k in sd:
                if k.endswith("logits.weight"):
                    sd[k] = sd[k] * scale
            model.load_state_dict(sd, strict=True)
            with MG.cuda_semantics(), torch.no_grad():
                (out, loss), margins = decode_with_margins(head, lambda: model(dt, criterion, cc, "queries", eval_mode=True))
            if acceptable(out["seq"], margins, opt.max_caption_len):
                found = (seed, scale)
                break
        if found:
            break
    if not found:
        raise RuntimeError("model: no (seed, scale) meets the near-tie conditions")
    keep = out["seq"].shape[-1]
    print(f"model: seed {found[0]} scale {found[1]} keep {keep} min margin {margins[:keep].min():.2e}")
    loaded = model.state_dict()
    ties = [f"{a}={b}" for i, a in enumerate(names) for b in names[i + 1:] if loaded[a].data_ptr() == loaded[b].data_ptr()]
    rec = dict(meta_T=np.array(T), valid=np.array(VALID), n_gt=np.array(N_GT), seed=np.array(found[0]),
               logit_scale=np.array(found[1]), param_names=np.array(names), param_shapes=np.array([str(shapes[k]) for k in names]),
               ties=np.array(ties if ties else ["-"]), margins=margins[:keep],
               pred_logits=out["pred_logits"], pred_boxes=out["pred_boxes"], pred_count=out["pred_count"], seq=out["seq"],
               cap_prob_eval=out["caption_probs"]["cap_prob_eval"])
    for k, v in loss.items():
        rec[f"loss.{k}"] = torch.as_tensor(v)

    class _Tr:
        @staticmethod
        def rtranslate(s):
            return " ".join(str(int(x)) for x in s if x > 0)
    loader = type("L", (), {"dataset": type("D", (), {"translator": _Tr})})
    with torch.no_grad():
        res = MG.post["bbox"](out, dt["video_length"][:, 1], loader)
    for i, r in enumerate(res):
        for k in ("scores", "labels", "boxes", "query_id", "raw_idx", "pred_seq_len"):
            rec[f"post.{i}.{k}"] = r[k]
        rec[f"post.{i}.caption_scores"] = np.asarray(r["caption_scores"], np.float64)
        rec[f"post.{i}.captions"] = np.array(r["captions"])

    # a dropout-0 training forward / backward on make_train's batch form, same weights
    over.update(transformer_dropout_prob=0.0, drop_prob=0.0)
    opt, model, criterion, cc = MG.build_pdvc(overrides=over)
    model.load_state_dict(sd, strict=True)
    model.train()
    g = torch.Generator().manual_seed(11)
    cap_len = 7
    caps = torch.randint(1, opt.vocab_size, (sum(N_GT), cap_len), generator=g)
    caps[:, 0] = 0
    caps[:, -1] = 0
    caps[1, 4:] = 0
    cap_mask = (torch.arange(cap_len)[None] <= (caps != 0).sum(1)[:, None]).float()
    dt = MG.synth_dt(B, T, opt.feature_dim, valid=VALID, n_gt=N_GT)
    dt.update(cap_tensor=caps, cap_mask=cap_mask, gt_boxes_mask=torch.tensor([[1, 1, 1], [1, 1, 0]]).bool(),
              gt_gather_idx=torch.tensor([0, 0, 0, 1, 1]))
    with MG.cuda_semantics():
        out_t, loss_t = model(dt, criterion, cc, "queries")
        wd = criterion.weight_dict
        final = sum(loss_t[k] * wd[k] for k in loss_t.keys() if k in wd)
        final.backward()
    params = dict(model.named_parameters())
    gn = sorted(n for n, p_ in params.items() if p_.grad is not None)
    rec.update(cap_tensor=caps, cap_mask=cap_mask, final_loss=final.detach(), grad_names=np.array(gn),
               grad_norms=torch.stack([params[n].grad.double().norm() for n in gn]))
    for k, v in loss_t.items():
        rec[f"train_loss.{k}"] = torch.as_tensor(v).detach()
    for n in gn:
        rec["grad." + n] = R.grad_sample(params[n].grad)[::4]
    for i, (a, b) in enumerate(out_t["matched_indices"][0]):
        rec[f"match_{i}"] = torch.stack([a, b])
    MG.save("pdvc_transformer_cap", **rec)


if __name__ == "__main__":
    what = [a for a in sys.argv[1:] if not a.startswith("-")]
    if not what or "head" in what:
        make_head([a for a in what if a in R.HEAD_CASES] or None)
    if not what or "model" in what:
        make_model()

#!/usr/bin/env python3
"""What the contrastive branch costs at cfg A dimensions (B = 16, Q = 300, T = 100, 160 sentences of 20 words, text width 768),
with gvl_amd.text.PrecomputedTextEncoder:

  1. eager eval forward and eager train step with the branch on, against the same model with enable_contrastive=False;
  2. both again with the criterion forced onto its PyTorch formulation (ContrastiveCriterion.force_torch) -- kernels and
     formulation alternate in ONE process on ONE device, never a run against itself;
  3. the three kernels' own durations from the library's per-dispatch stamps.

Medians over --reps timed calls after --warmup, every timed call bracketed by device synchronisation; the shader clock
(gvl_clock_probe) is printed beside each block.  Writes profiles/contrastive_timing.txt.  Nothing is gated on these numbers.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contrastive_timing.txt"))
    a = ap.parse_args()
    import bench
    from gvl_amd import MultiScaleDeformableAttention as MSDA
    from gvl_amd.config import make_opt
    from gvl_amd.parallel import TrainStep
    from gvl_amd.pdvc import build
    dev = torch.device("cuda:0")
    B, Q, T, per_video, words, width = 16, 300, 100, 10, 20, 768
    lines = [f"contrastive branch at B={B} Q={Q} T={T}, {B * per_video} sentences of {words} words, text width {width}; "
             f"median [min .. max] ms over {a.reps} calls, {a.rounds} alternating rounds"]

    def make(contrastive):
        opt = make_opt("anet_tsp_ssvg", num_queries=Q, enable_contrastive=contrastive, text_feature_dim=width,
                       contrastive_loss_start_coef=0.1, enable_e2t_cl=contrastive, enable_bg_for_cl=contrastive)
        torch.manual_seed(0)
        model, crit, cc, _ = build(opt)
        return opt, model.to(dev), crit, cc

    dt = bench.synth_batch(B, T, 512, 8517, per_video, dev)
    g = torch.Generator().manual_seed(2)
    dt["text_encoder_input"] = {"last_hidden_state": torch.randn(B * per_video, words, width, generator=g).to(dev),
                                "attention_mask": torch.ones(B * per_video, words, device=dev)}
    runs = {}
    for label, contrastive in (("branch off", False), ("branch on", True)):
        opt, model, crit, cc = make(contrastive)
        step = TrainStep(model, crit, opt, contrastive_criterion=cc)

        def ev():
            model.eval()
            with torch.no_grad():
                model(dt, crit, cc, "queries", eval_mode=True)

        def tr():
            model.train()
            step(dt)
        runs[label] = (ev, tr, cc)
    order = [("branch off", False), ("branch on", False), ("branch on", True)]
    res = {}
    for r in range(a.rounds):
        for label, force in order:
            ev, tr, cc = runs[label]
            if cc is not None:
                cc.force_torch = force
            name = label + (", PyTorch formulation" if force else ", kernels" if cc is not None else "")
            mhz = MSDA.clock_probe_mhz(dev)
            res.setdefault(name, []).append((timed(ev, a.reps, a.warmup), timed(tr, a.reps, a.warmup), mhz))
    for name, rows in res.items():
        for r, (e_, t_, mhz) in enumerate(rows):
            lines.append(f"  {name:38s} round {r}: eval {e_[0]:7.3f} [{e_[1]:.3f} .. {e_[2]:.3f}]   train {t_[0]:7.3f} "
                         f"[{t_[1]:.3f} .. {t_[2]:.3f}]   clock {mhz:.0f} MHz")
    # the kernels' own durations
    ev, tr, cc = runs["branch on"]
    cc.force_torch = False
    MSDA.profile_enable(2)
    try:
        MSDA.profile_collect()
        for _ in range(10):
            tr()
        torch.cuda.synchronize()
        stamps = [e for e in MSDA.profile_collect() if e[0].startswith("cl_")]
    finally:
        MSDA.profile_enable(0)
    for tag in ("cl_logits", "cl_loss_fwd", "cl_loss_bwd"):
        us = [e[3] for e in stamps if e[0] == tag]
        if us:
            lines.append(f"  kernel {tag:12s} {len(us)} launches in 10 train steps: median {statistics.median(us):.1f} us "
                         f"[{min(us):.1f} .. {max(us):.1f}]")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

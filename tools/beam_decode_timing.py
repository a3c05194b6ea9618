"""Time the captioner's beam search beside the greedy decode, in one process on one GPU:

  * one eval forward at cfg A (B = 16, Q = 300, 100 frames, max_caption_len = 30) with beam_size 1 and with beam_size W, the
    token loop replayed from a hipGraph (caption head's graph_decode) -- alternating, median of --reps;
  * the same forward with captioning disabled, so that (forward - that) / max_caption_len is the time of one token;
  * gvl_beam_step_f32 alone on n W rows of random logits (row stride padded to 16 bytes): time per launch and the share of
    8 TB/s its n W (V + 1) 4 bytes of logits amount to.

    python tools/beam_decode_timing.py [--beam 3] [--reps 7] [--out profiles/beam_decode.txt]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 8e12


def timed(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--beam", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--queries", type=int, default=300)
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from bench import synth_batch
    from gvl_amd import MultiScaleDeformableAttention as MSDA
    from gvl_amd.config import make_opt
    from gvl_amd.pdvc import build
    from gvl_amd.tuning import enable_tuned_gemms
    enable_tuned_gemms()
    dev = torch.device("cuda", 0)
    opt = make_opt("anet_tsp_ssvg", num_queries=a.queries, frame_embedding_num=a.T, device="cuda")
    torch.manual_seed(0)
    model, _, _, _ = build(opt)
    model = model.to(dev).eval()
    dt = synth_batch(a.batch, a.T, opt.feature_dim, opt.vocab_size, 3, dev)
    for head in model.caption_head:
        head.graph_decode = True
    W, L = a.beam, opt.max_caption_len

    def forward(beam, captioning=True):
        def fn():
            model.opt.beam_size, model.opt.eval_disable_captioning = beam, not captioning
            with torch.no_grad():
                model(dt, None, None, "queries", eval_mode=True)
        return fn
    variants = {"no captions": forward(1, False), "beam_size 1": forward(1), f"beam_size {W}": forward(W)}
    for fn in variants.values():                                    # captures, lazy initialisation
        fn()
        fn()
    times = {k: [] for k in variants}
    for _ in range(a.reps):                                         # alternating: drift hits every variant alike
        for k, fn in variants.items():
            times[k] += timed(fn, 1)
    med = {k: statistics.median(v) for k, v in times.items()}
    model.opt.beam_size, model.opt.eval_disable_captioning = 1, False
    lines = [f"eval forward, B = {a.batch}, Q = {a.queries}, {a.T} frames, max_caption_len = {L}, vocabulary {opt.vocab_size}; "
             f"median of {a.reps} alternating runs, ms (min .. max)"]
    for k, v in times.items():
        lines.append(f"  {k:14s} {med[k]:8.3f}  ({min(v):.3f} .. {max(v):.3f})")
    tok1 = (med["beam_size 1"] - med["no captions"]) / L
    tokw = (med[f"beam_size {W}"] - med["no captions"]) / L
    lines.append(f"  per token: greedy {1e3 * tok1:.1f} us, beam_size {W} {1e3 * tokw:.1f} us ({tokw / tok1:.2f} x)")

    n, V1, H = a.batch * a.queries, opt.vocab_size + 1, opt.rnn_size
    ld = (V1 + 3) // 4 * 4
    g = torch.Generator(device=dev).manual_seed(0)
    logits = torch.randn(n * W, ld, device=dev, generator=g)[:, :V1]
    score = -torch.rand(n, W, device=dev, generator=g)
    fin = torch.zeros(n, W, dtype=torch.uint8, device=dev)
    h, c = torch.randn(n * W, H, device=dev, generator=g), torch.randn(n * W, H, device=dev, generator=g)
    outs = (torch.empty_like(score), torch.empty_like(fin), torch.empty(n, W, dtype=torch.int32, device=dev),
            torch.empty(n, W, dtype=torch.long, device=dev), torch.empty_like(score), torch.zeros(1, dtype=torch.int32, device=dev),
            torch.empty_like(h), torch.empty_like(c))
    step = lambda: MSDA.beam_step(logits, score, fin, h, c, *outs)   # noqa: E731
    for _ in range(3):
        step()
    per = statistics.median(timed(lambda: [step() for _ in range(20)], a.reps)) / 20
    nbytes = n * W * V1 * 4
    floor = nbytes / HBM_BYTES_PER_S * 1e3
    lines.append(f"gvl_beam_step_f32 alone, n = {n}, W = {W}, V + 1 = {V1}, H = {H}: {1e3 * per:.1f} us per launch; its "
                 f"{nbytes / 1e6:.0f} MB of logits at 8 TB/s are {1e3 * floor:.1f} us ({100 * floor / per:.0f} % of that rate)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

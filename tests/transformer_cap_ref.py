"""Host side of the Transformer-DSA caption head's tests: the fp64 restatement of one cached self-attention step
(gvl_amd/csrc/gvl_cap_tr.hip: k_capt_attend), full causal attention in one shot to hold it against, and the shapes / seeded inputs
that tests/golden/make_golden_transformer_cap.py and the GPU tests share (the fixtures hold outputs and name / shape lists only)."""
import argparse
import math

import numpy as np
import torch

from synth import synth_array, level_lengths

LOGPROB_TOL = 5e-4                   # tests/test_gpu_model.py: log-probs of the greedy captions
LOSS_TOL = 1e-3                      # ... loss terms of a training step
GRAD_TOL = 2e-3                      # ... gradients, relative to max(1, the gradient's scale)
STRICT_MARGIN = 10 * LOGPROB_TOL     # a row is strict when its smallest top-2 log-prob margin over all steps is at least this
GRAD_SAMPLES = 1024


# ---- one cached attention step, fp64 -----------------------------------------------------------------------------------------------
def embed_ref(embed, pos_table, it, t):
    """x[r] = embed[it[r]] + pos_table[t] (rows beyond the table stay zero), fp64 -> (x, max |x[r]|)"""
    x = embed.double()[it]
    if t < pos_table.shape[0]:
        x = x + pos_table.double()[t]
    return x, x.abs().amax(1)


def cached_attention_step(qkv, x, cache, t, H, weight, bias, eps):
    """append k_t, v_t at position t of cache (2, n, positions, C), attend q_t over positions 0..t per head at scale 1 / sqrt(D),
    add the residual x, LayerNorm -> y (n, C).  Everything in the dtype of the inputs (the tests pass fp64)."""
    n, C = x.shape
    D = C // H
    q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    cache[0, :, t] = k
    cache[1, :, t] = v
    keys = cache[0, :, :t + 1].reshape(n, t + 1, H, D)
    vals = cache[1, :, :t + 1].reshape(n, t + 1, H, D)
    scores = torch.einsum("nhd,nphd->nhp", q.reshape(n, H, D), keys) / math.sqrt(D)
    ctx = torch.einsum("nhp,nphd->nhd", torch.softmax(scores, -1), vals).reshape(n, C)
    return torch.nn.functional.layer_norm(x + ctx, (C,), weight, bias, eps)


def full_causal_attention(qkv_all, x_all, H, weight, bias, eps):
    """qkv_all (n, L, 3C), x_all (n, L, C): causal self-attention over all L positions at once (the additive -10000 mask of
    Transformer_DSA.py:39), residual, LayerNorm -> (n, L, C)"""
    n, L, C = x_all.shape
    D = C // H
    q, k, v = (qkv_all[..., i * C:(i + 1) * C].reshape(n, L, H, D).transpose(1, 2) for i in range(3))
    mask = (1.0 - torch.ones(L, L, dtype=x_all.dtype).tril()) * -10000.0
    probs = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(D) + mask, -1)
    ctx = (probs @ v).transpose(1, 2).reshape(n, L, C)
    return torch.nn.functional.layer_norm(x_all + ctx, (C,), weight, bias, eps)


# ---- the head-level cases of the fixtures ------------------------------------------------------------------------------------------
# name -> C, heads, layers, vocabulary, videos, queries, max_caption_len, teacher-forced length (a6: 9 positions against a table of
# 8 rows -- the rows beyond the table stay zero, Transformer_DSA.py:203-206)
HEAD_CASES = {
    "a6": dict(C=128, H=2, layers=2, V=40, B=2, Q=3, T=6, Lc=9),
    "a34": dict(C=128, H=2, layers=2, V=40, B=2, Q=3, T=34, Lc=12),
    "b": dict(C=512, H=8, layers=1, V=60, B=2, Q=5, T=6, Lc=7),
}
FRAMES = 20


def head_opt(case, **over):
    c = HEAD_CASES[case] if isinstance(case, str) else case
    o = dict(vocab_size=c["V"], input_encoding_size=c["C"], hidden_dim=c["C"], num_layers=c["layers"], drop_prob=0.0,
             max_caption_len=c["T"], cap_num_feature_levels=4, cap_nheads=c["H"], cap_dec_n_points=4, num_feature_levels=4,
             caption_decoder_type="transformer")
    o.update(over)
    return argparse.Namespace(**o)


def head_inputs(case, seed=1):
    """seeded inputs of a head case: video 1 has a masked memory tail on every level and valid ratios below one"""
    c = HEAD_CASES[case]
    B, Q, C, Lc, V = c["B"], c["Q"], c["C"], c["Lc"], c["V"]
    lens = level_lengths(FRAMES)
    S = sum(lens)
    tshapes = torch.tensor(lens, dtype=torch.long)
    lsi = torch.cat([tshapes.new_zeros(1), tshapes.cumsum(0)[:-1]])
    tag = "trcap." + case
    hs = torch.from_numpy(synth_array(tag + ".hs", (B, Q, C), seed))
    memory = torch.from_numpy(synth_array(tag + ".memory", (B, S, C), seed))
    ref = torch.from_numpy(synth_array(tag + ".ref", (B, Q, 2), seed, 0.05, 0.95))
    ref[..., 1] *= 0.5
    mask = torch.zeros(B, S, dtype=torch.bool)
    vr = torch.ones(B, len(lens))
    for l_, (s0, n_) in enumerate(zip(lsi.tolist(), lens)):
        keep = max(1, (2 * n_) // 3)
        mask[1, s0 + keep:s0 + n_] = True
        vr[1, l_] = keep / n_
    rs = np.random.RandomState(seed + 17)
    n = B * Q
    seq = torch.from_numpy(rs.randint(1, V + 1, size=(n, Lc)).astype(np.int64))
    seq[:, 0] = 0
    lengths = rs.randint(2, Lc - 1, size=n)                    # words per caption; <pad> behind them
    lengths[0] = Lc - 2
    for r, k in enumerate(lengths):
        seq[r, 1 + k:] = 0
    cap_mask = (torch.arange(Lc)[None] <= torch.from_numpy(lengths)[:, None] + 1).float()
    gout = torch.from_numpy(synth_array(tag + ".gout", (n, Lc, V + 1), seed))
    others = {"memory": memory, "spatial_shapes": tshapes, "level_start_index": lsi, "mask_flatten": mask, "valid_ratios": vr}
    return dict(hs=hs, reference=ref, others=others, seq=seq, cap_mask=cap_mask, gout=gout, lens=lens)


def grad_sample(g):
    """what the fixtures keep of a gradient: GRAD_SAMPLES evenly strided elements at most (the full tensors of the C = 512 head
    are 12 MB)"""
    flat = g.reshape(-1)
    stride = max(1, -(-flat.numel() // GRAD_SAMPLES))
    return flat[::stride]


def strict_rows(margins, keep):
    """margins (steps, n) top-2 log-prob margins of the reference's decode -> bool (n,): rows whose smallest margin over the `keep`
    returned steps is at least STRICT_MARGIN; and per row the first step below it (keep when none)"""
    m = np.asarray(margins)[:keep]
    below = m < STRICT_MARGIN
    first = np.where(below.any(0), below.argmax(0), keep)
    return ~below.any(0), first

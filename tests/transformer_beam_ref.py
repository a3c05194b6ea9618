"""Host side of the tests of the Transformer-DSA head's beam search over its KV cache: the restatement of the lineage update
(gvl_amd/csrc/gvl_beam.hip: k_beam_step_lineage), of one cached attention step read through a lineage table
(gvl_amd/csrc/gvl_cap_tr.hip: k_capt_attend<true>), and the seeded lineages the CPU and GPU tests share.

The scheme: the n W rows of a search are W consecutive beams per event, row r W + j appends the keys and
values of position t at ITS OWN slot of the cache (2, n W, P, C), and lineage[r][j][p] names the slot (0 .. W-1) of event r that
holds position p of beam j's prefix.  The cache is never re-ordered by parent beam; the table is."""
import math

import torch


def lineage_update(lin_in, parent, t):
    """lin_in (n, W, P) uint8, parent (n, W) the parent beam of every new beam, t the position the step computed -> lin_out:
    the parent's bytes in front of t, the parent itself at t, the bytes behind t untouched (returned as they were in lin_in's
    clone: a caller that checks "not written" pre-fills its own buffer and copies [..., :t + 1] of this result over it)"""
    n, W, P = lin_in.shape
    assert 0 <= t < P and parent.shape == (n, W)
    out = lin_in.clone()
    if t > 0:
        out[:, :, :t] = lin_in.gather(1, parent.long()[:, :, None].expand(n, W, P))[:, :, :t]
    out[:, :, t] = parent.to(lin_in.dtype)
    return out


def lineage_attention_step(qkv, x, cache, lineage, t, H, weight, bias, eps):
    """qkv (n W, 3C) rows [q | k | v] of position t, x (n W, C), cache (2, n W, P, C), lineage (n, W, P): row (r, j) appends k_t,
    v_t at position t of slot r W + j, attends q_t per head at scale 1 / sqrt(D) over position p < t of slot r W + lineage[r, j, p]
    and over its own position t, adds the residual x, LayerNorm -> y (n W, C).  Written with explicit loops over rows and positions
    (no gather shared with the code under test); everything in the dtype of the inputs (the tests pass fp64)."""
    R, C = x.shape
    n, W, P = lineage.shape
    D = C // H
    assert R == n * W and cache.shape == (2, R, P, C) and 0 <= t < P
    k, v = qkv[:, C:2 * C], qkv[:, 2 * C:]
    cache[0, :, t] = k
    cache[1, :, t] = v
    keys, vals = x.new_empty(R, t + 1, C), x.new_empty(R, t + 1, C)
    for r in range(n):
        for j in range(W):
            row = r * W + j
            for p in range(t):
                slot = r * W + int(lineage[r, j, p])
                keys[row, p], vals[row, p] = cache[0, slot, p], cache[1, slot, p]
            keys[row, t], vals[row, t] = k[row], v[row]
    q = qkv[:, :C].reshape(R, H, D)
    scores = torch.einsum("nhd,nphd->nhp", q, keys.view(R, t + 1, H, D)) / math.sqrt(D)
    ctx = torch.einsum("nhp,nphd->nhd", torch.softmax(scores, -1), vals.view(R, t + 1, H, D)).reshape(R, C)
    return torch.nn.functional.layer_norm(x + ctx, (C,), weight, bias, eps)


def random_lineage(n, W, P, seed):
    """valid bytes (< W), uint8 (n, W, P).  For W > 1 every aligned group of four consecutive positions names at least two different
    slots -- the four positions a wavefront's quarter-waves load together then come from different slots -- except in row (0, 0),
    which names ONE slot other than its own throughout (slot 1: a row that never reads what it wrote)."""
    g = torch.Generator().manual_seed(seed)
    lin = torch.randint(0, W, (n, W, P), generator=g, dtype=torch.int64)
    if W > 1:
        for p0 in range(0, P - 1, 4):
            same = lin[:, :, p0 + 1] == lin[:, :, p0]
            lin[:, :, p0 + 1] = torch.where(same, (lin[:, :, p0] + 1) % W, lin[:, :, p0 + 1])
        lin[0, 0, :] = 1
    return lin.to(torch.uint8)


def named_positions(lineage, t):
    """bool (n W, P): (slot, p) with p < t that some row of the slot's event reads at step t"""
    n, W, P = lineage.shape
    named = torch.zeros(n * W, P, dtype=torch.bool)
    for r in range(n):
        for j in range(W):
            for p in range(t):
                named[r * W + int(lineage[r, j, p]), p] = True
    return named

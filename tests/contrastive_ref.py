"""fp64-capable PyTorch restatement of the contrastive criterion (pdvc/criterion.py:269-373) and of the word-level attention pool
(pdvc/pdvc.py:1092-1104), written from their arithmetic: what the tests hold the kernels to.

    cos[g][e]   = <t_g / max(|t_g|, 1e-12), e_e / max(|e_e|, 1e-12)>              (row G: the background embedding)
    t2e         = mean over the matched pairs (g, e*) of  logsumexp_e(cos[g][.] / tau) - cos[g][e*] / tau
                  (per-video mode: e ranges over the pair's own video; mean per video, then over the B videos)
    e2t         = mean over events of  logsumexp over {matched texts, background}(cos[.][e] / tau) - cos[label(e)][e] / tau,
                  label(e) = the text matched to e, else the background; without enable_bg_for_cl only matched events count
    loss        = t2e, or (t2e + e2t) / 2 with enable_e2t_cl
"""
import torch


def unit_rows(x):
    return x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12)


def cosines(text, event, bg=None):
    """(G, D), (E, D)[, (1, D)] -> (G [+ 1], E)"""
    rows = text if bg is None else torch.cat([text, bg.reshape(1, -1)], dim=0)
    return unit_rows(rows) @ unit_rows(event).t()


def contrastive_loss(text, event, pair_text, pair_event, pair_video, B, Q, temperature, cross_video=True, e2t=False,
                     bg_for_cl=False, bg=None):
    """text (G, D), event (B Q, D); pair_text / pair_event / pair_video: row of the sentence, row of the event and the video of
    every matched pair -> (loss, t2e, e2t)"""
    cos = cosines(text, event)
    x = cos[pair_text] / temperature                                   # (P, E)
    P, E = x.shape
    picked = x[torch.arange(P), pair_event]
    if cross_video:
        t2e = (torch.logsumexp(x, dim=1) - picked).sum() / P
    else:
        t2e = x.new_zeros(())
        for v in range(B):
            mine = pair_video == v
            lse = torch.logsumexp(x[mine][:, v * Q:(v + 1) * Q], dim=1)
            t2e = t2e + (lse - picked[mine]).sum() / mine.sum()
        t2e = t2e / B
    if not e2t:
        return t2e, t2e, x.new_zeros(())
    bg_row = (unit_rows(event) @ unit_rows(bg.reshape(1, -1)).t()).t() / temperature          # (1, E)
    y = torch.cat([x, bg_row], dim=0)                                   # (P + 1, E)
    label = torch.full((E,), P, dtype=torch.long)
    for p in range(P - 1, -1, -1):
        label[pair_event[p]] = p
    per_event = torch.logsumexp(y, dim=0) - y[label, torch.arange(E)]
    if bg_for_cl:
        e2t_loss = per_event.sum() / E
    else:
        keep = label < P
        e2t_loss = per_event[keep].sum() / keep.sum()
    return 0.5 * (t2e + e2t_loss), t2e, e2t_loss


def word_attention_pool(x, mask, w1, b1, w2, b2):
    """x (S, W, H), mask (S, W) -> (S, H): softmax over the words of w2 . gelu(w1 x + b1) + b2, padded words at -10000"""
    m = mask.to(x.dtype)[..., None]
    score = (torch.nn.functional.gelu(x @ w1.t() + b1) @ w2.t() + b2) * m - 10000 * (1 - m)
    return (torch.softmax(score, dim=1) * x).sum(dim=1)

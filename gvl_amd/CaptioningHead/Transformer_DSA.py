"""Transformer captioner with deformable cross-attention -- mirror of pdvc/CaptioningHead/Transformer_DSA.py
(``caption_decoder_type: transformer``).

Parameter names follow the reference (``embed, logits, pos_table``; per layer ``self_attention.{query,key,value}, norm1..3,
dim_project, cross_attention.*, linear1, linear2``), so its checkpoints load with ``strict=True``.  The reference's
``BertSelfAttention`` is three ``nn.Linear``s and a dropout on the attention probabilities; it has no output projection, and
``transformers`` is not imported here.  One layer on rows x (n, L, C), n = videos x queries (Transformer_DSA.py:89-113):

    x = norm1(x + dropout1(softmax(q k^T / sqrt(D) + causal mask) v))        q, k, v = query(x), key(x), value(x) per head
    z = dim_project([x | hs])                                               hs: the event feature of the row, same for every position
    x = norm2(z + dropout2(MSDeformAttn(z, ref, memory)))
    x = norm3(x + dropout4(linear2(dropout3(relu(linear1(x))))))

What is restructured for the GPU (results equal up to fp32 rounding):
  * the cross-attention runs with Len_q = queries x positions per VIDEO against the un-replicated memory (the reference copies the
    memory and its mask once per query and layer call, :100-101, and attends with Len_q = positions);
  * greedy decoding keeps a key / value cache per layer.  The head is strictly causal (the mask of :208 and nothing else mixes
    positions), so position t of a layer depends on positions 0..t of the layer below only: a token costs ONE new position per row,
    where the reference runs the whole prefix through every layer again for each token (:226-238);
  * value_proj(memory) and the event-feature half of dim_project do not depend on the token: once per decode;
  * the loop runs without a per-step device->host read (the reference tests ``unfinished.sum() == 0`` every step, :246); the
    all-finished cut is applied once at the end, as in the LSTM-DSA head.
  * beam search (beam_size > 1) runs on the same cache without ever re-ordering it by parent beam: every beam appends at its own
    slot, the kernel that selects the beams re-orders a byte table of lineages (MSDA.beam_step_lineage), and the attention reads each
    earlier position from the slot the lineage names (attend_step_beam): DESIGN.md section 10.
The decode's new kernels are gvl_amd/csrc/gvl_cap_tr.hip (embed_step, attend_step below); everything else on the token path is the
split-fp16 Linear / LayerNorm / deformable-attention launches of gvl_amd/layers.py and the fused vocabulary argmax of the LSTM head.
Teacher forcing (forward) keeps the self-attention and the dropouts on PyTorch ops: DESIGN.md section 10.
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import MultiScaleDeformableAttention as MSDA
from .. import _lib
from ..linear import split_gemm_enabled
from ..ops.functions import MSDeformAttnFunction
from ..ops.modules import MSDeformAttn
from ..ops.modules.ms_deform_attn import temporal_shapes_2d
from .decoding import BeamBooks, DecodingHead, _fp32_island, zero_views


# ---- the two kernels of the token step -----------------------------------------------------------------------------------------
def embed_step(embed_weight, pos_table, it, t):
    """x[r] = embed_weight[it[r]] + pos_table[t] (rows beyond the table: the embedding alone) -> (x (n, C), max |x[r]| (n,))
    (include/gvl_msda.h: gvl_capt_embed_f32)"""
    n, C = it.shape[0], embed_weight.shape[1]
    if not (embed_weight.is_cuda and embed_weight.dtype == torch.float32 and embed_weight.is_contiguous()
            and pos_table.dtype == torch.float32 and pos_table.is_contiguous() and pos_table.shape[1] == C
            and it.dtype == torch.int64 and it.is_contiguous() and C % 4 == 0):
        raise ValueError("embed_step: needs contiguous fp32 CUDA tables of C % 4 == 0 columns and contiguous int64 ids")
    x = torch.empty(n, C, device=it.device, dtype=torch.float32)
    am = torch.empty(n, device=it.device, dtype=torch.float32)
    with torch.cuda.device(it.device):
        rc = _lib.lib().gvl_capt_embed_f32(embed_weight.data_ptr(), embed_weight.shape[0], pos_table.data_ptr(), pos_table.shape[0],
                                           it.data_ptr(), int(t), n, C, x.data_ptr(), am.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "capt_embed")
    return x, am


def attend_beam_kernel_eligible(qkv, x, cache, lineage, H):
    """domain of gvl_capt_attend_f32 (lineage None): fp32 on the device, head dimension 64, H <= 8, at most 64 cached positions; of
    gvl_capt_attend_beam_f32: that, a contiguous uint8 lineage table and at most 8 beams"""
    C = x.shape[1]
    if not (x.is_cuda and qkv.dtype == x.dtype == cache.dtype == torch.float32 and C % H == 0 and qkv.stride(1) == 1
            and x.stride(1) == 1 and qkv.stride(0) % 4 == 0 and x.stride(0) % 4 == 0 and cache.is_contiguous()
            and qkv.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0):
        return False
    if lineage is None:
        return bool(_lib.lib().gvl_capt_attend_applicable(H, C // H, cache.shape[2]))
    return bool(lineage.is_contiguous() and _lib.lib().gvl_capt_attend_beam_applicable(H, C // H, cache.shape[2], lineage.shape[1]))


def attend_kernel_eligible(qkv, x, cache, H):
    """domain of gvl_capt_attend_f32"""
    return attend_beam_kernel_eligible(qkv, x, cache, None, H)


def attend_step_torch(qkv, x, cache, t, H, weight, bias, eps):
    """the PyTorch formulation of attend_step, on the same cache"""
    n, C = x.shape
    D = C // H
    q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:3 * C]
    cache[0, :, t] = k
    cache[1, :, t] = v
    keys = cache[0, :, :t + 1].view(n, t + 1, H, D)
    vals = cache[1, :, :t + 1].view(n, t + 1, H, D)
    scores = torch.einsum("nhd,nphd->nhp", q.reshape(n, H, D), keys) / math.sqrt(D)
    ctx = torch.einsum("nhp,nphd->nhd", torch.softmax(scores, -1), vals).reshape(n, C)
    return F.layer_norm(x + ctx, (C,), weight, bias, eps)


def attend_step(qkv, x, cache, t, H, weight, bias, eps, want_amax=False):
    """One cached self-attention step (Transformer_DSA.py:95-99 for the newest position): qkv (n, 3C) rows [q | k | v] of position
    t, x (n, C) the residual rows, cache (2, n, positions, C) with positions [0, t) filled.  Writes k, v into row t of the cache
    (nothing else of it), attends over positions 0..t per head at scale 1 / sqrt(D), adds the residual and applies the LayerNorm
    (weight, bias, eps) -> (y (n, C), max |y[r]| (n,) or None).  gvl_capt_attend_f32 where it applies (attend_kernel_eligible),
    the PyTorch formulation of the same step otherwise."""
    return attend_step_beam(qkv, x, cache, None, t, H, weight, bias, eps, want_amax=want_amax)


def attend_step_beam_torch(qkv, x, cache, lineage, t, H, weight, bias, eps):
    """the PyTorch formulation of attend_step_beam, on the same cache: the prefix gathered by lineage, the same single write"""
    R, C = x.shape
    n, W, _ = lineage.shape
    D = C // H
    q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:3 * C]
    cache[0, :, t] = k
    cache[1, :, t] = v
    slot = (torch.arange(n, device=x.device)[:, None, None] * W + lineage[:, :, :t].long().clamp(max=W - 1)).view(R, t)
    pos = torch.arange(t, device=x.device)[None].expand(R, t)
    keys = torch.cat([cache[0][slot, pos], k[:, None]], 1).view(R, t + 1, H, D)
    vals = torch.cat([cache[1][slot, pos], v[:, None]], 1).view(R, t + 1, H, D)
    scores = torch.einsum("nhd,nphd->nhp", q.reshape(R, H, D), keys) / math.sqrt(D)
    ctx = torch.einsum("nhp,nphd->nhd", torch.softmax(scores, -1), vals).reshape(R, C)
    return F.layer_norm(x + ctx, (C,), weight, bias, eps)


def attend_step_beam(qkv, x, cache, lineage, t, H, weight, bias, eps, want_amax=False):
    """attend_step for beam search: the n W rows are W consecutive beams per event, cache (2, n W, positions, C), lineage
    (n, W, positions) uint8.  Row (r, j) writes k, v at position t of its own slot r W + j (nothing else of the cache is written) and
    attends over position p < t of slot r W + lineage[r, j, p] and over its own position t -- the cache is never re-ordered by
    parent beam, the table is (MSDA.beam_step_lineage).  Nothing at or behind t is read, of the cache or of the table; a byte above
    W - 1 is read as W - 1.  gvl_capt_attend_beam_f32 where it applies, the PyTorch formulation of the same step otherwise.
    lineage None: the plain step (attend_step) -- one body for both."""
    R, C = x.shape
    P = cache.shape[2]
    assert qkv.shape == (R, 3 * C) and cache.shape == (2, R, P, C) and 0 <= t < P
    if lineage is not None:
        n, W, _ = lineage.shape
        assert R == n * W and lineage.shape[2] == P and lineage.dtype == torch.uint8
    if attend_beam_kernel_eligible(qkv, x, cache, lineage, H):
        y = torch.empty(R, C, device=x.device, dtype=torch.float32)
        am = torch.empty(R, device=x.device, dtype=torch.float32) if want_amax else None
        tail = (int(t), H, weight.data_ptr(), bias.data_ptr(), float(eps), y.data_ptr(), am.data_ptr() if am is not None else None)
        with torch.cuda.device(x.device):
            stream = torch.cuda.current_stream().cuda_stream
            if lineage is None:
                rc = _lib.lib().gvl_capt_attend_f32(qkv.data_ptr(), qkv.stride(0), x.data_ptr(), x.stride(0), cache.data_ptr(), R,
                                                    P, *tail, stream)
            else:
                rc = _lib.lib().gvl_capt_attend_beam_f32(qkv.data_ptr(), qkv.stride(0), x.data_ptr(), x.stride(0), cache.data_ptr(),
                                                         lineage.data_ptr(), n, W, P, *tail, stream)
        _lib.check(rc, "capt_attend" if lineage is None else "capt_attend_beam")
        return y, am
    if lineage is None:
        y = attend_step_torch(qkv, x, cache, t, H, weight, bias, eps)
    else:
        y = attend_step_beam_torch(qkv, x, cache, lineage, t, H, weight, bias, eps)
    if want_amax:
        from .. import layers as L
        return y, L.row_absmax(y)[0]
    return y, None


# ---- modules ----------------------------------------------------------------------------------------------------------------------
class _SelfAttention(nn.Module):
    """the parameters (and the one dropout) of transformers' BertSelfAttention as the reference configures it"""

    def __init__(self, d_model, n_heads, dropout):
        super().__init__()
        if d_model % n_heads != 0:
            raise ValueError(f"The hidden size ({d_model}) is not a multiple of the number of attention heads ({n_heads})")
        self.num_attention_heads = n_heads
        self.attention_head_size = d_model // n_heads
        self.query = nn.Linear(d_model, d_model)
        self.key = nn.Linear(d_model, d_model)
        self.value = nn.Linear(d_model, d_model)
        self.dropout = nn.Dropout(dropout)

    def forward(self, x, attention_mask):
        """x (n, L, C), attention_mask additive, broadcastable to (n, H, L, L) -> context (n, L, C)"""
        n, L_, C = x.shape
        H, D = self.num_attention_heads, self.attention_head_size
        q = self.query(x).view(n, L_, H, D).transpose(1, 2)
        k = self.key(x).view(n, L_, H, D).transpose(1, 2)
        v = self.value(x).view(n, L_, H, D).transpose(1, 2)
        scores = torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(D) + attention_mask
        probs = self.dropout(F.softmax(scores, dim=-1))
        return torch.matmul(probs, v).transpose(1, 2).reshape(n, L_, C)


class TransformerDSACapLayer(nn.Module):
    def __init__(self, d_model, d_ffn=1024, dropout=0.1, n_heads=8, n_levels=4, n_points=4, activation='relu', im2col_step=500):
        super().__init__()
        if activation != 'relu':
            raise ValueError("gvl_amd's Transformer-DSA layer is built with activation='relu' (as the reference constructs it)")
        self.self_attention = _SelfAttention(d_model, n_heads, dropout)
        self.dropout1 = nn.Dropout(dropout)
        self.norm1 = nn.LayerNorm(d_model)
        self.dim_project = nn.Linear(2 * d_model, d_model)
        self.cross_attention = MSDeformAttn(d_model, n_levels, n_heads, n_points, im2col_step)
        self.dropout2 = nn.Dropout(dropout)
        self.norm2 = nn.LayerNorm(d_model)
        self.linear1 = nn.Linear(d_model, d_ffn)
        self.activation = F.relu
        self.dropout3 = nn.Dropout(dropout)
        self.linear2 = nn.Linear(d_ffn, d_model)
        self.dropout4 = nn.Dropout(dropout)
        self.norm3 = nn.LayerNorm(d_model)

    def forward_ffn(self, x):
        return self.norm3(x + self.dropout4(self.linear2(self.dropout3(self.activation(self.linear1(x))))))

    def forward(self, hidden_states, query, reference_points, input_flatten, input_spatial_shapes, input_level_start_index,
                input_padding_mask, attention_mask):
        """hidden_states (N_ * pairs, L, C); query (N_, pairs, C); reference_points (N_, pairs, levels, 1|2), already scaled by the
        valid ratios; input_flatten (N_, S, C) -- never repeated per query (Transformer_DSA.py:89-113)"""
        N_, pairs, C = query.shape
        n, L_, _ = hidden_states.shape
        x = self.norm1(hidden_states + self.dropout1(self.self_attention(hidden_states, attention_mask)))
        z = self.dim_project(torch.cat([x, query.reshape(n, 1, C).expand(n, L_, C)], -1))
        ref = reference_points[:, :, None].expand(N_, pairs, L_, *reference_points.shape[2:])
        ca = self.cross_attention(z.view(N_, pairs * L_, C), ref.reshape(N_, pairs * L_, *reference_points.shape[2:]),
                                  input_flatten, input_spatial_shapes, input_level_start_index, input_padding_mask)
        x = self.norm2(z + self.dropout2(ca.view(n, L_, C)))
        return self.forward_ffn(x)


class TransformerDSACaptioner(DecodingHead):
    _reference_line = "Transformer_DSA.py:196, as LSTM_DSA.py:151"

    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        o = vars(opt)
        if o.get('enable_pos_emb_for_captioner', False):
            raise ValueError("enable_pos_emb_for_captioner with caption_decoder_type='transformer': the head's dim_project is "
                             "2 * hidden_dim wide and the reference itself fails on the 3 * hidden_dim input (Transformer_DSA.py:68,104)")
        if opt.hidden_dim != opt.input_encoding_size:
            raise ValueError(f"caption_decoder_type='transformer' needs hidden_dim == input_encoding_size (got {opt.hidden_dim} and "
                             f"{opt.input_encoding_size}): the token embeddings are the layers' input rows")
        self.vocab_size = opt.vocab_size
        self.input_encoding_size = opt.input_encoding_size
        self.hidden_size = opt.hidden_dim
        self.num_layers = opt.num_layers
        self.drop_prob_lm = opt.drop_prob
        self.max_caption_len = opt.max_caption_len
        self.n_levels = opt.cap_num_feature_levels
        self.n_heads = opt.cap_nheads
        self.n_points = opt.cap_dec_n_points
        self.embed = nn.Embedding(self.vocab_size + 1, self.input_encoding_size)
        self.register_buffer('pos_table', self._get_sin_encoding_table(self.max_caption_len + 2, self.input_encoding_size))
        self.layers = nn.ModuleList([TransformerDSACapLayer(d_model=self.hidden_size, n_heads=self.n_heads, n_levels=self.n_levels,
                                                            n_points=self.n_points, dropout=self.drop_prob_lm, activation='relu')
                                     for _ in range(self.num_layers)])
        self.lm_dropout = nn.Dropout(self.drop_prob_lm)
        self.logits = nn.Linear(self.hidden_size, self.vocab_size + 1)

    def init_weights(self):
        pass

    @staticmethod
    def _get_sin_encoding_table(max_len, hidden_dim):
        """sinusoid position table (1, max_len, hidden_dim)   (Transformer_DSA.py:154-162)"""
        table = torch.zeros(max_len, hidden_dim).float()
        pos = torch.arange(0, max_len).float().unsqueeze(1)
        div_term = (torch.arange(0, hidden_dim, 2).float() * -(math.log(10000.0) / hidden_dim)).exp()
        table[:, 0::2] = torch.sin(pos * div_term)
        table[:, 1::2] = torch.cos(pos * div_term)
        return table.unsqueeze(0)

    def _vocab_layer(self):
        return self.logits

    def build_loss(self, input, target, mask):
        """Transformer_DSA.py:165-170: the last position predicts nothing and is dropped"""
        return self._masked_row_nll(input[:, :-1, :], target, mask)

    @_fp32_island
    def forward(self, hs, reference, others, seq, steps=None):
        """Teacher-forced log-probs (Transformer_DSA.py:173-213) -> (N_ * pairs, positions, vocab + 1).
        steps: the caller knows that the masked loss reads the first `steps` positions only (PDVC.caption_prediction: the longest
        caption of the batch); positions [0, steps] are then computed -- build_loss drops the last one -- instead of all of
        seq.size(1).  The head is causal, so the positions kept are unchanged, and so are loss and gradients."""
        seq = seq.long()
        if steps is not None:
            seq = seq[:, :min(int(steps) + 1, seq.size(1))]
        ref_in = self._scaled_reference(reference, others)
        memory, tshapes, lsi, mask = self._level_inputs(others)
        x = self.embed(seq)
        L_ = x.size(1)
        # :203-206: rows beyond the table stay zero
        pos = x.new_zeros((L_, x.size(2)))
        rows = min(L_, self.pos_table.shape[1])
        pos[:rows] = self.pos_table[0, :rows]
        x = x + pos
        causal = (1.0 - x.new_ones(L_, L_).tril()) * -10000.0                 # :208-209, 39: one (L, L) matrix for every row and head
        for layer in self.layers:
            x = layer(x, hs, ref_in, memory, tshapes, lsi, mask, causal)
        return F.log_softmax(self.logits(self.lm_dropout(x)), dim=-1)

    # ---- greedy decoding over a KV cache -------------------------------------------------------------------------------------------
    def _layers_ok(self, hs, memory, tshapes):
        """whether the token step runs on the inference layers of gvl_amd/layers.py (split-fp16 Linear with fused epilogues, LayerNorm,
        fused deformable attention); otherwise the same step on PyTorch's Linear / LayerNorm, still cached"""
        from .. import layers as L
        C = self.hidden_size
        host = getattr(tshapes, "_gvl_host_lengths", None)
        if not (L.enabled() and L._plain(hs) and L._plain(memory) and not self.training and split_gemm_enabled()
                and hs.is_contiguous() and C % 64 == 0 and C <= 1024 and memory.shape[-1] == C and len(self.layers) > 0):
            return False
        return all(L._attn_ok(l_.cross_attention, host, memory.shape[1]) and l_.linear1.out_features % 64 == 0 for l_ in self.layers)

    def _torch_weights(self):
        """[query; key; value] of every layer as one matrix, for the PyTorch form of the token step: per parameter version"""
        ps = [p_ for l_ in self.layers for m_ in (l_.self_attention.query, l_.self_attention.key, l_.self_attention.value)
              for p_ in (m_.weight, m_.bias)]
        key = tuple((p_.data_ptr(), p_._version) for p_ in ps)
        cached = self.__dict__.get("_qkv_w")
        if cached is None or cached[0] != key:
            with torch.no_grad():
                ws = [(torch.cat([sa.query.weight, sa.key.weight, sa.value.weight], 0),
                       torch.cat([sa.query.bias, sa.key.bias, sa.value.bias], 0)) for sa in (l_.self_attention for l_ in self.layers)]
            cached = self.__dict__["_qkv_w"] = (key, ws)
        return cached[1]

    def _decode_constants(self, hs2, memory, mask, fast):
        """per layer: value_proj(memory) with its padded rows zeroed (B * S, C), and the event-feature half of dim_project
        (W[:, C:] hs, no bias) (n, C) -- neither depends on the token"""
        from .. import layers as L
        B, S, C = memory.shape
        values, qparts = [], []
        if fast:
            mem2 = memory.reshape(B * S, C)
            if not mem2.is_contiguous():
                mem2 = mem2.contiguous()
            am_mem = L.amax_of(memory, B * S)
            if am_mem is None:
                am_mem, _ = L.row_absmax(mem2)
            am_q, _ = L.row_absmax(hs2)
            m8 = mask.reshape(B * S).contiguous().view(torch.uint8) if mask is not None else None
            for layer in self.layers:
                att = layer.cross_attention
                value, qpart = L._new(B * S, C, mem2), L._new(hs2.shape[0], C, hs2)
                L.linear(mem2, L.cached(att, "capv", [(att.value_proj.weight, att.value_proj.bias)]),
                         [L.seg(0, value, am_mem, rowmask=m8)])
                w = layer.dim_project.weight
                L.linear(hs2, L.cached(layer, "dp_hs", lambda w=w: [(w[:, C:], None)], key_of=(w,)), [L.seg(0, qpart, am_q)])
                values.append(value)
                qparts.append(qpart)
            return values, qparts
        for layer in self.layers:
            att = layer.cross_attention
            value = F.linear(memory, att.value_proj.weight, att.value_proj.bias)
            if mask is not None:
                value = value.masked_fill(mask[..., None], 0.0)
            values.append(value.reshape(B * S, C))
            qparts.append(F.linear(hs2, layer.dim_project.weight[:, C:]))
        return values, qparts

    def _attend(self, i, layer, qkv, x, t, st, want_amax=False):
        """the cached self-attention of a token step: through the beams' lineage table when the state carries one (_beam_device)"""
        norm = layer.norm1
        return attend_step_beam(qkv, x, st["cache"][i], st["lineage"], t, self.n_heads, norm.weight, norm.bias, norm.eps,
                                want_amax=want_amax)

    def _layer_step_fast(self, i, layer, x, am, t, st):
        """one position through one layer on the hand-written launches: q | k | v, attention over the cache + residual + norm1,
        dim_project (+ the kept event-feature half), offsets | weights, sampling, output_proj + residual, norm2, FFN"""
        from .. import layers as L
        n, C = x.shape
        att, sa, arena = layer.cross_attention, layer.self_attention, st["arena"]
        wq = L.cached(sa, "qkv", [(sa.query.weight, sa.query.bias), (sa.key.weight, sa.key.bias), (sa.value.weight, sa.value.bias)])
        qkv = L._new(n, 3 * C, x)
        L.linear(x, wq, [L.seg(wq.starts[j], qkv[:, j * C:(j + 1) * C], am, width=C) for j in range(3)])
        y1, am1 = self._attend(i, layer, qkv, x, t, st, want_amax=True)
        w = layer.dim_project.weight
        z, am_z = L._new(n, C, x), arena.take(n)
        L.linear(y1, L.cached(layer, "dp_x", lambda: [(w[:, :C], layer.dim_project.bias)], key_of=(w, layer.dim_project.bias)),
                 [L.seg(0, z, am1, resid=st["qparts"][i], amax_out=am_z)])
        proj = L._new(n, 2 * att.n_heads * att.n_levels * att.n_points, x)
        L.linear(z, L.cached(att, "proj", [(att.sampling_offsets.weight, att.sampling_offsets.bias),
                                           (att.attention_weights.weight, att.attention_weights.bias)]), [L.seg(0, proj, am_z)])
        o, am_o = L._msda(att, st["values"][i], proj, st["ref_in"], st["shapes2d"], st["lsi"], st["B"], st["Q"], arena)
        y = L._new(n, C, x)
        L.linear(o, L.cached(att, "op", [(att.output_proj.weight, att.output_proj.bias)]), [L.seg(0, y, am_o, resid=z)])
        x2, am2, _ = L.layer_norm(y, layer.norm2)
        x3, am3, _ = L._ffn(layer, x2, am2, layer.norm3, arena)
        return x3, am3

    def _layer_step_torch(self, i, layer, x, t, st):
        """the same position on PyTorch's Linear / LayerNorm (shapes outside the inference layers' domain); the attention step and
        the sampling stay on the library's kernels where those apply"""
        n, C = x.shape
        att = layer.cross_attention
        B, Q = st["B"], st["Q"]
        w_qkv, b_qkv = st["qkv_w"][i]
        qkv = F.linear(x, w_qkv, b_qkv)
        y1, _ = self._attend(i, layer, qkv, x, t, st)
        z = F.linear(y1, layer.dim_project.weight[:, :C], layer.dim_project.bias) + st["qparts"][i]
        w_cat, b_cat = att._cat_projection()
        proj = F.linear(z, w_cat, b_cat)
        M, D, K = att.n_heads, C // att.n_heads, att.n_levels * att.n_points
        value = st["values"][i].view(B, -1, M, D)
        if att._fused_eligible(z, value.view(B, -1, C), st["host"]):
            o = MSDA.msda1d_fused_forward(value, st["shapes2d"], st["lsi"], proj.view(B, Q, -1), st["ref_in"], att.n_levels,
                                          att.n_points, att.pad_mode).view(n, C)
        else:
            off = proj[:, :M * K].reshape(B, Q, M, att.n_levels, att.n_points)
            aw = F.softmax(proj[:, M * K:].reshape(B, Q, M, K), -1).view(B, Q, M, att.n_levels, att.n_points)
            loc = att._locations(st["ref_in"], off, st["tshapes"])
            if att.pad_mode != "zeros":
                raise NotImplementedError("Transformer-DSA decode: MSDeformAttn.pad_mode other than 'zeros' outside the fused kernel")
            o = MSDeformAttnFunction.apply(value, st["shapes2d"], st["lsi"], loc.contiguous(), aw.contiguous(),
                                           att.im2col_step).view(n, C)
        x2 = layer.norm2(z + F.linear(o, att.output_proj.weight, att.output_proj.bias))
        return layer.norm3(x2 + layer.linear2(F.relu(layer.linear1(x2))))

    def _token_state(self, hs, reference, memory, mask, valid_ratios, tshapes, lsi, W, positions):
        """what the token steps of one decode read and write beside their ids, for W rows per event (W > 1: the beams of an
        event, W consecutive rows -- the event's reference points and its half of dim_project repeated over them):
        value_proj(memory) per video and layer, the key / value cache of `positions` positions per row, the arena of row maxima or
        the concatenated q | k | v weights.  st["lineage"] stays None in the greedy loop; the beam search sets its table per token."""
        from .. import layers as L
        B, Q, C = hs.shape
        n, T, nl, dev = B * Q, self.max_caption_len, len(self.layers), hs.device
        hs = hs.contiguous()
        fast = self._layers_ok(hs, memory, tshapes)
        values, qparts = self._decode_constants(hs.view(n, C), memory, mask, fast)
        if W > 1:
            qparts = [q_.repeat_interleave(W, 0) for q_ in qparts]
            reference = reference.repeat_interleave(W, 1)
        st = {"B": B, "Q": Q * W, "values": values, "qparts": qparts, "tshapes": tshapes, "lsi": lsi, "fast": fast, "lineage": None,
              "ref_in": self._scaled_reference(reference, {'valid_ratios': valid_ratios}).contiguous(),
              "shapes2d": temporal_shapes_2d(tshapes, lsi), "host": getattr(tshapes, "_gvl_host_lengths", None),
              # keys and values of every layer; position p of a row is written by step p and read by the steps behind it only (beam
              # search: by the beam that sits at the row then, and read through the lineages)
              "cache": torch.empty(nl, 2, n * W, positions, C, device=dev, dtype=torch.float32),
              "pos_table": self.pos_table[0], "kernel_embed": C % 4 == 0 and self.embed.weight.dtype == torch.float32}
        if fast:
            st["arena"] = L._Arena((3 * T * nl + 2) * (n * W + 4), dev)
        else:
            st["qkv_w"] = self._torch_weights()
        return st

    def _token_step(self, it, t, st):
        """ids (rows,) of position t -> the rows of the last layer (rows, C): the embedding + position row, then every layer on the
        hand-written launches or on PyTorch's (st["fast"])"""
        fast, pos_table = st["fast"], st["pos_table"]
        if st["kernel_embed"]:
            x, am = embed_step(self.embed.weight, pos_table, it, t)
        else:
            x, am = self.embed.weight[it] + (pos_table[t] if t < pos_table.shape[0] else 0.0), None
            if fast:
                from .. import layers as L
                am, _ = L.row_absmax(x)
        for i, layer in enumerate(self.layers):
            if fast:
                x, am = self._layer_step_fast(i, layer, x, am, t, st)
            else:
                x = self._layer_step_torch(i, layer, x, t, st)
        return x

    def _decode_device(self, hs, reference, memory, mask, valid_ratios, tshapes, lsi):
        """The whole greedy loop on the device, no host interaction: -> (seq (n, T), logprob (n, T), alive (T,)), T = max_caption_len.
        Capturable in a hipGraph.  Iteration t first books token t - 1 from the logits of the previous iteration (argmax, log-prob,
        unfinished / alive flags: one launch), then runs position t through the layers.  The reference also runs the layers after the
        LAST token (:237) and then leaves the loop without reading the result."""
        n, T, dev = hs.shape[0] * hs.shape[1], self.max_caption_len, hs.device
        st = self._token_state(hs, reference, memory, mask, valid_ratios, tshapes, lsi, 1, T + 1)
        # ONE zero fill, as LSTM_DSA.Captioner._decode_device: the log-prob table, the <bos> ids, the token table, the `alive` flags
        seq_lp, it, seq, alive = zero_views(dev, (torch.float32, (n, T)), (torch.long, (n,)), (torch.long, (n, T)), (torch.uint8, (T,)))
        unfinished = torch.empty(n, dtype=torch.uint8, device=dev)
        logits = None
        for t in range(T + 1):
            if t > 0:
                it = MSDA.greedy_step(logits, t - 1, unfinished, seq, seq_lp, alive)      # (the raw argmax is the next input, :230-232)
            if t == T:
                break
            x = self._token_step(it, t, st)
            planes = self._logit_planes(x)
            if planes is not None:                                   # fp32 product on the fp16 matrix cores, argmax in its epilogue
                logits = MSDA.gemm_f16x3_argmax(MSDA.split_rows(x), planes, self.logits.bias)      # never written out
            else:
                logits = F.linear(x, self.logits.weight, self.logits.bias).float().contiguous()
        return seq, seq_lp, alive.view(torch.bool)

    def _beam_device(self, hs, reference, memory, mask, valid_ratios, tshapes, lsi, beam_size, length_penalty):
        """The whole beam search on the device, no host interaction (DESIGN.md sections 4.3 and 10) -> (tokens (n, W, T), logprobs
        (n, W, T), scores (n, W), lengths (n, W), alive (T,)) in final rank order, T = max_caption_len.  Capturable in a hipGraph.
        The W beams of an event are W consecutive rows; the token step is the one of _decode_device on n W rows.  After every
        token the beams of an event are replaced by children of arbitrary parents, and a child attends over its parent's prefix:
        the cache is NOT re-ordered for that.  Every row appends at its own slot; the kernel that selects the beams
        (gvl_beam_step_lineage_f32, one launch per token) re-orders a byte table that names, per beam and position, the slot holding
        it, and the attention (attend_step_beam) reads through that table -- one table for all layers."""
        W, T = beam_size, self.max_caption_len
        n, dev = hs.shape[0] * hs.shape[1], hs.device
        st = self._token_state(hs, reference, memory, mask, valid_ratios, tshapes, lsi, W, T)
        # ONE zero fill: the <bos> ids, the `alive` words, the first step's finished flags, the two lineage tables
        it, alive, fin, lins = zero_views(dev, (torch.long, (n * W,)), (torch.int32, (T,)), (torch.uint8, (n, W)),
                                          (torch.uint8, (2, n, W, T)))
        books = BeamBooks(n, W, T, self.vocab_size + 1, fin, alive, dev)
        for t, (ins, outs, it_next) in enumerate(books.steps):
            st["lineage"] = lins[t & 1]                                 # positions [0, t) of the current beams
            x = self._token_step(it, t, st)
            planes = self._logit_planes(x)
            if planes is not None:                                      # fp32 product on the fp16 matrix cores, logits written
                logits = MSDA.gemm_f16x3(MSDA.split_rows(x), planes, self.logits.bias, out=books.logits_out)
            else:
                logits = F.linear(x, self.logits.weight, self.logits.bias).float().contiguous()
            MSDA.beam_step_lineage(logits, *ins, lins[t & 1], lins[(t + 1) & 1], t, *outs)
            it = it_next
        return books.finish(length_penalty)

    @_fp32_island
    def sample(self, hs, reference, others, opt={}):
        """Greedy decoding (Transformer_DSA.py:216-254) -> (seq (N_ * N_q, <= max_caption_len), logprobs), or ([], []) when every
        first token is <end>.  opt['beam_size'] > 1 (with opt['length_penalty'], default 0): the best beam of beam_search in the same
        form.  One host read (the `alive` flags), none with defer_trim set (the caller cuts at `last_alive`).  With
        graph_decode set the outputs are cut from the graph's static tensors and cloned."""
        if not opt.get('sample_max', 1):
            if int(opt.get('beam_size', 1) or 1) > 1:
                raise ValueError("beam_size > 1 needs sample_max = 1: beam search and multinomial sampling exclude each other")
            raise NotImplementedError('Do not support scale logprobs by temperture')            # (the reference's own, :235)
        beam_size = int(opt.get('beam_size', 1) or 1)
        if beam_size > 1:
            if getattr(self, "defer_trim", False):
                raise NotImplementedError("beam search inside a captured whole forward (defer_trim) is not built")
            with torch.no_grad():
                return self._best_beam(self.beam_search(hs, reference, others, beam_size, opt.get('length_penalty', 0.0)))
        memory, tshapes, lsi, mask = self._level_inputs(others)
        if not hs.is_cuda:
            raise RuntimeError(f"gvl_amd's Transformer-DSA head decodes on a ROCm device only (no CPU fallback); got {hs.device}")
        args = (hs, reference, memory, mask, others['valid_ratios'], tshapes, lsi)
        with torch.no_grad():
            if getattr(self, "defer_trim", False):
                # the caller is capturing the whole forward (gvl_amd.parallel.GraphedEvalForward): no host read in here
                seq, seq_lp, self.last_alive = self._decode_device(*args)
                return seq, seq_lp
            if getattr(self, "graph_decode", False) and getattr(tshapes, "_gvl_host_lengths", None) is not None:
                seq, seq_lp, alive = self._decode_graphed(*args)
            else:
                seq, seq_lp, alive = self._decode_device(*args)
        return self._trimmed(seq, seq_lp, alive)

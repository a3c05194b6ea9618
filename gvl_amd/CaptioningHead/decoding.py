"""What the two caption heads (LSTM_DSA.Captioner, Transformer_DSA.TransformerDSACaptioner) share around their token steps: the
level inputs and scaled reference points, the masked row loss, the vocabulary layer's operand planes, the refusals and the dispatch
of beam_search, the capture cache of graph_decode, the beam search's bookkeeping, the zero-filled decode state and the two tails of
`sample`.  DecodingHead adds no parameter, buffer or sub-module.  A head supplies:

    opt, vocab_size                        as the reference's heads keep them
    _vocab_layer()                         its vocabulary Linear (`logit` / `logits`: the reference's parameter names)
    _reference_line                        for the message of the one unsupported level configuration
    _decode_device(hs, reference, memory, mask, valid_ratios, tshapes, lsi)                             -> (seq, seq_lp, alive)
                                           (or _greedy_device of that form, where _decode_device takes more: the LSTM head's)
    _beam_device(hs, reference, memory, mask, valid_ratios, tshapes, lsi, beam_size, length_penalty)    -> beam_search's five entries
"""
import functools
import math

import torch
import torch.nn as nn

from .. import MultiScaleDeformableAttention as MSDA
from ..graphs import _LRU, capture_on, side_stream
from ..linear import split_gemm_enabled


def _fp32_island(fn):
    """Mixed-precision policy of gvl_amd under torch.autocast(bfloat16) (BASELINE config 4): the transformer runs its
    GEMMs / deformable attention on bf16 storage, the captioner stays fp32 -- its token-step kernels
    (gvl_cap_attend_f32, gvl_lstm_cell_f32, gvl_row_argmax_lse_f32) are fp32, the recurrence feeds its own rounding
    back 30 times, and greedy argmax over ~8.5k logits flips on bf16 near-ties.  Inputs arriving in bf16 are widened."""
    @functools.wraps(fn)
    def wrapped(self, hs, reference, others, *args, **kwargs):
        if not torch.is_autocast_enabled():
            return fn(self, hs, reference, others, *args, **kwargs)
        others = dict(others)
        for k in ("memory", "valid_ratios"):
            others[k] = others[k].float()
        with torch.autocast("cuda", enabled=False):
            return fn(self, hs.float(), reference.float(), others, *args, **kwargs)
    return wrapped


def zero_views(device, *specs):
    """ONE zero fill for a decode's whole zero-initialised state: specs are (dtype, shape) pairs -> one view per spec, each of
    its dtype and shape, each starting on a 16-byte boundary of the same byte buffer, none overlapping another"""
    sizes = [dt.itemsize * math.prod(shape) for dt, shape in specs]
    starts, end = [], 0
    for size in sizes:
        starts.append((end + 15) // 16 * 16)
        end = starts[-1] + size
    raw = torch.zeros(end, dtype=torch.uint8, device=device)
    return [raw[a:a + size].view(dt).view(shape) for (dt, shape), a, size in zip(specs, starts, sizes)]


class BeamBooks:
    """The records of a beam search of W beams over T tokens on n event rows: the running score (beam 0 at
    0, the rest at -inf: the first step yields W distinct beams), the ping-pong pairs of scores and finished flags, the per-step
    parents / tokens / log-probs, and the logits' buffer with rows padded to 16 bytes.  `fin` (n, W) uint8 and `alive` (T,) int32
    come zero-filled from the head's zero_views.  `steps[t]` holds what token t's selection kernel reads and writes, and what the
    next token step is fed -- laid out before the loop, which then only unpacks it:
        (score_in, fin_in), (score_out, fin_out, parent, token, logp, alive word), next ids (n W,)"""

    def __init__(self, n, W, T, V1, fin, alive, device):
        score = torch.full((n, W), float("-inf"), dtype=torch.float32, device=device)
        score[:, 0] = 0.0
        scores = (torch.empty_like(score), torch.empty_like(score))
        fins = (torch.empty_like(fin), torch.empty_like(fin))
        self.parents = torch.empty(T, n, W, dtype=torch.int32, device=device)
        self.tokens = torch.empty(T, n, W, dtype=torch.long, device=device)
        self.logps = torch.empty(T, n, W, dtype=torch.float32, device=device)
        ld = (V1 + 3) // 4 * 4                                          # rows of the logits padded to 16 bytes
        self.logits_out = torch.empty(n * W, ld, dtype=torch.float32, device=device)[:, :V1]
        self.alive, self.steps = alive, []
        for t in range(T):
            self.steps.append(((score, fin), (scores[t & 1], fins[t & 1], self.parents[t], self.tokens[t], self.logps[t],
                                              alive[t:t + 1]), self.tokens[t].view(-1)))
            score, fin = scores[t & 1], fins[t & 1]
        self.score = score

    def finish(self, length_penalty):
        """-> (tokens (n, W, T), logprobs (n, W, T), scores (n, W), lengths (n, W), alive (T,) bool) in final rank order"""
        return MSDA.beam_finish(self.parents, self.tokens, self.logps, self.score, length_penalty) + (self.alive != 0,)


class DecodingHead(nn.Module):
    _reference_line = None                 # "File.py:line" of the reference's branch for fewer caption levels than feature levels

    def _vocab_layer(self):
        raise NotImplementedError

    def _greedy_device(self, *args):
        """the greedy loop as graph_decode captures it: _decode_device, with whatever else a head's own takes"""
        return self._decode_device(*args)

    def _scaled_reference(self, reference, others):
        vr = others['valid_ratios']
        if reference.shape[-1] == 2:
            return reference[:, :, None] * torch.stack([vr] * 2, -1)[:, None]
        return reference[:, :, None] * vr[:, None, :, None]

    @staticmethod
    def _masked_row_nll(logprobs, target, mask):
        """the reference's build_loss multiplies by a materialised one-hot (n, len, vocab+1) tensor and sums the vocabulary axis: a
        sum of one term and zeros, i.e. exactly the gathered log-prob -- taken directly here"""
        max_len = logprobs.shape[1]
        picked = logprobs.gather(2, target[:, :max_len, None]).squeeze(2)
        return -(picked * mask[:, :max_len]).sum(1) / (mask.sum(1) + 1e-6)

    def _level_inputs(self, others):
        """-> (memory, temporal shapes, level start index, padding mask)"""
        if self.opt.cap_num_feature_levels < self.opt.num_feature_levels:
            # (the reference's own branch cannot run on temporal features: it takes torch.prod(dim=1) of the 1-D (L,) tensor of
            #  level lengths and raises IndexError -- verified by running the reference's LSTM head with cap_num_feature_levels = 2;
            #  there is no behaviour to mirror)
            raise NotImplementedError("cap_num_feature_levels < num_feature_levels: the reference itself raises on this branch for "
                                      f"temporal features ({self._reference_line}) and no config uses it")
        return others['memory'], others['spatial_shapes'], others['level_start_index'], others['mask_flatten']

    def _logit_planes(self, x):
        """fp16 planes of the vocabulary layer's weight (gvl_split_rows_f16), rebuilt when the weight changes; None when the split
        product does not apply (training / dropout active, autocast, a bf16 copy of x in use, GVL_GEMM=f32)"""
        w = self._vocab_layer().weight
        if (self.training or torch.is_grad_enabled() or torch.is_autocast_enabled() or x.dtype != torch.float32
                or hasattr(x, "_gvl_lowp") or not split_gemm_enabled() or not MSDA.split_eligible(w)):
            return None
        key = (w.data_ptr(), w._version)
        cached = self.__dict__.get("_logit_p")
        if cached is None or cached[0] != key:
            with torch.no_grad():
                cached = self.__dict__["_logit_p"] = (key, MSDA.split_rows(w.detach()))
        return cached[1]

    def beam_search(self, hs, reference, others, beam_size, length_penalty=0.0):
        """Beam-search decoding (the `beam_size` option the reference reads at LSTM_DSA.py:132 and drops; semantics: DESIGN.md
        section 4.3) -> dict, every entry in final rank order (rank = score / len ** length_penalty, len = emitted tokens with
        the end token; the penalty is never applied during the search):
            tokens (n, W, T) int64 and logprobs (n, W, T), zero behind a beam's end token;  scores (n, W) sum of log-probs;
            lengths (n, W) tokens in front of the end token;  alive (T,) bool: some beam is still live after token t.
        No host read in here.  With graph_decode set the loop is replayed from a hipGraph: the outputs are then the graph's static
        tensors, overwritten by the next call."""
        W = int(beam_size)
        if not 1 <= W <= MSDA.BEAM_MAX:
            raise ValueError(f"beam_size must be 1 .. {MSDA.BEAM_MAX} (got {beam_size})")
        if W > self.vocab_size + 1:
            raise ValueError(f"beam_size {W} exceeds the {self.vocab_size + 1} vocabulary entries")
        if not hs.is_cuda:
            raise NotImplementedError(f"beam_size > 1: {type(self).__name__} searches on a ROCm device only (no CPU fallback); "
                                      f"got {hs.device}")
        if torch.is_autocast_enabled():
            raise NotImplementedError("beam search decodes in fp32: the bf16-storage decode under torch.autocast is not built")
        if torch.is_grad_enabled():
            raise RuntimeError("beam search is inference only: call it under torch.no_grad()")
        memory, tshapes, lsi, mask = self._level_inputs(others)
        args = (hs, reference, memory, mask, others['valid_ratios'], tshapes, lsi)
        if getattr(self, "graph_decode", False) and getattr(tshapes, "_gvl_host_lengths", None) is not None:
            out = self._decode_graphed(*args, beam=(W, float(length_penalty)))
        else:
            out = self._beam_device(*args, W, float(length_penalty))
        return dict(zip(("tokens", "logprobs", "scores", "lengths", "alive"), out))

    def _decode_graphed(self, hs, reference, memory, mask, valid_ratios, tshapes, lsi, beam=(1, 0.0)):
        """Greedy decoding replayed from a hipGraph: the LSTM head's 31-step loop is ~800 kernel launches whose host-side issue
        cost exceeds their run time; captured once per input shape, replayed with one launch.
        beam = (beam_size, length_penalty) with beam_size > 1: the beam search (_beam_device) instead, by the same cache."""
        cache = self.__dict__.get("_decode_graphs")
        if cache is None:
            cache = self.__dict__["_decode_graphs"] = _LRU(16)
        # weight-derived operands (planes, re-laid-out and concatenated matrices, the pre-multiplied embedding table) are cached
        # per parameter version and become constants of the captured graph: a parameter update must lead to a new capture
        key = (tuple(hs.shape), tuple(reference.shape), tuple(memory.shape), str(hs.device), tuple(tshapes._gvl_host_lengths[0]),
               mask is not None, torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled() else None, tuple(beam),
               sum(p_._version for p_ in self.parameters()))
        if cache and next(iter(cache))[-1] != key[-1]:
            cache.clear()                                    # parameters changed: graphs of the old weights are dead
        entry = cache.lookup(key)
        ins = (hs, reference, memory, mask, valid_ratios)
        if entry is None:
            static = [t_.clone() if t_ is not None else None for t_ in ins]
            if beam[0] > 1:
                decode = lambda: self._beam_device(*static, tshapes, lsi, *beam)      # noqa: E731
            else:
                decode = lambda: self._greedy_device(*static, tshapes, lsi)           # noqa: E731
            with side_stream(hs.device) as side:                # warm-up off the capture (lazy inits, LDS attributes, weight planes)
                decode()
            with capture_on(side) as graph:
                outs = decode()
            entry = (graph, static, outs)
            cache.store(key, entry)
        graph, static, outs = entry
        for dst, src in zip(static, ins):
            if dst is not None:
                dst.copy_(src)
        graph.replay()
        return outs

    # ---- the two tails of `sample` ---------------------------------------------------------------------------------------------
    @staticmethod
    def _best_beam(res):
        """the best beam of beam_search in the greedy branch's form: (n, keep) with keep = the longest returned caption, ([], [])
        when every one is empty -- PostProcess reads it as it reads greedy output"""
        keep = int(res["lengths"][:, 0].max())                   # the one host read
        if keep == 0:
            return [], []
        return res["tokens"][:, 0, :keep].clone(), res["logprobs"][:, 0, :keep].clone()

    @staticmethod
    def _trimmed(seq, seq_lp, alive):
        """the reference stops at the first step where every row has finished (LSTM_DSA.py:186-187, Transformer_DSA.py:246-247):
        one host read here"""
        alive = alive.cpu().tolist()
        keep = alive.index(False) if False in alive else len(alive)
        if keep == 0:
            return [], []
        return seq[:, :keep].clone(), seq_lp[:, :keep].clone()

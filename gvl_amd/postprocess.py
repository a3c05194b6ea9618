"""PostProcess -- the result side of the eval loop, mirror of pdvc/pdvc.py:932-1089 for the LSTM-DSA path (what
eval_utils.py:213-216 calls on every eval batch), with the contrastive branch's sentence grounding (forward_grounding,
pdvc.py:947-1000) and event-caption matching scores (cl_scores, pdvc.py:1059-1081).  Per video: the N_q most confident (query, class) pairs,
their segments clipped to the video and scaled to seconds, their captions decoded with the dataset's translator and
scored by the sum of the token log-probabilities.  Host glue; the only device work is a top-k and a gather.
The record keys are the reference's wire format (eval_utils.py:216-239 reads them)."""
import torch
from torch import nn

from .matcher import box_cl_to_xy

RECORD_KEYS = ('scores', 'labels', 'boxes', 'raw_boxes', 'captions', 'caption_scores', 'cl_scores', 'query_id',
               'vid_duration', 'pred_seq_len', 'raw_idx')


def rank_events(pred_logits):
    """confidence ranking over all (query, class) pairs of a video (pdvc.py:1019-1023)
    -> (scores (N, N_q) descending, flat pair index, query id, class id)"""
    n_vid, n_query, n_class = pred_logits.shape
    scores, flat = torch.topk(pred_logits.sigmoid().reshape(n_vid, n_query * n_class), n_query, dim=1)
    return scores, flat, flat // n_class, flat % n_class


def segments_in_seconds(pred_boxes, query_id, durations):
    """(centre, length) in [0, 1] -> [start, end] seconds of the ranked queries, clipped to the video (pdvc.py:1024-1031)"""
    spans = box_cl_to_xy(pred_boxes).clamp(0, 1)
    picked = spans.gather(1, query_id[..., None].expand(-1, -1, 2))
    return picked * durations[:, None, None]


def decode_captions(seq, log_probs, query_id, translator):
    """token ids + per-token log-probs of every query -> (sentences, scores) re-ordered by the ranking (pdvc.py:1046-1066)"""
    n_vid, n_query = query_id.shape
    if not len(seq):                                         # captioning disabled / every caption empty
        return [[''] * n_query] * n_vid, [[-1e5] * n_query] * n_vid
    total = ((seq > 0).float() * log_probs).sum(2).cpu().numpy().astype('float')
    tokens = seq.detach().cpu().numpy().astype('int')
    ranking = query_id.cpu().tolist()
    sentences = [[translator.rtranslate(tokens[v][q]) for q in ranking[v]] for v in range(n_vid)]
    scores = [[total[v, q] for q in ranking[v]] for v in range(n_vid)]
    return sentences, scores


class PostProcess(nn.Module):
    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        o = vars(opt)
        if o.get('enable_contrastive', False) and o.get('eval_enable_grounding', False):            # pdvc.py:938-945
            from .matcher import HungarianMatcher
            self.grounding_matcher = HungarianMatcher(cost_class=o.get('eval_set_cost_class', 0.), cost_bbox=0.0, cost_giou=0.0,
                                                      cost_alpha=o.get('eval_grounding_cost_alpha', 0.25),
                                                      cost_gamma=o.get('eval_grounding_cost_gamma', 2),
                                                      cost_cl=o.get('eval_set_cost_cl', 1.0))

    @torch.no_grad()
    def forward_grounding(self, outputs, target_sizes, targets):
        """pdvc.py:947-1000: one event per ground-truth sentence -- the one the grounding matcher (class + contrastive cost only)
        assigns to it, or the cheapest one (always, with eval_enable_maximum_matching_for_grounding) -- with its segment in
        seconds, confidence and cost; and the contrastive scores, whole or per video with the background column appended.
        The targets' boxes and labels are zeroed in place, as the reference does.  Without the branch: (None, None)."""
        if not vars(self.opt).get('enable_contrastive', False):
            return None, None
        for target in targets:
            target['boxes'] = target['boxes'] * 0
            target['labels'] = target['labels'] * 0
        spans = (box_cl_to_xy(outputs['pred_boxes']).clamp(0, 1) * target_sizes[:, None, None]).cpu().numpy().tolist()
        conf = outputs['pred_logits'].sigmoid().cpu().numpy().tolist()
        main = {k: v for k, v in outputs.items() if k not in ('aux_outputs', 'enc_outputs')}
        indices, _, C = self.grounding_matcher(main, targets, return_C=True)
        always_cheapest = vars(self.opt).get('eval_enable_maximum_matching_for_grounding', False)
        results = []
        for i, (event_ind, cap_ind) in enumerate(indices):
            matched = {int(c): int(e) for e, c in zip(event_ind.tolist(), cap_ind.tolist())}
            picked = [int(C[i][:, j].argmin()) if (always_cheapest or j not in matched) else matched[j]
                      for j in range(len(targets[i]['boxes']))]
            results.append({'boxes': [spans[i][e] for e in picked], 'confs': [conf[i][e][0] for e in picked],
                            'cl_scores': [C[i][e, j].item() for j, e in enumerate(picked)]})
        cl_scores = outputs['cl_match_mats']
        sizes = [len(v["boxes"]) for v in targets]
        if cl_scores.shape[1] > sum(sizes):                                    # a background column
            bs, num_queries, _ = outputs['pred_boxes'].shape
            bg_score = cl_scores[:, -1:].reshape(bs, num_queries, 1)
            per_video = cl_scores[:, :-1].reshape(bs, num_queries, -1).split(sizes, dim=-1)
            cl_scores = [torch.cat((c[i], bg_score[i]), dim=1) for i, c in enumerate(per_video)]
        return results, cl_scores

    def matching_scores(self, outputs, sentences, flat, model, tokenizer):
        """pdvc.py:1059-1081: the generated captions go through the model's text branch; per video, row r (the caption of ranked
        event r) of the caption x event cosine table of that video, at column flat[v][r] -- the reference gathers with the flat
        (query, class) index, which is the query id for one class -> per video (N_q,) float array"""
        n_vid, n_query = flat.shape
        enc_in = tokenizer([s_ for vid in sentences for s_ in vid], return_tensors='pt', padding=True)
        dev = outputs['event_embed'].device
        enc_in = {k: v.to(dev) if isinstance(v, torch.Tensor) else v for k, v in enc_in.items()}
        counts = [len(vid) for vid in sentences]
        text_embed, _, _, _ = model.text_encoding(enc_in, counts, memory=outputs.get('memory', [None] * n_vid))
        text = torch.nn.functional.normalize(torch.cat(text_embed[-1], dim=0), p=2, dim=1)
        event = torch.nn.functional.normalize(outputs['event_embed'].reshape(-1, outputs['event_embed'].shape[-1]), p=2, dim=1)
        cos = (text @ event.t()).view(n_vid, n_query, n_vid, n_query)               # (video, caption, video, event)
        return [cos[v, :, v].gather(1, flat[v][:, None]).squeeze(1).cpu().numpy().astype('float') for v in range(n_vid)]

    @torch.no_grad()
    def forward(self, outputs, target_sizes, loader, model=None, tokenizer=None):
        """cl_scores: with enable_contrastive, eval_enable_matching_score and a tokenizer, the cosine of every ranked event with its
        own generated caption (pdvc.py:1059-1081); zeros otherwise"""
        logits = outputs['pred_logits']
        assert len(logits) == len(target_sizes)
        scores, flat, query_id, class_id = rank_events(logits)
        segments = segments_in_seconds(outputs['pred_boxes'], query_id, target_sizes)
        sentences, sentence_scores = decode_captions(outputs['seq'], outputs['caption_probs']['cap_prob_eval'], query_id,
                                                     loader.dataset.translator)
        n_events = outputs['pred_count'].argmax(dim=-1).clamp(min=1)          # predicted number of events, at least one
        o = vars(self.opt)
        if o.get('enable_contrastive', False) and o.get('eval_enable_matching_score', False) and tokenizer is not None:
            cl = self.matching_scores(outputs, sentences, flat, model, tokenizer)
        else:
            cl = [[0.0] * query_id.shape[1]] * len(logits)
        columns = (scores, class_id, segments, segments, sentences, sentence_scores, cl, query_id,
                   target_sizes, n_events, flat)
        return [dict(zip(RECORD_KEYS, row)) for row in zip(*columns)]

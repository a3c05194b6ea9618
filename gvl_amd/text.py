"""Text side of the contrastive branch: everything downstream of the frozen text encoder's ``last_hidden_state``.

The reference builds a HuggingFace RoBERTa (pdvc/pdvc.py:1185-1190) and every shipped configuration freezes it.  Nothing here imports
``transformers`` or loads weights: ``PDVC`` takes ANY module with the encoder's interface (``.config.hidden_size``; called with the
keywords of ``dt['text_encoder_input']``; returns an object with ``.last_hidden_state`` and ``['pooler_output']``), and
``PrecomputedTextEncoder`` is that interface over features the user extracted beforehand.
"""
import types

import torch
import torch.nn.functional as F
from torch import nn


class TextEncoderOutput(dict):
    """``out.last_hidden_state`` and ``out['pooler_output']``, as the HuggingFace model output offers them"""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None


class PrecomputedTextEncoder(nn.Module):
    """A frozen text encoder whose forward has already been run: ``dt['text_encoder_input'] = {'last_hidden_state': (S, W, H),
    'attention_mask': (S, W)}`` comes back as it is, ``pooler_output`` is word 0.  No parameters."""

    def __init__(self, hidden_size):
        super().__init__()
        self.config = types.SimpleNamespace(hidden_size=int(hidden_size))

    def forward(self, last_hidden_state, attention_mask=None, **unused):
        if last_hidden_state.shape[-1] != self.config.hidden_size:
            raise ValueError(f"PrecomputedTextEncoder({self.config.hidden_size}): features of width {last_hidden_state.shape[-1]}")
        return TextEncoderOutput(last_hidden_state=last_hidden_state, pooler_output=last_hidden_state[:, 0])


class WordLevelContextModeling(nn.Module):
    """pdvc/pdvc.py:1092-1104: attention pool over the words of a sentence.  One score per word, w2(gelu(w1 x)); padded words
    get the score -10000; the sentence feature is the softmax-weighted sum of its word features."""

    def __init__(self, hidden_size):
        super().__init__()
        self.w1 = nn.Linear(hidden_size, hidden_size)
        self.w2 = nn.Linear(hidden_size, 1)

    def forward(self, x, mask):
        m = mask.to(x.dtype).unsqueeze(2)
        score = self.w2(F.gelu(self.w1(x))) * m - 10000 * (1 - m)                    # (S, W, 1)
        return torch.matmul(F.softmax(score, dim=1).transpose(1, 2), x).squeeze(1)


def max_pool_words(x, mask):
    """word_context_modeling_type 'max_pool' (pdvc.py:97): the mask is not read, as in the reference"""
    return x.max(dim=1)[0]


def mean_pool_words(x, mask):
    """word_context_modeling_type 'mean_pool' (pdvc.py:99)"""
    return (x * mask.unsqueeze(2)).sum(dim=1) / (1e-5 + mask.sum(dim=1, keepdim=True))

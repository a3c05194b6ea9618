"""Captioning heads on the path: the LSTM-DSA head (``caption_decoder_type: standard``, used by every BASELINE config) and
the Transformer-DSA head (``transformer``), the two of the reference that sit on the deformable attention.  Its other heads
(light LSTM, GPT-2, puppet) are out of scope and raise here instead of silently degrading."""
from .LSTM_DSA import LSTMDSACaptioner
from .Transformer_DSA import TransformerDSACaptioner


def build_captioner(opt):
    if opt.caption_decoder_type == 'standard':
        return LSTMDSACaptioner(opt)
    if opt.caption_decoder_type == 'transformer':
        return TransformerDSACaptioner(opt)
    raise ValueError(f"gvl_amd builds caption_decoder_type='standard' and 'transformer' only (got {opt.caption_decoder_type!r}); "
                     "the other reference heads are outside the accelerated path")

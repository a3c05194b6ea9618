"""Deterministic stand-ins for the frozen text encoder and its tokenizer, shared by tests/golden/make_golden_contrastive.py and the
contrastive tests.  No weights are downloaded: the encoder is an embedding table filled from a closed formula."""
import json
import types

import numpy as np

import torch
from torch import nn

HIDDEN = 48
VOCAB = 64


class StubOutput(dict):
    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None


class StubTextEncoder(nn.Module):
    """input_ids (S, W), attention_mask (S, W) -> last_hidden_state (S, W, 48): table lookup plus a position term"""

    def __init__(self, hidden_size=HIDDEN, vocab=VOCAB):
        super().__init__()
        self.config = types.SimpleNamespace(hidden_size=hidden_size)
        i = torch.arange(vocab, dtype=torch.float64)[:, None]
        j = torch.arange(hidden_size, dtype=torch.float64)[None, :]
        table = torch.sin(0.37 * (i + 1) * (j + 1)) + 0.5 * torch.cos(1.3 * i + 0.11 * j * j)
        self.embeddings = nn.Embedding(vocab, hidden_size)
        self.embeddings.weight.data.copy_(table.float())

    def forward(self, input_ids, attention_mask=None, **unused):
        pos = torch.arange(input_ids.shape[1], device=input_ids.device, dtype=torch.float32)
        h = self.embeddings(input_ids) + 0.1 * torch.sin(pos)[None, :, None]
        return StubOutput(last_hidden_state=h, pooler_output=torch.tanh(h[:, 0]))


class StubTokenizer:
    """characters -> ids (1 + ord % 62; 0 pads), right padding, attention mask"""

    def __call__(self, sentences, return_tensors='pt', padding=True, **unused):
        ids = [[1 + ord(c) % (VOCAB - 2) for c in (s if s else " ")] for s in sentences]
        width = max(len(x) for x in ids)
        input_ids = torch.zeros(len(ids), width, dtype=torch.long)
        mask = torch.zeros(len(ids), width, dtype=torch.long)
        for r, x in enumerate(ids):
            input_ids[r, :len(x)] = torch.tensor(x)
            mask[r, :len(x)] = 1
        return {'input_ids': input_ids, 'attention_mask': mask}


class StubTranslator:
    """token ids -> a sentence: one letter per non-zero token"""

    @staticmethod
    def rtranslate(tokens):
        return "".join(chr(97 + int(k) % 26) for k in tokens if int(k) > 0)


class StubLoader:
    """what PostProcess.forward reads of the data loader: loader.dataset.translator"""
    dataset = types.SimpleNamespace(translator=StubTranslator())


def sentences(n_gt, seed=0):
    """per video n sentences of 3..9 characters"""
    out = []
    for v, n in enumerate(n_gt):
        out.append(["".join(chr(97 + (7 * v + 3 * k + 5 * c + seed) % 26) for c in range(3 + (v + 2 * k) % 7)) for k in range(n)])
    return out


# ---- fixture packing: the model fixtures hold ~70 small arrays; stored one per zip entry the entries' headers outweigh the data, so
# they travel as three flat buffers (float32 / float64 / int64) and one JSON index (name -> buffer, offset, shape; string lists)
def pack_fixture(rec):
    import torch
    index, strings, bufs, fill = {}, {}, {"f4": [], "f8": [], "i8": []}, {"f4": 0, "f8": 0, "i8": 0}
    for k, v in rec.items():
        a = np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v)
        if a.dtype.kind in "US":
            strings[k] = a.tolist()
            continue
        code = "f4" if a.dtype == np.float32 else "f8" if a.dtype.kind == "f" else "i8"
        index[k] = [code, fill[code], list(a.shape)]
        bufs[code].append(a.astype({"f4": np.float32, "f8": np.float64, "i8": np.int64}[code]).ravel())
        fill[code] += a.size
    out = {c: (np.concatenate(b) if b else np.zeros(0, {"f4": np.float32, "f8": np.float64, "i8": np.int64}[c])) for c, b in bufs.items()}
    out["index"] = np.array(json.dumps({"arrays": index, "strings": strings}))
    return out


def unpack_fixture(path):
    f = np.load(path, allow_pickle=False)
    meta = json.loads(str(f["index"]))
    rec = {k: np.array(v) for k, v in meta["strings"].items()}
    for k, (code, off, shape) in meta["arrays"].items():
        n = int(np.prod(shape)) if shape else 1
        rec[k] = f[code][off:off + n].reshape(shape)
    return rec


def grounding_spans(pred_boxes, durations):
    """(centre, length) -> per video the [start, end] seconds of every event as forward_grounding reports them, float64 lists"""
    import torch
    c, l_ = pred_boxes[..., 0], pred_boxes[..., 1]
    spans = torch.stack([c - 0.5 * l_, c + 0.5 * l_], dim=-1).clamp(0, 1) * durations[:, None, None]
    return spans.cpu().numpy().tolist()


def events_of_boxes(boxes, spans):
    """the event id behind every reported box: the one event of the video whose span is nearest (and, asserted, unambiguous:
    the runner-up is at least 1000 times farther or 1e-3 s away)"""
    out = []
    for b in boxes:
        d = np.abs(np.asarray(spans) - np.asarray(b)[None]).max(axis=1)
        order = np.argsort(d)
        assert len(order) == 1 or d[order[1]] > max(1e-3, 1000 * d[order[0]]), (d[order[0]], d[order[1]])
        out.append(int(order[0]))
    return out

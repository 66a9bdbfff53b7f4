"""References and shared inputs of the RoBERTa tests (test_roberta.py, test_roberta_gpu.py): the position rule
of SPI_BERT_POS_FROM_IDS restated in numpy, the embedding's float64 reference under that rule, and the pad
patterns both files walk.  Nothing here touches a GPU; test_roberta.py holds the restatements to HF's own code.
"""
import numpy as np
import torch

PAD = 1  # SPI_ROBERTA_PAD_ID
PATTERNS = ("none", "trailing", "leading", "interior", "edges", "all_pad")


def err1(got, ref):
    """The project's metric with the floor the issue states: max|got - ref| / max(1, max|ref|)."""
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / max(1.0, np.abs(ref).max()))


def position_ids(ids):
    """p(b,s) = 1 + #{j <= s : ids[b][j] != 1} for a non-pad token, 1 for a pad token; ids int64 [B][S], raw."""
    tok = np.asarray(ids, np.int64) != PAD
    return np.where(tok, PAD + np.cumsum(tok, axis=1), PAD).astype(np.int64)


def pad_ids(ids, pattern):
    """A copy of ids [B][S] (none of them 1) with pad ids placed by `pattern`, differently in every row r:
    trailing: the last S // 3 + r tokens, never token 0; leading: the first 1 + S // 4 + r tokens;
    interior: token S // 2 - r alone; edges: tokens 0, 63 and 64 (those the row has; row r also 63 - r);
    all_pad: the last row entirely, the others as "interior"."""
    ids = np.array(ids, np.int64)
    B, S = ids.shape
    assert pattern in PATTERNS and not (ids == PAD).any()
    for r in range(B):
        if pattern == "trailing":
            ids[r, max(1, S - S // 3 - r):] = PAD
        elif pattern == "leading":
            ids[r, :min(S, 1 + S // 4 + r)] = PAD
        elif pattern == "interior" or (pattern == "all_pad" and r < B - 1):
            ids[r, max(0, S // 2 - r)] = PAD
        elif pattern == "edges":
            for s in (0, 63 - r, 63, 64):
                if 0 <= s < S:
                    ids[r, s] = PAD
        elif pattern == "all_pad":
            ids[r, :] = PAD
    return ids


def token_ids(rng, B, S, vocab, clamped=True):
    """Random ids in [0, vocab) without the pad id; with `clamped`, three that the kernel clamps for the word
    row but counts as tokens (-1, vocab, 2^40) and both ends of the table."""
    ids = rng.integers(0, vocab, (B, S), dtype=np.int64)
    ids[ids == PAD] = 2
    if clamped:
        edge = np.int64([-1, vocab, 2 ** 40, 0, vocab - 1])[:S]
        ids[-1, S - edge.size:] = edge
    return ids


def embed_ref(ids, word, pos, type_table, type_ids, gamma, beta, eps):
    """The embedding sum as the kernels take it, (word[clamp(id)] + type_row) + pos[p(b,s)] in fp32, then the
    LayerNorm in float64 (op_refs.bert_embed_ref with the position row replaced).  Returns float64 [B S][D]."""
    ids = np.asarray(ids, np.int64)
    p = position_ids(ids).reshape(-1)
    w = np.clip(ids.reshape(-1), 0, word.shape[0] - 1)
    t = np.zeros_like(w) if type_ids is None else np.clip(np.asarray(type_ids, np.int64).reshape(-1), 0,
                                                          type_table.shape[0] - 1)
    v = ((word[w] + type_table[t]).astype(np.float32) + pos[p]).astype(np.float32).astype(np.float64)
    mean = v.mean(-1, keepdims=True)
    var = ((v - mean) ** 2).mean(-1, keepdims=True)
    return (v - mean) / np.sqrt(var + eps) * gamma.astype(np.float64) + beta.astype(np.float64)


class Renamed(torch.nn.Module):
    """A module's fp32 tensors under other names (and with other values where `edit` returns them): what
    ModelReplica reads from a module, without its config.  rename: [(old substring, new substring)], applied in
    order; edit: name -> function of the array."""

    def __init__(self, spi, module, rename=(), edit=None):
        super().__init__()
        self._named = {}
        for name, a in spi.named_tensors(module):
            if edit and name in edit:
                a = np.ascontiguousarray(edit[name](a))
            for old, new in rename:
                name = name.replace(old, new)
            self._named[name] = torch.from_numpy(a)

    def named_parameters(self, *a, **k):
        return iter([])

    def named_buffers(self, *a, **k):
        return iter(self._named.items())

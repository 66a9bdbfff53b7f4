"""MPNet, host side: ops.rel_bias_rows against HF's own bucket function; the packer on host-only replicas."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import roberta_refs as RR

ROWS, D, HEADS = 130, 128, 2
KW = dict(layers=2, hidden=D, heads=HEADS, intermediate=256, vocab=100, max_position=ROWS)
TABLE = "bert.encoder.relative_attention_bias.weight"
TO_BERT = [(f"attention.attn.{a}.", f"attention.{b}.") for a, b in zip("qkvo", ("self.query", "self.key", "self.value", "output.dense"))]
TO_BERT += [("attention.LayerNorm.", "attention.output.LayerNorm."), ("encoder.relative_attention_bias.", "embeddings.token_type_embeddings.")]


@pytest.fixture(scope="module")
def small(zoo):
    return zoo.mpnet(**KW)


@pytest.mark.parametrize("nb", [8, 32])
def test_rows_are_hfs_buckets(spi, nb):
    from transformers.models.mpnet.modeling_mpnet import MPNetEncoder
    ops = importlib.import_module("starpu-inference-server_amd.ops")
    P, heads = 512, 3
    table = np.random.default_rng(nb).standard_normal((nb, heads)).astype(np.float32)
    bucket = MPNetEncoder.relative_position_bucket(torch.arange(P)[None] - torch.arange(P)[:, None], num_buckets=nb).numpy()
    rows = ops.rel_bias_rows(table, P)
    assert rows.shape == (heads, 1024) and not rows[:, 2 * P - 1:].any()
    q, k = np.meshgrid(np.arange(P), np.arange(P), indexing="ij")
    assert np.array_equal(rows[:, k - q + P - 1], table[bucket].transpose(2, 0, 1))


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_replica_metadata(spi, small, prec):
    rep = spi.ModelReplica(small, -1, prec, max_batch=2)  # family, positions and eps from the names and the config
    assert rep.bert_io == 1024 and f" S<={ROWS - 2} " in rep.description and rep.description.endswith(" pos[ids] relbias32")
    n = C.c_int32(-1)
    assert spi.lib.spi_model_plan_check(rep.handle, 2, ROWS - 2, C.byref(n)) == 0 and n.value > 0
    as_bert = RR.Renamed(spi, small, rename=TO_BERT, edit={TABLE: lambda a: np.zeros((1, D), np.float32)})
    plain = spi.ModelReplica(as_bert, -1, prec, max_batch=2, num_heads=HEADS, eps=1e-5, bert_io="roberta_positions")
    assert plain.description + " relbias32" == rep.description and plain.flops(2) == rep.flops(2)
    assert rep.weight_bytes - plain.weight_bytes == HEADS * 256 * 4  # ld = round_up(2 * 128 - 1, 4)


def test_refusals(spi, zoo, small):
    def refuses(module, match, **kw):
        with pytest.raises(spi.InferenceExecutionException, match=match):
            spi.ModelReplica(module, -1, "fp16", **{**dict(num_heads=HEADS, eps=1e-5), **kw})
    refuses(small, "SPI_BERT_TOKEN_TYPES: an MPNet replica has no token-type table", bert_io="token_types")
    refuses(zoo.mpnet(**{**KW, "heads": 4}), r"relative_attention_bias\.weight.*64-wide heads only", num_heads=4)
    refuses(RR.Renamed(spi, small, edit={TABLE: lambda a: np.zeros((32, HEADS + 1), np.float32)}), r"must be \[nb\]\[heads\]")
    refuses(RR.Renamed(spi, small, edit={TABLE: lambda a: a[:30]}), "30 buckets")
    refuses(RR.Renamed(spi, small, rename=[("layer.1.attention.attn.q.", "layer.1.attention.self.query.")]),
            r"mixed BERT and MPNet attention names: 'encoder\.layer\.1\.attention\.self\.query\.weight'")
    refuses(RR.Renamed(spi, small, rename=[("relative_attention_bias", "other")]), "mixed BERT and MPNet attention names")

"""Replicas with 32-wide attention heads on the GPU against the CPU oracle, at test_parity_gpu's bars: the
2-layer, 128-wide, 4-head BERT (max_position 512) at S = 17, 128, 129 and 300, and a 4-head, 128-wide ViT at
S = 65 and 197.  32-wide heads always take the QKV GEMM + the standalone attention kernels (the fused QKV +
attention kernel serves 64-wide heads only), whatever SPI_QKV_ATTN says: S = 17 .. 128 run
attn_f16_swapped_kernel<4, 0, 32>, 129 and 197 the whole-sequence <16, 224, 32>, 300 the tiled <8, 0, 32>.

Measured on an MI355X (each test prints its figure):
  BERT (init_std 0.05) against the oracle, S = 17 / 128 / 129 / 300: fp32 3.0e-7 .. 4.1e-7, fp16x3 3.6e-7 ..
  4.1e-7, fp16 2.2e-4 .. 2.3e-4 (2.5e-4 / 2.7e-4 without the LayerNorm fold), fp16m 1.5e-4 .. 1.6e-4.  The same
  weights served as two 64-wide heads land 8.6e-3 from the oracle, past every precision's bar.
  ViT against the oracle: fp32 6.7e-7 (S = 197) and 6.8e-7 (S = 65); fp16 4.7e-4 (S = 197) and 6.7e-4 (S = 65).
"""
import functools
import importlib

import numpy as np
import pytest
import torch

from oracle.cpu_codelet import cpu_inference, normalized_max_error
from test_bert_io_gpu import TOL_NEW, mean_ref
from test_parity_gpu import TOL, assert_standalone_route, bert_inputs, hip_forward, image, op_names

pytestmark = pytest.mark.gpu

B = 3
KW = dict(max_batch=B, seq_len=512)


@functools.lru_cache(maxsize=None)
def bert32():
    zoo = importlib.import_module("starpu-inference-server_amd.zoo")
    # init_std 0.05 (test_parity_gpu.bert_long's): HF's 0.02 keeps every softmax near uniform, and the same
    # weights split into two 64-wide heads then land inside the fp16 bar of the right model
    return zoo.bert(layers=2, hidden=128, heads=4, intermediate=512, vocab=1000, max_position=512, init_std=0.05)


@functools.lru_cache(maxsize=None)
def bert_case(S):
    """Three sequences of S tokens, the last padded from about 0.6 S, and the oracle's output, computed once."""
    ids, mask = bert_inputs(np.random.default_rng(53 + S), B, S, vocab=1000, pad_from=max(1, int(0.6 * S)))
    ref = cpu_inference(bert32(), [ids, mask])[0]
    ref.setflags(write=False)
    return ids, mask, ref


def attention_ops(names):
    return sorted(n for n in names if "attention" in n)


@pytest.mark.parametrize("prec", ["fp32", "fp16", "fp16m", "fp16x3"])
@pytest.mark.parametrize("S", [17, 128, 129, 300])
def test_bert_oracle_parity(spi, gpu, S, prec):
    ids, mask, ref = bert_case(S)
    rep = spi.ModelReplica(bert32(), 0, prec, num_heads=4, **KW)
    assert " H4 " in rep.description
    got = hip_forward(spi, rep, [ids, mask], ref.shape)
    names = op_names(rep, [ids, mask], ref.shape)
    e = normalized_max_error(got, ref)
    print(f"bert hd32 S{S} {prec}: vs oracle {e:.3e}, ops {attention_ops(names)}")
    assert_standalone_route(names, S)
    assert np.isfinite(got).all() and e < TOL[prec], e


@pytest.mark.parametrize("fold", ["1", "0"])
@pytest.mark.parametrize("S", [17, 128])
def test_bert_default_is_the_pair(spi, gpu, S, fold, monkeypatch):
    """fp16, with and without the LayerNorm fold: the default route and SPI_QKV_ATTN=0 / 2 are the same launches
    at width 32 (test_parity_gpu.test_bert_qkv_attention_fused's comparison, which at width 64 is fused against
    pair), so the outputs are equal bit for bit."""
    ids, mask, ref = bert_case(S)
    monkeypatch.setenv("SPI_LN_FOLD", fold)
    outs = {}
    for knob in (None, "0", "2"):
        if knob is not None:
            monkeypatch.setenv("SPI_QKV_ATTN", knob)
        rep = spi.ModelReplica(bert32(), 0, "fp16", num_heads=4, **KW)
        outs[knob] = hip_forward(spi, rep, [ids, mask], ref.shape)
        assert_standalone_route(op_names(rep, [ids, mask], ref.shape), S)
    e = normalized_max_error(outs[None], ref)
    print(f"bert hd32 S{S} fold{fold}: vs oracle {e:.3e}")
    assert e < TOL["fp16"], e
    assert np.array_equal(outs[None], outs["0"]) and np.array_equal(outs[None], outs["2"])


@pytest.mark.parametrize("S", [128, 300])
def test_bert_graphs(spi, gpu, S):
    ids, mask, ref = bert_case(S)
    rep = spi.ModelReplica(bert32(), 0, "fp16", num_heads=4, **KW)
    eager = hip_forward(spi, rep, [ids, mask], ref.shape)
    graph = hip_forward(spi, rep, [ids, mask], ref.shape, graphs=True)
    assert np.array_equal(eager, graph) and normalized_max_error(graph, ref) < TOL["fp16"]


def test_bert_masked_mean(spi, gpu):
    ids, mask, ref = bert_case(128)
    rep = spi.ModelReplica(bert32(), 0, "fp16", num_heads=4, bert_io="mean", **KW)
    ins = [torch.from_numpy(x).cuda() for x in (ids, mask)]
    outs = [torch.full(s, float("nan"), device="cuda") for s in (ref.shape, (B, 128))]
    spi.run_hip(rep, ins, outs, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    hidden, mean = (o.cpu().numpy() for o in outs)
    e, em = normalized_max_error(hidden, ref), normalized_max_error(mean, mean_ref(hidden, mask))
    print(f"bert hd32 mean: hidden {e:.3e}, mean on the GPU's hidden {em:.3e}")
    assert e < TOL["fp16"] and em < TOL_NEW


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_head_count_from_the_module_is_the_same_replica(spi, gpu, prec):
    ids, mask, ref = bert_case(128)
    stated = spi.ModelReplica(bert32(), 0, prec, num_heads=4, **KW)
    found = spi.ModelReplica(bert32(), 0, prec, num_heads=0, **KW)
    assert found.description == stated.description and found.weight_digest == stated.weight_digest
    a, b = (hip_forward(spi, r, [ids, mask], ref.shape) for r in (stated, found))
    assert np.array_equal(a, b)
    two = hip_forward(spi, spi.ModelReplica(bert32(), 0, prec, num_heads=2, **KW), [ids, mask], ref.shape)
    d = normalized_max_error(two, ref)  # two 64-wide heads on the same weights: another model
    print(f"bert hd32 {prec}: the replica of two 64-wide heads is {d:.3e} from the oracle")
    assert d > 2 * TOL["fp16"], d  # every precision's parity bar tells the wrong head split apart


@pytest.mark.parametrize("qkv_attn", [None, "2"], ids=["default", "fused256"])
@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("img", [64, 112])
def test_vit_oracle_parity(spi, zoo, gpu, img, prec, qkv_attn, monkeypatch):
    S = (img // 8) ** 2 + 1
    m = zoo.vit(image=img, patch=8, layers=2, heads=4, dim=128, mlp_dim=256, num_classes=10)
    x = image(np.random.default_rng(59 + img), 2, img)
    ref = cpu_inference(m, [x])[0]
    if qkv_attn is not None:
        monkeypatch.setenv("SPI_QKV_ATTN", qkv_attn)
    rep = spi.ModelReplica(m, 0, prec, max_batch=2, image_size=img)
    assert " H4 " in rep.description
    got = hip_forward(spi, rep, [x], ref.shape)
    names = op_names(rep, [x], ref.shape)
    e = normalized_max_error(got, ref)
    print(f"vit hd32 S{S} {prec} SPI_QKV_ATTN={qkv_attn}: vs oracle {e:.3e}, ops {attention_ops(names)}")
    assert_standalone_route(names, S)
    assert np.isfinite(got).all() and e < TOL[prec], e

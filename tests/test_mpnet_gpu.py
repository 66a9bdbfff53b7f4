"""MPNet replicas on the GPU against HF's MPNetModel on the CPU (oracle.cpu_codelet), ids with trailing and interior
pads; bars and helpers are test_roberta_gpu's.  Measured on an MI355X, hidden state: small fp32 1.7e-7, fp16 2.9e-5,
unfolded 2.8e-5; wide fp32 4.0e-7, fp16 1.25e-4, unfolded 1.21e-4; pooler and mean on the GPU's own rows <= 1.6e-7."""
import functools

import numpy as np
import pytest

import roberta_refs as RR
from test_roberta_gpu import (MODELS, MODES, ROWS, TOL, TOL_NEW, VOCAB, dense64, forward, make_inputs, mean64, npw, oracle,
                              setenv_mode)

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def model(zoo, which, head=None):
    kw = {k: v for k, v in MODELS[which][0].items() if k != "init_std"}
    return zoo.mpnet(vocab=VOCAB, max_position=ROWS, head=head, num_labels=3, **kw)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("which", ["small", "wide"])
def test_parity_with_the_hf_module(spi, zoo, gpu, which, mode, monkeypatch):
    prec = setenv_mode(monkeypatch, mode)
    m = model(zoo, which)
    (B, S), D = MODELS[which][1], m.bert.config.hidden_size
    ids, mask = make_inputs(B, S)
    ref_h = oracle(("mpnet", which), zoo.BertTupleWrapper(m.bert), [ids, mask], 2)[0]
    rep = spi.ModelReplica(m, 0, prec, max_batch=B, bert_io=("pooler", "mean"))
    got_h, got_p, got_m = forward(spi, rep, [ids, mask], D)
    eh = RR.err1(got_h, ref_h)
    ep = RR.err1(got_p, np.tanh(dense64(got_h[:, 0], *npw(m.bert.pooler.dense))))
    em = RR.err1(got_m, mean64(got_h, mask))
    print(f"mpnet {which} {mode}: hidden {eh:.3e}; on the GPU's own rows: pooler {ep:.3e} mean {em:.3e}")
    assert eh < TOL[prec]
    assert max(ep, em) < TOL_NEW
    for _ in range(2):  # graphs on (two replays) equals graphs off, and sequence 0 alone its slice of the batch, bit for bit
        assert np.array_equal(forward(spi, rep, [ids, mask], D, graphs=True)[0], got_h)
    for graphs in ((False, True) if which == "small" else ()):  # wide: the GEMM plans of 128 and 256 rows differ
        assert np.array_equal(forward(spi, rep, [ids[:1], mask[:1]], D, graphs=graphs)[0][0], got_h[0]), graphs


def test_two_layer_sequence_head(spi, zoo, gpu):
    m = model(zoo, "small", "sequence")
    B, (ids, mask) = 3, make_inputs(*MODELS["small"][1])
    ref = oracle(("mpnet", "seq"), m, [ids, mask], 2)
    hidden, logits = forward(spi, spi.ModelReplica(m, 0, "fp16", max_batch=B, bert_io="seq_head"), [ids, mask], 128)
    want = dense64(np.tanh(dense64(hidden[:, 0], *npw(m.model.classifier.dense))), *npw(m.model.classifier.out_proj))
    assert logits.shape == (B, 3) and RR.err1(hidden, ref[0]) < TOL["fp16"] and RR.err1(logits, want) < TOL_NEW

"""RoBERTa-class encoders (SPI_BERT_POS_FROM_IDS and the two-layer sequence head), host side: what the packer
accepts, resolves and refuses on host-only replicas (device -1), the Python surface (auto-detection from the HF
config, the pad-id refusal, eps from the config), and the numpy restatements of roberta_refs.py against HF's own
create_position_ids_from_input_ids and RobertaEmbeddings."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import roberta_refs as RR

VOCAB, ROWS, D = 100, 34, 128
KW = dict(layers=2, hidden=D, heads=2, intermediate=256, vocab=VOCAB, max_position=ROWS)


@pytest.fixture(scope="module")
def cd():
    return importlib.import_module("starpu-inference-server_amd.codelet")


@pytest.fixture(scope="module")
def small(zoo):
    return zoo.roberta(**KW)


@pytest.fixture(scope="module")
def seq_model(zoo):
    return zoo.roberta(head="sequence", num_labels=3, **KW)


def steps(spi, rep, B, S):
    n = C.c_int32(-1)
    st = spi.lib.spi_model_plan_check(rep.handle, B, S, C.byref(n))
    return st, n.value, spi.lib.spi_last_error().decode()


@pytest.mark.parametrize("prec", ["fp32", "fp16", "fp16m"])
def test_the_bit_changes_the_description_only(spi, cd, small, prec):
    """The same tensors packed with and without the bit: digest, bytes, FLOPs and the workspace walk are equal,
    the description gains the marker, and bert_io carries the bit for the Python side."""
    assert cd.BERT_IO["roberta_positions"] == 1024 == spi._native.BERT_POS_FROM_IDS and spi._native.ROBERTA_PAD_ID == 1
    plain_tensors = RR.Renamed(spi, small)  # no config: nothing is detected
    off = spi.ModelReplica(plain_tensors, -1, prec, num_heads=2, seq_len=16, eps=1e-5)
    on = spi.ModelReplica(plain_tensors, -1, prec, num_heads=2, seq_len=16, eps=1e-5, bert_io="roberta_positions")
    auto = spi.ModelReplica(small, -1, prec, seq_len=16)
    assert off.bert_io == 0 and on.bert_io == 1024 == auto.bert_io
    assert " pos[ids]" not in off.description
    for r in (on, auto):
        assert r.description == off.description + " pos[ids]"
        assert (r.weight_digest, r.weight_bytes) == (off.weight_digest, off.weight_bytes)
        assert r.flops(3) == off.flops(3) and r.num_labels == 0
        assert steps(spi, r, 3, 16)[:2] == steps(spi, off, 3, 16)[:2]
    typed = spi.ModelReplica(small, -1, prec, seq_len=16, bert_io=("mean", "no_hidden"))
    assert typed.bert_io == 1024 | 2 | 4 and typed.description.endswith(" out[mean] in[ids,mask] pos[ids]")
    assert cd.output_specs(2, seq=16, dim=D, bert_io=typed.bert_io) == cd.output_specs(2, seq=16, dim=D, bert_io=6)


def test_seq_len_is_the_table_minus_two(spi, small):
    rep = spi.ModelReplica(small, -1, "fp16", max_batch=2)
    assert f" S<={ROWS - 2} " in rep.description
    st, n, err = steps(spi, rep, 2, ROWS - 2)
    assert st == 0 and n > 0, err
    st, n, err = steps(spi, rep, 1, ROWS - 1)
    assert st != 0 and "plan_check" in err, err
    assert f" S<={ROWS - 2} " in spi.ModelReplica(small, -1, "fp16", seq_len=ROWS - 2).description
    for too_long in (ROWS - 1, ROWS, 4 * ROWS):
        with pytest.raises(spi.InferenceExecutionException, match=rf"seq_len {too_long} .*{ROWS} rows.*rows - 2 = {ROWS - 2}"):
            spi.ModelReplica(small, -1, "fp16", seq_len=too_long)
    # without the bit the same table serves its whole length, as before
    assert f" S<={ROWS} " in spi.ModelReplica(RR.Renamed(spi, small), -1, "fp16", num_heads=2).description


def test_an_over_long_task_is_refused(spi, small):
    N = spi._native
    rep = spi.ModelReplica(small, -1, "fp16", max_batch=2)

    def call(S):
        ins = [torch.zeros(2 * S, dtype=torch.int64) for _ in range(2)]
        out = torch.zeros(2 * S * D)
        params = spi.make_params([[2, S]] * 2, [torch.int64] * 2, models_gpu=[rep])
        bufs = [spi.tensor_interface(t) for t in ins] + [spi.tensor_interface(out)]
        with spi.worker_context(0, 0, None):
            with pytest.raises(spi.StarPUCodeletException) as e:
                spi.InferenceCodelet.hip_inference_func(bufs, params)
        return e.value.status, str(e.value)
    st, msg = call(ROWS - 2)  # the contract holds: only the missing device stops it
    assert st == N.SPI_ERR_DEVICE and "host-only replica" in msg, msg
    st, msg = call(ROWS - 1)
    assert st != N.SPI_ERR_DEVICE and f"sequence length {ROWS - 1} exceeds {ROWS - 2}" in msg, msg


def test_refusals(spi, zoo, small):
    def refuses(module, io, match, **kw):
        with pytest.raises(spi.InferenceExecutionException, match=match):
            spi.ModelReplica(module, -1, "fp16", bert_io=io, **kw)
    resnet = zoo.resnet([1, 1, 1, 1], False, image=64, calibrate=False)
    vit = zoo.vit(image=32, patch=16, layers=2, heads=2, dim=128, mlp_dim=256, num_classes=10)
    refuses(resnet, "roberta_positions", "not a BERT", image_size=64)
    refuses(vit, 1024, "not a BERT", num_heads=2, image_size=32)
    with pytest.raises(spi.InferenceExecutionException, match="not a BERT"):
        spi.ModelReplica(None, -1, "fp32", family="affine", bert_io="roberta_positions")
    # bits 16, 32 and 64 stay unknown, with and without the new one (test_bert_io's assertion, restated)
    refuses(small, 16, "unknown bits 16", seq_len=16)
    refuses(small, 1 | 32 | 64, "unknown bits 96", seq_len=16)
    refuses(small, 1024 | 16, "unknown bits 16", seq_len=16)
    refuses(small, 2048, "unknown bits 2048", seq_len=16)
    tiny = RR.Renamed(spi, small, edit={"bert.embeddings.position_embeddings.weight": lambda a: a[:2]})
    refuses(tiny, "roberta_positions", "2 rows", num_heads=2)


def test_two_layer_sequence_head(spi, seq_model):
    """classifier.dense / classifier.out_proj are packed where pooler.dense / classifier go: the digest of the
    same tensors under BERT's names."""
    names = [n for n, _ in spi.named_tensors(seq_model)]
    assert "model.classifier.out_proj.weight" in names and not any("pooler" in n for n in names)
    rep = spi.ModelReplica(seq_model, -1, "fp16", seq_len=16, bert_io="seq_head")
    assert rep.num_labels == 3 and rep.bert_io == 1024 | 128
    assert rep.description.endswith(" out[hidden,seq_logits3] in[ids,mask] pos[ids]")
    renamed = RR.Renamed(spi, seq_model, rename=[("model.classifier.dense.", "model.roberta.pooler.dense."),
                                                 ("model.classifier.out_proj.", "model.classifier.")])
    for io in (("seq_head",), ("no_hidden", "seq_head"), ("mean", "seq_head")):
        a = spi.ModelReplica(seq_model, -1, "fp16", seq_len=16, bert_io=io)
        b = spi.ModelReplica(renamed, -1, "fp16", num_heads=2, seq_len=16, eps=1e-5, bert_io=io + ("roberta_positions",))
        assert (a.weight_digest, a.weight_bytes, a.description, a.flops(3), a.num_labels) == \
               (b.weight_digest, b.weight_bytes, b.description, b.flops(3), b.num_labels), io
    # the names decide, not the position bit: the same head under BERT's position rule
    plain = spi.ModelReplica(RR.Renamed(spi, seq_model), -1, "fp16", num_heads=2, seq_len=16, bert_io="seq_head")
    assert plain.bert_io == 128 and plain.num_labels == 3 and plain.weight_digest == rep.weight_digest
    plan_on, plan_off = steps(spi, rep, 3, 16), steps(spi, plain, 3, 16)
    assert plan_on[0] == 0 and plan_on[:2] == plan_off[:2]


def test_two_layer_sequence_head_refusals(spi, seq_model):
    def refuses(module, io, match):
        with pytest.raises(spi.InferenceExecutionException, match=match):
            spi.ModelReplica(module, -1, "fp16", num_heads=2, seq_len=16, bert_io=io)
    refuses(seq_model, ("pooler", "seq_head"), r"SPI_BERT_OUT_POOLER.*'classifier\.dense\.weight'.*'classifier\.out_proj\.weight'")
    refuses(seq_model, "pooler", r"needs parameter 'pooler\.dense\.weight'")  # RoBERTa's head model has no pooler
    for gone in ("weight", "bias"):
        m = RR.Renamed(spi, seq_model, rename=[(f"classifier.dense.{gone}", f"classifier.other.{gone}")])
        refuses(m, "seq_head", rf"SPI_BERT_HEAD_SEQUENCE needs parameter 'classifier\.dense\.{gone}'")
    m = RR.Renamed(spi, seq_model, rename=[("classifier.out_proj.bias", "classifier.other.bias")])
    refuses(m, "seq_head", r"needs parameter 'classifier\.out_proj\.bias'")
    m = RR.Renamed(spi, seq_model, edit={"model.classifier.dense.weight": lambda a: a[:, :64]})
    refuses(m, "seq_head", r"classifier\.dense must be \[D\]\[D\]")
    m = RR.Renamed(spi, seq_model, edit={"model.classifier.dense.bias": lambda a: a[:64]})
    refuses(m, "seq_head", r"classifier\.dense must be \[D\]\[D\]")
    m = RR.Renamed(spi, seq_model, edit={"model.classifier.out_proj.weight": lambda a: a[:, :64]})
    refuses(m, "seq_head", r"classifier\.out_proj\.weight must be \[L\]\[D\]")
    m = RR.Renamed(spi, seq_model, edit={"model.classifier.out_proj.bias": lambda a: a[:2]})
    refuses(m, "seq_head", r"classifier\.out_proj\.weight must be \[L\]\[D\]")


def test_token_and_qa_heads_match_the_existing_lookups(spi, zoo):
    for head, bit, labels, out in (("token", "token_head", 5, "token_logits5"), ("qa", "qa_head", 2, "qa_start,qa_end")):
        m = zoo.roberta(head=head, num_labels=5, **KW)
        rep = spi.ModelReplica(m, -1, "fp16", seq_len=16, bert_io=bit)
        assert rep.num_labels == labels and rep.description.endswith(f" out[hidden,{out}] in[ids,mask] pos[ids]")


def test_detection_pad_id_and_eps(spi, zoo, cd, small, monkeypatch):
    assert cd.module_roberta_positions(small) and cd.module_layer_norm_eps(small) == 1e-5
    bert = zoo.bert(layers=1, hidden=128, heads=2, intermediate=256, vocab=VOCAB, max_position=ROWS)
    assert not cd.module_roberta_positions(bert) and cd.module_layer_norm_eps(bert) == 1e-12
    assert not cd.module_roberta_positions(RR.Renamed(spi, small)) and cd.module_layer_norm_eps(RR.Renamed(spi, small)) == 0.0
    assert spi.ModelReplica(bert, -1, "fp16").bert_io == 0
    for model_type in ("xlm-roberta", "camembert"):
        monkeypatch.setattr(small.bert.config, "model_type", model_type, raising=False)
        assert spi.ModelReplica(small, -1, "fp16").bert_io == 1024
    monkeypatch.setattr(small.bert.config, "model_type", "roberta", raising=False)
    monkeypatch.setattr(small.bert.config, "pad_token_id", 0)
    with pytest.raises(spi.InferenceExecutionException, match=r"pad_token_id 0\b"):
        spi.ModelReplica(small, -1, "fp16")
    monkeypatch.setattr(small.bert.config, "pad_token_id", None)
    with pytest.raises(spi.InferenceExecutionException, match="pad_token_id None"):
        spi.ModelReplica(small, -1, "fp16")
    monkeypatch.undo()
    # eps: the config's where the caller states none, the caller's otherwise (seen through the native config)
    seen = []
    real = spi.lib.spi_model_create

    def spy(dev, cfg, *a):
        seen.append((cfg._obj.eps, cfg._obj.bert_io))
        return real(dev, cfg, *a)
    monkeypatch.setattr(cd.lib, "spi_model_create", spy)
    spi.ModelReplica(small, -1, "fp16")
    spi.ModelReplica(small, -1, "fp16", eps=1e-6)
    spi.ModelReplica(bert, -1, "fp16")
    spi.ModelReplica(RR.Renamed(spi, small), -1, "fp16", num_heads=2)
    f32 = lambda x: float(np.float32(x))  # noqa: E731
    assert seen == [(f32(1e-5), 1024), (f32(1e-6), 1024), (f32(1e-12), 0), (0.0, 0)]


def test_zoo_roberta_entries(zoo, monkeypatch):
    m = zoo.build("roberta_base", layers=1, vocab=VOCAB)
    cfg = m.bert.config
    assert (cfg.model_type, cfg.pad_token_id, cfg.type_vocab_size, cfg.layer_norm_eps) == ("roberta", 1, 1, 1e-5)
    assert (cfg.hidden_size, cfg.num_attention_heads, cfg.intermediate_size, cfg.max_position_embeddings) == (768, 12, 3072, 514)
    assert float(m.bert.embeddings.position_embeddings.weight[1].detach().abs().max()) > 0  # the pad row is not zero
    large = zoo.build("xlm_roberta_large", layers=1, vocab=VOCAB).bert.config
    assert (large.hidden_size, large.num_attention_heads, large.intermediate_size, large.vocab_size) == (1024, 16, 4096, VOCAB)
    with pytest.raises(ValueError, match="no pooler"):
        zoo.roberta(head="sequence", outputs=("hidden", "pooler"), **KW)
    # the named entries' own sizes, without allocating their 250002-row tables
    monkeypatch.setattr(zoo, "roberta", lambda **kw: kw)
    assert zoo.build("roberta_base", seed=3) == dict(seed=3)
    assert zoo.build("xlm_roberta_base") == dict(vocab=250002, seed=0)
    assert zoo.build("xlm_roberta_large", head="token") == dict(layers=24, hidden=1024, heads=16, intermediate=4096,
                                                                 vocab=250002, head="token", seed=0)
    assert zoo.build("xlm_roberta_base", vocab=VOCAB)["vocab"] == VOCAB


# ---- the position rule and the embedding reference against HF's own code -----------------------------

@pytest.mark.parametrize("S", [1, 17, 64, 65, 130])
@pytest.mark.parametrize("pattern", RR.PATTERNS)
def test_position_rule_is_hfs(pattern, S):
    from transformers.models.roberta import modeling_roberta as M
    hf = getattr(M.RobertaEmbeddings, "create_position_ids_from_input_ids", None) or M.create_position_ids_from_input_ids
    for B in (1, 3):
        ids = RR.pad_ids(RR.token_ids(np.random.default_rng(S + B), B, S, VOCAB), pattern)
        want = hf(torch.from_numpy(ids), 1).numpy()
        got = RR.position_ids(ids)
        assert np.array_equal(got, want), (pattern, B, S)
        assert got.max() <= S + 1 and (got[ids == 1] == 1).all() and (got[ids != 1] >= 2).all()
    if pattern == "none":
        assert np.array_equal(got, np.broadcast_to(np.arange(S) + 2, got.shape))


@pytest.mark.parametrize("pattern", RR.PATTERNS)
def test_embedding_reference_is_roberta_embeddings(small, pattern):
    """roberta_refs.embed_ref (fp32 sum, float64 LayerNorm) against HF's RobertaEmbeddings on the zoo model, whose
    position row 1 is not zero; the bar is the op's fp32 one (2e-6)."""
    emb = small.bert.embeddings
    B, S = 3, ROWS - 2
    ids = RR.pad_ids(RR.token_ids(np.random.default_rng(5), B, S, VOCAB, clamped=False), pattern)
    with torch.inference_mode():
        want = emb(input_ids=torch.from_numpy(ids)).numpy().reshape(B * S, D)
    f = lambda t: t.detach().numpy()  # noqa: E731
    got = RR.embed_ref(ids, f(emb.word_embeddings.weight), f(emb.position_embeddings.weight),
                       f(emb.token_type_embeddings.weight), None, f(emb.LayerNorm.weight), f(emb.LayerNorm.bias), 1e-5)
    err = RR.err1(want, got)
    print(f"embed_ref against RobertaEmbeddings, {pattern}: {err:.3e}")
    assert err < 2e-6

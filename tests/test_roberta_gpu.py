"""RoBERTa-class encoders on the GPU: spi_op_bert_embed_posids against a float64 reference (roberta_refs.py,
which test_roberta.py holds to HF's code) and, bit for bit, against spi_op_bert_embed on pad-free ids; then
replicas -- exact against a BERT-style replica of the same tensors, parity against the HF module on the CPU,
the two-layer sequence head, batch independence, TorchScript and the mini-runtime.

Bars (the project's existing ones, metric max|got - ref| / max(1, max|ref|)): op yf 2e-6 and fp16 yt 1e-3;
replica hidden state against the CPU oracle 1e-5 fp32 / 1e-3 fp16; head logits, pooler and mean against the float64
formula on the GPU's own rows 1e-5.  The position table of the op tests is N(0,1), so a wrong row is an O(1) error.
"""
import importlib

import numpy as np
import pytest
import torch

import roberta_refs as RR
from oracle.cpu_codelet import cpu_inference

pytestmark = pytest.mark.gpu

TOL = {"fp32": 1e-5, "fp16": 1e-3}  # test_parity_gpu.TOL
TOL_NEW = 1e-5
TOL_LN32, TOL16 = 2e-6, 1e-3        # test_elementwise_ops_gpu's bars for bert_embed (yf; fp16 yt)
GUARD = 8
NAN = float("nan")
EPS = 1e-5
FMIN = np.finfo(np.float32).min


@pytest.fixture(scope="module")
def ops(spi, gpu):
    return importlib.import_module("starpu-inference-server_amd.ops")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def guarded(rows, *tail, dtype=torch.float32):
    return torch.full((rows + GUARD, *tail), NAN, dtype=dtype, device="cuda")


def take(t, rows, what):
    torch.cuda.synchronize()
    assert bool(torch.isnan(t[rows:]).all()), f"{what}: rows past the output were written"
    got = t[:rows].cpu()
    assert not bool(torch.isnan(got).any()), f"{what}: rows of the output were left unwritten"
    return got


def offset_copy(a, elems=1):
    """A device copy of fp32 `a` that starts `elems` floats past an aligned allocation."""
    flat = torch.zeros(a.size + elems, device="cuda", dtype=torch.float32)
    view = flat[elems:].view(a.shape)
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return view


# ---- op: bert_embed_posids -------------------------------------------------------------------------

OP_VOCAB, NPOS = 50, 514
OP_S = (1, 17, 64, 65, 130, 512)  # the wave counts 64 ids a step and loads four steps at once: 64 | 65, 256 | 257
OP_B = (1, 3)
_tables = {}


def tables(D):
    """word, pos ~ N(0,1) (a wrong position row is an O(1) error), a two-row type table, gamma, beta: host
    arrays and device copies, made once per D."""
    if D not in _tables:
        rng = np.random.default_rng(D)
        h = dict(word=rng.standard_normal((OP_VOCAB, D)), pos=rng.standard_normal((NPOS, D)),
                 types=0.3 * rng.standard_normal((2, D)), gamma=1 + 0.3 * rng.standard_normal(D),
                 beta=rng.standard_normal(D))
        h = {k: v.astype(np.float32) for k, v in h.items()}
        for v in h.values():
            v.setflags(write=False)
        _tables[D] = (h, {k: dev(v) for k, v in h.items()})
    return _tables[D]


def op_inputs(B, S, pattern, extras):
    rng = np.random.default_rng(B * 1000 + S)
    ids = RR.pad_ids(RR.token_ids(rng, B, S, OP_VOCAB), pattern)
    if not extras:
        return ids, None, None
    mask = (np.arange(B * S) % 3 != 1).astype(np.int64).reshape(B, S)  # unrelated to the pads: the rule reads ids only
    type_ids = rng.integers(0, 2, (B, S), dtype=np.int64)
    type_ids[0, :2] = (-1, 5)[:S]  # clamped to rows 0 and 1
    return ids, mask, type_ids


def run_posids(ops, prec, D, ids, mask, type_ids, pos=None, yt=True):
    h, d = tables(D)
    B, S = ids.shape
    M = B * S
    yf = guarded(M, D)
    ytd = guarded(M, D, dtype=torch.float16 if prec == "fp16" else torch.float32) if yt else None
    mb = guarded(M) if mask is not None else None
    ops.bert_embed_posids(prec, dev(ids), d["word"], d["pos"] if pos is None else pos, d["types"],
                          dev(type_ids) if type_ids is not None else None, d["gamma"], d["beta"], yf, ytd, B, S, D, EPS,
                          mask=dev(mask) if mask is not None else None, mask_bias=mb)
    what = f"bert_embed_posids {prec} B{B} S{S} D{D}"
    got_mb = take(mb, M, what).numpy() if mb is not None else None
    return take(yf, M, what).numpy(), (take(ytd, M, what).float().numpy() if yt else None), got_mb


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("D", [64, 128, 768, 1024])  # 64, 128: the scalar form; 768, 1024: the vector form
def test_embed_posids_op(ops, D, prec):
    h, _ = tables(D)
    worst_f = worst_t = 0.0
    for S in OP_S:
        for B in OP_B:
            for extras in (False, True):
                for pattern in RR.PATTERNS:
                    ids, mask, type_ids = op_inputs(B, S, pattern, extras)
                    ref = RR.embed_ref(ids, h["word"], h["pos"], h["types"], type_ids, h["gamma"], h["beta"], EPS)
                    yf, yt, mb = run_posids(ops, prec, D, ids, mask, type_ids)
                    ef, et = RR.err1(yf, ref), RR.err1(yt, ref)
                    what = f"bert_embed_posids {prec} D{D} B{B} S{S} {pattern} extras={extras}"
                    worst_f, worst_t = max(worst_f, ef), max(worst_t, et)
                    assert ef < TOL_LN32, f"{what}: yf {ef:.3e}"
                    assert et < (TOL16 if prec == "fp16" else TOL_LN32), f"{what}: yt {et:.3e}"
                    if extras:
                        assert np.array_equal(mb, np.where(mask.reshape(-1) != 0, np.float32(0), FMIN)), what
    print(f"bert_embed_posids {prec} D{D}: worst yf {worst_f:.3e} yt {worst_t:.3e} over S {OP_S} x B {OP_B} x "
          f"{len(RR.PATTERNS)} pad patterns, with and without mask + segment ids")


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("D", [64, 128, 768, 1024])
def test_embed_posids_on_pad_free_ids_has_the_bits_of_bert_embed(ops, D, prec):
    """Pad-free ids take position rows 2 .. S + 1: spi_op_bert_embed (and _types) given pos + 2 D, bit for bit."""
    h, d = tables(D)
    for B, S in ((3, 17), (1, 130), (3, 512)):
        ids, mask, type_ids = op_inputs(B, S, "none", True)
        M = B * S
        yf, yt, mb = run_posids(ops, prec, D, ids, mask, None)
        zf, zt, zb = guarded(M, D), guarded(M, D, dtype=torch.float16 if prec == "fp16" else torch.float32), guarded(M)
        ops.bert_embed(prec, dev(ids), d["word"], d["pos"][2:], d["types"][0], d["gamma"], d["beta"], zf, zt, B, S, D, EPS,
                       mask=dev(mask), mask_bias=zb)
        what = f"bert_embed on pos + 2 D, {prec} B{B} S{S} D{D}"
        assert np.array_equal(yf, take(zf, M, what).numpy()), what
        assert np.array_equal(yt, take(zt, M, what).float().numpy()), what
        assert np.array_equal(mb, take(zb, M, what).numpy()), what
        yf, yt, _ = run_posids(ops, prec, D, ids, mask, type_ids)
        zf, zt = guarded(M, D), guarded(M, D, dtype=zt.dtype)
        ops.bert_embed_types(prec, dev(ids), d["word"], d["pos"][2:], d["types"], dev(type_ids), d["gamma"], d["beta"], zf,
                             zt, B, S, D, EPS)
        assert np.array_equal(yf, take(zf, M, what).numpy()) and np.array_equal(yt, take(zt, M, what).float().numpy()), what


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_embed_posids_on_unaligned_tables_takes_the_scalar_form(ops, prec):
    """D = 768 with the position table one float past an aligned address: the 16-byte gathers cannot run.
    Same bars; and without yt."""
    D, B, S = 768, 3, 65
    h, d = tables(D)
    ids, mask, type_ids = op_inputs(B, S, "edges", True)
    ref = RR.embed_ref(ids, h["word"], h["pos"], h["types"], type_ids, h["gamma"], h["beta"], EPS)
    pos1 = offset_copy(h["pos"])
    assert pos1.data_ptr() % 16 == 4
    yf, yt, _ = run_posids(ops, prec, D, ids, mask, type_ids, pos=pos1)
    ef, et = RR.err1(yf, ref), RR.err1(yt, ref)
    print(f"bert_embed_posids {prec} D768 unaligned pos: yf {ef:.3e} yt {et:.3e}")
    assert ef < TOL_LN32 and et < (TOL16 if prec == "fp16" else TOL_LN32)
    yf, yt, _ = run_posids(ops, prec, D, ids, mask, type_ids, yt=False)
    assert yt is None and RR.err1(yf, ref) < TOL_LN32


def test_embed_posids_rejections(ops):
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device="cuda")  # noqa: E731

    def call(B=2, S=8, D=64, npos=10, yf=True, mask=False, mask_bias=False, ok=False):
        M = B * S
        args = ("fp16", z(M, dt=torch.int64), z(OP_VOCAB, D), z(npos, D), z(2, D), None, z(D), z(D),
                z(M, D) if yf else None, z(M, D, dt=torch.float16), B, S, D, EPS)
        kw = dict(mask=z(M, dt=torch.int64) if mask else None, mask_bias=z(M) if mask_bias else None)
        if ok:
            return ops.bert_embed_posids(*args, **kw)
        with pytest.raises(ops.OpError):
            ops.bert_embed_posids(*args, **kw)

    call(ok=True)            # S + 2 == npos is served
    call(npos=9)             # S + 2 > npos
    call(S=8, npos=8)        # what spi_op_bert_embed takes
    call(D=1088, npos=16)    # D past the 16 values a lane holds
    call(yf=False)
    call(mask=True)          # mask without mask_bias
    call(mask_bias=True)
    torch.cuda.synchronize()


# ---- replicas --------------------------------------------------------------------------------------

VOCAB, ROWS = 1000, 130
MODELS = {  # which -> (zoo.roberta keywords, (B, S))
    "small": (dict(layers=2, hidden=128, heads=2, intermediate=256, init_std=0.05), (3, 17)),
    "wide": (dict(layers=1, hidden=768, heads=12, intermediate=3072), (2, 128)),  # the vector form
}
MODES = ["fp32", "fp16", "fp16_nofold"]
_cache = {}


def make_inputs(B, S, pads=True):
    """ids with trailing pads (row 1) and interior pads (the last row); token 0 is never a pad, so no sequence is
    fully masked.  mask = (ids != 1), as a tokenizer gives it."""
    ids = RR.token_ids(np.random.default_rng(B * S), B, S, VOCAB, clamped=False)
    if pads:
        ids[1, S // 2:] = RR.PAD
        ids[B - 1, [3, S // 3, S - 2]] = RR.PAD
        ids[B - 1, -1] = 7
    return ids, (ids != RR.PAD).astype(np.int64)


def model(zoo, which, head=None, labels=0):
    key = ("model", which, head, labels)
    if key not in _cache:
        kw = MODELS[which][0]
        _cache[key] = zoo.roberta(vocab=VOCAB, max_position=ROWS, head=head, num_labels=labels or 2, **kw)
    return _cache[key]


def oracle(key, module, inputs, n=1):
    if key not in _cache:
        ref = cpu_inference(module, inputs, num_outputs=n)
        for a in ref:
            a.setflags(write=False)
        _cache[key] = ref
    return _cache[key]


def forward(spi, rep, inputs, D, graphs=False):
    """One codelet call; every output with GUARD NaN words behind it that must stay NaN."""
    cd = importlib.import_module("starpu-inference-server_amd.codelet")
    B, S = inputs[0].shape
    shapes = [s for s, _ in cd.output_specs(B, seq=S, dim=D, bert_io=rep.bert_io, num_labels=rep.num_labels)]
    ins = [dev(x) for x in inputs]
    bufs = [torch.full((int(np.prod(s)) + GUARD,), NAN, device="cuda", dtype=torch.float32) for s in shapes]
    outs = [b[:int(np.prod(s))].view(s) for b, s in zip(bufs, shapes)]
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    rep.set_graphs(graphs)
    spi.run_hip(rep, ins, outs, stream=stream.cuda_stream)
    torch.cuda.synchronize()
    for b, s in zip(bufs, shapes):
        assert bool(torch.isnan(b[int(np.prod(s)):]).all()), f"output {s}: written past its end"
    got = [o.cpu().numpy() for o in outs]
    assert not any(np.isnan(g).any() for g in got)
    return got


def setenv_mode(monkeypatch, mode):
    if mode.endswith("nofold"):
        monkeypatch.setenv("SPI_LN_FOLD", "0")
    return mode.split("_")[0]


def dense64(h, W, b):
    return np.asarray(h, np.float64) @ np.asarray(W, np.float64).T + np.asarray(b, np.float64)


def mean64(h, mask):
    m = (np.asarray(mask) != 0).astype(np.float64)[..., None]
    return (np.asarray(h, np.float64) * m).sum(1) / np.maximum(m.sum(1), 1e-9)


def npw(linear):
    return linear.weight.detach().numpy(), linear.bias.detach().numpy()


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_replica_on_pad_free_ids_has_the_bits_of_a_bert_replica(spi, zoo, gpu, prec):
    """The RoBERTa replica against a BERT-style replica of the same tensors with position rows [2:]: on pad-free
    ids every row reads the same values, so the hidden state is equal bit for bit (the mask holds zeros: it does
    not enter the rule)."""
    m = model(zoo, "small")
    B, S = 3, 17
    ids, mask = make_inputs(B, S, pads=False)
    mask[1, 9:] = 0
    rob = spi.ModelReplica(m, 0, prec, max_batch=B)
    assert rob.bert_io == 1024 and rob.description.endswith(" pos[ids]") and f" S<={ROWS - 2} " in rob.description
    shifted = RR.Renamed(spi, m, edit={"bert.embeddings.position_embeddings.weight": lambda a: a[2:]})
    bert = spi.ModelReplica(shifted, 0, prec, max_batch=B, num_heads=2, eps=1e-5)
    assert bert.bert_io == 0 and f" S<={ROWS - 2} " in bert.description
    got, want = forward(spi, rob, [ids, mask], 128)[0], forward(spi, bert, [ids, mask], 128)[0]
    assert np.array_equal(got, want)
    padded = make_inputs(B, S)[0]
    assert not np.array_equal(forward(spi, rob, [padded, mask], 128)[0], forward(spi, bert, [padded, mask], 128)[0])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("which", ["small", "wide"])
def test_parity_with_the_hf_module(spi, zoo, gpu, which, mode, monkeypatch):
    """Hidden state against HF's RobertaModel on the CPU, with trailing and interior pads; the same with the
    third input (all-zero segment ids); then the pooler and masked-mean outputs."""
    prec = setenv_mode(monkeypatch, mode)
    m = model(zoo, which)
    B, S = MODELS[which][1]
    D = m.bert.config.hidden_size
    ids, mask = make_inputs(B, S)
    ref_h, ref_p = oracle(("tuple", which), zoo.BertTupleWrapper(m.bert), [ids, mask], 2)
    rep = spi.ModelReplica(m, 0, prec, max_batch=B)
    got = forward(spi, rep, [ids, mask], D)[0]
    eh = RR.err1(got, ref_h)
    zeros = np.zeros_like(ids)
    ref_t = oracle(("types", which), zoo.BertSegmentsWrapper(m.bert), [ids, mask, zeros])[0]
    typed = spi.ModelReplica(m, 0, prec, max_batch=B, bert_io="token_types")
    assert typed.description.endswith(" in[ids,mask,types] pos[ids]")
    got_t = forward(spi, typed, [ids, mask, zeros], D)[0]
    et = RR.err1(got_t, ref_t)
    pm = spi.ModelReplica(m, 0, prec, max_batch=B, bert_io=("pooler", "mean"))
    got_h, got_p, got_m = forward(spi, pm, [ids, mask], D)
    W, b = npw(m.bert.pooler.dense)
    ep = RR.err1(got_p, np.tanh(dense64(got_h[:, 0], W, b)))
    em = RR.err1(got_m, mean64(got_h, mask))
    print(f"roberta {which} {mode}: hidden {eh:.3e}, with segment ids {et:.3e}; on the GPU's own rows: pooler {ep:.3e} "
          f"mean {em:.3e}; against the oracle: pooler {RR.err1(got_p, ref_p):.3e} mean {RR.err1(got_m, mean64(ref_h, mask)):.3e}")
    assert eh < TOL[prec] and et < TOL[prec]
    assert np.array_equal(got_t, got) and np.array_equal(got_h, got)
    assert ep < TOL_NEW and em < TOL_NEW


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("L", [1, 3])  # 1: a reranker's single score
def test_two_layer_sequence_head(spi, zoo, gpu, L, prec):
    m = model(zoo, "small", "sequence", L)
    B, S = MODELS["small"][1]
    ids, mask = make_inputs(B, S)
    ref = oracle(("seq", L), m, [ids, mask], 2)
    rep = spi.ModelReplica(m, 0, prec, max_batch=B, bert_io="seq_head")
    assert rep.num_labels == L and rep.description.endswith(f" out[hidden,seq_logits{L}] in[ids,mask] pos[ids]")
    hidden, logits = forward(spi, rep, [ids, mask], 128)
    head = m.model.classifier
    want = dense64(np.tanh(dense64(hidden[:, 0], *npw(head.dense))), *npw(head.out_proj))
    eh, el = RR.err1(hidden, ref[0]), RR.err1(logits, want)
    print(f"roberta two-layer head L{L} {prec}: hidden {eh:.3e}; logits on the GPU's own rows {el:.3e}; "
          f"logits against the HF head model {RR.err1(logits, ref[1]):.3e}")
    assert logits.shape == (B, L) and eh < TOL[prec] and el < TOL_NEW
    renamed = RR.Renamed(spi, m, rename=[("model.classifier.dense.", "model.roberta.pooler.dense."),
                                         ("model.classifier.out_proj.", "model.classifier.")])
    twin = spi.ModelReplica(renamed, 0, prec, max_batch=B, num_heads=2, eps=1e-5, bert_io=("seq_head", "roberta_positions"))
    h2, l2 = forward(spi, twin, [ids, mask], 128)
    assert np.array_equal(h2, hidden) and np.array_equal(l2, logits)
    alone = forward(spi, spi.ModelReplica(m, 0, prec, max_batch=B, bert_io=("no_hidden", "seq_head")), [ids, mask], 128)
    assert len(alone) == 1 and RR.err1(alone[0], logits) < TOL_NEW


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("head", ["token", "qa"])
def test_token_and_qa_heads(spi, zoo, gpu, head, prec):
    m = model(zoo, "small", head, 5)
    B, S = MODELS["small"][1]
    ids, mask = make_inputs(B, S)
    n = 3 if head == "qa" else 2
    ref = oracle((head,), m, [ids, mask], n)
    rep = spi.ModelReplica(m, 0, prec, max_batch=B, bert_io=head + "_head")
    got = forward(spi, rep, [ids, mask], 128)
    y = dense64(got[0], *npw(m.model.qa_outputs if head == "qa" else m.model.classifier))
    want = [y[..., 0], y[..., 1]] if head == "qa" else [y]
    eh = RR.err1(got[0], ref[0])
    el = max(RR.err1(g, w) for g, w in zip(got[1:], want))
    direct = max(RR.err1(g, r) for g, r in zip(got[1:], ref[1:]))
    print(f"roberta {head} head {prec}: hidden {eh:.3e}; logits on the GPU's own rows {el:.3e}; against HF {direct:.3e}")
    assert len(got) == n and eh < TOL[prec] and el < TOL_NEW


@pytest.mark.parametrize("mode", MODES)
def test_independence(spi, zoo, gpu, mode, monkeypatch):
    """A row's output depends on its own sequence's ids alone: sequence 0 (and the padded sequence 1) served alone
    equal their slices of the B = 3 task; graphs on equals off; two runs are equal."""
    prec = setenv_mode(monkeypatch, mode)
    m = model(zoo, "small")
    B, S = MODELS["small"][1]
    ids, mask = make_inputs(B, S)
    rep = spi.ModelReplica(m, 0, prec, max_batch=B)
    batch = forward(spi, rep, [ids, mask], 128)[0]
    assert np.array_equal(forward(spi, rep, [ids, mask], 128)[0], batch)
    assert np.array_equal(forward(spi, rep, [ids, mask], 128, graphs=True)[0], batch)
    for r in (0, 1):
        for graphs in (False, True):
            alone = forward(spi, rep, [ids[r:r + 1], mask[r:r + 1]], 128, graphs=graphs)[0]
            assert np.array_equal(alone[0], batch[r]), f"sequence {r} alone, graphs={graphs}"


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_runtime_adaptive_batching(spi, zoo, gpu, prec):
    """Three jobs of 1, 2 and 1 samples, merged by the adaptive batcher into one task of four: each job's slice
    equals, bit for bit, a direct codelet call on that job's inputs (test_bert_heads_gpu's arrangement)."""
    rtmod = importlib.import_module("starpu-inference-server_amd.runtime")
    m = model(zoo, "small")
    S, D = 32, 128
    rep = spi.ModelReplica(m, 0, prec, max_batch=4, seq_len=S)
    specs = rtmod.bert_output_specs(rep, S, D)
    assert specs == [(S * D, np.float32)]
    b = rtmod.batching_config("adaptive", min_batch=1, batch_limit=4, coalesce_timeout_us=30_000_000, congestion=False)
    rt = rtmod.Runtime([rep], [((S,), np.int64), ((S,), np.int64)], specs, max_batch=4, workers_per_device=1, batching=b)
    rng = np.random.default_rng(11)
    jobs = []
    for rid, n in enumerate([1, 2, 1]):
        ids = RR.token_ids(rng, n, S, VOCAB, clamped=False)
        ids[-1, 20 - rid:] = RR.PAD
        ids[0, 5 + rid] = RR.PAD
        mask = (ids != RR.PAD).astype(np.int64)
        outs = [np.full((n, S * D), np.nan, dtype=np.float32)]
        rt.submit(rid, [ids, mask], outs)
        jobs.append((ids, mask, outs))
    rt.drain()
    assert rt.stats() == (len(jobs), 0)
    merged = max(c.task_jobs for c in rt.completions)
    rt.close()
    assert merged == 3, f"the three jobs were not merged into one task (largest task: {merged} jobs)"
    for ids, mask, outs in jobs:
        want = forward(spi, rep, [ids, mask], D)[0]
        assert np.array_equal(outs[0], want.reshape(outs[0].shape))


def test_torchscript_roberta(spi, zoo, gpu, tmp_path):
    """A traced zoo.roberta as a .pt states neither the rule nor eps: the caller passes both."""
    m = model(zoo, "small")
    B, S = MODELS["small"][1]
    ids, mask = make_inputs(B, S)
    ref = oracle(("tuple", "small"), zoo.BertTupleWrapper(m.bert), [ids, mask], 2)[0]
    path = str(tmp_path / "roberta.pt")
    ex = (torch.from_numpy(make_inputs(B, S, pads=False)[0]), torch.ones((B, S), dtype=torch.int64))
    torch.jit.trace(m, ex, strict=False).save(path)
    for prec in ("fp32", "fp16"):
        rep = spi.ModelReplica(path, 0, prec, max_batch=B, num_heads=2, eps=1e-5, bert_io="roberta_positions")
        assert rep.bert_io == 1024 and rep.description.endswith(" pos[ids]")
        got = forward(spi, rep, [ids, mask], 128)[0]
        err = RR.err1(got, ref)
        print(f".pt roberta {prec}: hidden {err:.3e}")
        assert err < TOL[prec]
        assert np.array_equal(got, forward(spi, spi.ModelReplica(m, 0, prec, max_batch=B), [ids, mask], 128)[0])

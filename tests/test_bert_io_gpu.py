"""BERT sentence outputs and segment ids (spi_model_config.bert_io) on the GPU: the pooler and masked-mean
kernels and the typed embedding at op level, then the replica's outputs in every bert_io mode, through
TorchScript and through the mini-runtime.

The new arithmetic is fp32 and small, so it is held to the project's fp32 bar (1e-5 normalised max error)
against float64 torch run on the GPU's OWN last_hidden_state -- which keeps the fp16 error that the hidden
state already carries out of the comparison.  The hidden state itself keeps test_parity_gpu's TOL.
"""
import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle.cpu_codelet import cpu_inference, normalized_max_error

pytestmark = pytest.mark.gpu

TOL = {"fp32": 1e-5, "fp16": 1e-3}  # test_parity_gpu.TOL
TOL_NEW = 1e-5                      # fp32 pooler / mean against float64 on the same rows
TOL_LN32, TOL16 = 2e-6, 1e-3        # test_elementwise_ops_gpu's bars for bert_embed (yf; fp16 yt)
GUARD = 8
NAN = float("nan")
VOCAB = 1000


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
    return t[:rows].cpu()


def pooler_ref(rows, W, b):
    """tanh(W . rows + b) in float64; rows [B][D]."""
    return np.tanh(np.asarray(rows, np.float64) @ np.asarray(W, np.float64).T + np.asarray(b, np.float64))


def mean_ref(h, mask):
    """sum_s m h / max(sum_s m, 1e-9) in float64, m = (mask != 0); h [B][S][D], mask [B][S] or None."""
    h = np.asarray(h, np.float64)
    m = np.ones(h.shape[:2]) if mask is None else (np.asarray(mask) != 0).astype(np.float64)
    return (m[:, :, None] * h).sum(1) / np.maximum(m.sum(1), 1e-9)[:, None]


# ---- ops ------------------------------------------------------------------------------------------


def op_mask(rng, B, S):
    """Random zeros and ones, -7 for a one somewhere (any non-zero counts), row 0 with a single valid token."""
    mask = rng.integers(0, 2, (B, S)).astype(np.int64)
    mask[:, 0] = 1
    mask[0, :] = 0
    mask[0, S // 2] = -7
    return mask


# S 130: three passes of the mean's 64-row step, the last ragged; B 9: a second pass of the pooler's 8 rows
POOL_CASES = [(B, S, D) for B in (1, 3) for S in (1, 17, 130) for D in (64, 128, 768, 1024)] + [(9, 17, 128), (9, 17, 768)]


@pytest.mark.parametrize("B,S,D", POOL_CASES)
def test_pooler_and_masked_mean_ops(ops, B, S, D):
    rng = np.random.default_rng(B * 1000 + S * 10 + D)
    h = rng.standard_normal((B, S, D)).astype(np.float32)
    W = (rng.standard_normal((D, D)) / np.sqrt(D)).astype(np.float32)
    b = (0.1 * rng.standard_normal(D)).astype(np.float32)
    hd, Wd, bd = dev(h), dev(W), dev(b)
    packed = hd[:, 0].contiguous()
    want = pooler_ref(h[:, 0], W, b)
    for name, src, ld in (("ld=S*D", hd, S * D), ("ld=D", packed, D)):
        what = f"bert_pooler B{B} S{S} D{D} {name}"
        runs = []
        for _ in range(2):
            y = guarded(B, D)
            ops.bert_pooler(src, ld, Wd, bd, y, B, D)
            runs.append(take(y, B, what).numpy())
        err = normalized_max_error(runs[0], want)
        print(f"{what}: {err:.3e}")
        assert err < TOL_NEW, f"{what}: {err:.3e}"
        assert np.array_equal(runs[0], runs[1]), f"{what}: two runs differ"
    for name, mask in (("mask", op_mask(rng, B, S)), ("no mask", None)):
        what = f"masked_mean B{B} S{S} D{D} {name}"
        md = None if mask is None else dev(mask)
        runs = []
        for _ in range(2):
            y = guarded(B, D)
            ops.masked_mean(hd, md, y, B, S, D)
            runs.append(take(y, B, what).numpy())
        err = normalized_max_error(runs[0], mean_ref(h, mask))
        print(f"{what}: {err:.3e}")
        assert err < TOL_NEW, f"{what}: {err:.3e}"
        assert np.array_equal(runs[0], runs[1]), f"{what}: two runs differ"


def test_masked_mean_skips_masked_rows_and_all_zero_mask(ops):
    """A masked-out row does not enter the sum even when it holds NaN (the attention never reads it
    either); a row with no valid token gives 0 / 1e-9 = 0."""
    B, S, D = 2, 5, 64
    h = np.random.default_rng(0).standard_normal((B, S, D)).astype(np.float32)
    mask = np.int64([[1, 0, 1, 1, 0], [0, 0, 0, 0, 0]])
    want = mean_ref(h, mask)
    h[0, 1] = np.nan
    y = guarded(B, D)
    ops.masked_mean(dev(h), dev(mask), y, B, S, D)
    got = take(y, B, "masked_mean").numpy()
    assert normalized_max_error(got[0], want[0]) < TOL_NEW and not got[1].any()


@pytest.mark.parametrize("D", [128, 768])
def test_pool_ops_on_unaligned_rows_take_the_scalar_loads(ops, D):
    """h one float past a 16-byte boundary: the 16-byte loads cannot run; same bars, same bits twice."""
    B, S = 3, 17
    rng = np.random.default_rng(D)
    h = rng.standard_normal((B, S, D)).astype(np.float32)
    W = (rng.standard_normal((D, D)) / np.sqrt(D)).astype(np.float32)
    b = (0.1 * rng.standard_normal(D)).astype(np.float32)
    mask = op_mask(rng, B, S)
    flat = torch.zeros(h.size + 1, device="cuda")
    hd = flat[1:].view(B, S, D)
    hd.copy_(torch.from_numpy(h))
    assert hd.data_ptr() % 16 == 4
    runs = []
    for _ in range(2):
        yp, ym = guarded(B, D), guarded(B, D)
        ops.bert_pooler(hd, S * D, dev(W), dev(b), yp, B, D)
        ops.masked_mean(hd, dev(mask), ym, B, S, D)
        runs.append((take(yp, B, "bert_pooler unaligned").numpy(), take(ym, B, "masked_mean unaligned").numpy()))
    assert normalized_max_error(runs[0][0], pooler_ref(h[:, 0], W, b)) < TOL_NEW
    assert normalized_max_error(runs[0][1], mean_ref(h, mask)) < TOL_NEW
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])


def test_pool_op_rejections(ops):
    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    for D in (0, 32, 96, 1088):
        with pytest.raises(ops.OpError):
            ops.bert_pooler(z(2, max(D, 1)), max(D, 1), z(max(D, 1), max(D, 1)), z(max(D, 1)), z(2, max(D, 1)), 2, D)
        with pytest.raises(ops.OpError):
            ops.masked_mean(z(2, 3, max(D, 1)), None, z(2, max(D, 1)), 2, 3, D)
    with pytest.raises(ops.OpError):
        ops.bert_pooler(z(2, 64), 32, z(64, 64), z(64), z(2, 64), 2, 64)  # ld < D
    with pytest.raises(ops.OpError):
        ops.masked_mean(z(2, 3, 64), None, z(2, 64), 2, 0, 64)


def embed_ref(ids, types, word, pos, table, gamma, beta, S, eps):
    """torch: the sum in fp32 in the kernel's order, (word + type) + pos, then layer_norm in float64."""
    ids = torch.from_numpy(np.clip(ids, 0, word.shape[0] - 1))
    t = torch.from_numpy(np.clip(types, 0, table.shape[0] - 1))
    s = torch.arange(ids.numel()) % S
    v = (torch.from_numpy(word)[ids] + torch.from_numpy(table)[t]) + torch.from_numpy(pos)[s]
    return F.layer_norm(v.double(), (word.shape[1],), torch.from_numpy(gamma).double(),
                        torch.from_numpy(beta).double(), eps).numpy()


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("D", [128, 768, 1024])  # the scalar kernel, the vector kernels NV = 3 and 4
def test_bert_embed_types_op(ops, D, prec):
    B, S, NT, eps = 3, 7, 3, 1e-5  # 21 rows: a ragged last block of 4
    M = B * S
    rng = np.random.default_rng(D)
    word = rng.standard_normal((VOCAB, D)).astype(np.float32)
    pos = (0.5 * rng.standard_normal((16, D))).astype(np.float32)
    table = rng.standard_normal((NT, D)).astype(np.float32)  # rows far apart: a wrong row shows
    gamma = (1 + 0.3 * rng.standard_normal(D)).astype(np.float32)
    beta = rng.standard_normal(D).astype(np.float32)
    ids = rng.integers(0, VOCAB, M).astype(np.int64)
    types = rng.integers(0, NT, M).astype(np.int64)
    types[:3] = [-1, NT, 2 ** 40]  # clamped to 0, NT - 1, NT - 1
    mask = (np.arange(M) % 3 != 1).astype(np.int64)
    ydt = torch.float16 if prec == "fp16" else torch.float32
    d = [dev(a) for a in (ids, word, pos, table, gamma, beta)]

    def run(type_ids, typed=True):
        yf, yt, mb = guarded(M, D), guarded(M, D, dtype=ydt), guarded(M)
        if typed:
            ops.bert_embed_types(prec, d[0], d[1], d[2], d[3], type_ids, d[4], d[5], yf, yt, B, S, D, eps,
                                 mask=dev(mask), mask_bias=mb)
        else:  # the existing op on the table's first row
            ops.bert_embed(prec, d[0], d[1], d[2], d[3][0].contiguous(), d[4], d[5], yf, yt, B, S, D, eps,
                           mask=dev(mask), mask_bias=mb)
        what = f"bert_embed_types {prec} D{D}"
        return take(yf, M, what).numpy(), take(yt, M, what), take(mb, M, what).numpy()

    yf, yt, mb = run(dev(types))
    ref = embed_ref(ids, types, word, pos, table, gamma, beta, S, eps)
    ef, et = normalized_max_error(yf, ref), normalized_max_error(yt.double().numpy(), ref)
    print(f"bert_embed_types {prec} D{D}: yf {ef:.3e} yt {et:.3e}")
    assert ef < TOL_LN32 and et < (TOL16 if prec == "fp16" else TOL_LN32)
    assert np.array_equal(mb, np.where(mask != 0, np.float32(0), np.finfo(np.float32).min))
    plain = run(None, typed=False)
    for name, type_ids in (("null ids", None), ("all-zero ids", dev(np.zeros(M, np.int64)))):
        got = run(type_ids)
        assert np.array_equal(got[0], plain[0]) and torch.equal(got[1], plain[1]) and np.array_equal(got[2], plain[2]), name


# ---- models ---------------------------------------------------------------------------------------

SHAPES = {"B3_S80": (3, 80), "B2_S128": (2, 128)}


def make_model(zoo, which):
    if which == "small":
        return zoo.bert(layers=2, hidden=128, heads=2, intermediate=256, vocab=VOCAB, max_position=128, init_std=0.05)
    return zoo.bert(layers=1, hidden=768, heads=12, intermediate=3072, vocab=VOCAB, max_position=128)  # vector embed


def make_inputs(shape):
    """ids, mask, segment ids.  Mask rows: one full, one valid to 50, one (B = 3) with a single valid token."""
    B, S = SHAPES[shape]
    rng = np.random.default_rng(B * S)
    ids = rng.integers(0, VOCAB, (B, S), dtype=np.int64)
    mask = np.ones((B, S), dtype=np.int64)
    mask[1, 50:] = 0
    if B > 2:
        mask[2, 1:] = 0
    types = rng.integers(0, 2, (B, S), dtype=np.int64)
    return ids, mask, types


_cache = {}


def case(zoo, which, shape):
    """Model, inputs and the oracle's (last_hidden_state, pooler_output), computed once per case."""
    key = (which, shape)
    if key not in _cache:
        if ("model", which) not in _cache:
            _cache[("model", which)] = make_model(zoo, which)
        m = _cache[("model", which)]
        ids, mask, types = make_inputs(shape)
        hidden, pooled = cpu_inference(zoo.BertTupleWrapper(m.bert), [ids, mask], num_outputs=2)
        for a in (hidden, pooled):
            a.setflags(write=False)
        _cache[key] = (m, ids, mask, types, hidden, pooled)
    return _cache[key]


def out_shapes(io, B, S, D):
    shapes = [] if "no_hidden" in io else [(B, S, D)]
    return shapes + [(B, D)] * (("pooler" in io) + ("mean" in io))


def hip_forward(spi, rep, inputs, shapes, graphs=False):
    ins = [dev(x) for x in inputs]
    outs = [torch.full(s, NAN, device="cuda", dtype=torch.float32) for s in shapes]
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    rep.set_graphs(graphs)
    spi.run_hip(rep, ins, outs, stream=stream.cuda_stream)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs]


def pooler_weights(m):
    return m.bert.pooler.dense.weight.detach().numpy(), m.bert.pooler.dense.bias.detach().numpy()


@pytest.mark.parametrize("mode", ["fp32", "fp16", "fp16_nofold"])
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("which", ["small", "wide"])
def test_hidden_pooler_and_mean(spi, zoo, gpu, which, shape, mode, monkeypatch):
    """bert_io pooler|mean: three outputs.  The pooled outputs' direct error against the oracle is printed
    and recorded in DESIGN.md 3.3.2, not asserted: a hidden state inside 1e-3 can legitimately give a few
    1e-3 after the pooler's dense layer."""
    prec = mode.split("_")[0]
    if mode.endswith("nofold"):
        monkeypatch.setenv("SPI_LN_FOLD", "0")
    m, ids, mask, _, ref_h, ref_p = case(zoo, which, shape)
    B, S = ids.shape
    D = ref_h.shape[-1]
    rep = spi.ModelReplica(m, 0, prec, max_batch=B, seq_len=128, bert_io=("pooler", "mean"))
    assert rep.description.endswith("out[hidden,pooler,mean] in[ids,mask]")
    got_h, got_p, got_m = hip_forward(spi, rep, [ids, mask], out_shapes("pooler|mean", B, S, D))
    W, b = pooler_weights(m)
    eh = normalized_max_error(got_h, ref_h)
    ep = normalized_max_error(got_p, pooler_ref(got_h[:, 0], W, b))
    em = normalized_max_error(got_m, mean_ref(got_h, mask))
    dp, dm = normalized_max_error(got_p, ref_p), normalized_max_error(got_m, mean_ref(ref_h, mask))
    print(f"bert_io pooler|mean {which} {shape} {mode}: hidden {eh:.3e}; on the GPU's hidden: pooler {ep:.3e} "
          f"mean {em:.3e}; against the oracle: pooler {dp:.3e} mean {dm:.3e}")
    assert eh < TOL[prec]
    assert ep < TOL_NEW and em < TOL_NEW


@pytest.mark.parametrize("prec", ["fp16", "fp32"])  # fp16: the folded epilogue (two-plane rows); fp32: the unfolded one
@pytest.mark.parametrize("io", ["no_hidden|pooler", "no_hidden|mean", "no_hidden|pooler|mean"])
@pytest.mark.parametrize("which", ["small", "wide"])
def test_sentence_only_modes(spi, zoo, gpu, which, io, prec):
    """Without the hidden output the LayerNorm lands in a workspace buffer (class-token rows only for the
    pooler alone): the same fp32 math on the same rows as with the hidden state selected."""
    m, ids, mask, _, ref_h, _ = case(zoo, which, "B3_S80")
    B, S = ids.shape
    D = ref_h.shape[-1]
    key = ("with_hidden", which, prec)
    if key not in _cache:
        full = spi.ModelReplica(m, 0, prec, max_batch=B, seq_len=128, bert_io=("pooler", "mean"))
        _cache[key] = hip_forward(spi, full, [ids, mask], out_shapes("pooler|mean", B, S, D))
    _, want_p, want_m = _cache[key]
    want = ([want_p] if "pooler" in io else []) + ([want_m] if "mean" in io else [])
    rep = spi.ModelReplica(m, 0, prec, max_batch=B, seq_len=128, bert_io=tuple(io.split("|")))
    for graphs in (False, True):
        got = hip_forward(spi, rep, [ids, mask], out_shapes(io, B, S, D), graphs=graphs)
        assert len(got) == len(want)
        for g, w in zip(got, want):
            err = normalized_max_error(g, w)
            print(f"bert_io {io} {which} {prec} graphs={graphs}: {err:.3e} against the run with hidden, "
                  f"equal={np.array_equal(g, w)}")
            assert err < 1e-6


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_token_types(spi, zoo, gpu, prec):
    m, ids, mask, types, ref_h, _ = case(zoo, "small", "B3_S80")
    B, S = ids.shape
    shape = [ref_h.shape]
    ref = cpu_inference(zoo.BertSegmentsWrapper(m.bert), [ids, mask, types])[0]
    assert normalized_max_error(ref, ref_h) > 1e-2  # the segment ids matter to the oracle
    rep = spi.ModelReplica(m, 0, prec, max_batch=B, seq_len=128, bert_io="token_types")
    got = hip_forward(spi, rep, [ids, mask, types], shape)[0]
    err = normalized_max_error(got, ref)
    print(f"bert_io token_types small B3_S80 {prec}: hidden {err:.3e}")
    assert err < TOL[prec]
    plain = spi.ModelReplica(m, 0, prec, max_batch=B, seq_len=128)
    want = hip_forward(spi, plain, [ids, mask], shape)[0]
    assert np.array_equal(hip_forward(spi, rep, [ids, mask, np.zeros_like(types)], shape)[0], want)
    assert np.array_equal(hip_forward(spi, rep, [ids, mask], shape)[0], want)
    assert np.array_equal(hip_forward(spi, rep, [ids, mask, types], shape, graphs=True)[0], got)


def test_profile_hooks_pass_every_output(spi, zoo, gpu):
    """profile / launch_table / profile_op with a list of outputs: the epilogue's ops by name, each launch
    attributed, and the outputs written as by the codelet."""
    m, ids, mask, _, ref_h, _ = case(zoo, "small", "B3_S80")
    B, S = ids.shape
    D = ref_h.shape[-1]
    ins = [dev(ids), dev(mask)]
    stream = torch.cuda.Stream()
    for io, names in (("pooler|mean", ["layernorm_out", "bert_pooler", "bert_mean_pool"]),
                      ("no_hidden|pooler", ["layernorm_cls", "bert_pooler"]),
                      ("no_hidden|mean", ["layernorm_out", "bert_mean_pool"])):
        rep = spi.ModelReplica(m, 0, "fp16", max_batch=B, seq_len=128, bert_io=tuple(io.split("|")))
        want = hip_forward(spi, rep, [ids, mask], out_shapes(io, B, S, D))
        outs = [torch.full(s, NAN, device="cuda") for s in out_shapes(io, B, S, D)]
        torch.cuda.synchronize()
        recs = rep.profile(ins, outs, stream.cuda_stream)
        assert [r["name"] for r in recs][-len(names):] == names, io
        for o, w in zip(outs, want):
            assert np.array_equal(o.cpu().numpy(), w), io
        table = rep.launch_table(ins, outs, stream.cuda_stream)
        assert [r["op"] for r in table][-len(names):] == names, io
        assert "bert_pooler_kernel" in table[-1]["kernel"] or "masked_mean_kernel" in table[-1]["kernel"]
        one = rep.profile_op(ins, outs, stream.cuda_stream, names[-1], reps=3)
        assert one["ms"] > 0 and one["bytes"] > 0


def test_torchscript_tuple_model(spi, zoo, gpu, tmp_path):
    """The tuple-returning BertModel as a traced .pt: the replica built from the path with "pooler"
    against the LibTorch CPU codelet on the same file."""
    lt = importlib.import_module("starpu-inference-server_amd.libtorch")
    m, ids, mask, _, _, _ = case(zoo, "small", "B2_S128")
    B, S = ids.shape
    D = m.bert.config.hidden_size
    path = str(tmp_path / "bert_tuple.pt")
    ex = (torch.randint(0, VOCAB, ids.shape), torch.ones(ids.shape, dtype=torch.int64))  # traced at the served shape
    torch.jit.trace(zoo.BertTupleWrapper(m.bert), ex, strict=False).save(path)
    ts = lt.TorchScriptModule(path)
    ref = [np.full(s, np.nan, dtype=np.float32) for s in ((B, S, D), (B, D))]
    params = spi.make_params([list(ids.shape), list(mask.shape)], [torch.int64] * 2, num_outputs=2, model_cpu=ts)
    bufs = [spi.tensor_interface(torch.from_numpy(x)) for x in (ids, mask, *ref)]
    with spi.worker_context(0, -1, None):
        spi.InferenceCodelet.cpu_inference_func(bufs, params)
    W, b = pooler_weights(m)
    for prec in ("fp32", "fp16"):
        rep = spi.ModelReplica(path, 0, prec, max_batch=B, seq_len=128, bert_io="pooler")
        assert rep.bert_io == 1 and rep.description.endswith("out[hidden,pooler] in[ids,mask]")
        got_h, got_p = hip_forward(spi, rep, [ids, mask], [(B, S, D), (B, D)])
        eh = normalized_max_error(got_h, ref[0])
        ep = normalized_max_error(got_p, pooler_ref(got_h[:, 0], W, b))
        print(f".pt bert tuple {prec}: hidden {eh:.3e}, pooler on the GPU's hidden {ep:.3e}, "
              f"pooler against the CPU codelet {normalized_max_error(got_p, ref[1]):.3e}")
        assert eh < TOL[prec] and ep < TOL_NEW


def test_runtime_two_outputs_dynamic_batching(spi, zoo, gpu):
    """(hidden, pooler) through the mini-runtime with jobs of batch 1 and 2 merged into one codelet call:
    each job's slice of both outputs equals, bit for bit, a direct codelet call on that job's inputs
    (fp32: the GEMMs take the same plan at M = 32 .. 128 rows, and every other kernel works per row or
    per sequence, so batching changes no sum).  Five jobs of 1, 2, 1, 2, 2 samples queue well inside the
    coalescing delay and fill two tasks of four."""
    rtmod = importlib.import_module("starpu-inference-server_amd.runtime")
    m = case(zoo, "small", "B3_S80")[0]
    S, D = 32, m.bert.config.hidden_size
    rep = spi.ModelReplica(m, 0, "fp32", max_batch=4, seq_len=S, bert_io="pooler")
    rt = rtmod.Runtime([rep], [((S,), np.int64), ((S,), np.int64)], [(S * D, np.float32), (D, np.float32)],
                       max_batch=4, workers_per_device=1, coalesce_max_jobs=4, coalesce_delay_us=100_000)
    rng = np.random.default_rng(5)
    jobs = []
    for rid, b in enumerate([1, 2, 1, 2, 2]):  # two full tasks of four samples
        ids = rng.integers(0, VOCAB, (b, S), dtype=np.int64)
        mask = np.ones((b, S), dtype=np.int64)
        mask[-1, 20:] = 0
        outs = [np.full((b, S, D), np.nan, dtype=np.float32), np.full((b, D), np.nan, dtype=np.float32)]
        rt.submit(rid, [ids, mask], outs)
        jobs.append((ids, mask, outs))
    rt.drain()
    assert rt.stats() == (len(jobs), 0)
    assert max(c.task_jobs for c in rt.completions) > 1  # something was merged
    rt.close()
    for ids, mask, (h, p) in jobs:
        b = ids.shape[0]
        want_h, want_p = hip_forward(spi, rep, [ids, mask], [(b, S, D), (b, D)])
        eh, ep = normalized_max_error(h, want_h), normalized_max_error(p, want_p)
        print(f"runtime (hidden, pooler) job of {b}: hidden {eh:.3e} pooler {ep:.3e}")
        assert np.array_equal(h, want_h) and np.array_equal(p, want_p)

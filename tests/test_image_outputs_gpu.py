"""Classification outputs of image replicas (spi_model_set_image_outputs) on the GPU: the softmax / top-k
kernel at op level, then the replicas' outputs for ViT and both ResNet classifier routes, with graphs, 8-bit
tasks, the mini-runtime and the profiling hooks.

The new arithmetic is fp32, so the probabilities are held to the project's fp32 bar: normalised max error
max|p - p64| / max p64 <= 1e-5 per row against the float64 softmax of the SAME fp32 logits, and
|sum p - 1| <= 1e-5.  Indices and top-k values are exact: np.argsort(-x, kind="stable") and the bits of the
logits (or of the probability output) at those indices.
"""
import importlib

import numpy as np
import pytest
import torch

from oracle.cpu_codelet import cpu_inference

pytestmark = pytest.mark.gpu

TOL = 1e-5
GUARD = 16
PROBS, TOPK, NO_LOGITS, TOPK_PROBS = 1, 2, 4, 8
NAN = float("nan")


@pytest.fixture(scope="module")
def ops(spi, gpu):
    return importlib.import_module("starpu-inference-server_amd.ops")


def softmax64(x):
    x = x.astype(np.float64)
    e = np.exp(x - x.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def check_probs(p, x, what):
    """The bar of the module docstring; -inf logits have probability exactly 0."""
    p64 = softmax64(x)
    err = float(np.max(np.abs(p - p64).max(1) / p64.max(1)))
    dsum = float(np.max(np.abs(p.astype(np.float64).sum(1) - 1)))
    assert err <= TOL and dsum <= TOL, f"{what}: normalised max error {err:.3e}, |sum - 1| {dsum:.3e}"
    assert np.all(p[np.isneginf(x)] == 0), f"{what}: a -inf logit has a non-zero probability"
    return err


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- op level -----------------------------------------------------------------------------------------


def fixtures(rng, B, N):
    """name -> fp32 [B][N] logits."""
    normal = rng.standard_normal((B, N)).astype(np.float32)
    dup = normal.copy()
    dup[:, 0] = dup[:, N - 1] = dup.max(1) + 1  # the maximum at both ends
    special = normal.copy()  # -inf entries and both signed zeros; column 0 stays finite
    if N == 1:
        special[:] = -0.0
    elif N == 2:
        special[0::2] = (-0.0, 0.0)
        special[1::2] = (0.0, -0.0)
    else:
        special[:, 1::5] = -np.inf
        special[:, 2::7] = 0.0
        special[:, 3::7] = -0.0
        special[:, N - 1] = -0.0 if N % 2 else -np.inf
    return {"normal": normal, "x80": normal * np.float32(80), "quarter": np.round(normal * 4) / 4,
            "equal": np.full((B, N), 1.5, np.float32), "dupmax": dup, "special": special.astype(np.float32)}


def layouts(x):
    """name -> (device tensor whose data pointer is row 0, ldx): packed rows; rows N + 3 apart from a base one
    float past the allocation's (the scalar-load path); rows a multiple of four apart from an aligned base
    (16-byte loads with a scalar tail when N % 4 != 0)."""
    B, N = x.shape
    out = {}
    for name, ldx, off in (("ldx=N", N, 0), ("ldx=N+3 base+1", N + 3, 1), ("ldx=4n", (N + 3) // 4 * 4 + 4, 0)):
        buf = torch.full((off + B * ldx,), NAN, device="cuda")
        rows = buf[off:].view(B, ldx)
        rows[:, :N] = torch.from_numpy(x).cuda()
        out[name] = (buf[off:], ldx)
    return out


def guarded(rows, cols, dtype):
    fill = NAN if dtype == torch.float32 else -77
    return torch.full((rows * cols + GUARD,), fill, dtype=dtype, device="cuda")


def take(t, rows, cols, what):
    """The [rows][cols] result; whatever follows it must still hold the canary."""
    tail = t[rows * cols:]
    ok = torch.isnan(tail).all() if t.dtype == torch.float32 else (tail == -77).all()
    assert bool(ok), f"{what}: memory past the output was written"
    return t[:rows * cols].view(rows, cols).cpu().numpy()


def run_op(ops, xd, ldx, B, N, k, probs, topk, topk_probs, what):
    p = guarded(B, N, torch.float32) if probs else None
    v = guarded(B, k, torch.float32) if topk else None
    i = guarded(B, k, torch.int64) if topk else None
    ops.softmax_topk(xd, ldx, p, v, i, B, N, k if topk else 0, topk_probs)
    torch.cuda.synchronize()
    return (take(p, B, N, what) if probs else None, take(v, B, k, what) if topk else None,
            take(i, B, k, what) if topk else None)


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 1000, 1001, 4097, 16384])
def test_softmax_topk_op(ops, N):
    worst = 0.0
    for B in (1, 3, 9):
        rng = np.random.default_rng(1000 * N + B)
        for fname, x in fixtures(rng, B, N).items():
            order = np.argsort(-x, kind="stable")
            if fname == "equal":
                assert np.array_equal(order, np.tile(np.arange(N), (B, 1)))
            for lname, (xd, ldx) in layouts(x).items():
                for k in sorted({1, min(5, N), min(N, 64)}):
                    what = f"softmax_topk B{B} N{N} k{k} {fname} {lname}"
                    idx = order[:, :k]
                    # both outputs, top-k values as logits
                    p, v, i = run_op(ops, xd, ldx, B, N, k, True, True, False, what)
                    worst = max(worst, check_probs(p, x, what))
                    assert i.dtype == np.int64 and np.array_equal(i, idx), what
                    assert np.array_equal(bits(v), bits(np.take_along_axis(x, idx, 1))), what
                    # both outputs, top-k values as probabilities: the bits of this call's probability output
                    p2, v2, i2 = run_op(ops, xd, ldx, B, N, k, True, True, True, what)
                    assert np.array_equal(bits(p2), bits(p)) and np.array_equal(i2, idx), what
                    assert np.array_equal(bits(v2), bits(np.take_along_axis(p, idx, 1))), what
                    # one output each: the same bits as together (also: two runs are bit-identical)
                    p3, _, _ = run_op(ops, xd, ldx, B, N, k, True, False, False, what)
                    assert np.array_equal(bits(p3), bits(p)), what
                    _, v4, i4 = run_op(ops, xd, ldx, B, N, k, False, True, False, what)
                    assert np.array_equal(bits(v4), bits(v)) and np.array_equal(i4, idx), what
                    _, v5, i5 = run_op(ops, xd, ldx, B, N, k, False, True, True, what)
                    assert np.array_equal(bits(v5), bits(v2)) and np.array_equal(i5, idx), what
    print(f"softmax_topk N{N}: worst normalised max error of the probabilities {worst:.3e}")


def test_softmax_topk_rejects_before_launch(ops):
    B, N, k = 2, 10, 3
    x = torch.zeros(B, N, device="cuda")
    p = guarded(B, N, torch.float32)
    v = guarded(B, k, torch.float32)
    i = guarded(B, k, torch.int64)
    big = torch.zeros(16385, device="cuda")
    for args, match in (((None, N, p, v, i, B, N, k), "x is null"),
                        ((x, N, None, None, None, B, N, 0), "no output selected"),
                        ((x, N, p, v, None, B, N, k), "both or neither"),
                        ((x, N, p, None, i, B, N, k), "both or neither"),
                        ((x, N, p, v, i, 0, N, k), "B >= 1"),
                        ((x, N, p, v, i, B, 0, k), "1 <= N <= 16384"),
                        ((big, 16385, p, v, i, 1, 16385, k), "1 <= N <= 16384"),
                        ((x, N - 1, p, v, i, B, N, k), "ldx >= N"),
                        ((x, N, p, v, i, B, N, 0), r"1 <= k <= min\(N, 64\)"),
                        ((x, N, p, v, i, B, N, N + 1), r"1 <= k <= min\(N, 64\)"),
                        ((big, 100, p, v, i, 1, 100, 65), r"1 <= k <= min\(N, 64\)"),
                        ((x, N, p, None, None, B, N, 2), "need the top-k outputs")):
        with pytest.raises(ops.OpError, match=match):
            ops.softmax_topk(*args)
    with pytest.raises(ops.OpError, match="need the top-k outputs"):
        ops.softmax_topk(x, N, p, None, None, B, N, 0, topk_probs=True)
    torch.cuda.synchronize()
    assert bool(torch.isnan(p).all()) and bool(torch.isnan(v).all()) and bool((i == -77).all())  # nothing ran


# ---- models -------------------------------------------------------------------------------------------

B, MAXB, K = 3, 4, 5
KINDS = {"vit": 32, "resnet_pooled": 64, "resnet_avgpool": 288}  # kind -> image size (288: a 9 x 9 final map)
_models = {}


def model(zoo, kind, classes):
    """(module, ModelReplica keywords, fp32 images, 8-bit NHWC images, the oracle's logits), once per case."""
    key = (kind, classes)
    if key not in _models:
        image = KINDS[kind]
        if kind == "vit":
            m = zoo.vit(image=32, patch=16, layers=2, heads=2, dim=128, mlp_dim=256, num_classes=classes)
            kw = dict(num_heads=2, image_size=32)
        else:
            m = zoo.resnet([1, 1, 1, 1], False, image=image, num_classes=classes)
            kw = dict(image_size=image)
        rng = np.random.default_rng(classes + image)
        x = rng.random((B, 3, image, image), dtype=np.float32)
        u8 = rng.integers(0, 256, (B, image, image, 3), dtype=np.uint8)
        ref = cpu_inference(m, [x])[0]
        ref.setflags(write=False)
        _models[key] = (m, kw, x, u8, ref)
    return _models[key]


def forward(spi, rep, x, classes, stream, graphs=False):
    specs = spi.output_specs(x.shape[0], classes, rep.image_io, rep.top_k)
    outs = [torch.full(s, NAN if dt == torch.float32 else -77, dtype=dt, device="cuda") for s, dt in specs]
    torch.cuda.synchronize()
    rep.set_graphs(graphs)
    spi.run_hip(rep, [torch.from_numpy(x).cuda()], outs, stream=stream.cuda_stream)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs]


def check_replicas(a, b, c, what):
    """A's logits against B's four outputs and C's two (module docstring)."""
    (logits,), (b_logits, b_probs, b_vals, b_idx), (c_vals, c_idx) = a, b, c
    assert np.array_equal(bits(b_logits), bits(logits)), what
    idx = np.argsort(-logits, kind="stable")[:, :K]
    assert b_idx.dtype == np.int64 and np.array_equal(b_idx, idx), what
    assert np.array_equal(bits(b_vals), bits(np.take_along_axis(logits, idx, 1))), what
    err = check_probs(b_probs, logits, what)
    assert c_idx.dtype == np.int64 and np.array_equal(c_idx, b_idx), what
    assert np.array_equal(bits(c_vals), bits(np.take_along_axis(b_probs, b_idx, 1))), what
    return err


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("classes", [10, 1000])
@pytest.mark.parametrize("kind", list(KINDS))
def test_replica_outputs(spi, zoo, gpu, kind, classes, prec):
    m, kw, x, u8, ref = model(zoo, kind, classes)
    scale = [1 / 255.0] * 3

    def make(io, k):
        rep = spi.ModelReplica(m, 0, prec, max_batch=MAXB, image_io=io, top_k=k, **kw)
        rep.set_input_transform(scale, [0.0] * 3)
        return rep
    reps = [make(0, 0), make(("probs", "topk"), K), make(("no_logits", "topk", "topk_probs"), K)]
    assert reps[1].description == reps[0].description + " out[logits,probs,top5]"
    assert reps[2].description == reps[0].description + " out[top5]"
    stream = torch.cuda.Stream()
    for graphs in (False, True):
        # an fp32 task, then an 8-bit NHWC task, on the one stream of each replica
        for task, name in ((x, "fp32"), (u8, "u8 nhwc")):
            what = f"{kind} classes{classes} {prec} graphs={graphs} {name}"
            a, b, c = (forward(spi, r, task, classes, stream, graphs) for r in reps)
            err = check_replicas(a, b, c, what)
            if name == "fp32" and not graphs:
                p_ref = softmax64(ref)
                direct = float(np.max(np.abs(b[1] - p_ref).max(1) / p_ref.max(1)))
                print(f"{what}: probabilities on the GPU's logits {err:.3e}, against the oracle's softmax {direct:.3e}")
                if prec == "fp32":  # top-1 of B against the oracle
                    assert np.array_equal(b[3][:, 0], np.argmax(ref, 1)), what
    # once a forward has run the contract is fixed: the setter is refused and the replica serves on
    before = forward(spi, reps[1], x, classes, stream)
    for rep, args in ((reps[1], (0, 0)), (reps[1], ("probs", 0)), (reps[0], ("probs", 0)), (reps[2], ("topk", 3))):
        with pytest.raises(spi.InferenceExecutionException, match="a stream workspace of the replica exists"):
            rep.set_image_outputs(*args)
    assert (reps[1].image_io, reps[1].top_k) == (PROBS | TOPK, K)
    after = forward(spi, reps[1], x, classes, stream)
    assert all(np.array_equal(p, q) for p, q in zip(before, after))
    assert len(forward(spi, reps[0], x, classes, stream)) == 1


def test_runtime_four_outputs_dynamic_batching(spi, zoo, gpu):
    """Replica B through the mini-runtime with jobs of batch 1 and 2 merged into one codelet call: each job gets
    its own rows of all four outputs, the indices as int64, equal bit for bit to a direct codelet call on the
    merged task's images (five jobs of 1, 2, 1, 2, 2 samples queue well inside the coalescing delay and fill two
    tasks of four in submission order; a conv's split-K plan may depend on the batch, so the direct call takes
    the task's batch, not the job's)."""
    rtmod = importlib.import_module("starpu-inference-server_amd.runtime")
    classes = 10
    m, kw, _, _, _ = model(zoo, "resnet_pooled", classes)
    image = KINDS["resnet_pooled"]
    rep = spi.ModelReplica(m, 0, "fp32", max_batch=MAXB, image_io=("probs", "topk"), top_k=K, **kw)
    rt = rtmod.Runtime([rep], [((3, image, image), np.float32)],
                       [(classes, np.float32), (classes, np.float32), (K, np.float32), (K, np.int64)],
                       max_batch=MAXB, workers_per_device=1, coalesce_max_jobs=4, coalesce_delay_us=100_000)
    rng = np.random.default_rng(5)
    jobs = []
    for rid, b in enumerate([1, 2, 1, 2, 2]):  # two full tasks of four samples
        x = rng.random((b, 3, image, image), dtype=np.float32)
        outs = [np.full((b, classes), np.nan, np.float32), np.full((b, classes), np.nan, np.float32),
                np.full((b, K), np.nan, np.float32), np.full((b, K), -77, np.int64)]
        rt.submit(rid, [x], outs)
        jobs.append((x, outs))
    rt.drain()
    assert rt.stats() == (len(jobs), 0)
    assert all(c.task_batch == MAXB for c in rt.completions)  # jobs 0-2 and 3-4 merged
    rt.close()
    stream = torch.cuda.Stream()
    for task in (jobs[:3], jobs[3:]):
        want = forward(spi, rep, np.concatenate([x for x, _ in task]), classes, stream)
        row = 0
        for x, outs in task:
            b = x.shape[0]
            assert outs[3].dtype == np.int64
            for got, w in zip(outs, want):
                assert np.array_equal(got, w[row:row + b]), f"runtime job of {b}"
            row += b
            # and what holds whatever the batch: the job's own rows are consistent
            idx = np.argsort(-outs[0], kind="stable")[:, :K]
            assert np.array_equal(outs[3], idx)
            assert np.array_equal(bits(outs[2]), bits(np.take_along_axis(outs[0], idx, 1)))
            check_probs(outs[1], outs[0], f"runtime job of {b}")


@pytest.mark.parametrize("kind", ["vit", "resnet_pooled", "resnet_avgpool"])
def test_profile_lists_the_op_once(spi, zoo, gpu, kind):
    classes = 10
    m, kw, x, _, _ = model(zoo, kind, classes)
    xd = [torch.from_numpy(x).cuda()]
    stream = torch.cuda.Stream()
    never = spi.ModelReplica(m, 0, "fp16", max_batch=MAXB, **kw)  # the setter is never called
    a = spi.ModelReplica(m, 0, "fp16", max_batch=MAXB, **kw)
    a.set_image_outputs(("probs", "topk"), K)
    a.set_image_outputs(0, 0)
    b = spi.ModelReplica(m, 0, "fp16", max_batch=MAXB, image_io=("probs", "topk"), top_k=K, **kw)

    def buffers(rep):
        return [torch.full(s, NAN if dt == torch.float32 else -77, dtype=dt, device="cuda")
                for s, dt in spi.output_specs(B, classes, rep.image_io, rep.top_k)]
    torch.cuda.synchronize()
    names_a = [r["name"] for r in a.profile(xd, buffers(a), stream.cuda_stream)]
    assert "softmax_topk" not in names_a
    assert a.launch_table(xd, buffers(a), stream.cuda_stream) == never.launch_table(xd, buffers(never), stream.cuda_stream)
    outs = buffers(b)
    recs = b.profile(xd, outs, stream.cuda_stream)
    names_b = [r["name"] for r in recs]
    assert names_b == names_a + ["softmax_topk"]
    assert recs[-1]["flops"] == 0 and recs[-1]["bytes"] > 0
    want = forward(spi, b, x, classes, stream)
    for o, w in zip(outs, want):
        assert np.array_equal(o.cpu().numpy(), w)
    table = b.launch_table(xd, outs, stream.cuda_stream)
    assert [r["op"] for r in table].count("softmax_topk") == 1 and "softmax_topk_kernel" in table[-1]["kernel"]
    assert table[-1]["grid"] == (B, 1, 1)
    one = b.profile_op(xd, outs, stream.cuda_stream, "softmax_topk", reps=3)
    assert one["ms"] > 0 and one["bytes"] > 0

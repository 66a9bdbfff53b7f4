"""Op-level parity of the LayerNorm fold (ln_fold.hpp) through include/spi_ops.h:
the producer / consumer / post-LN-residual epilogues of gemm.hip and gemm256.hip, the two-plane
residual stream, layernorm_planes and vit_assemble_planes -- each against the same formula in
numpy float64 on the same rounded operands (A = fp16(x), W as packed, statistics as passed), so
the bars are the operand-exact ones of test_gemm256_tiles / test_layernorm: 1e-5 normalised max
error for fp32 and two-plane outputs, 2e-3 for fp16 outputs.

Rows are built so that a wrong-row, wrong-chunk or masked-chunk statistic shows (make_rows): per-row
sigma in [0.5, 2], per-row mean in {0, +2 sigma, -3 sigma}, a +-0.5 sigma shift per 64-column chunk
(Chan's between-chunk term carries a quarter of the variance).  Every output buffer has 8 spare
rows of NaN behind it that must survive the call (ragged-tile stores).
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import op_refs

pytestmark = pytest.mark.gpu

EPS = 1e-5
GUARD = 8
TOL32, TOL16 = 1e-5, 2e-3
# producer statistics (issue: the 1e-5 output bar carried through max|ref| / sigma <= 10 for these rows)
TOL_STAT = 1e-4
NAN = float("nan")


@pytest.fixture(scope="module")
def ops(spi, gpu):
    import importlib
    return importlib.import_module("starpu-inference-server_amd.ops")


@pytest.fixture(scope="module")
def ws(ops):
    return ops.workspace()


@pytest.fixture(params=["1", "0,1,3", "0,1,2"], ids=["bm256", "bm128", "bm128b2"])
def gemm256_everywhere(ops, request):
    """Every eligible fp16 GEMM on gemm256.hip: 256-row tiles (SPI_GEMM_256_MIN=1) or 128-row tiles
    on three / two k-tile buffers (=0,1,3 / =0,1,2)."""
    os.environ["SPI_GEMM_256_MIN"] = request.param
    ops.lib.spi_debug_gemm_reload_env()
    yield request.param
    os.environ.pop("SPI_GEMM_256_MIN", None)
    ops.lib.spi_debug_gemm_reload_env()


# ---------------------------------------------------------------------------------------------
# inputs, references, buffers


def make_rows(rng, M, D):
    ch = -(-D // 64)
    sigma = rng.uniform(0.5, 2.0, (M, 1))
    mean = sigma * rng.choice([0.0, 2.0, -3.0], (M, 1))
    shift = 0.5 * sigma * rng.choice([-1.0, 1.0], (M, ch))
    return (rng.standard_normal((M, D)) * sigma + mean + np.repeat(shift, 64, axis=1)[:, :D]).astype(np.float32)


def make_ln(rng, D):
    gamma = (1 + 0.3 * rng.standard_normal(D)).astype(np.float32)
    beta = (0.1 * rng.standard_normal(D)).astype(np.float32)
    gamma[[1, D // 2, D - 3]] = 8.0
    beta[[2, D // 3, D - 1]] = [3.0, -3.0, 3.0]
    return gamma, beta


def make_linear(rng, N, K):
    return (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32), rng.standard_normal(N).astype(np.float32)


_linear_cache = {}


def plain_linear(ops, N, K):
    """(packed W on the device, fp16(W) as float64, bias float32 numpy, bias on the device)."""
    key = ("plain", N, K)
    if key not in _linear_cache:
        W, b = make_linear(np.random.default_rng(N * 7 + K), N, K)
        _linear_cache[key] = (ops.pack_weight("fp16", W), W.astype(np.float16).astype(np.float64), b,
                              torch.from_numpy(b).cuda())
    return _linear_cache[key]


def folded_linear(ops, N, K):
    """A linear layer behind a LayerNorm, packed for the fold: (packed W', fp16(W') float64, bias', c1,
    bias' and c1 on the device)."""
    key = ("folded", N, K)
    if key not in _linear_cache:
        rng = np.random.default_rng(N * 11 + K)
        W, b = make_linear(rng, N, K)
        gamma, beta = make_ln(rng, K)
        wf, bias, c1 = ops.fold_linear("fp16", W, b, gamma, beta)
        _linear_cache[key] = (ops.pack_weight("fp16", wf), wf.astype(np.float16).astype(np.float64), bias, c1,
                              torch.from_numpy(bias).cuda(), torch.from_numpy(c1).cuda())
    return _linear_cache[key]


def gelu64(x):
    t = torch.from_numpy(x)
    return (0.5 * t * (1 + torch.erf(t / 2 ** 0.5))).numpy()


def nerr(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max())


def guarded(rows, *tail, dtype=torch.float32):
    """[rows + GUARD][...] of NaN on the device (fp16 NaN = 0x7e00)."""
    return torch.full((rows + GUARD, *tail), NAN, dtype=dtype, device="cuda")


def assert_guard(t, rows, what):
    torch.cuda.synchronize()
    assert bool(torch.isnan(t[rows:]).all()), f"{what}: rows past M were written"


def planes_buf(ops, M, N, init=None):
    """A two-plane [M + GUARD][N] buffer, NaN in the guard rows of both planes (and everywhere
    without init): (flat fp16 buffer, [2][M + GUARD][N] view, plane)."""
    plane = (M + GUARD) * N
    if init is None:
        buf = torch.full((2 * plane,), NAN, dtype=torch.float16, device="cuda")
    else:
        buf = ops.to_planes(torch.from_numpy(init).cuda(), plane)
    v = buf.view(2, M + GUARD, N)
    v[:, M:] = NAN
    return buf, v, plane


def planes64(v, M):
    return v[0, :M].double().cpu().numpy() + v[1, :M].double().cpu().numpy()


def check_planes(v, M, ref, what):
    """|lo| <= ulp(hi) / 2 and hi + lo against the reference."""
    hi, lo = v[0, :M].cpu().numpy(), v[1, :M].cpu().numpy()
    assert np.isfinite(hi).all() and np.isfinite(lo).all(), what
    assert (np.abs(lo.astype(np.float64)) <= np.spacing(np.abs(hi)).astype(np.float64) / 2).all(), f"{what}: |lo| > ulp(hi) / 2"
    e = nerr(hi.astype(np.float64) + lo.astype(np.float64), ref)
    print(f"{what}: planes err {e:.3e}")
    assert e < TOL32, f"{what}: {e:.3e}"


def check_stats(ops, got, ref_rows, eps, what):
    """Producer statistics two ways: per chunk against the float64 statistics of the reference rows, and
    after Chan's combine against the rows' mean and rstd.  mean within 1e-4 sigma_row, M2 and rstd within
    1e-4 relative."""
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), what
    ref = ops.chunk_stats(ref_rows)
    sigma = ref_rows.std(axis=1)
    e_mean = float((np.abs(got[..., 0] - ref[..., 0]) / sigma[:, None]).max())
    e_m2 = float((np.abs(got[..., 1] - ref[..., 1]) / ref[..., 1]).max())
    mean, rstd = ops.combine_stats(got, eps)
    rstd_ref = 1.0 / np.sqrt(ref_rows.var(axis=1) + eps)
    e_rm = float((np.abs(mean - ref_rows.mean(axis=1)) / sigma).max())
    e_rs = float((np.abs(rstd - rstd_ref) / rstd_ref).max())
    print(f"{what}: chunk mean {e_mean:.3e} sigma, M2 {e_m2:.3e}; row mean {e_rm:.3e} sigma, rstd {e_rs:.3e}")
    assert max(e_mean, e_m2, e_rm, e_rs) < TOL_STAT, f"{what}: {(e_mean, e_m2, e_rm, e_rs)}"


ACT_F, RES_F32_F, RES_PLANES_F, OUT_PLANES_F, OUT_F32_F = 1, 2, 4, 8, 32  # spi_debug_gemm_plan's flag word


def gemm_plan(ops, M, N, K, flags=0, ln_in=0, res_ln=0):
    """(gemm256 tile height or 0 for the general kernel, gemm256 slices, the general kernel's split-K)."""
    out = (C.c_longlong * 14)()
    rc = ops.lib.spi_debug_gemm_plan(1, M, N, K, K, 1, 0, C.c_uint(flags | ln_in << 8 | res_ln << 16), out)
    assert rc == 0
    return int(out[0]), int(out[1]), int(out[7])


# ---------------------------------------------------------------------------------------------
# a / b: the consumer epilogue  y = rstd (acc - mean c1) + bias'


def run_consumer(ops, ws, M, N, K, act, want_g256):
    Wp, W16, bias, c1, bias_d, c1_d = folded_linear(ops, N, K)
    x = make_rows(np.random.default_rng(M * 13 + N + K), M, K)
    A16 = x.astype(np.float16)
    # as the model: the statistics of the fp32 rows, not of their fp16 copy
    stats = ops.chunk_stats(x.astype(np.float64)).astype(np.float32)
    mean, rstd = ops.combine_stats(stats, EPS)
    ref = rstd[:, None] * (A16.astype(np.float64) @ W16.T - mean[:, None] * c1.astype(np.float64)) + bias
    if act == "gelu":
        ref = gelu64(ref)
    g256 = gemm_plan(ops, M, N, K, flags=ACT_F if act else 0, ln_in=K // 64)[0]
    assert (g256 != 0) == want_g256, f"routing: gemm256 tile height {g256}"
    out = guarded(M, N, dtype=torch.float16)
    ops.gemm_ln(torch.from_numpy(A16).cuda(), Wp, N, out, "fp16", bias=bias_d, in_stats=torch.from_numpy(stats).cuda(),
                c1=c1_d, eps=EPS, act=act, ws=ws)
    assert_guard(out, M, "C")
    e = nerr(out[:M].float().cpu().numpy(), ref)
    print(f"consumer {M}x{N}x{K} {act} g256={g256}: {e:.3e}")
    assert e < TOL16, f"consumer {M}x{N}x{K} {act}: {e:.3e}"


@pytest.mark.parametrize("act", [None, "gelu"])
@pytest.mark.parametrize("N,K", [(128, 64), (256, 192), (384, 640), (256, 1024), (128, 1088)])
@pytest.mark.parametrize("M", [1, 100, 394])
def test_consumer_general_kernel(ops, ws, M, N, K, act):
    """gemm.hip's consumer fold at 1, 3, 10, 16 chunks (ln_row_stats' all-loads-first form) and 17 (its
    loop form, past every model's width), one row / ragged tiles."""
    run_consumer(ops, ws, M, N, K, act, want_g256=False)


def run_consumer_hilo(ops, ws, M, N, K, act, out_dtype):
    """run_consumer on hi + lo weights (the fp16m transformers: krep = 2): W', bias' and c1 from
    fold_linear(hilo=True), W' packed by pack_weight_hilo, the reference on hilo_values(W')."""
    A16, stats, wf, bias, c1 = op_refs.krep_fold_case(ops, M, N, K)
    ref = op_refs.fold_consumer64(A16.astype(np.float64) @ op_refs.hilo_values(wf).T, stats, c1, bias, EPS)
    if act == "gelu":
        ref = gelu64(ref)
    out = (C.c_longlong * 14)()
    flags = (ACT_F if act else 0) | (OUT_F32_F if out_dtype == torch.float32 else 0) | (K // 64) << 8
    assert ops.lib.spi_debug_gemm_plan(1, M, N, K, K, 2, 0, C.c_uint(flags), out) == 0
    assert int(out[0]) == 0, f"routing: krep = 2 on gemm256 (tile height {int(out[0])})"
    y = guarded(M, N, dtype=out_dtype)
    ops.gemm_ln(torch.from_numpy(A16).cuda(), ops.pack_weight_hilo(wf), N, y,
                "fp32" if out_dtype == torch.float32 else "fp16", bias=torch.from_numpy(bias).cuda(),
                in_stats=torch.from_numpy(stats).cuda(), c1=torch.from_numpy(c1).cuda(), eps=EPS, act=act, ws=ws,
                hilo=True)
    assert_guard(y, M, "C")
    e = nerr(y[:M].float().cpu().numpy(), ref)
    print(f"consumer hi + lo {M}x{N}x{K} {act} splits={int(out[7])}: {e:.3e}")
    return e


@pytest.mark.parametrize("M,N,K", op_refs.KREP_FOLD)
def test_consumer_hilo_weights(ops, ws, M, N, K):
    """The consumer fold over the hi + lo k-loop at 1, 3, 10 and 16 chunks into an fp32 output: the bar that
    sees the lo half (test_op_refs.test_krep_folded_consumer_discriminates: without it > 1e-4)."""
    assert run_consumer_hilo(ops, ws, M, N, K, None, torch.float32) < TOL32


@pytest.mark.parametrize("M,N,K", [(100, 384, 640)])
def test_consumer_hilo_weights_gelu_fp16_out(ops, ws, M, N, K):
    assert run_consumer_hilo(ops, ws, M, N, K, "gelu", torch.float16) < TOL16


@pytest.mark.parametrize("K", [128, 384, 640, 1024])
@pytest.mark.parametrize("N", [256, 512])
@pytest.mark.parametrize("M", [1, 129, 300])
def test_consumer_gemm256(ops, ws, gemm256_everywhere, M, N, K):
    """gemm256.hip's consumer fold (four lanes per row, masked chunks past the count) at 2, 6, 10 and
    16 chunks."""
    run_consumer(ops, ws, M, N, K, "gelu" if K % 256 else None, want_g256=True)


@pytest.mark.parametrize("K", [64, 192, 1088])
def test_consumer_odd_chunk_counts_keep_general_kernel(ops, ws, gemm256_everywhere, K):
    """gemm256_ln_chunks_ok: 1, 3 and 17 chunks are not gemm256's; the router keeps them on the general
    kernel although everything else is forced onto gemm256."""
    run_consumer(ops, ws, 129, 256, K, None, want_g256=False)


# ---------------------------------------------------------------------------------------------
# c: the producer epilogue (chunk statistics + fp16 copy), all residual / output forms

PRODUCER_FORMS = [("f32", None), ("f32", "fp32"), ("f32", "fp16"), ("planes", None), ("planes", "fp32"),
                  ("planes", "inplace")]


def run_producer(ops, ws, M, N, K, out_form, res_form, want_g256=None, want_splits=None):
    Wp, W16, b, b_d = plain_linear(ops, N, K)
    rng = np.random.default_rng(M * 17 + N + K)
    A16 = (rng.standard_normal((M, K)) * 1.5).astype(np.float16)
    R = make_rows(rng, M, N)  # the residual makes the output rows distinguishable
    acc = A16.astype(np.float64) @ W16.T + b
    flags = {"f32": OUT_F32_F, "planes": OUT_PLANES_F}[out_form] | \
        {None: 0, "fp32": RES_F32_F, "fp16": 0, "inplace": RES_PLANES_F}[res_form]
    g256, g256_splits, splits = gemm_plan(ops, M, N, K, flags=flags)
    what = f"producer {M}x{N}x{K} out {out_form} res {res_form} g256={g256}x{g256_splits} splits={splits}"
    if want_g256 is not None:
        assert (g256 != 0) == want_g256, what
    if want_splits == "general":
        assert g256 == 0 and splits > 1, what
    elif want_splits is not None:
        assert g256 != 0 and g256_splits == want_splits, what
    stats = guarded(M, N // 64, 2)
    kw = dict(bias=b_d, out_stats=stats, eps=EPS, ws=ws)
    pv = c16 = Cf = None
    if out_form == "planes":
        buf, pv, plane = planes_buf(ops, M, N, R if res_form == "inplace" else None)
        kw.update(plane=plane)
        C_d = buf
    else:
        Cf = C_d = guarded(M, N)
        c16 = guarded(M, N, dtype=torch.float16)
        kw.update(c16=c16)
    if res_form == "inplace":
        ref = acc + planes64(pv, M)
        kw.update(residual=buf, res_kind="planes")
    elif res_form == "fp32":
        ref = acc + R
        kw.update(residual=torch.from_numpy(R).cuda(), res_kind="fp32")
    elif res_form == "fp16":
        R16 = R.astype(np.float16)
        ref = acc + R16.astype(np.float64)
        kw.update(residual=torch.from_numpy(R16).cuda(), res_kind="fp16")
    else:
        ref = acc
    ops.gemm_ln(torch.from_numpy(A16).cuda(), Wp, N, C_d, out_form if out_form == "planes" else "fp32", M=M, **kw)
    assert_guard(stats, M, "statistics")
    if out_form == "planes":
        assert_guard(pv[0], M, "hi plane")
        assert_guard(pv[1], M, "lo plane")
        check_planes(pv, M, ref, what)
    else:
        assert_guard(Cf, M, "C")
        assert_guard(c16, M, "c16")
        e = nerr(Cf[:M].cpu().numpy(), ref)
        print(f"{what}: {e:.3e}")
        assert e < TOL32, f"{what}: {e:.3e}"
        assert torch.equal(c16[:M], Cf[:M].half()), f"{what}: c16 is not C rounded to fp16"
    check_stats(ops, stats[:M].cpu().numpy(), ref, EPS, what)


@pytest.mark.parametrize("out_form,res_form", PRODUCER_FORMS)
@pytest.mark.parametrize("N,K", [(128, 64), (384, 320), (1024, 64)])
@pytest.mark.parametrize("M", [1, 100, 300])
def test_producer_general_kernel(ops, ws, M, N, K, out_form, res_form):
    run_producer(ops, ws, M, N, K, out_form, res_form, want_g256=False)


@pytest.mark.parametrize("out_form,res_form", [("f32", "fp32"), ("planes", "inplace")])
def test_producer_split_k(ops, ws, out_form, res_form):
    """The producer epilogue in the general kernel's split-K reduction (the last slice to arrive
    runs it)."""
    run_producer(ops, ws, 100, 128, 3072, out_form, res_form, want_splits="general")


@pytest.mark.parametrize("out_form,res_form", [("f32", "fp32"), ("planes", "inplace")])
@pytest.mark.parametrize("K", [64, 320])
@pytest.mark.parametrize("N", [256, 512])
@pytest.mark.parametrize("M", [129, 300])
def test_producer_gemm256(ops, ws, gemm256_everywhere, M, N, K, out_form, res_form):
    """gemm256.hip's producer epilogue: fp32 over an fp32 residual, two planes in place (ViT)."""
    run_producer(ops, ws, M, N, K, out_form, res_form, want_g256=True)


@pytest.mark.parametrize("out_form,res_form", [("f32", None), ("f32", "fp16"), ("planes", None), ("planes", "fp32")])
def test_producer_forms_outside_gemm256_keep_general_kernel(ops, ws, gemm256_everywhere, out_form, res_form):
    """Producers gemm256 has no epilogue for (no residual, a residual of another form than the output):
    the plan alone would route them to gemm256, which rejects them; gemm() keeps the general kernel."""
    run_producer(ops, ws, 300, 512, 320, out_form, res_form)


@pytest.mark.parametrize("out_form,res_form", [("f32", "fp32"), ("planes", "inplace")])
def test_producer_gemm256_split_k(ops, ws, gemm256_everywhere, out_form, res_form):
    """gemm256's split-K (opt-in: SPI_GEMM_256_LONGK's third field), two slices of 16 k-tiles."""
    os.environ["SPI_GEMM_256_LONGK"] = "48,1024,4"
    os.environ["SPI_GEMM_MAXSPLIT"] = "2"
    ops.lib.spi_debug_gemm_reload_env()
    try:
        run_producer(ops, ws, 300, 512, 2048, out_form, res_form, want_splits=2)
    finally:
        os.environ.pop("SPI_GEMM_MAXSPLIT", None)
        os.environ.pop("SPI_GEMM_256_LONGK", None)
        ops.lib.spi_debug_gemm_reload_env()


# ---------------------------------------------------------------------------------------------
# c': the general kernel's residual and output forms without a fold, on both store paths: the vector
# path (tiles inside N, 16-byte aligned rows; 64 x 64 tiles prefetch the residual tile into LDS, taller
# ones load it from global memory) and the per-element path (tiles crossing N, unaligned strides)

PLAIN_FORMS = [
    # M, N, K, output, residual, ldc, ldr, tile rows
    (100, 72, 64, "planes", "inplace", None, None, 64),   # per element: two planes over two planes
    (65, 72, 128, "fp16", "fp32", None, None, 64),        # per element: fp16 over an fp32 residual
    (100, 72, 64, "fp16", "fp16", None, None, 64),        # per element: fp16 over fp16
    (65, 128, 64, "f32", "fp16", 132, None, 64),          # per element by an unaligned ldc
    (65, 128, 64, "planes", "fp32", None, 130, 64),       # per element by an unaligned ldr
    (65, 128, 64, "fp16", "fp32", None, None, 64),        # vector, prefetched: fp32 rows under an fp16 output
    (65, 128, 64, "fp16", "fp16", None, None, 64),        # vector, prefetched: fp16 rows
    (300, 3072, 64, "planes", "inplace", None, None, 128),  # vector, two-plane residual from global memory
]


@pytest.mark.parametrize("M,N,K,out_form,res_form,ldc,ldr,bm", PLAIN_FORMS)
def test_plain_forms_both_store_paths(ops, ws, M, N, K, out_form, res_form, ldc, ldr, bm):
    Wp, W16, b, b_d = plain_linear(ops, N, K)
    rng = np.random.default_rng(M * 23 + N + K)
    A16 = (rng.standard_normal((M, K)) * 1.5).astype(np.float16)
    R = make_rows(rng, M, N)
    acc = A16.astype(np.float64) @ W16.T + b
    ldc, ldr = ldc or N, ldr or N
    flags = {"f32": OUT_F32_F, "planes": OUT_PLANES_F, "fp16": 0}[out_form] | \
        {"fp32": RES_F32_F, "fp16": 0, "inplace": RES_PLANES_F}[res_form]
    plan = (C.c_longlong * 14)()
    assert ops.lib.spi_debug_gemm_plan(1, M, N, K, K, 1, 0, C.c_uint(flags), plan) == 0
    what = f"plain {M}x{N}x{K} out {out_form} ldc {ldc} res {res_form} ldr {ldr}"
    assert (int(plan[0]), int(plan[4]), int(plan[7])) == (0, bm, 1), f"{what}: routing {list(plan)}"
    kw = dict(bias=b_d, ldc=ldc, ldr=ldr, ws=ws)
    pv = None
    if out_form == "planes":
        C_d, pv, plane = planes_buf(ops, M, N, R if res_form == "inplace" else None)
        kw.update(plane=plane)
    else:
        C_d = guarded(M, ldc, dtype=torch.float32 if out_form == "f32" else torch.float16)
    if res_form == "inplace":
        ref = acc + planes64(pv, M)
        kw.update(residual=C_d, res_kind="planes")
    else:
        Rs = R.astype(np.float32 if res_form == "fp32" else np.float16)
        ref = acc + Rs.astype(np.float64)
        Rd = guarded(M, ldr, dtype=torch.from_numpy(Rs).dtype)  # NaN past N: a read there shows
        Rd[:M, :N] = torch.from_numpy(Rs).cuda()
        kw.update(residual=Rd, res_kind=res_form)
    ops.gemm_ln(torch.from_numpy(A16).cuda(), Wp, N, C_d, {"f32": "fp32"}.get(out_form, out_form), M=M, **kw)
    if out_form == "planes":
        assert_guard(pv[0], M, "hi plane")
        assert_guard(pv[1], M, "lo plane")
        check_planes(pv, M, ref, what)
        return
    assert_guard(C_d, M, "C")
    assert bool(torch.isnan(C_d[:M, N:]).all()), f"{what}: columns past N were written"
    e = nerr(C_d[:M, :N].float().cpu().numpy(), ref)
    print(f"{what}: {e:.3e}")
    assert e < (TOL32 if out_form == "f32" else TOL16), f"{what}: {e:.3e}"


# ---------------------------------------------------------------------------------------------
# d: the post-LN residual  C = A W^T + b + LN(R) g + beta  (BERT's out-proj / FFN2)


def run_res_ln(ops, ws, M, N, r_form, producer, want_general=False):
    K = 64
    Wp, W16, b, b_d = plain_linear(ops, N, K)
    rng = np.random.default_rng(M * 19 + N)
    A16 = rng.standard_normal((M, K)).astype(np.float16)
    R = make_rows(rng, M, N)
    g, beta = make_ln(rng, N)
    # as the model: statistics of the fp32 rows the producing GEMM held, R as stored (fp32 or hi + lo)
    st = ops.chunk_stats(R.astype(np.float64)).astype(np.float32)
    mean, rstd = ops.combine_stats(st, EPS)
    flags = RES_F32_F | OUT_F32_F if r_form == "fp32" else RES_PLANES_F | OUT_PLANES_F
    g256 = gemm_plan(ops, M, N, K, flags=flags, res_ln=N // 64)[0]
    what = f"res_ln {M}x{N} R {r_form} producer {producer} g256={g256}"
    if want_general:
        assert g256 == 0, what
    kw = dict(bias=b_d, res_stats=torch.from_numpy(st).cuda(), res_g=torch.from_numpy(g).cuda(),
              res_b=torch.from_numpy(beta).cuda(), eps=EPS, ws=ws)
    stats = c16 = None
    if producer:
        stats = guarded(M, N // 64, 2)
        kw.update(out_stats=stats)
    if r_form == "fp32":
        R_st = R.astype(np.float64)
        C_d = guarded(M, N)
        kw.update(residual=torch.from_numpy(R).cuda(), res_kind="fp32")
        if producer:
            c16 = guarded(M, N, dtype=torch.float16)
            kw.update(c16=c16)
    else:
        rbuf, rv, plane = planes_buf(ops, M, N, R)
        R_st = planes64(rv, M)
        C_d, cv, _ = planes_buf(ops, M, N)
        kw.update(residual=rbuf, res_kind="planes", plane=plane)
    ref = A16.astype(np.float64) @ W16.T + b + ((R_st - mean[:, None]) * rstd[:, None] * g + beta)
    ops.gemm_ln(torch.from_numpy(A16).cuda(), Wp, N, C_d, "fp32" if r_form == "fp32" else "planes", M=M, **kw)
    if r_form == "fp32":
        assert_guard(C_d, M, "C")
        e = nerr(C_d[:M].cpu().numpy(), ref)
        print(f"{what}: {e:.3e}")
        assert e < TOL32, f"{what}: {e:.3e}"
        if producer:
            assert_guard(c16, M, "c16")
            assert torch.equal(c16[:M], C_d[:M].half())
    else:
        assert_guard(cv[0], M, "hi plane")
        assert_guard(cv[1], M, "lo plane")
        check_planes(cv, M, ref, what)
    if producer:
        assert_guard(stats, M, "statistics")
        check_stats(ops, stats[:M].cpu().numpy(), ref, EPS, what)


@pytest.mark.parametrize("producer", [False, True], ids=["alone", "producer"])
@pytest.mark.parametrize("r_form", ["fp32", "planes"])
@pytest.mark.parametrize("N", [128, 640, 1024, 1152])
@pytest.mark.parametrize("M", [1, 100])
def test_res_ln(ops, ws, M, N, r_form, producer):
    """res_ln_chunks at 2, 10, 16 chunks and 18 (ln_row_stats' loop form)."""
    run_res_ln(ops, ws, M, N, r_form, producer)


@pytest.mark.parametrize("r_form", ["fp32", "planes"])
def test_res_ln_keeps_general_kernel(ops, ws, gemm256_everywhere, r_form):
    """gemm256 has no post-LN residual epilogue: N = 1024 stays on the general kernel under forcing."""
    run_res_ln(ops, ws, 100, 1024, r_form, True, want_general=True)


# ---------------------------------------------------------------------------------------------
# e: producer -> consumer / post-LN residual on the device's own buffers


def run_chain(ops, ws):
    M, D, N, K1 = 394, 256, 512, 64
    rng = np.random.default_rng(2024)
    # producer, two planes in place: x = R + A1 W1^T + b1, statistics Sx
    W1p, W1, b1, b1_d = plain_linear(ops, D, K1)
    A1 = rng.standard_normal((M, K1)).astype(np.float16)
    xbuf, xv, plane = planes_buf(ops, M, D, make_rows(rng, M, D))
    x_ref = planes64(xv, M) + A1.astype(np.float64) @ W1.T + b1
    Sx = guarded(M, D // 64, 2)
    ops.gemm_ln(torch.from_numpy(A1).cuda(), W1p, D, xbuf, "planes", M=M, bias=b1_d, residual=xbuf, res_kind="planes",
                plane=plane, out_stats=Sx, eps=EPS, ws=ws)
    assert_guard(Sx, M, "Sx")
    check_planes(xv, M, x_ref, "chain producer")
    hi = xv[0, :M].double().cpu().numpy()
    x_st = planes64(xv, M)
    # float64 statistics of the reference producer output: the device's fp32 ones have to agree
    mean, rstd = x_ref.mean(axis=1), 1.0 / np.sqrt(x_ref.var(axis=1) + EPS)
    # consumer on the hi plane (lda = D) with the device's Sx
    W2p, W2, bias2, c1, bias2_d, c1_d = folded_linear(ops, N, D)
    y = guarded(M, N, dtype=torch.float16)
    ops.gemm_ln(xbuf, W2p, N, y, "fp16", M=M, K=D, lda=D, bias=bias2_d, in_stats=Sx, c1=c1_d, eps=EPS, act="gelu", ws=ws)
    assert_guard(y, M, "consumer C")
    ref_y = gelu64(rstd[:, None] * (hi @ W2.T - mean[:, None] * c1.astype(np.float64)) + bias2)
    e_y = nerr(y[:M].float().cpu().numpy(), ref_y)
    # post-LN residual GEMM over the same rows and Sx, into another two-plane tensor
    W3p, W3, b3, b3_d = plain_linear(ops, D, 128)
    A3 = rng.standard_normal((M, 128)).astype(np.float16)
    g, beta = make_ln(rng, D)
    zbuf, zv, _ = planes_buf(ops, M, D)
    ops.gemm_ln(torch.from_numpy(A3).cuda(), W3p, D, zbuf, "planes", M=M, bias=b3_d, residual=xbuf, res_kind="planes",
                plane=plane, res_stats=Sx, res_g=torch.from_numpy(g).cuda(), res_b=torch.from_numpy(beta).cuda(),
                eps=EPS, ws=ws)
    ref_z = A3.astype(np.float64) @ W3.T + b3 + ((x_st - mean[:, None]) * rstd[:, None] * g + beta)
    print(f"chain: consumer {e_y:.3e}")
    assert e_y < TOL16, e_y
    assert_guard(zv[0], M, "res_ln hi")
    check_planes(zv, M, ref_z, "chain res_ln")


def test_chain_default_routing(ops, ws):
    run_chain(ops, ws)


def test_chain_gemm256(ops, ws, gemm256_everywhere):
    run_chain(ops, ws)


# ---------------------------------------------------------------------------------------------
# f: layernorm_planes


def run_layernorm_planes(ops, rows, D, prec, with_yf, stride_rows=1):
    rng = np.random.default_rng(rows * 23 + D)
    total = rows * stride_rows
    x = make_rows(rng, total, D)
    g, beta = make_ln(rng, D)
    xbuf = ops.to_planes(torch.from_numpy(x).cuda())
    plane = total * D
    x64 = (xbuf[:plane].double() + xbuf[plane:].double()).cpu().numpy().reshape(total, D)[::stride_rows]
    eps = 1e-6
    ref = (x64 - x64.mean(1, keepdims=True)) / np.sqrt(x64.var(1, keepdims=True) + eps) * g + beta
    yf = guarded(rows, D) if with_yf else None
    yt = guarded(rows, D, dtype=torch.float16 if prec == "fp16" else torch.float32)
    ops.layernorm_planes(prec, xbuf, plane, stride_rows * D, torch.from_numpy(g).cuda(), torch.from_numpy(beta).cuda(),
                         rows, D, eps, yf=yf, yt=yt)
    assert_guard(yt, rows, "yt")
    e_t = nerr(yt[:rows].float().cpu().numpy(), ref)
    e_f = 0.0
    if with_yf:
        assert_guard(yf, rows, "yf")
        e_f = nerr(yf[:rows].cpu().numpy(), ref)
    print(f"layernorm_planes {rows}x{D} {prec} stride {stride_rows}: yt {e_t:.3e} yf {e_f:.3e}")
    # test_layernorm's bars: 2e-6 for fp32 rows, 1e-3 for the fp16 copy
    assert e_f < 2e-6 and e_t < (1e-3 if prec == "fp16" else 2e-6), (e_f, e_t)


@pytest.mark.parametrize("with_yf", [False, True], ids=["yt", "yt+yf"])
@pytest.mark.parametrize("prec", ["fp16", "fp32"])
@pytest.mark.parametrize("D", [128, 200, 768, 1024])
@pytest.mark.parametrize("rows", [1, 5, 394])
def test_layernorm_planes(ops, rows, D, prec, with_yf):
    run_layernorm_planes(ops, rows, D, prec, with_yf)


@pytest.mark.parametrize("prec", ["fp16", "fp32"])
@pytest.mark.parametrize("D", [128, 768, 1024])
def test_layernorm_planes_strided_rows(ops, D, prec):
    """The class-token read: rows ldx = S D apart."""
    run_layernorm_planes(ops, 2, D, prec, True, stride_rows=3)


def test_layernorm_planes_rejects_wide_rows(ops):
    D = 1088
    xbuf = torch.zeros(2 * D, dtype=torch.float16, device="cuda")
    v = torch.ones(D, device="cuda")
    yt = guarded(1, D)
    with pytest.raises(ops.OpError, match="1024"):
        ops.layernorm_planes("fp32", xbuf, D, D, v, v, 1, D, 1e-6, yt=yt)
    torch.cuda.synchronize()
    assert bool(torch.isnan(yt).all())


# ---------------------------------------------------------------------------------------------
# g: vit_assemble_planes


@pytest.mark.parametrize("with_stats", [False, True], ids=["nostats", "stats"])
@pytest.mark.parametrize("B,P,D", [(1, 4, 64), (3, 196, 128), (2, 9, 1024)])
def test_vit_assemble_planes(ops, B, P, D, with_stats):
    """Planes and chunk statistics of cls / patch + pos; (1, 4, 64) is 40 eight-column groups, one
    partial block whose idle lanes still take part in the chunk shuffles."""
    rng = np.random.default_rng(B * 29 + P + D)
    S, T = P + 1, B * (P + 1)
    patches = make_rows(rng, B * P, D)
    cls = make_rows(rng, 1, D)[0]
    pos = (make_rows(rng, S, D) * 0.25).astype(np.float32)
    y32 = np.empty((B, S, D), np.float32)
    y32[:, 0] = cls + pos[0]
    y32[:, 1:] = patches.reshape(B, P, D) + pos[1:]  # float32 adds, as the kernel's
    y32 = y32.reshape(T, D)
    buf, pv, plane = planes_buf(ops, T, D)
    stats = guarded(T, D // 64, 2) if with_stats else None
    ops.vit_assemble_planes(torch.from_numpy(patches).cuda(), torch.from_numpy(cls).cuda(), torch.from_numpy(pos).cuda(),
                            buf, plane, stats, B, P, D)
    assert_guard(pv[0], T, "hi plane")
    assert_guard(pv[1], T, "lo plane")
    assert np.array_equal(pv[0, :T].cpu().numpy(), y32.astype(np.float16)), "hi plane is not fp16(patch + pos)"
    check_planes(pv, T, y32.astype(np.float64), f"vit_assemble_planes {B}x{P}x{D}")
    if with_stats:
        assert_guard(stats, T, "statistics")
        check_stats(ops, stats[:T].cpu().numpy(), y32.astype(np.float64), 1e-6, f"vit_assemble_planes {B}x{P}x{D}")


def test_vit_assemble_planes_rejects_bad_shapes(ops):
    z = torch.zeros(4096, device="cuda")
    buf = torch.zeros(8192, dtype=torch.float16, device="cuda")
    with pytest.raises(ops.OpError):
        ops.vit_assemble_planes(z, z, z, buf, 1024, None, 1, 3, 96)   # D % 64
    with pytest.raises(ops.OpError):
        ops.vit_assemble_planes(z, z, z, buf, 1028, None, 1, 3, 64)   # plane % 8


# ---------------------------------------------------------------------------------------------
# h: calls gemm() documents as invalid return an error and launch nothing


def test_gemm_ln_rejections(ops, ws):
    M, K = 100, 128
    rng = np.random.default_rng(5)
    A = torch.from_numpy(rng.standard_normal((M, K)).astype(np.float16)).cuda()
    st = torch.from_numpy(ops.chunk_stats(A.double().cpu().numpy()).astype(np.float32)).cuda()

    def rejected(N, out, out_kind, **kw):
        Wp = folded_linear(ops, N, K)[0]
        with pytest.raises(ops.OpError) as ei:
            ops.gemm_ln(A, Wp, N, out, out_kind, eps=EPS, ws=ws, **kw)
        assert str(ei.value), "no message"
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()), f"{kw.keys()}: a kernel ran"
        return str(ei.value)

    vec = lambda n: torch.ones(n, device="cuda")  # noqa: E731
    # the fold needs whole 128-column tiles
    rejected(192, guarded(M, 192, dtype=torch.float16), "fp16", in_stats=st, c1=vec(192), bias=vec(192))
    # a two-plane output with an fp16-typed residual that is not two planes
    buf, _, plane = planes_buf(ops, M, 256)
    rejected(256, buf, "planes", plane=plane, residual=torch.zeros(M, 256, dtype=torch.float16, device="cuda"),
             res_kind="fp16")
    # plane offset off the 16-byte grid
    buf = torch.full((2 * M * 256 + 8,), NAN, dtype=torch.float16, device="cuda")
    rejected(256, buf, "planes", plane=M * 256 + 4)
    # c1 off 16-byte alignment
    c1 = vec(257)
    rejected(256, guarded(M, 256, dtype=torch.float16), "fp16", in_stats=st, c1=c1.data_ptr() + 4, bias=vec(256))
    # half a consumer fold
    rejected(256, guarded(M, 256, dtype=torch.float16), "fp16", in_stats=st)
    # the consumer fold writes fp16 on gemm256: an fp32 output on that route is rejected, not rerouted
    os.environ["SPI_GEMM_256_MIN"] = "1"
    ops.lib.spi_debug_gemm_reload_env()
    try:
        assert gemm_plan(ops, M, 256, K, flags=OUT_F32_F, ln_in=K // 64)[0] != 0
        msg = rejected(256, guarded(M, 256), "fp32", in_stats=st, c1=vec(256), bias=vec(256))
        assert "gemm256" in msg
    finally:
        os.environ.pop("SPI_GEMM_256_MIN", None)
        ops.lib.spi_debug_gemm_reload_env()

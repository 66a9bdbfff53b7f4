"""Op-level parity of the hi + lo weight k-loop (GemmDesc::krep = 2: fp16m's downsample convs, every GEMM
of the fp16m transformers, ViT's patch projection and head) through spi_op_gemm_hilo / spi_op_conv2d_hilo.

The reference is numpy / torch float64 on the values the kernel multiplies -- fp16 activations and
op_refs.hilo_values(w) = fp16(w) + fp16(w - fp16(w)) -- so only the fp32 accumulation separates the two and
the bars are the project's operand-exact ones: 1e-5 normalised max error into an fp32 output, 2e-3 into fp16.
test_op_refs.test_krep_cases_discriminate shows, for these same inputs, that a contraction which lost the lo
half sits above 1e-4 and an fp32-accumulated emulation below 3e-6.

Every output buffer has 8 rows of NaN behind it that must survive; split-K cases run twice on one
workspace (tickets back at zero, slabs summed in slice order: the same bits).
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import op_refs as R
from oracle.cpu_codelet import normalized_max_error

pytestmark = pytest.mark.gpu

TOL32, TOL16 = 1e-5, 2e-3
GUARD = 8
NAN = float("nan")


@pytest.fixture(scope="module")
def ops(spi, gpu):
    import importlib
    return importlib.import_module("starpu-inference-server_amd.ops")


@pytest.fixture(scope="module")
def ws(ops):
    return ops.workspace()


def guarded(rows, *tail, dtype=torch.float32):
    return torch.full((rows + GUARD, *tail), NAN, dtype=dtype, device="cuda")


def assert_guard(t, rows, what):
    torch.cuda.synchronize()
    assert bool(torch.isnan(t[rows:]).all()), f"{what}: rows past M were written"


def dense_plan(ops, M, N, K):
    """The plan of a krep = 2 fp16 GEMM: (gemm256 tile height, the general kernel's plan as a dict)."""
    out = (C.c_longlong * 14)()
    assert ops.lib.spi_debug_gemm_plan(1, M, N, K, K, 2, 0, C.c_uint(0), out) == 0
    return int(out[0]), dict(zip(ops.PAIR_PLAN_FIELDS, [int(v) for v in out[4:12]]))


_dense_cache = {}


def dense_inputs(ops, M, N, K):
    """One shape's inputs on the device and its float64 accumulator, shared by its forms."""
    key = (M, N, K)
    if key not in _dense_cache:
        A16, W, b, Rr = R.krep_dense_case(M, N, K)
        _dense_cache[key] = dict(A=torch.from_numpy(A16).cuda(), Wp=ops.pack_weight_hilo(W), b=b, R=Rr,
                                 b_d=torch.from_numpy(b).cuda(), R_d=torch.from_numpy(Rr).cuda(),
                                 acc=R.dense_acc64(A16, R.hilo_values(W)))
    return _dense_cache[key]


def run_dense(ops, ws, M, N, K, form, out_dtype=torch.float32, runs=1):
    c = dense_inputs(ops, M, N, K)
    res, act = (c["R"] if form == "res32" else None), {"relu": "relu", "gelu": "gelu"}.get(form)
    ref = R.epilogue64(c["acc"], c["b"], res, act)
    outs = []
    for _ in range(runs):
        out = guarded(M, N, dtype=out_dtype)
        ops.gemm_hilo(c["A"], c["Wp"], N, bias=c["b_d"], residual=c["R_d"] if form == "res32" else None, out=out[:M],
                      act=act, ws=ws)
        assert_guard(out, M, f"{M}x{N}x{K} {form}")
        outs.append(out[:M].float().cpu().numpy())
    return outs, ref


@pytest.mark.parametrize("form", R.KREP_FORMS)
@pytest.mark.parametrize("M,N,K", R.KREP_DENSE)
def test_gemm_hilo(ops, ws, M, N, K, form):
    """Ragged M and N, a K tail of half a block (96, 160), one to 18 A steps; the default plan splits the
    last three shapes into 4 to 6 slices of whole (hi, lo) step pairs."""
    g256, pl = dense_plan(ops, M, N, K)
    assert g256 == 0, "krep = 2 stays on the general kernel"
    assert pl["k_per_split"] % 128 == 0, pl
    if K >= 768:
        assert 4 <= pl["splits"] <= 6, pl
    (o1, o2), ref = run_dense(ops, ws, M, N, K, form, runs=2)
    e = normalized_max_error(o1, ref)
    print(f"gemm_hilo {M}x{N}x{K} {form} splits={pl['splits']}: {e:.3e}")
    assert e < TOL32, f"gemm_hilo {M}x{N}x{K} {form}: {e:.3e}"
    assert np.array_equal(o1, o2), "two launches on one workspace differ"


def test_gemm_hilo_gelu_fp16_out(ops, ws):
    M, N, K = R.KREP_GELU
    (o,), ref = run_dense(ops, ws, M, N, K, "gelu", out_dtype=torch.float16)
    e = normalized_max_error(o, ref)
    print(f"gemm_hilo {M}x{N}x{K} gelu fp16 out: {e:.3e}")
    assert e < TOL16


@pytest.mark.parametrize("plan,shape", R.KREP_FORCED, ids=[p for p, _ in R.KREP_FORCED])
def test_gemm_hilo_forced_plans(ops, ws, plan, shape):
    """SPI_GEMM_PLAN: the other tile shapes and ring depths, and a split count that does not divide the
    packed steps -- 14 steps five ways must round to whole (hi, lo) pairs: 4 slices of 4, 4, 4, 2."""
    M, N, K = shape
    bm, bn, stages, splits = (int(v) for v in plan.split(","))
    os.environ["SPI_GEMM_PLAN"] = plan
    ops.lib.spi_debug_gemm_reload_env()
    try:
        g256, pl = dense_plan(ops, M, N, K)
        assert g256 == 0 and (pl["bm"], pl["bn"], pl["stages"]) == (bm, bn, stages), pl
        assert pl["k_per_split"] % 128 == 0, pl
        if plan == "64,64,2,5":
            assert (pl["splits"], pl["k_per_split"]) == (4, 256), pl
        else:
            assert pl["splits"] == (splits if bn == 64 else 1), pl
        (o1, o2), ref = run_dense(ops, ws, M, N, K, "plain", runs=2)
    finally:
        os.environ.pop("SPI_GEMM_PLAN", None)
        ops.lib.spi_debug_gemm_reload_env()
    e = normalized_max_error(o1, ref)
    print(f"gemm_hilo {M}x{N}x{K} plan {plan} -> {pl}: {e:.3e}")
    assert e < TOL32, f"gemm_hilo {M}x{N}x{K} plan {plan}: {e:.3e}"
    assert np.array_equal(o1, o2), "two launches on one workspace differ"


def test_gemm_hilo_identity_exact(ops, ws):
    """A = I (three A steps), W = hi + lo with hi small integers and lo integer multiples of 2^-13 below
    half an ulp of hi, a different pattern in every 64-k block of either half: fp16(w) = hi exactly, every
    product and sum is exact, and the fp32 output must be W^T to the bit.  A lo block applied to the wrong A
    step, or dropped, changes it."""
    n = 192
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    # 2 <= |hi| <= 8: fp16 spacing >= 2^-10 on either side of hi, so |lo| <= 3 * 2^-13 < 2^-11 rounds away
    hi = (((i * 5 + j * 3) % 7 + 2) * (1 - 2 * ((i + j) % 2))).astype(np.float32)
    lo = (((i * 7 + j * 11 + (j // 64) * 5) % 7 - 3) * 2.0 ** -13).astype(np.float32)
    W = hi + lo
    assert np.array_equal(W.astype(np.float16).astype(np.float32), hi) and np.array_equal(R.hilo_values(W), W)
    out = guarded(n, n)
    ops.gemm_hilo(torch.eye(n, device="cuda", dtype=torch.float16), ops.pack_weight_hilo(W), n, out=out[:n], ws=ws)
    assert_guard(out, n, "identity")
    np.testing.assert_array_equal(out[:n].cpu().numpy(), W.T)


def conv_ref(case, res):
    B, H, cin, cout, k, stride, pad = case
    x, [(w, b)] = R.conv_case(B, H, cin, [(cout, k, stride, pad)])
    x16 = x.astype(np.float16)
    acc = R.conv_acc(x16, R.hilo_values(w), stride, pad)
    r = np.random.default_rng(H + cout).standard_normal(acc.shape).astype(np.float32) if res else None
    return x16, w, b, r, R.epilogue64(acc, b, r)


def run_conv(ops, ws, case, res, out_dtype):
    B, H, cin, cout, k, stride, pad = case
    x16, w, b, r, ref = conv_ref(case, res)
    M = ref.shape[0] * ref.shape[1] * ref.shape[2]
    out = guarded(M, cout, dtype=out_dtype)
    ops.conv2d_hilo(torch.from_numpy(x16).cuda(), ops.pack_weight_hilo(w.reshape(cout, -1)), cout, k, k, stride, pad,
                    bias=torch.from_numpy(b).cuda(), residual=None if r is None else torch.from_numpy(r).cuda(),
                    out=out[:M], ws=ws)
    assert_guard(out, M, f"conv {case}")
    return normalized_max_error(out[:M].float().cpu().numpy().reshape(ref.shape), ref)


@pytest.mark.parametrize("case", R.KREP_CONV, ids=["x".join(map(str, c)) for c in R.KREP_CONV])
def test_conv2d_hilo(ops, ws, case):
    """The tap walk under krep = 2 (the channel block / tap advance after the odd step only): the model's
    1x1/s2 downsample form at one and two channel blocks, and a 3x3/s2/p1 conv over an odd map -- nine taps
    of two steps each, padding taps included."""
    e = run_conv(ops, ws, case, False, torch.float32)
    print(f"conv2d_hilo {case}: {e:.3e}")
    assert e < TOL32, f"conv2d_hilo {case}: {e:.3e}"


def test_conv2d_hilo_fp32_residual_fp16_out(ops, ws):
    e = run_conv(ops, ws, R.KREP_CONV_RES, True, torch.float16)
    print(f"conv2d_hilo {R.KREP_CONV_RES} fp32 residual, fp16 out: {e:.3e}")
    assert e < TOL16


def test_conv2d_hilo_rejects_cin_32(ops, ws):
    x = torch.zeros(1, 8, 8, 32, device="cuda", dtype=torch.float16)
    wp = ops.pack_weight_hilo(np.zeros((64, 32), np.float32))
    with pytest.raises(ops.OpError):
        ops.conv2d_hilo(x, wp, 64, 1, 1, 2, 0, ws=ws)

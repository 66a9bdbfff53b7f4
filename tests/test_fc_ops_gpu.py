"""Op-level parity of the fused avgpool + FC (GemmDesc::pool_rows, the pooled epilogue of csrc/gemm.hip) through
spi_op_avgpool_fc, and of the dense GEMM at fp32 / fp16x3 / split fp16x3 through spi_op_gemm (fp16 dense is
test_ln_fold_ops_gpu.py's and test_hilo_weight_ops_gpu.py's).

The reference is float64 on the values the kernel multiplies (op_refs.operand_values), so the bar is the
project's operand-exact 1e-5 normalised max error for every output here -- the pooled FC at fp16 included: its
operands are exact and its output fp32.  Every output has GUARD NaN rows behind it (and NaN in the slack of a
strided C) that must survive; every case runs twice on the module's one workspace, never re-zeroed, to the same
bits; plans are asserted through spi_debug_gemm_plan / spi_debug_gemm_args before a launch.

avgpool + FC.  x carries NaN rows behind row B HW, so a row past the last image's limit that reached a sum would
show; HW = 1, 2, 3, 5 leave some of the four row parts empty, 63 / 64 fill the tile, B = 65 has more images than
a tile has rows, C = 2048 takes the 3-stage ring (asserted).  test_op_refs.test_fc_cases_discriminate shows on
these inputs that the next image's rows, a division by 64 and a dropped row part sit above 1e-4.
The forced-plan question: every dense instance SPI_GEMM_PLAN can force (128 x 128 x 2, 128 x 64 x 2 / 3,
64 x 64 x 2 / 3 / 4) compiles the pooled epilogue -- its 256 partial sums fit behind the fp32 C tile in each
(gemm_tile.hpp holds that with a static_assert) -- so the planner keeps taking a forced tile for pooled problems,
test_avgpool_fc_forced_plans covers those tiles, a forced split-K among them, and tests/test_gemm_plan.py pins
the plans and the workspace check a forced split needs.

Dense.  Ragged M and N, K tails of half a 32-step (176, 40; the packed K pads to 64), lda > K with NaN in A's
slack, ldc > N, ldr > N, an in-place residual, C one element off 16 bytes (the scalar epilogue), the default
plan's split-K (4 to 6 slices), the six forced plans -- a 5-way split of 14 steps among them -- and a 5 x 5 grid
of tiles whose rows do not divide into the XCD rectangles.

Worst normalised max errors measured on an MI355X (bar 1e-5; each case prints its own):
  avgpool + FC   fp32 2.6e-7, fp16 1.5e-7, fp16x3 4.3e-7, fp16x3s 4.4e-7; under the forced plans 2.4e-7
  dense          fp32 4.7e-7, fp16x3 6.7e-7, fp16x3s 6.5e-7 (197 x 128 x 1024, gelu, 5 slices)
  forced plans   7.1e-7 (64 x 64 x 1152 at "64,64,3,3"); scalar epilogue / in-place residual 4.7e-7; XCD grid 2.6e-7
"""
import ctypes as C
import importlib
import os

import numpy as np
import pytest
import torch

import op_refs as R
from oracle.cpu_codelet import normalized_max_error

pytestmark = pytest.mark.gpu

TOL = 1e-5
GUARD = 8
NAN = float("nan")
FC_PRECS = ("fp32", "fp16", "fp16x3", "fp16x3s")
OUT_F32 = 32  # flag word of spi_debug_gemm_plan


@pytest.fixture(scope="module")
def ops(spi, gpu):
    return importlib.import_module("starpu-inference-server_amd.ops")


@pytest.fixture(scope="module")
def ws(ops):
    return ops.workspace()


class forced_plan:
    """with forced_plan(ops, "bm,bn,stages,splits"): SPI_GEMM_PLAN set and re-read; put back on the way out."""

    def __init__(self, ops, plan):
        self.ops, self.plan = ops, plan

    def __enter__(self):
        self.saved = os.environ.pop("SPI_GEMM_PLAN", None)
        if self.plan:
            os.environ["SPI_GEMM_PLAN"] = self.plan
        self.ops.lib.spi_debug_gemm_reload_env()

    def __exit__(self, *exc):
        os.environ.pop("SPI_GEMM_PLAN", None)
        if self.saved is not None:
            os.environ["SPI_GEMM_PLAN"] = self.saved
        self.ops.lib.spi_debug_gemm_reload_env()


def query_plan(ops, prec, M, N, K, lda, pool_rows=0, flags=OUT_F32):
    out = (C.c_longlong * 14)()
    assert ops.lib.spi_debug_gemm_plan(R.PREC_ID[prec], M, N, K, lda, 1, pool_rows, C.c_uint(flags), out) == 0
    assert int(out[0]) == 0 or prec == "fp16" and not pool_rows, "the general kernel"
    return dict(zip(R.PLAN_FIELDS, [int(v) for v in out[4:12]]))


def nan_buffer(rows, cols, split=False):
    """[rows][cols] of NaN: float32, or for the split layout float32 storage whose fp16 halves are all NaN."""
    if split:
        return torch.full((rows, 2 * cols), NAN, dtype=torch.float16, device="cuda").view(torch.float32)
    return torch.full((rows, cols), NAN, dtype=torch.float32, device="cuda")


def all_nan(t, split):
    t = t.contiguous()
    return bool(torch.isnan(t.view(torch.float16) if split else t).all())


# ---- avgpool + FC -------------------------------------------------------------------------------

_fc_cache = {}


def fc_inputs(ops, prec, B, HW, Cc, N, exact=False):
    """x on the device with GUARD NaN rows behind row B HW, the packed weight, bias, and the operand values."""
    key = (prec, B, HW, Cc, N, exact)
    if key not in _fc_cache:
        x, W, b = (R.fc_exact_case if exact else R.fc_case)(B, HW, Cc, N)
        M = B * HW
        if prec == "fp16":
            buf = torch.full((M + GUARD, Cc), NAN, dtype=torch.float16, device="cuda")
            buf[:M] = torch.from_numpy(x.reshape(M, Cc)).cuda().half()
        else:
            buf = nan_buffer(M + GUARD, Cc, split=prec == "fp16x3s")
            t = torch.from_numpy(x.reshape(M, Cc))
            buf[:M] = (ops.to_split(t) if prec == "fp16x3s" else t).cuda()
        xv, wv = R.operand_values(prec, x, W)
        _fc_cache[key] = dict(x=buf[:M].view(B, HW, Cc), keep=buf, b=b, b_d=torch.from_numpy(b).cuda(), xv=xv, wv=wv,
                              Wp=ops.pack_weight("fp16x3" if prec == "fp16x3s" else prec, W))
    return _fc_cache[key]


def run_fc(ops, ws, prec, B, HW, Cc, N, has_bias, act, exact=False):
    """Two launches on one workspace; returns (the output, the float64 reference)."""
    c = fc_inputs(ops, prec, B, HW, Cc, N, exact)
    outs = []
    for _ in range(2):
        y = nan_buffer(B + GUARD, N)
        ops.avgpool_fc(prec, c["x"], c["Wp"], N, bias=c["b_d"] if has_bias else None, act=act, ws=ws, out=y[:B])
        torch.cuda.synchronize()
        assert all_nan(y[B:], False), f"avgpool_fc {prec} {(B, HW, Cc, N)}: rows past B were written"
        outs.append(y[:B].cpu().numpy())
    assert np.array_equal(outs[0].view(np.int32), outs[1].view(np.int32)), "two launches on one workspace differ"
    return outs[0], R.fc_ref(c["xv"], c["wv"], c["b"] if has_bias else None, act)


def fc_stages(prec, Cc):
    ksteps = -(-Cc // 64) * (1 if prec == "fp16" else 2)
    return 3 if ksteps >= 12 else 2


@pytest.mark.parametrize("prec", FC_PRECS)
@pytest.mark.parametrize("case", R.FC_CASES, ids=["x".join(map(str, c[:4])) for c in R.FC_CASES])
def test_avgpool_fc(ops, ws, case, prec):
    B, HW, Cc, N, has_bias, act = case
    pl = query_plan(ops, prec, B * HW, N, Cc, Cc, pool_rows=HW)
    assert (pl["bm"], pl["bn"], pl["splits"], pl["stages"]) == (64, 64, 1, fc_stages(prec, Cc)), pl
    if Cc == 2048:
        assert pl["stages"] == 3
    got, ref = run_fc(ops, ws, prec, *case)
    e = normalized_max_error(got, ref)
    print(f"avgpool_fc {prec} {case} stages={pl['stages']}: {e:.3e}")
    assert e < R.FC_BAR, f"avgpool_fc {prec} {case}: {e:.3e}"


@pytest.mark.parametrize("prec", FC_PRECS)
@pytest.mark.parametrize("B,HW,Cc,N", R.FC_EXACT)
def test_avgpool_fc_exact(ops, ws, prec, B, HW, Cc, N):
    """Integers, HW a power of two: sums, the division and the bias add are exact -- bit for bit."""
    got, ref = run_fc(ops, ws, prec, B, HW, Cc, N, True, None, exact=True)
    np.testing.assert_array_equal(got, ref.astype(np.float32))


@pytest.mark.parametrize("plan", R.FC_FORCED)
def test_avgpool_fc_forced_plans(ops, ws, plan):
    """Every tile SPI_GEMM_PLAN can force holds the pooled epilogue (module docstring): each writes [B][N]."""
    B, HW, Cc, N, has_bias, act = R.FC_FORCED_CASE
    bm, bn, stages, splits = (int(v) for v in plan.split(","))
    with forced_plan(ops, plan):
        for prec in FC_PRECS:
            ksteps = -(-Cc // 64) * (1 if prec == "fp16" else 2)
            want_splits, kt = R.forced_splits(ksteps, splits if bn == 64 else 1)
            pl = query_plan(ops, prec, B * HW, N, Cc, Cc, pool_rows=HW)
            assert (pl["bm"], pl["bn"], pl["stages"], pl["splits"]) == (bm, bn, stages, want_splits), pl
            got, ref = run_fc(ops, ws, prec, B, HW, Cc, N, has_bias, act)
            e = normalized_max_error(got, ref)
            print(f"avgpool_fc {prec} plan {plan} -> {pl}: {e:.3e}")
            assert e < R.FC_BAR, f"avgpool_fc {prec} plan {plan}: {e:.3e}"


def test_avgpool_fc_refusals(ops, ws):
    """HW = 65, HW = 0 and a split C of 48: refused before any launch (the output keeps its NaNs)."""
    y = nan_buffer(3 + GUARD, 70)
    wp = ops.pack_weight("fp32", np.zeros((70, 96), np.float32))
    for hw in (65, 0):
        with pytest.raises(ops.OpError, match="invalid avgpool_fc arguments"):
            ops.avgpool_fc("fp32", torch.zeros(3, max(hw, 1), 96, device="cuda")[:, :hw], wp, 70, ws=ws, out=y[:3])
    wp48 = ops.pack_weight("fp16x3", np.zeros((70, 48), np.float32))
    with pytest.raises(ops.OpError, match="multiple of 32"):
        ops.avgpool_fc("fp16x3s", torch.zeros(3, 4, 48, device="cuda"), wp48, 70, ws=ws, out=y[:3])
    torch.cuda.synchronize()
    assert all_nan(y, False)


# ---- dense GEMM at fp32 / fp16x3 / fp16x3s ------------------------------------------------------

_dense_cache = {}


def dense_inputs(ops, prec, M, N, K):
    """One (precision, shape)'s device operands -- A in a buffer of lda = K + 8 (split: + 32) columns whose slack
    is NaN, the residual at ldr = N + 16 (+ 64) -- and the float64 accumulator and residual values."""
    key = (prec, M, N, K)
    if key not in _dense_cache:
        split = prec == "fp16x3s"
        A, W, b, Rr = R.dense32_case(M, N, K)
        a_buf = nan_buffer(M, K + (32 if split else 8), split)
        r_buf = nan_buffer(M, N + (64 if split else 16), split)
        tA, tR = torch.from_numpy(A), torch.from_numpy(Rr)
        a_buf[:, :K] = (ops.to_split(tA) if split else tA).cuda()
        r_buf[:, :N] = (ops.to_split(tR) if split else tR).cuda()
        av, wv = R.operand_values(prec, A, W)
        _dense_cache[key] = dict(A=a_buf[:, :K], R=r_buf[:, :N], b=b, b_d=torch.from_numpy(b).cuda(),
                                 Wp=ops.pack_weight("fp16x3" if split else prec, W), acc=R.dense_acc64(av, wv),
                                 rv=R.operand_values(prec, Rr))
    return _dense_cache[key]


def run_dense(ops, ws, prec, M, N, K, form, c_kind="strided"):
    """Two launches on one workspace into NaN buffers.  c_kind "strided": ldc = N + 8 (split: + 32), the slack
    checked unwritten; "unaligned": C one float past a 16-byte boundary; "inplace": C holds the residual.
    Returns (the output's values, the float64 reference)."""
    split = prec == "fp16x3s"
    c = dense_inputs(ops, prec, M, N, K)
    res = form == "res" or c_kind == "inplace"
    act = {"relu": "relu", "gelu": "gelu"}.get(form)
    outs = []
    for _ in range(2):
        if c_kind == "unaligned":
            flat = nan_buffer(1, 1 + (M + GUARD) * N, split).view(-1)
            buf = flat[1:].view(M + GUARD, N)
            assert buf.data_ptr() % 16 == 4
        else:
            buf = nan_buffer(M + GUARD, N + (32 if split else 8), split)
        out = buf[:M, :N]
        residual = c["R"] if res else None
        if c_kind == "inplace":
            out.copy_(c["R"])
            residual = out
        ops.gemm(prec, c["A"], c["Wp"], N, bias=c["b_d"], residual=residual, out=out, act=act, ws=ws)
        torch.cuda.synchronize()
        what = f"gemm {prec} {M}x{N}x{K} {form} {c_kind}"
        assert all_nan(buf[M:], split), f"{what}: rows past M were written"
        assert buf.shape[1] == N or all_nan(buf[:M, N:], split), f"{what}: C's slack columns were written"
        o = out.contiguous().cpu()
        outs.append((ops.from_split(o) if split else o).numpy())
    assert np.array_equal(outs[0].view(np.int32), outs[1].view(np.int32)), "two launches on one workspace differ"
    return outs[0], R.epilogue64(c["acc"], c["b"], c["rv"] if res else None, act)


@pytest.mark.parametrize("form", R.DENSE32_FORMS)
@pytest.mark.parametrize("shape", R.DENSE32_SHAPES, ids=["x".join(map(str, s)) for s in R.DENSE32_SHAPES])
@pytest.mark.parametrize("prec", R.DENSE32_PRECS)
def test_gemm32(ops, ws, prec, shape, form):
    """Strided A, C and residual with guards; the last three shapes split K 4 to 6 ways by the default plan."""
    M, N, K = R.dense32_shape(prec, *shape)
    pl = query_plan(ops, prec, M, N, K, K + (32 if prec == "fp16x3s" else 8))
    if shape[2] >= 768:
        assert 4 <= pl["splits"] <= 6 and pl["k_per_split"] % 32 == 0, pl
    else:
        assert pl["splits"] == 1, pl
    got, ref = run_dense(ops, ws, prec, M, N, K, form)
    e = normalized_max_error(got, ref)
    print(f"gemm {prec} {M}x{N}x{K} {form} splits={pl['splits']}: {e:.3e}")
    assert e < TOL, f"gemm {prec} {M}x{N}x{K} {form}: {e:.3e}"


@pytest.mark.parametrize("c_kind", ["unaligned", "inplace"])
@pytest.mark.parametrize("prec", R.DENSE32_PRECS)
def test_gemm32_scalar_epilogue_and_inplace_residual(ops, ws, prec, c_kind):
    """C one element off 16 bytes (vec_ok false: the per-element epilogue on every tile), one shape unsplit and
    one under split-K; the residual read from the buffer C overwrites."""
    for shape in ((100, 96, 176), (8, 128, 768)):
        M, N, K = R.dense32_shape(prec, *shape)
        got, ref = run_dense(ops, ws, prec, M, N, K, "res", c_kind)
        e = normalized_max_error(got, ref)
        print(f"gemm {prec} {M}x{N}x{K} res {c_kind}: {e:.3e}")
        assert e < TOL, f"gemm {prec} {M}x{N}x{K} {c_kind}: {e:.3e}"


@pytest.mark.parametrize("plan,shape", R.DENSE32_FORCED, ids=[p for p, _ in R.DENSE32_FORCED])
@pytest.mark.parametrize("prec", R.DENSE32_PRECS)
def test_gemm32_forced_plans(ops, ws, prec, plan, shape):
    """The other tiles and ring depths; "64,64,2,5" on 14 steps: five slices of 3, 3, 3, 3, 2 steps."""
    M, N, K = R.dense32_shape(prec, *shape)
    bm, bn, stages, splits = (int(v) for v in plan.split(","))
    want_splits, kt = R.forced_splits(R.dense32_ksteps(K), splits if bn == 64 else 1)
    with forced_plan(ops, plan):
        pl = query_plan(ops, prec, M, N, K, K + (32 if prec == "fp16x3s" else 8))
        assert (pl["bm"], pl["bn"], pl["stages"], pl["splits"], pl["k_per_split"]) == \
            (bm, bn, stages, want_splits, 32 * kt), pl
        if plan == "64,64,2,5":
            assert (pl["splits"], pl["k_per_split"]) == (5, 96) and R.dense32_ksteps(K) % 5
        got, ref = run_dense(ops, ws, prec, M, N, K, "plain")
    e = normalized_max_error(got, ref)
    print(f"gemm {prec} {M}x{N}x{K} plan {plan} -> {pl}: {e:.3e}")
    assert e < TOL, f"gemm {prec} {M}x{N}x{K} plan {plan}: {e:.3e}"


@pytest.mark.parametrize("prec", R.DENSE32_PRECS)
def test_gemm32_uneven_xcd_rectangles(ops, ws, prec):
    """5 x 5 tiles of 64 x 64 in two XCD row groups: rg_m0 = 0, 2, 5 -- the rectangles differ in height.  Random
    operands make every tile's result its own, the output starts as NaN: a dropped tile cannot pass."""
    M, N, K = R.DENSE32_XCD
    lda = K + (32 if prec == "fp16x3s" else 8)
    with forced_plan(ops, "64,64,2,1"):
        info, digest = (C.c_int * 5)(), C.c_ulonglong()
        assert ops.lib.spi_debug_gemm_args(R.PREC_ID[prec], M, N, K, lda, 1, 0, C.c_uint(OUT_F32), 0, C.byref(digest),
                                           info, None, 0) == 0
        tm, tn, sp, xg_m, xg_n = (int(v) for v in info)
        assert tm * tn >= 16 and sp == 1 and xg_m > 1 and tm % xg_m != 0, list(info)
        got, ref = run_dense(ops, ws, prec, M, N, K, "plain")
    e = normalized_max_error(got, ref)
    print(f"gemm {prec} {M}x{N}x{K} xcd {xg_m}x{xg_n} over {tm}x{tn} tiles: {e:.3e}")
    assert e < TOL
    # per tile as well: a tile holding another tile's (finite, plausible) values would hide in a global maximum
    for i in range(tm):
        for j in range(tn):
            t = (slice(64 * i, min(M, 64 * i + 64)), slice(64 * j, min(N, 64 * j + 64)))
            assert normalized_max_error(got[t], ref[t]) < TOL, (i, j)

"""Op-level tests of the fused QKV projection + attention kernel (qkv_attn.hip) through
spi_op_qkv_attention, against op_refs.qkv_attention_ref (float64 on the same fp16 operands, q / k / v
rounded to fp16 where the kernel rounds): every tile boundary of the 128- and 256-row tiles, S = 1, odd
head counts, two heads, D = 1024 with the fold's 16 statistics chunks, strided A, both SPI_QKV_HP forms.

Every ctx buffer is NaN-filled with 8 NaN guard rows behind it: after a call the guard rows are still
NaN and all B S rows are finite.
"""
import functools
import importlib
import os

import numpy as np
import pytest
import torch

import op_refs as R

pytestmark = pytest.mark.gpu

GUARD = 8
NAN = float("nan")
# Normalised max error of ctx against qkv_attention_ref.  From the CPU emulation of the kernel's arithmetic
# (test_op_refs.test_qkv_emulation_within_bar: 2.5e-4 .. 5.2e-4 over these cases): 3x its worst case, half
# of test_attention's fp16 bar.  The slack is for the MFMA's summation order, the online softmax and
# __expf; a dropped k-step, a wrong bias column or a wrong row statistic exceeds it tenfold.
TOL_QKV = 1.5e-3
# Near-exact cases: every probability is exactly 1 or 0 and every value is a small integer, so ctx is the
# fp16 rounding of an exact quotient: one fp16 ulp at 1, 2^-10 (relative for the all-masked mean).  One
# tail row of the tile entering the softmax gives S / (S + 1), off by at least 1 / 257 = 3.9e-3.
TOL_EXACT = 2.0 ** -10


@pytest.fixture(scope="module")
def ops(spi, gpu):
    return importlib.import_module("starpu-inference-server_amd.ops")


@pytest.fixture(scope="module")
def ws(ops):
    return ops.workspace()


@functools.lru_cache(maxsize=None)
def case(B, S, heads, fold, masked):
    """One parity case and its float64 reference, computed once and left unchanged."""
    ops = importlib.import_module("starpu-inference-server_amd.ops")
    c = R.qkv_case(ops, B, S, heads, fold, masked)
    c["ref"] = R.qkv_attention_ref(c["A16"], c["W16"], c["bias"], c["mask"], B, S, heads, 0.125, stats=c["stats"],
                                   c1=c["c1"], eps=R.EPS)
    return c


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def guarded_ctx(M, D):
    return torch.full((M + GUARD, D), NAN, dtype=torch.float16, device="cuda")


def run_fused(ops, c, W=None, bias=None, A=None, lda=None, mask=None, scale=0.125, what="ctx"):
    """One launch on fresh device buffers; checks the guard rows and that every row was written.
    Returns ctx [B S][D] fp16 on the host."""
    B, S, heads = c["B"], c["S"], c["heads"]
    M, D = B * S, heads * 64
    Wp = ops.pack_weight("fp16", c["W"] if W is None else W)
    ctx = guarded_ctx(M, D)
    ops.qkv_attention(dev(c["A16"]) if A is None else A, Wp, heads, dev(c["bias"] if bias is None else bias), ctx, B, S,
                      lda=lda, in_stats=dev(c["stats"]), c1=dev(c["c1"]), eps=R.EPS,
                      mask_bias=dev(c["mask"] if mask is None else mask), scale=scale)
    torch.cuda.synchronize()
    assert bool(torch.isnan(ctx[M:]).all()), f"{what}: rows past B S were written"
    out = ctx[:M].cpu()
    assert bool(torch.isfinite(out).all()), f"{what}: rows left unwritten or not finite"
    return out


def run_unfused(ops, ws, c):
    """The unfused pair on the same inputs: the QKV GEMM into fp16, then the attention kernel."""
    B, S, heads = c["B"], c["S"], c["heads"]
    D = heads * 64
    A, Wp, bias = dev(c["A16"]), ops.pack_weight("fp16", c["W"]), dev(c["bias"])
    if c["stats"] is None:
        qkv = ops.gemm("fp16", A, Wp, 3 * D, bias=bias, out_f32=False, ws=ws)
    else:
        qkv = torch.empty(B * S, 3 * D, dtype=torch.float16, device="cuda")
        ops.gemm_ln(A, Wp, 3 * D, qkv, "fp16", bias=bias, in_stats=dev(c["stats"]), c1=dev(c["c1"]), eps=R.EPS, ws=ws)
    out = ops.attention("fp16", qkv, B, S, heads, mask_bias=dev(c["mask"]))
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("B,S,heads,fold,masked", R.QKV_CASES)
def test_parity(ops, ws, B, S, heads, fold, masked):
    c = case(B, S, heads, fold, masked)
    what = f"qkv_attention B{B} S{S} H{heads} fold{int(fold)} mask{int(masked)}"
    got = run_fused(ops, c, what=what).numpy()
    e = R.nerr(got, c["ref"])
    print(f"{what}: fused {e:.3e}")
    try:  # reported, not asserted (the folded GEMM needs 3 D % 128 == 0: no pair for an odd head count)
        pair = run_unfused(ops, ws, c).numpy()
        d = float(np.abs(got.astype(np.float64) - pair).max() / np.abs(c["ref"]).max())
        print(f"{what}: unfused pair {R.nerr(pair, c['ref']):.3e}, fused - unfused {d:.3e}")
    except ops.OpError as err:
        print(f"{what}: unfused pair not available ({err})")
    assert e < TOL_QKV, f"{what}: {e:.3e}"


def exact_inputs(S, all_masked):
    """B = 2, heads = 2.  W and bias: query rows zero (every score is 0), key rows random, value rows zero
    but for column 0, which is 1 (V[t, :] = A[t, 0]).  A: N(0, 1) with column 0 set per variant."""
    B, heads, D = 2, 2, 128
    rng = np.random.default_rng(S)
    W = (rng.standard_normal((3 * D, D)) * 1.5 / np.sqrt(D)).astype(np.float32)
    bias = (rng.standard_normal(3 * D) * 0.5).astype(np.float32)
    W[:D] = 0
    bias[:D] = 0
    W[2 * D:] = 0
    W[2 * D:, 0] = 1
    bias[2 * D:] = 0
    A = rng.standard_normal((B, S, D)).astype(np.float16)
    A[:, :, 0] = 1
    mask = np.zeros((B, S), np.float32)
    want = np.ones((B, S), np.float64)
    if all_masked:  # sequence 1: every key masked -> the mean of its values, drawn from {1, -7}
        A[1, :, 0] = np.where(rng.random(S) < 0.4, -7, 1)
        if A[1, :, 0].astype(np.float64).sum() == 0:  # the bar is relative: keep the mean off zero
            A[1, 0, 0] = -7 if A[1, 0, 0] == 1 else 1
        mask[1, :] = R.FMIN
        want[1, :] = A[1, :, 0].astype(np.float64).mean()
    else:  # sequence 1: keys 0 .. min(69, S - 2) masked (whole first tiles) and holding -7
        n = min(69, S - 2) + 1
        A[1, :n, 0] = -7
        mask[1, :n] = R.FMIN
    c = {"B": B, "S": S, "heads": heads, "A16": A.reshape(B * S, D), "W": W, "bias": bias, "stats": None, "c1": None,
         "mask": mask}
    return c, want


@pytest.mark.parametrize("all_masked", [False, True], ids=["first_keys_masked", "all_keys_masked"])
@pytest.mark.parametrize("S", [1, 15, 16, 17, 63, 65, 127, 128, 129, 255, 256])
def test_key_range_and_mask_near_exact(ops, S, all_masked):
    c, want = exact_inputs(S, all_masked)
    got = run_fused(ops, c, what=f"exact S{S}").double().numpy().reshape(2, S, 128)
    rel = np.abs(got - want[:, :, None]) / np.abs(want[:, :, None])
    print(f"exact S{S} all_masked{int(all_masked)}: want {want[:, 0]}, worst relative {rel.max():.3e}")
    assert rel[0].max() <= TOL_EXACT, f"S{S}: unmasked sequence off by {rel[0].max():.3e}"
    assert rel[1].max() <= TOL_EXACT, f"S{S}: masked sequence off by {rel[1].max():.3e}"


@pytest.mark.parametrize("fold", [False, True], ids=["plain", "fold"])
@pytest.mark.parametrize("B,S,heads", [(2, 128, 2), (3, 80, 4), (2, 17, 3), (1, 33, 16)])
def test_two_heads_per_workgroup_bit_identical(ops, B, S, heads, fold):
    """SPI_QKV_HP=2: two heads per 16-wave workgroup; an odd head count takes the one-head kernel."""
    c = case(B, S, heads, fold, True)
    one = run_fused(ops, c, what="HP=1")
    try:
        os.environ["SPI_QKV_HP"] = "2"
        ops.lib.spi_debug_gemm_reload_env()
        two = run_fused(ops, c, what="HP=2")
    finally:
        os.environ.pop("SPI_QKV_HP", None)
        ops.lib.spi_debug_gemm_reload_env()
    assert R.nerr(two.numpy(), c["ref"]) < TOL_QKV
    assert torch.equal(one.view(torch.int16), two.view(torch.int16))


@pytest.mark.parametrize("fold", [False, True], ids=["plain", "fold"])
@pytest.mark.parametrize("B,S,heads", [(2, 80, 4), (1, 197, 2)])
def test_strided_rows(ops, B, S, heads, fold):
    """lda = D + 8: A is a column slice of a wider NaN-filled buffer."""
    c = case(B, S, heads, fold, True)
    D = heads * 64
    wide = torch.full((B * S, D + 8), NAN, dtype=torch.float16, device="cuda")
    wide[:, :D] = dev(c["A16"])
    got = run_fused(ops, c, A=wide, lda=D + 8, what="strided A").numpy()
    e = R.nerr(got, c["ref"])
    print(f"strided B{B} S{S} H{heads} fold{int(fold)}: {e:.3e}")
    assert e < TOL_QKV


def test_scale(ops):
    B, S, heads = 2, 64, 2
    c = case(B, S, heads, False, True)
    ref = R.qkv_attention_ref(c["A16"], c["W16"], c["bias"], c["mask"], B, S, heads, 0.2)
    e = R.nerr(run_fused(ops, c, scale=0.2).numpy(), ref)
    print(f"scale 0.2: {e:.3e}")
    assert e < TOL_QKV
    assert R.nerr(c["ref"], ref) > 10 * TOL_QKV  # the scale matters at this bar


@pytest.mark.parametrize("B,S,heads,fold", [(2, 127, 2, True), (2, 197, 3, False)])
def test_two_calls_bit_identical(ops, B, S, heads, fold):
    c = case(B, S, heads, fold, True)
    a, b = run_fused(ops, c), run_fused(ops, c)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


def reject_case(ops, heads, S, B=2):
    """Zero-filled buffers sized for the nominal shape, so a wrongly accepted call stays in bounds."""
    D, M = heads * 64, B * S
    z = functools.partial(torch.zeros, device="cuda")
    return dict(A=z(M, D, dtype=torch.float16), W=ops.pack_weight("fp16", np.zeros((3 * D, D), np.float32)), bias=z(3 * D),
                stats=z(M, D // 64, 2), c1=z(3 * D), ctx=z(M + GUARD, D, dtype=torch.float16))


def test_rejections(ops):
    def call(t, heads, S, B=2, **kw):
        args = dict(A=t["A"], W_packed=t["W"], heads=heads, bias=t["bias"], ctx=t["ctx"], B=B, S=S)
        args.update(kw)
        with pytest.raises(ops.OpError):
            ops.qkv_attention(**args)

    call(reject_case(ops, 2, 257), 2, 257)                                   # S past the 256-row tile
    call(reject_case(ops, 1, 16), 1, 16)                                     # one head: K = 64
    t = reject_case(ops, 2, 16)
    wide = torch.zeros(2 * 16, 128 + 4, dtype=torch.float16, device="cuda")
    call(t, 2, 16, A=wide, lda=128 + 4)                                 # lda % 8 != 0
    flat = torch.zeros(2 * 16 * 128 + 8, dtype=torch.float16, device="cuda")
    off = flat[4:4 + 2 * 16 * 128].view(2 * 16, 128)
    assert off.data_ptr() % 16 == 8
    call(t, 2, 16, A=off)                                               # A off 16-byte alignment
    call(t, 2, 16, bias=None)                                           # the kernel reads the bias unconditionally
    call(t, 2, 16, in_stats=t["stats"])                                 # in_stats without c1
    call(t, 2, 16, c1=t["c1"])                                          # c1 without in_stats
    t17 = reject_case(ops, 17, 16)
    call(t17, 17, 16, in_stats=t17["stats"], c1=t17["c1"])              # the fold holds 16 statistics chunks
    ops.qkv_attention(t17["A"], t17["W"], 17, t17["bias"], t17["ctx"], 2, 16)  # ... and is what rejects it
    ops.qkv_attention(t["A"], t["W"], 2, t["bias"], t["ctx"], 2, 16, in_stats=t["stats"], c1=t["c1"])
    torch.cuda.synchronize()

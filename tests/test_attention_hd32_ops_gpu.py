"""Op-level tests of the standalone attention kernels (attention.hip) at head_dim 32 through spi_op_attention_hd,
laid out like test_attention_ops_gpu.py: op_refs.ATTN_CASES with the head count doubled at the same D, scale
1 / sqrt(32), against hd_refs.attention_ref (float64 on the operand rounded to the kernel's input type).  fp16:
attn_f16_swapped_kernel<4, 0, 32> up to 128 keys, <16, 224, 32> / <8, 224, 32> (SPI_ATTN_WHOLE = 2 / 1) for
129..224, <8, 0, 32> on 64-key tiles from 225 on and for 129..224 under SPI_ATTN_WHOLE = 0 -- the instance whose
64-key tile has half as many 16-byte chunks (256) as the workgroup has threads; fp32: attn_kernel<float, 32>.

Every ctx buffer is NaN-filled with 8 NaN guard rows behind it: after a call the guard rows are still NaN and
all B S rows are finite.

Bars (normalised max error of ctx against attention_ref):
  fp32  1e-5, the project's bar for exact fp32 MFMA.
  fp16  3x the worst case of the CPU emulation of the kernels' arithmetic over the parity list at width 32:
        measured 4.49e-4 (test_head_dim.test_attention_emulation_sets_the_fp16_bar), hd_refs.ATTN_EMU_WORST =
        4.5e-4, so the bar is 1.35e-3, below the fused kernel's TOL_QKV = 1.5e-3.
Near-exact cases (hd_refs.attn_exact_case: four 32-wide heads, the value column negated on odd heads so that a
neighbouring sub-head's column shows): relative 2^-10 for fp16, 1e-6 for fp32.

Measured on an MI355X (each test prints its figure), worst over the mask kinds and kernel instances:
  parity (B, S, heads)    fp16      fp32      |  parity (B, S, heads)    fp16      fp32
  (1, 1, 4)               0         0         |  (1, 224, 4)             3.45e-4   9.21e-7
  (2, 17, 6)              2.99e-4   3.52e-7   |  (1, 225, 4)             2.64e-4   8.89e-7
  (2, 127, 4)             3.99e-4   6.26e-7   |  (1, 257, 4)             4.49e-4   7.84e-7
  (2, 128, 4)             3.78e-4   9.65e-7   |  (2, 384, 4)             3.94e-4   1.44e-6
  (1, 129, 4)             3.87e-4   7.68e-7   |  (1, 512, 6)             3.78e-4   1.28e-6
  (2, 197, 6)             3.38e-4   7.84e-7   |  (1, 577, 4)             2.76e-4   1.40e-6
The fp16 kernels land on the emulation's figures (worst 4.49e-4 against the 1.35e-3 bar), fp32 at 1.4e-6 against
1e-5.  Near-exact: fp32 at most 9.8e-8 relative; fp16 at most 4.3e-4 (the fp16 rounding of the all-masked mean)
against 2^-10 = 9.8e-4.  Scale 0.25: fp16 3.6e-4, fp32 7.9e-7.
"""
import functools
import importlib
import os

import numpy as np
import pytest
import torch

import hd_refs as H
import op_refs as R
from test_qkv_attention_ops_gpu import TOL_QKV

pytestmark = pytest.mark.gpu

GUARD = 8
NAN = float("nan")
HD = H.HD
TOL = {"fp32": 1e-5, "fp16": 3 * H.ATTN_EMU_WORST}
TOL_EXACT = {"fp32": 1e-6, "fp16": 2.0 ** -10}
DT = {"fp32": torch.float32, "fp16": torch.float16}


def test_fp16_bar_is_three_times_the_emulation_and_within_the_fused_kernels():
    assert TOL["fp16"] == 3 * H.ATTN_EMU_WORST <= TOL_QKV


@pytest.fixture(scope="module")
def ops(spi, gpu):
    return importlib.import_module("starpu-inference-server_amd.ops")


def rounded(qkv, prec):
    """The operand as the kernel reads it: fp32 values, rounded through fp16 for the fp16 kernels."""
    return qkv.astype(np.float16).astype(np.float32) if prec == "fp16" else qkv


@functools.lru_cache(maxsize=None)
def case(B, S, heads, kind, prec, scale=H.SCALE):
    """One parity case and its float64 reference, computed once and left unchanged."""
    qkv, mask = rounded(H.attn_case(B, S, heads), prec), R.attn_mask(B, S, kind)
    return qkv, mask, H.attention_ref(qkv, mask, B, S, heads, scale)


def dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def run(ops, prec, qkv, mask, B, S, heads, scale=H.SCALE, what="ctx"):
    """One launch on fresh device buffers; checks the guard rows and that every row was written.
    Returns ctx [B S][D] on the host in the kernel's type."""
    M, D = B * S, heads * HD
    ctx = torch.full((M + GUARD, D), NAN, dtype=DT[prec], device="cuda")
    ret = ops.attention(prec, dev(qkv, DT[prec]), B, S, heads, mask_bias=dev(mask), scale=scale, out=ctx, head_dim=HD)
    torch.cuda.synchronize()
    assert ret is ctx
    assert bool(torch.isnan(ctx[M:]).all()), f"{what}: rows past B S were written"
    out = ctx[:M].cpu()
    assert bool(torch.isfinite(out).all()), f"{what}: rows left unwritten or not finite"
    return out


def run_instances(ops, prec, qkv, mask, B, S, heads, what):
    """The launches of one case: one, but for fp16 at 129 <= S <= 224 one each under SPI_ATTN_WHOLE = 2, 1 and
    0.  The three instances run the same arithmetic in the same order, so they must agree bit for bit."""
    if not (prec == "fp16" and 129 <= S <= 224):
        return [run(ops, prec, qkv, mask, B, S, heads, what=what)]
    outs = []
    try:
        for whole in ("2", "1", "0"):
            os.environ["SPI_ATTN_WHOLE"] = whole
            ops.lib.spi_debug_gemm_reload_env()
            outs.append(run(ops, prec, qkv, mask, B, S, heads, what=f"{what} SPI_ATTN_WHOLE={whole}"))
    finally:
        os.environ.pop("SPI_ATTN_WHOLE", None)
        ops.lib.spi_debug_gemm_reload_env()
    for o in outs[1:]:
        assert torch.equal(o.view(torch.int16), outs[0].view(torch.int16)), f"{what}: the instances differ"
    return outs


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("B,S,heads,kind", H.ATTN_CASES)
def test_parity(ops, B, S, heads, kind, prec):
    qkv, mask, ref = case(B, S, heads, kind, prec)
    what = f"attention hd32 {prec} B{B} S{S} H{heads} mask {kind}"
    for got in run_instances(ops, prec, qkv, mask, B, S, heads, what):
        e = R.nerr(got.numpy(), ref)
        print(f"{what}: {e:.3e}")
        assert e < TOL[prec], f"{what}: {e:.3e}"


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_differs_from_the_64_wide_reading(ops, prec):
    """The same operand served as half as many 64-wide heads is another function: the parity bars tell them apart."""
    qkv, mask, ref = case(2, 197, 6, "tail", prec)
    assert R.nerr(R.attention_ref(qkv, mask, 2, 197, 3, H.SCALE), ref) > 100 * TOL["fp16"]


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("S,variant", R.ATTN_EXACT_CASES)
def test_key_range_and_mask_near_exact(ops, S, variant, prec):
    qkv, mask, want = H.attn_exact_case(S, variant)
    what = f"exact hd32 {prec} S{S} {variant}"
    worst = 0.0
    for got in run_instances(ops, prec, qkv, mask, 2, S, 4, what):
        got = got.double().numpy().reshape(2, S, 4, HD)[..., 0]  # column 0 of each head
        rel = np.abs(got - want) / np.abs(want)
        worst = max(worst, rel.max())
        assert rel[0].max() <= TOL_EXACT[prec], f"{what}: sequence 0 off by {rel[0].max():.3e}"
        assert rel[1].max() <= TOL_EXACT[prec], f"{what}: sequence 1 off by {rel[1].max():.3e}"
    print(f"{what}: want {want[:, 0, 0]} on even heads, negated on odd ones, worst relative {worst:.3e}")


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_two_calls_bit_identical(ops, prec):
    qkv, mask, _ = case(1, 512, 6, "middle", prec)
    a, b = (run(ops, prec, qkv, mask, 1, 512, 6) for _ in range(2))
    assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("B,S,heads", [(2, 17, 6), (2, 384, 4)])
def test_scale(ops, B, S, heads, prec):
    qkv, mask, ref0 = case(B, S, heads, "tail", prec)
    ref = H.attention_ref(qkv, mask, B, S, heads, 0.25)
    e = R.nerr(run(ops, prec, qkv, mask, B, S, heads, scale=0.25).numpy(), ref)
    print(f"scale 0.25 hd32 {prec} B{B} S{S} H{heads}: {e:.3e}")
    assert e < TOL[prec]
    assert R.nerr(ref0, ref) > 10 * TOL["fp16"]  # the scale matters at these bars


# ---- argument checks: decided in spi_op_attention_hd's host code, before any launch ----------------


def reject(ops, prec_code, dtype, B, S, heads, head_dim=HD, nb=2, ns=16, nh=4, qkv_off=0, ctx_off=0):
    """A call that must be refused, on buffers sized for the (nb, ns, nh) shape or the nominal one at 64 columns a
    head, whichever is larger where the nominal one is positive; the NaN-filled ctx must come back untouched."""
    rows = max(nb * ns, B * S if min(B, S) > 0 else 0)
    h = max(nh, heads)
    es = torch.empty((), dtype=dtype).element_size()
    qkv = torch.zeros(rows * 3 * h * 64 + 16, dtype=dtype, device="cuda")[qkv_off // es:]
    ctx = torch.full((rows * h * 64 + 16,), NAN, dtype=dtype, device="cuda")
    assert qkv.data_ptr() % 16 == qkv_off % 16 and ctx.data_ptr() % 16 == 0
    with pytest.raises(ops.OpError):
        ops.attention(prec_code, qkv, B, S, heads, out=ctx[ctx_off // es:], head_dim=head_dim)
    torch.cuda.synchronize()
    assert bool(torch.isnan(ctx).all()), "a rejected call wrote ctx"


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_rejections(ops, dtype):
    code = 0 if dtype == torch.float32 else 1
    for hd in (0, 16, 63, 65, -32, 128):                        # a head_dim other than 32 or 64
        reject(ops, code, dtype, 2, 16, 4, head_dim=hd)
    for bad in (-1, 2, 3, 4):                                   # a precision other than 0 or 1
        reject(ops, bad, dtype, 2, 16, 4)
    for B, S, heads in [(0, 16, 4), (-1, 16, 4), (2, 0, 4), (2, -16, 4), (2, 16, 0), (2, 16, -2)]:
        reject(ops, code, dtype, B, S, heads)                   # non-positive B, S or heads
    reject(ops, code, dtype, 16384, 1, 4)                       # B heads = 65536: past the grid's y extent
    reject(ops, code, dtype, 21846, 1, 3)                       # 65538
    for off in (4, 8):                                          # qkv off 16-byte alignment
        reject(ops, code, dtype, 2, 16, 4, qkv_off=off)
    reject(ops, code, dtype, 2, 16, 4, ctx_off=4)               # ctx off 8-byte alignment


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_limits_are_served(ops, dtype):
    """The other side of test_rejections' limits: B heads = 65535 and a ctx at 8 bytes.  v = 0, so ctx = 0."""
    B, heads = 21845, 3
    qkv = torch.zeros(B * 3 * heads * HD, dtype=dtype, device="cuda")
    ctx = torch.full((B * heads * HD + 16,), NAN, dtype=dtype, device="cuda")
    off = 8 // qkv.element_size()
    ops.attention(int(dtype == torch.float16), qkv, B, 1, heads, out=ctx[off:], head_dim=HD)
    torch.cuda.synchronize()
    assert bool((ctx[off:off + B * heads * HD] == 0).all())
    assert bool(torch.isnan(ctx[:off]).all()) and bool(torch.isnan(ctx[off + B * heads * HD:]).all())

"""Op-level tests of the shifted-window attention kernel (window_attn.hip) through spi_op_window_attention, against
swin_refs.window_attention_ref (float64, torchvision's formulation) on the operand rounded to the kernel's input
type.  B = 2, heads = 3 (C = 96), bias table N(0, 1), scale 1 / sqrt(32).  ctx is NaN-filled with 8 NaN guard rows
behind it: after a call the guard rows are still NaN and every row is finite.

Cases (ws, H / ws, W / ws, shift): (7, 2, 2, 3) every mask class, padded keys, wave 3 with one live query;
(7, 3, 2, 3) a non-square map; (7, 1, 1, 0) the map is the window; (7, 2, 2, 0); (4, 2, 3, 2) N = 16, one key block,
three dead waves; (8, 2, 2, 4) N = 64, nothing padded.

Bars (normalised max error): fp32 1e-5, the project's bar for the exact fp32 MFMA; fp16 3 * hd_refs.ATTN_EMU_WORST =
1.35e-3, the project's bar for this arithmetic at width 32 over one key tile.

Measured on an MI355X (each test prints its figure):
  case            fp16      fp32      |  case            fp16      fp32
  (7, 2, 2, 3)    3.08e-4   2.9e-7    |  (7, 2, 2, 0)    3.38e-4   4.6e-7
  (7, 3, 2, 3)    3.28e-4   7.9e-7    |  (4, 2, 3, 2)    3.54e-4   2.9e-7
  (7, 1, 1, 0)    2.86e-4   4.3e-7    |  (8, 2, 2, 4)    3.42e-4   4.2e-7
"""
import functools
import importlib

import numpy as np
import pytest
import torch

import hd_refs as H
import op_refs as R
import swin_refs as S

pytestmark = pytest.mark.gpu

GUARD, B, HEADS, SCALE = 8, 2, 3, 32 ** -0.5
TOL = {"fp32": 1e-5, "fp16": 3 * H.ATTN_EMU_WORST}
DT = {"fp32": torch.float32, "fp16": torch.float16}
CASES = [(7, 2, 2, 3), (7, 3, 2, 3), (7, 1, 1, 0), (7, 2, 2, 0), (4, 2, 3, 2), (8, 2, 2, 4)]


@pytest.fixture(scope="module")
def ops(spi, gpu):
    return importlib.import_module("starpu-inference-server_amd.ops")


@functools.lru_cache(maxsize=None)
def case(ws, nh, nw, shift, prec):
    qkv, table = S.window_case(B, nh * ws, nw * ws, HEADS, ws)
    if prec == "fp16":
        qkv = qkv.astype(np.float16).astype(np.float32)
    return qkv, table, S.window_attention_ref(qkv, table, B, nh * ws, nw * ws, HEADS, ws, shift, SCALE)


def launch(ops, prec, qkv, table, Hh, W, ws, shift, heads=HEADS, head_dim=32):
    ctx = torch.full((B * Hh * W + GUARD, heads * head_dim), float("nan"), dtype=DT[prec], device="cuda")
    dq = torch.from_numpy(qkv).to("cuda", DT[prec])
    ops.window_attention(prec, dq, ops.window_bias(table, ws), B, Hh, W, heads, ws, shift, scale=SCALE, out=ctx, head_dim=head_dim)
    torch.cuda.synchronize()
    return ctx.cpu()


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("ws,nh,nw,shift", CASES)
def test_parity(ops, ws, nh, nw, shift, prec):
    qkv, table, ref = case(ws, nh, nw, shift, prec)
    M = B * nh * nw * ws * ws
    ctx = launch(ops, prec, qkv, table, nh * ws, nw * ws, ws, shift)
    assert bool(torch.isnan(ctx[M:]).all()), "rows past B H W were written"
    assert bool(torch.isfinite(ctx[:M]).all()), "rows left unwritten or not finite"
    e = R.nerr(ctx[:M].numpy(), ref)
    print(f"window_attention {prec} ws{ws} {nh}x{nw} windows shift {shift}: {e:.3e}")
    assert e < TOL[prec], f"{e:.3e}"


@pytest.mark.parametrize("ws,Hh,W,shift,head_dim,why", [
    (9, 18, 18, 0, 32, "window 9"), (7, 15, 14, 0, 32, "multiples of the window"), (7, 14, 14, 7, 32, "shift 7"),
    (7, 14, 14, 0, 64, "head_dim 64")])
def test_refusals_leave_the_output_untouched(ops, ws, Hh, W, shift, head_dim, why):
    qkv = torch.zeros((B * Hh * W, 3 * HEADS * head_dim), dtype=torch.float16, device="cuda")
    out = torch.full((B * Hh * W, HEADS * head_dim), float("nan"), dtype=torch.float16, device="cuda")
    bias = ops.window_bias(np.zeros(((2 * min(ws, 8) - 1) ** 2, HEADS), np.float32), min(ws, 8))
    with pytest.raises(RuntimeError, match=why):  # the op returned non-zero; its reason is the message
        ops.window_attention("fp16", qkv, bias, B, Hh, W, HEADS, ws, shift, scale=SCALE, out=out, head_dim=head_dim)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())

"""Op-level tests of the cosine window attention (the COS instances of window_attn.hip) through
spi_op_window_attention_cos, against swin_v2_refs.cos_window_attention_ref (float64, torchvision's order) on the
operand rounded to the kernel's input type.  B = 2, 3 heads with logit_scale (log 5, log 30, log 200) -- the third
runs at the clamp, tau 100 -- and the bias table cpb_table_ref gives for random cpb_mlp weights.  ctx is
NaN-filled with 8 guard rows behind it.

Cases (ws, H / ws, W / ws, shift): (8, 2, 2, 4) production, N = 64; (8, 1, 1, 0) the map is the window;
(7, 2, 2, 3) padded keys of zero norm, wave 3 with one live query; (4, 2, 3, 2) one key block, three dead waves.

Bars (normalised max error): fp32 1e-5 and fp16 3 * hd_refs.ATTN_EMU_WORST = 1.35e-3, the v1 kernel's.  A float32
numpy evaluation of the formula is 0.9e-6 / 1.8e-6 / 3.1e-6 from float64 at tau 10 / 30 / 100, and with P rounded to
fp16 on fp16 inputs at most 1.8e-4 (CPU emulations).

Measured on an MI355X (each test prints its figure):
  case            fp16      fp32      |  case            fp16      fp32
  (8, 2, 2, 4)    2.82e-4   1.7e-6    |  (7, 2, 2, 3)    3.13e-4   2.2e-6
  (8, 1, 1, 0)    3.28e-4   2.9e-6    |  (4, 2, 3, 2)    3.20e-4   3.3e-6
"""
import functools
import importlib
import math

import numpy as np
import pytest
import torch

import hd_refs as H
import op_refs as R
import swin_refs as S
import swin_v2_refs as V

pytestmark = pytest.mark.gpu

GUARD, B, HEADS, HIDDEN = 8, 2, 3, 512
LOGIT_SCALE = (math.log(5), math.log(30), math.log(200))
TOL = {"fp32": 1e-5, "fp16": 3 * H.ATTN_EMU_WORST}
DT = {"fp32": torch.float32, "fp16": torch.float16}
CASES = [(8, 2, 2, 4), (8, 1, 1, 0), (7, 2, 2, 3), (4, 2, 3, 2)]


@pytest.fixture(scope="module")
def ops(spi, gpu):
    return importlib.import_module("starpu-inference-server_amd.ops")


def tau_of(logit_scale):
    return np.exp(np.minimum(np.asarray(logit_scale, np.float32), np.float32(math.log(100.0)))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(ws, nh, nw, shift, prec):
    qkv, _ = S.window_case(B, nh * ws, nw * ws, HEADS, ws)
    if prec == "fp16":
        qkv = qkv.astype(np.float16).astype(np.float32)
    rng = np.random.default_rng(7)
    w0, b0 = rng.standard_normal((HIDDEN, 2)).astype(np.float32), rng.standard_normal(HIDDEN).astype(np.float32)
    w2 = (rng.standard_normal((HEADS, HIDDEN)) / 8).astype(np.float32)
    table = V.cpb_table_ref(w0, b0, w2, ws).astype(np.float32)
    return qkv, table, V.cos_window_attention_ref(qkv, table, tau_of(LOGIT_SCALE), B, nh * ws, nw * ws, HEADS, ws, shift)


def launch(ops, prec, qkv, table, tau, Hh, W, ws, shift):
    ctx = torch.full((B * Hh * W + GUARD, HEADS * 32), float("nan"), dtype=DT[prec], device="cuda")
    dq = torch.from_numpy(qkv).to("cuda", DT[prec])
    ops.window_attention_cos(prec, dq, ops.window_bias(table, ws), tau, B, Hh, W, HEADS, ws, shift, out=ctx)
    torch.cuda.synchronize()
    return ctx.cpu()


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("ws,nh,nw,shift", CASES)
def test_parity(ops, ws, nh, nw, shift, prec):
    qkv, table, ref = case(ws, nh, nw, shift, prec)
    M = B * nh * nw * ws * ws
    ctx = launch(ops, prec, qkv, table, torch.from_numpy(tau_of(LOGIT_SCALE)).cuda(), nh * ws, nw * ws, ws, shift)
    assert bool(torch.isnan(ctx[M:]).all()), "rows past B H W were written"
    assert bool(torch.isfinite(ctx[:M]).all()), "rows left unwritten or not finite"
    e = R.nerr(ctx[:M].numpy(), ref)
    print(f"window_attention_cos {prec} ws{ws} {nh}x{nw} windows shift {shift}: {e:.3e}")
    assert e < TOL[prec], f"{e:.3e}"


def test_the_clamp_is_at_100(ops):
    """logit_scale log 200 and log 100 on every head: the same tau, hence the same bits."""
    qkv, table, _ = case(8, 2, 2, 4, "fp16")
    got = [launch(ops, "fp16", qkv, table, torch.from_numpy(tau_of([math.log(t)] * HEADS)).cuda(), 16, 16, 8, 4)
           for t in (200.0, 100.0)]
    assert torch.equal(got[0][:-GUARD], got[1][:-GUARD]) and bool(torch.isfinite(got[0][:-GUARD]).all())


@pytest.mark.parametrize("tau,why", [(None, "null tau"), ("misaligned", "4-byte aligned")])
def test_refusals_leave_the_output_untouched(ops, tau, why):
    qkv = torch.zeros((B * 64, 3 * HEADS * 32), dtype=torch.float16, device="cuda")
    out = torch.full((B * 64, HEADS * 32), float("nan"), dtype=torch.float16, device="cuda")
    if tau is not None:
        tau = torch.zeros(4 * HEADS + 2, dtype=torch.uint8, device="cuda")[2:]  # two bytes past an aligned address
    with pytest.raises(RuntimeError, match=why):
        ops.window_attention_cos("fp16", qkv, ops.window_bias(np.zeros((225, HEADS), np.float32), 8), tau, B, 8, 8, HEADS, 8, 0, out=out)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())

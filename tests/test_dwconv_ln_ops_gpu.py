"""Op-level parity of the ConvNeXt kernels (dwconv_ln.hip) through spi_op_dwconv7_ln, spi_op_ln_space_to_depth and
spi_op_ln_rows.  Reference: F.conv2d(groups=C, padding=3) in float64 on the values the kernel sees (fp16-rounded x and w in fp16
mode, fp32 in fp32 mode), plus the fp32 bias, then F.layer_norm in float64.  Bars: fp32 the project's 1e-5; fp16
TOL16 = 2e-3 of test_gconv_ops_gpu.py -- exact fp16 products accumulated in fp32, then one fp16 rounding of an
O(1) normalised value.  Every launch writes into a buffer with 8 guard rows of NaN that must survive, and runs
twice for identical bits (no atomics, no split).
"""
import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle.cpu_codelet import normalized_max_error

pytestmark = pytest.mark.gpu

TOL = {"fp32": 1e-5, "fp16": 2e-3}
GUARD, EPS, B = 8, 1e-6, 2  # guard rows, LayerNorm eps, batch of the row-kernel cases

# (B, H, W, C)
CASES = [
    (1, 1, 1, 96),     # only the centre tap is live
    (2, 3, 5, 96),     # the map is smaller than the window; non-square
    (1, 7, 7, 768),    # stage-4 shape: every window covers the whole map
    (2, 9, 13, 128),   # odd sizes, partial tiles on both axes
    (1, 4, 70, 192),   # a row longer than any tile
    (1, 14, 14, 384),  # real stage-3 shape
    (1, 56, 56, 96),   # real stage-1 shape
    (1, 7, 7, 1536),   # largest C
    (1, 5, 5, 32),     # smallest C
]


case_id = "b{}_{}x{}_c{}".format
dt = {"fp16": torch.float16, "fp32": torch.float32}.get


@pytest.fixture(scope="module")
def ops(spi, gpu):
    return importlib.import_module("starpu-inference-server_amd.ops")


def seen(a, prec):
    return torch.from_numpy(a.astype(np.float16 if prec == "fp16" else np.float32).astype(np.float64))


def layer_norm64(v, g, b):
    return F.layer_norm(v, (v.shape[-1],), torch.from_numpy(g.astype(np.float64)), torch.from_numpy(b.astype(np.float64)), EPS)


def twice(launch, rows, cols, prec):
    """Two launches into NaN-guarded buffers: guard rows intact, identical bits; returns the rows as float64."""
    got = []
    for _ in range(2):
        buf = torch.full((rows + GUARD, cols), float("nan"), dtype=dt(prec), device="cuda")
        launch(buf)
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf[rows:]).all()), "rows past the output were written"
        got.append(buf[:rows])
    assert torch.equal(got[0].view(torch.uint8), got[1].view(torch.uint8)), "two launches differ"
    return got[0].double().cpu().numpy()


def run_dwconv(ops, prec, x, w, bias, g, b):
    B, H, W, C = x.shape
    x_d = torch.from_numpy(x).to("cuda", dt(prec))
    wp = ops.pack_weight_dwconv7(prec, w)
    bias_d, g_d, b_d = (torch.from_numpy(v).cuda() for v in (bias, g, b))
    got = twice(lambda buf: ops.dwconv7_ln(prec, x_d, wp, bias_d, g_d, b_d, EPS, buf), B * H * W, C, prec)
    conv = F.conv2d(seen(x, prec).permute(0, 3, 1, 2), seen(w, prec), torch.from_numpy(bias.astype(np.float64)),
                    padding=3, groups=C).permute(0, 2, 3, 1)
    return got, layer_norm64(conv, g, b).reshape(B * H * W, C).numpy()


@pytest.mark.parametrize("prec", ["fp16", "fp32"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: case_id(*c))
def test_dwconv7_ln_matches_float64(ops, case, prec):
    B, H, W, C = case
    rng = np.random.default_rng(list(case))
    x = rng.standard_normal((B, H, W, C), dtype=np.float32)
    w = rng.standard_normal((C, 1, 7, 7), dtype=np.float32) / 7.0
    bias = rng.standard_normal(C, dtype=np.float32) * 0.5
    g = (1.0 + 0.1 * rng.standard_normal(C)).astype(np.float32)
    b = (0.05 * rng.standard_normal(C)).astype(np.float32)
    got, ref = run_dwconv(ops, prec, x, w, bias, g, b)
    err = normalized_max_error(got, ref)
    print(f"dwconv7_ln {case_id(*case)} {prec}: err {err:.3e}")
    assert err < TOL[prec]


@pytest.mark.parametrize("prec", ["fp16", "fp32"])
def test_exact_sums_separate_tap_indexing_from_rounding(ops, prec):
    """Integer x in [-3, 3], w in [-2, 2]: every partial sum is an integer below 2^11, exact in both types; with gamma 1,
    beta 0 LayerNorm is the only inexact step.  The second launch's one-hot filters check each tap's place alone."""
    B, H, W, C = 2, 9, 13, 96
    rng = np.random.default_rng(7)
    x = rng.integers(-3, 4, (B, H, W, C)).astype(np.float32)
    one, zero = np.ones(C, np.float32), np.zeros(C, np.float32)
    w = rng.integers(-2, 3, (C, 1, 7, 7)).astype(np.float32)
    hot = np.zeros((C, 49), np.float32)
    hot[np.arange(C), np.arange(C) % 49] = 1.0  # channel c copies the pixel at tap c % 49
    for name, wt in (("integer", w), ("one-hot", hot.reshape(C, 1, 7, 7))):
        got, ref = run_dwconv(ops, prec, x, wt, zero, one, zero)
        err = normalized_max_error(got, ref)
        print(f"dwconv7_ln exact {name} {prec}: err {err:.3e}")
        assert err < TOL[prec]


def test_large_row_mean_needs_centred_statistics(ops):
    """fp32 rows of mean 50, spread 1: E[x^2] - E[x]^2 in fp32 loses ~2500 * 2^-24 = 1.5e-4 of the variance."""
    B, H, W, C = 1, 6, 6, 96
    rng = np.random.default_rng(11)
    x = rng.standard_normal((B, H, W, C), dtype=np.float32)
    w = np.zeros((C, 1, 7, 7), np.float32)
    w[:, 0, 3, 3] = 1.0  # identity conv: the rows are x + 50
    bias = np.full(C, 50.0, np.float32)
    got, ref = run_dwconv(ops, "fp32", x, w, bias, np.ones(C, np.float32), np.zeros(C, np.float32))
    err = normalized_max_error(got, ref)
    print(f"dwconv7_ln mean 50 fp32: err {err:.3e}")
    assert err < TOL["fp32"]


ROW_CASES = [(c, h, w) for c in (96, 768) for (h, w) in ((2, 2), (6, 4))]


def row_data(C, H, W, prec):
    rng = np.random.default_rng([C, H, W])
    x = (rng.standard_normal((B, H, W, C), dtype=np.float32) + 0.5)
    g = (1.0 + 0.1 * rng.standard_normal(C)).astype(np.float32)
    b = (0.05 * rng.standard_normal(C)).astype(np.float32)
    return x, g, b, torch.from_numpy(g).cuda(), torch.from_numpy(b).cuda()


@pytest.mark.parametrize("prec", ["fp16", "fp32"])
@pytest.mark.parametrize("C,H,W", ROW_CASES)
def test_ln_space_to_depth(ops, C, H, W, prec):
    x, g, b, g_d, b_d = row_data(C, H, W, prec)
    x_d = torch.from_numpy(x).to("cuda", dt(prec))
    rows = B * (H // 2) * (W // 2)
    got = twice(lambda buf: ops.ln_space_to_depth(prec, x_d, g_d, b_d, EPS, buf), rows, 4 * C, prec)
    ln = layer_norm64(seen(x, prec), g, b)  # [B][H][W][C] -> [B][H/2][W/2][kh][kw][C]
    ref = ln.reshape(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(rows, 4 * C).numpy()
    err = normalized_max_error(got, ref)
    print(f"ln_space_to_depth c{C} {H}x{W} {prec}: err {err:.3e}")
    assert err < TOL[prec]


@pytest.mark.parametrize("prec,x_f32", [("fp16", False), ("fp16", True), ("fp32", True)])
@pytest.mark.parametrize("pooled", [False, True])
@pytest.mark.parametrize("C,H,W", ROW_CASES)
def test_ln_rows(ops, C, H, W, prec, x_f32, pooled):
    x, g, b, g_d, b_d = row_data(C, H, W, prec)
    xin = "fp32" if x_f32 else prec
    x_d = torch.from_numpy(x).to("cuda", dt(xin))
    rows = B if pooled else B * H * W
    got = twice(lambda buf: ops.ln_rows(prec, x_d, rows, C, g_d, b_d, EPS, buf, pool_hw=H * W if pooled else 0),
                rows, C, prec)
    v = seen(x, xin).reshape(B, H * W, C)
    ref = layer_norm64(v.mean(1) if pooled else v.reshape(rows, C), g, b).numpy()
    err = normalized_max_error(got, ref)
    print(f"ln_rows c{C} {H}x{W} {prec} x_f32={x_f32} pooled={pooled}: err {err:.3e}")
    assert err < TOL[prec]

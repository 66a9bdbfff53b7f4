"""Op-level test of the patch-merging row kernel (s2d_ln in dwconv_ln.hip) through spi_op_s2d_ln against float64:
torchvision's cat(x[0::2, 0::2], x[1::2, 0::2], x[0::2, 1::2], x[1::2, 1::2]) then LayerNorm over 4 C.  C in
{32, 96, 512} (one, two and eight float4 per lane) on a 4 x 6 map, B = 2; in fp32 also rows of mean 50, where a
one-pass variance would cancel.  Bars: those test_dwconv_ln_ops_gpu.py holds the row kernels to, fp16 2e-3 and
fp32 1e-5 (normalised max error).  Measured on an MI355X: fp16 at most 2.9e-4, fp32 1.4e-7 (mean 50: 2.4e-6).
"""
import importlib

import numpy as np
import pytest
import torch

import op_refs as R

pytestmark = pytest.mark.gpu

TOL = {"fp32": 1e-5, "fp16": 2e-3}
DT = {"fp32": torch.float32, "fp16": torch.float16}
B, Hh, W, EPS, GUARD = 2, 4, 6, 1e-5, 4


@pytest.mark.parametrize("prec,mean", [("fp32", 0.0), ("fp32", 50.0), ("fp16", 0.0)])
@pytest.mark.parametrize("C", [32, 96, 512])
def test_s2d_ln(spi, gpu, C, prec, mean):
    ops = importlib.import_module("starpu-inference-server_amd.ops")
    rng = np.random.default_rng(C)
    x = (rng.standard_normal((B, Hh, W, C)) + mean).astype(np.float32)
    if prec == "fp16":
        x = x.astype(np.float16).astype(np.float32)
    g, b = (1 + 0.1 * rng.standard_normal(4 * C)).astype(np.float32), (0.1 * rng.standard_normal(4 * C)).astype(np.float32)
    x64 = x.astype(np.float64)
    rows = np.concatenate([x64[:, 0::2, 0::2], x64[:, 1::2, 0::2], x64[:, 0::2, 1::2], x64[:, 1::2, 1::2]], -1).reshape(-1, 4 * C)
    ref = (rows - rows.mean(1, keepdims=True)) / np.sqrt(rows.var(1, keepdims=True) + EPS) * g + b
    M = ref.shape[0]
    out = torch.full((M + GUARD, 4 * C), float("nan"), dtype=DT[prec], device="cuda")
    ops.s2d_ln(prec, torch.from_numpy(x).to("cuda", DT[prec]), torch.from_numpy(g).cuda(), torch.from_numpy(b).cuda(), EPS, out)
    torch.cuda.synchronize()
    got = out.cpu()
    assert bool(torch.isnan(got[M:]).all()) and bool(torch.isfinite(got[:M]).all())
    e = R.nerr(got[:M].numpy(), ref)
    print(f"s2d_ln {prec} C{C} mean {mean}: {e:.3e}")
    assert e < TOL[prec], f"{e:.3e}"

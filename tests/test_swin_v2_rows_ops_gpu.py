"""Op-level tests of Swin v2's two row kernels (dwconv_ln.hip) against float64.  ln_rows_add, the residual-post-norm
y = res + LN(x) gamma + beta: C in {64, 96, 1024} (one, two and four float4 per lane), 5 rows (two workgroups, the
second with one live wave), fp32 and fp16, once with y aliasing res and, in fp32, with rows of mean 50, where a
one-pass variance would cancel.  s2d_rows, patch merging's gather: exact equality with torchvision's cat on a 4 x 6
map, B = 2, C = 32 and 512.  Bars: those test_s2d_ln_ops_gpu.py holds the row kernels to, fp16 2e-3 and fp32 1e-5
(normalised max error).  Measured on an MI355X: fp16 at most 3.7e-4, fp32 6.4e-8 (mean 50: 6.7e-7).
"""
import importlib

import numpy as np
import pytest
import torch

import op_refs as R

pytestmark = pytest.mark.gpu

TOL = {"fp32": 1e-5, "fp16": 2e-3}
DT = {"fp32": torch.float32, "fp16": torch.float16}
ROWS, EPS, GUARD = 5, 1e-5, 4


@pytest.mark.parametrize("prec,mean,alias", [("fp32", 0.0, False), ("fp32", 50.0, False), ("fp16", 0.0, False), ("fp16", 0.0, True)])
@pytest.mark.parametrize("C", [64, 96, 1024])
def test_ln_rows_add(spi, gpu, C, prec, mean, alias):
    ops = importlib.import_module("starpu-inference-server_amd.ops")
    rng = np.random.default_rng(C)
    x, res = (rng.standard_normal((ROWS, C)) + mean).astype(np.float32), (2 * rng.standard_normal((ROWS, C))).astype(np.float32)
    if prec == "fp16":
        x, res = (a.astype(np.float16).astype(np.float32) for a in (x, res))
    g, b = (1 + 0.1 * rng.standard_normal(C)).astype(np.float32), (0.1 * rng.standard_normal(C)).astype(np.float32)
    x64 = x.astype(np.float64)
    ref = res + (x64 - x64.mean(1, keepdims=True)) / np.sqrt(x64.var(1, keepdims=True) + EPS) * g + b
    out = torch.full((ROWS + GUARD, C), float("nan"), dtype=DT[prec], device="cuda")
    dres = torch.from_numpy(res).to("cuda", DT[prec])
    if alias:
        out[:ROWS] = dres
        dres = out
    ops.ln_rows_add(prec, torch.from_numpy(x).to("cuda", DT[prec]), dres, ROWS, C, torch.from_numpy(g).cuda(),
                    torch.from_numpy(b).cuda(), EPS, out)
    torch.cuda.synchronize()
    got = out.cpu()
    assert bool(torch.isnan(got[ROWS:]).all()) and bool(torch.isfinite(got[:ROWS]).all())
    e = R.nerr(got[:ROWS].numpy(), ref)
    print(f"ln_rows_add {prec} C{C} mean {mean} alias {alias}: {e:.3e}")
    assert e < TOL[prec], f"{e:.3e}"


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("C", [32, 512])
def test_s2d_rows(spi, gpu, C, prec):
    ops = importlib.import_module("starpu-inference-server_amd.ops")
    x = torch.from_numpy(np.random.default_rng(C).standard_normal((2, 4, 6, C)).astype(np.float32)).to(DT[prec])
    want = torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], -1).reshape(-1, 4 * C)
    out = torch.full((want.shape[0] + GUARD, 4 * C), float("nan"), dtype=DT[prec], device="cuda")
    ops.s2d_rows(prec, x.cuda(), out)
    torch.cuda.synchronize()
    got = out.cpu()
    assert bool(torch.isnan(got[want.shape[0]:]).all()) and torch.equal(got[:want.shape[0]], want)

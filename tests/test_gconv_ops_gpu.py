"""Op-level parity of the grouped 3x3 conv kernel (conv_group.hip) through spi_op_conv2d_grouped.

Reference: torch.nn.functional.conv2d(..., groups=g) in float64 on the fp16-rounded x and the fp16-rounded
weights (the values the kernel sees), plus the fp32 bias and ReLU.  The bar is the project's operand-exact
fp16-output bar, 2e-3 normalised max error (TOL16 of test_conv_pair_ops_gpu.py): fp32 accumulation of exact
fp16 products, then one rounding of the output to fp16 (2^-11 relative).

Every launch writes into a buffer with 8 rows of NaN behind the M output rows, which must survive, and every
case runs twice: the kernel has no atomics and no split, so the two launches give the same bits.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle.cpu_codelet import normalized_max_error

pytestmark = pytest.mark.gpu

TOL16 = 2e-3
GUARD = 8
NAN = float("nan")

# (B, H, W, C, groups, stride)
CASES = [
    (2, 7, 5, 128, 32, 1),     # cpg 4
    (2, 7, 5, 128, 16, 1),     # cpg 8
    (1, 8, 8, 128, 8, 2),      # cpg 16
    (2, 7, 7, 128, 4, 2),      # cpg 32, odd size under stride 2
    (1, 6, 6, 128, 2, 1),      # cpg 64
    (1, 5, 9, 256, 32, 1),     # two channel tiles
    (3, 2, 2, 256, 4, 2),      # 1x1 output
    (1, 1, 1, 128, 32, 1),     # every tap but the centre is padding
    (1, 3, 70, 128, 32, 1),    # a row longer than any 64-pixel tile
    (1, 56, 56, 128, 32, 1),   # real stage-1 shape
    (2, 14, 14, 1024, 32, 2),  # real stage-4 shape
]


def case_id(c):
    return "b{}_{}x{}_c{}_g{}_s{}".format(*c)


@pytest.fixture(scope="module")
def ops(spi, gpu):
    import importlib
    return importlib.import_module("starpu-inference-server_amd.ops")


_cache = {}


def case_data(case):
    """x fp16 NHWC, w fp32 [C][cpg][3][3], bias fp32 [C] and the float64 accumulator reference (no bias, no
    activation) [B][OH][OW][C] of a case; computed once."""
    if case not in _cache:
        B, H, W, Cc, g, stride = case
        rng = np.random.default_rng(list(case))
        cpg = Cc // g
        x = rng.standard_normal((B, H, W, Cc), dtype=np.float32).astype(np.float16)
        w = (rng.standard_normal((Cc, cpg, 3, 3), dtype=np.float32) / np.sqrt(9.0 * cpg)).astype(np.float32)
        bias = rng.standard_normal(Cc, dtype=np.float32) * 0.5
        x64 = torch.from_numpy(x.astype(np.float64)).permute(0, 3, 1, 2)
        w64 = torch.from_numpy(w.astype(np.float16).astype(np.float64))
        acc = F.conv2d(x64, w64, None, stride, 1, groups=g).permute(0, 2, 3, 1).contiguous().numpy()
        _cache[case] = (x, w, bias, acc)
    return _cache[case]


def reference(acc, bias, relu):
    y = acc + (bias.astype(np.float64) if bias is not None else 0.0)
    return np.maximum(y, 0.0) if relu else y


def launch(ops, x_d, wp, g, stride, bias_d, relu, M, Cc):
    """One launch into a NaN-filled buffer with GUARD rows behind the output; returns the [M][C] rows."""
    buf = torch.full((M + GUARD, Cc), NAN, dtype=torch.float16, device="cuda")
    ops.conv2d_grouped(x_d, wp, g, stride, bias=bias_d, act="relu" if relu else None, out=buf)
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[M:]).all()), "rows past M were written"
    return buf[:M]


def run(ops, case, with_bias, relu):
    B, H, W, Cc, g, stride = case
    x, w, bias, acc = case_data(case)
    M = acc.shape[0] * acc.shape[1] * acc.shape[2]
    x_d = torch.from_numpy(x).cuda()
    wp = ops.pack_weight_grouped(w, g)
    bias_d = torch.from_numpy(bias).cuda() if with_bias else None
    y0 = launch(ops, x_d, wp, g, stride, bias_d, relu, M, Cc)
    y1 = launch(ops, x_d, wp, g, stride, bias_d, relu, M, Cc)
    assert torch.equal(y0.view(torch.int16), y1.view(torch.int16)), "two launches differ"
    ref = reference(acc, bias if with_bias else None, relu).reshape(M, Cc)
    err = normalized_max_error(y0.float().cpu().numpy(), ref)
    print(f"gconv {case_id(case)} bias={with_bias} relu={relu}: err {err:.3e}")
    return err


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_grouped_conv_matches_float64(ops, case):
    assert run(ops, case, True, True) < TOL16


@pytest.mark.parametrize("case", CASES[:3], ids=case_id)
@pytest.mark.parametrize("with_bias,relu", [(False, False), (True, False), (False, True)])
def test_grouped_conv_bias_and_relu(ops, case, with_bias, relu):
    assert run(ops, case, with_bias, relu) < TOL16


@pytest.mark.parametrize("case", [CASES[0], CASES[1]], ids=case_id)
def test_finite_values_do_not_leak_between_groups(ops, case):
    """Groups of one 16-channel slice share MFMAs over zero-packed off-group weights: scaling one group's
    inputs by 1000 (finite) changes that group's outputs only; every other channel keeps its bits."""
    B, H, W, Cc, g, stride = case
    x, w, bias, acc = case_data(case)
    cpg = Cc // g
    M = acc.shape[0] * acc.shape[1] * acc.shape[2]
    wp = ops.pack_weight_grouped(w, g)
    bias_d = torch.from_numpy(bias).cuda()
    base = launch(ops, torch.from_numpy(x).cuda(), wp, g, stride, bias_d, False, M, Cc).cpu()
    for grp in (1, g - 2):  # a middle group of the first slice and one of the last
        xs = x.astype(np.float32)
        xs[..., grp * cpg:(grp + 1) * cpg] *= 1000.0
        xs = xs.astype(np.float16)
        assert np.isfinite(xs).all()
        got = launch(ops, torch.from_numpy(xs).cuda(), wp, g, stride, bias_d, False, M, Cc).cpu()
        own = np.zeros(Cc, dtype=bool)
        own[grp * cpg:(grp + 1) * cpg] = True
        assert torch.equal(got[:, ~own].view(torch.int16), base[:, ~own].view(torch.int16)), f"group {grp} leaked"
        assert not torch.equal(got[:, own], base[:, own]), f"group {grp}: its own outputs did not change"
        x64 = torch.from_numpy(xs.astype(np.float64)).permute(0, 3, 1, 2)
        ref = F.conv2d(x64, torch.from_numpy(w.astype(np.float16).astype(np.float64)), torch.from_numpy(
            bias.astype(np.float64)), stride, 1, groups=g).permute(0, 2, 3, 1).reshape(M, Cc).numpy()
        assert normalized_max_error(got[:, own].float().numpy(), ref[:, own]) < TOL16


def test_grouped_conv_rejections(ops, spi):
    """One call per rule of spi_ops.h: non-zero, a message, y untouched."""
    lib = spi.lib
    B, H, W, Cc, g = 1, 4, 4, 128, 32
    x = torch.zeros(B * H * W * Cc + 8, dtype=torch.float16, device="cuda")
    w = torch.zeros(lib.spi_op_gconv_packed_bytes(Cc, g, 3, 3) + 16, dtype=torch.uint8, device="cuda")
    bias = torch.zeros(Cc + 4, dtype=torch.float32, device="cuda")
    y = torch.full((B * H * W * Cc + 8,), NAN, dtype=torch.float16, device="cuda")
    ok = dict(x=x.data_ptr(), B=B, H=H, W=W, C=Cc, w=w.data_ptr(), groups=g, KH=3, KW=3, stride=1, pad=1,
              bias=bias.data_ptr(), y=y.data_ptr(), act=1)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.spi_op_conv2d_grouped(C.c_void_p(a["x"]), a["B"], a["H"], a["W"], a["C"], C.c_void_p(a["w"]),
                                         a["groups"], a["KH"], a["KW"], a["stride"], a["pad"], C.c_void_p(a["bias"]),
                                         C.c_void_p(a["y"]), a["act"], None)

    bad = {
        "C not a multiple of 128": dict(C=64, groups=16),
        "cpg 2": dict(C=128, groups=64),
        "cpg 128": dict(C=256, groups=2),
        "groups 1": dict(groups=1),
        "groups not dividing C": dict(groups=24),
        "5x5 kernel": dict(KH=5, KW=5, pad=2),
        "1x1 kernel": dict(KH=1, KW=1, pad=0),
        "pad 0": dict(pad=0),
        "stride 3": dict(stride=3),
        "stride 0": dict(stride=0),
        "null x": dict(x=None),
        "null W_packed": dict(w=None),
        "null y": dict(y=None),
        "B 0": dict(B=0),
        "H 0": dict(H=0),
        "W -1": dict(W=-1),
        "x off alignment": dict(x=x.data_ptr() + 2),
        "y off alignment": dict(y=y.data_ptr() + 8),
        "W_packed off alignment": dict(w=w.data_ptr() + 4),
        "act gelu": dict(act=2),
        "act -1": dict(act=-1),
    }
    for what, kw in bad.items():
        rc = call(**kw)
        msg = spi.lib.spi_last_error()
        assert rc != 0 and msg, f"{what}: accepted"
        print(f"{what}: {msg.decode()}")
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all()), "a rejected call wrote y"
    assert lib.spi_op_gconv_packed_bytes(64, 8, 3, 3) == 0 and lib.spi_op_gconv_packed_bytes(128, 32, 1, 1) == 0
    host = np.zeros(16, dtype=np.float32)
    assert lib.spi_op_gconv_pack_weight(host.ctypes.data, 64, 8, 3, 3, host.ctypes.data) != 0
    assert call() == 0  # the valid call the rules were varied from
    torch.cuda.synchronize()
    assert not bool(torch.isnan(y[:B * H * W * Cc]).any()) and bool(torch.isnan(y[B * H * W * Cc:]).all())

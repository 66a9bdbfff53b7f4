"""Op-level parity of the MBConv kernels (mbconv.hip) through spi_op_dwconv_act, spi_op_se_gate and
spi_op_scale_channels, and of act 3 (SiLU) in spi_op_gemm / spi_op_conv2d.  Reference: float64 on the values the
kernel sees (fp16-rounded x and w in fp16 mode).  Bars: the conv output fp32 1e-5 and fp16 2e-3 (TOL16 of
test_gconv_ops_gpu.py: exact fp16 products accumulated in fp32, one fp16 rounding); the pooled means and the gate
1e-5 in both precisions (fp32 sums of fp32 values); scale_channels bit equality; act 3 the bars test_ops_gpu.py
holds the same calls to.  Every launch writes into a buffer with 8 guard rows of NaN that must survive, and runs
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
GUARD = 8

# (B, H, W, C, k, stride)
CASES = [
    (1, 1, 1, 8, 3, 1),       # only the centre tap is live; one slab, one chunk
    (2, 3, 5, 72, 5, 1),      # the map is smaller than the window; a partial second slab
    (2, 8, 12, 40, 3, 2),     # even map at stride 2: the last row and column are never read
    (2, 9, 13, 144, 5, 2),    # odd map at stride 2, partial tiles on both axes
    (1, 4, 70, 96, 3, 1),     # a row longer than a tile
    (1, 7, 7, 1152, 5, 1),    # real last-stage shape
    (1, 112, 112, 32, 3, 1),  # real first-stage shape: 98 tiles of pool sums
]

dt = {"fp16": torch.float16, "fp32": torch.float32}.get


@pytest.fixture(scope="module")
def ops(spi, gpu):
    return importlib.import_module("starpu-inference-server_amd.ops")


def seen(a, prec):
    return torch.from_numpy(np.asarray(a).astype(np.float16 if prec == "fp16" else np.float32).astype(np.float64))


def twice(launch, rows, cols, dtype):
    """Two launches into NaN-guarded buffers: guard rows intact, identical bits; returns the rows of the first."""
    got = []
    for _ in range(2):
        buf = torch.full((rows + GUARD, cols), float("nan"), dtype=dtype, device="cuda")
        launch(buf)
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf[rows:]).all()), "rows past the output were written"
        got.append(buf[:rows])
    assert torch.equal(got[0].view(torch.uint8), got[1].view(torch.uint8)), "two launches differ"
    return got[0]


def run_dwconv(ops, prec, case, act, pool):
    B, H, W, C, k, s = case
    rng = np.random.default_rng(list(case))
    x = rng.standard_normal((B, H, W, C), dtype=np.float32)
    w = rng.standard_normal((C, 1, k, k), dtype=np.float32) / k
    bias = rng.standard_normal(C, dtype=np.float32) * 0.5
    x_d, bias_d, wp = torch.from_numpy(x).to("cuda", dt(prec)), torch.from_numpy(bias).cuda(), ops.pack_weight_dwconv(prec, w)
    ref = F.conv2d(seen(x, prec).permute(0, 3, 1, 2), seen(w, prec), torch.from_numpy(bias.astype(np.float64)),
                   stride=s, padding=k // 2, groups=C).permute(0, 2, 3, 1)
    ref = F.silu(ref) if act == "silu" else ref
    OH, OW = ref.shape[1:3]
    tiles = ops.dwconv_tiles(H, W, k, s)
    part = []  # the pool sums of each launch, NaN-filled first: every row must be written

    def launch(buf):
        part.append(torch.full((B, tiles, C), float("nan"), device="cuda") if pool else None)
        ops.dwconv_act(prec, x_d, wp, bias_d, k, s, buf, act=act, pool_part=part[-1])

    got = twice(launch, B * OH * OW, C, dt(prec)).double().cpu().numpy()
    if pool:
        assert torch.equal(part[0], part[1]), "the pool sums of two launches differ"
    mean = part[0].double().sum(1).cpu().numpy() / (OH * OW) if pool else None
    return got, ref.reshape(B * OH * OW, C).numpy(), mean, ref.mean((1, 2)).numpy()


@pytest.mark.parametrize("prec", ["fp16", "fp32"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "b{}_{}x{}_c{}_k{}s{}".format(*c))
def test_dwconv_silu_and_pool_sums_match_float64(ops, case, prec):
    got, ref, mean, ref_mean = run_dwconv(ops, prec, case, "silu", True)
    err, perr = normalized_max_error(got, ref), normalized_max_error(mean, ref_mean)
    print(f"dwconv_act {case} {prec}: err {err:.3e} pooled mean err {perr:.3e}")
    assert err < TOL[prec] and perr < 1e-5


@pytest.mark.parametrize("prec", ["fp16", "fp32"])
def test_dwconv_without_activation_or_pool(ops, prec):
    got, ref, _, _ = run_dwconv(ops, prec, (2, 9, 13, 144, 5, 2), None, False)
    err = normalized_max_error(got, ref)
    print(f"dwconv_act act 0 {prec}: err {err:.3e}")
    assert err < TOL[prec]


@pytest.mark.parametrize("B,C,sq,tiles", [(2, 32, 8, 1), (2, 1152, 48, 5), (1, 2112, 1, 3)])
def test_se_gate_matches_float64(ops, B, C, sq, tiles):
    rng = np.random.default_rng([B, C, sq, tiles])
    hw = 37
    part = rng.standard_normal((B, tiles, C), dtype=np.float32) * hw / tiles
    W1 = rng.standard_normal((sq, C), dtype=np.float32) / C ** 0.5
    W2 = rng.standard_normal((C, sq), dtype=np.float32) / sq ** 0.5
    b1, b2 = rng.standard_normal(sq, dtype=np.float32) * 0.5, rng.standard_normal(C, dtype=np.float32) * 0.5
    dev = [torch.from_numpy(v).cuda() for v in (part, W1, b1, W2, b2)]
    got = twice(lambda buf: ops.se_gate(dev[0], hw, *dev[1:], buf), B, C, torch.float32).double().cpu().numpy()
    p64, W1_, b1_, W2_, b2_ = (torch.from_numpy(v.astype(np.float64)) for v in (part, W1, b1, W2, b2))
    ref = torch.sigmoid(F.silu(p64.sum(1) / hw @ W1_.T + b1_) @ W2_.T + b2_).numpy()
    err = normalized_max_error(got, ref)
    print(f"se_gate b{B} c{C} sq{sq} tiles{tiles}: err {err:.3e}")
    assert err < 1e-5


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("prec", ["fp16", "fp32"])
def test_scale_channels_bits(ops, prec, in_place):
    B, HW, C = 2, 35, 72
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.standard_normal((B, HW, C), dtype=np.float32)).to(dt(prec))
    gate = torch.from_numpy(rng.random((B, C), dtype=np.float32))
    want = (x.float() * gate[:, None, :]).to(dt(prec)).reshape(B * HW, C)
    gate_d = gate.cuda()

    def launch(buf):
        src = buf[:B * HW].view(B, HW, C).copy_(x) if in_place else x.cuda()
        ops.scale_channels(prec, src, gate_d, buf)

    got = twice(launch, B * HW, C, dt(prec)).cpu()
    assert torch.equal(got.view(torch.uint8), want.view(torch.uint8))


@pytest.mark.parametrize("prec", ["fp16", "fp32"])
def test_silu_epilogue_of_gemm_and_conv2d(ops, prec):
    """Act 3 of spi_op_gemm (M 70, K 24, N 40) and spi_op_conv2d (3x3 / stride 2, 8 -> 32 channels, a 9 x 11 map)
    against float64; bars: test_ops_gpu.py's for the same calls (gemm fp16 5e-3, conv fp16 2e-3, fp32 1e-5)."""
    rng = np.random.default_rng(3)
    M, K, N = 70, 24, 40
    A, W, b = (rng.standard_normal(s, dtype=np.float32) for s in ((M, K), (N, K), (N,)))
    W /= K ** 0.5
    out = ops.gemm(prec, torch.from_numpy(A).to("cuda", dt(prec)), ops.pack_weight(prec, W), N,
                   bias=torch.from_numpy(b).cuda(), act="silu")
    ref = F.silu(seen(A, prec) @ seen(W, prec).T + torch.from_numpy(b.astype(np.float64))).numpy()
    err = normalized_max_error(out.double().cpu().numpy(), ref)
    print(f"gemm silu {prec}: err {err:.3e}")
    assert err < {"fp32": 1e-5, "fp16": 5e-3}[prec]
    B, H, Wd, cin, cout = 2, 9, 11, 8, 32
    x = rng.standard_normal((B, H, Wd, cin), dtype=np.float32)
    w = rng.standard_normal((cout, cin, 3, 3), dtype=np.float32) / (cin * 9) ** 0.5
    out = ops.conv2d(prec, torch.from_numpy(x).to("cuda", dt(prec)), ops.pack_weight(prec, ops.conv_weight_matrix(torch.from_numpy(w), cin)),
                     cout, 3, 3, 2, 1, bias=torch.from_numpy(b[:cout]).cuda(), act="silu")
    ref = F.silu(F.conv2d(seen(x, prec).permute(0, 3, 1, 2), seen(w, prec), torch.from_numpy(b[:cout].astype(np.float64)),
                          stride=2, padding=1)).permute(0, 2, 3, 1).numpy()
    err = normalized_max_error(out.double().cpu().numpy(), ref)
    print(f"conv2d silu {prec}: err {err:.3e}")
    assert err < TOL[prec]

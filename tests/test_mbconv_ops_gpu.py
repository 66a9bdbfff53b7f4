"""Op-level parity of the MBConv kernels (mbconv.hip) through spi_op_dwconv_act, spi_op_se_gate and
spi_op_scale_channels, and of act 3 (SiLU) in spi_op_gemm / spi_op_conv2d.  Reference: float64 on the values the
kernel sees (fp16-rounded x and w in fp16 mode).  Bars: the conv output fp32 1e-5 and fp16 2e-3 (TOL16 of
test_gconv_ops_gpu.py: exact fp16 products accumulated in fp32, one fp16 rounding); the pooled means and the gate
1e-5 in both precisions (fp32 sums of fp32 values); scale_channels bit equality; act 3 the bars test_ops_gpu.py
holds the same calls to.  Every launch writes into a buffer with 8 guard rows of NaN that must survive, and runs
twice for identical bits (no atomics, no split).  The SiLU conv cases also hold op_refs.silu_lobe_err -- the
error over the entries with a pre-activation <= 0, over the lobe's depth 0.2785 -- to the conv's bar (measured:
fp16 4.4e-4, the output's rounding; fp32 7.4e-7).  Every refusal of the three ops is tested with its message and
with NaN-filled outputs that must stay NaN.  (act 3 on every GEMM and conv route: test_silu_routes_ops_gpu.py.)
"""
import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import op_refs as R
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
    (2, 16, 8, 8, 3, 1),      # exactly one tile
    (1, 17, 9, 16, 5, 1),     # one pixel past it on both axes
    (2, 16, 16, 8, 3, 2),     # one 8 x 8 tile at stride 2
    (1, 17, 17, 24, 5, 2),    # one pixel past that
    (1, 1, 40, 8, 5, 1),      # a map one pixel high
    (1, 40, 1, 8, 3, 2),      # a map one pixel wide
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
    pre = ref.reshape(-1, C).numpy()
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
    return got, ref.reshape(B * OH * OW, C).numpy(), mean, ref.mean((1, 2)).numpy(), pre


@pytest.mark.parametrize("prec", ["fp16", "fp32"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "b{}_{}x{}_c{}_k{}s{}".format(*c))
def test_dwconv_silu_and_pool_sums_match_float64(ops, case, prec):
    got, ref, mean, ref_mean, pre = run_dwconv(ops, prec, case, "silu", True)
    err, perr = normalized_max_error(got, ref), normalized_max_error(mean, ref_mean)
    lobe = R.silu_lobe_err(got, ref, pre)  # the error on the negative lobe, over its depth: the same bar
    print(f"dwconv_act {case} {prec}: err {err:.3e} lobe {lobe:.3e} pooled mean err {perr:.3e}")
    assert err < TOL[prec] and lobe < TOL[prec] and perr < 1e-5


@pytest.mark.parametrize("prec", ["fp16", "fp32"])
def test_dwconv_without_activation_or_pool(ops, prec):
    got, ref, _, _, _ = run_dwconv(ops, prec, (2, 9, 13, 144, 5, 2), None, False)
    err = normalized_max_error(got, ref)
    print(f"dwconv_act act 0 {prec}: err {err:.3e}")
    assert err < TOL[prec]


@pytest.mark.parametrize("prec", ["fp16", "fp32"])
def test_dwconv_without_activation_with_pool_sums(ops, prec):
    """act 0 pools the conv's own fp32 values: the pooled mean is the mean of the pre-activation."""
    got, ref, mean, ref_mean, _ = run_dwconv(ops, prec, (2, 9, 13, 144, 5, 2), None, True)
    err, perr = normalized_max_error(got, ref), normalized_max_error(mean, ref_mean)
    print(f"dwconv_act act 0 with pool sums {prec}: err {err:.3e} pooled mean err {perr:.3e}")
    assert err < TOL[prec] and perr < 1e-5


# C % 64 in {8, 40, 16, 48, 32, 0}; (1, 240, 33, 8): a second slice of one column and two whole quads of tiles;
# (1, 4608, 256, 1): both maxima
@pytest.mark.parametrize("B,C,sq,tiles", [(2, 32, 8, 1), (2, 1152, 48, 5), (1, 2112, 1, 3), (1, 8, 1, 1), (2, 40, 4, 2),
                                          (2, 144, 6, 4), (1, 240, 33, 8), (2, 672, 28, 9), (1, 4608, 256, 1)])
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


def refused(ops, message, call, *untouched):
    """call() must raise OpError with the kernel's own message and leave the NaN-filled buffers as they were."""
    import re
    with pytest.raises(ops.OpError, match=re.escape(message)):
        call()
    torch.cuda.synchronize()
    for t in untouched:
        assert bool(torch.isnan(t).all()), f"a call refused with '{message}' wrote to an output"


def nan(n, dtype=torch.float32):
    return torch.full((n,), float("nan"), dtype=dtype, device="cuda")


@pytest.mark.parametrize("prec", ["fp16", "fp32"])
def test_dwconv_act_refusals(ops, prec):
    """C = 12 and 4616, k = 7, stride 3, ReLU, B = 0 and an x one element off 16 bytes: refused before any launch.
    Where the wrapper cannot express a case (it sizes pool_part from k and stride; an empty tensor has no address)
    the call goes to the library itself."""
    import ctypes as Ct
    x = torch.zeros((1 << 16) + 8, dtype=dt(prec), device="cuda")
    w = torch.zeros(1 << 17, dtype=dt(prec), device="cuda")
    bias = torch.zeros(8192, device="cuda")
    y, part = nan(1 << 16, dt(prec)), nan(1 << 14)

    def wrapped(C, act="silu", off=0, H=2, W=2, k=3, s=1):
        rows = ops.dwconv_tiles(H, W, k, s)
        assert rows == 1
        return lambda: ops.dwconv_act(prec, x[off:off + H * W * C].view(1, H, W, C), w, bias, k, s, y, act=act,
                                      pool_part=part[:rows * C].view(1, rows, C))

    def raw(B, k, s, C=16, H=2, W=2):
        tiles = Ct.c_int32(-1)
        return lambda: ops._check(ops.lib.spi_op_dwconv_act(ops.PREC[prec], ops._ptr(x), B, H, W, C, k, s, ops._ptr(w),
                                                            ops._ptr(bias), ops.ACT["silu"], ops._ptr(y), ops._ptr(part),
                                                            Ct.byref(tiles), ops._stream(None)))

    shape_msg = "dwconv_act: C a multiple of 8 from 8 to 4608, k 3 or 5, stride 1 or 2"
    for call in (wrapped(12), wrapped(4616), raw(1, 7, 1), raw(1, 3, 3)):
        refused(ops, shape_msg, call, y, part)
    refused(ops, "dwconv_act: act 0 (none) or 3 (silu)", wrapped(16, act="relu"), y, part)
    refused(ops, "dwconv_act: 1 <= B <= 65535, H and W positive", raw(0, 3, 1), y, part)
    assert x[1:].data_ptr() % 16 == x.element_size()
    refused(ops, "dwconv_act: 16-byte aligned x, w_packed, bias and y", wrapped(16, off=1), y, part)
    pack_msg = "dwconv: C a multiple of 8 from 8 to 4608, k 3 or 5"
    refused(ops, pack_msg, lambda: ops.pack_weight_dwconv(prec, np.zeros((12, 1, 3, 3), np.float32)))
    refused(ops, pack_msg, lambda: ops.pack_weight_dwconv(prec, np.zeros((16, 1, 4, 4), np.float32)))
    assert ops.dwconv_tiles(8, 8, 7, 1) == 0 and ops.dwconv_tiles(8, 8, 3, 1) == 1
    wrapped(16)()  # the same buffers are served once the arguments are right
    torch.cuda.synchronize()
    assert not bool(torch.isnan(y[:64]).any()) and not bool(torch.isnan(part[:16]).any())


def test_se_gate_refusals(ops):
    """sq = 0 and 257, C = 12, tiles = 0 (through the library: an empty part has no address)."""
    z = torch.zeros(1 << 15, device="cuda")
    gate = nan(4096)

    def wrapped(C, sq, tiles=1, B=2):
        return lambda: ops.se_gate(z[:B * tiles * C].view(B, tiles, C), 9, z[:sq * C].view(sq, C), z[:sq], z[:C * sq].view(C, sq),
                                   z[:C], gate)

    def raw(C, sq, tiles, B=2):
        p = ops._ptr(z)
        return lambda: ops._check(ops.lib.spi_op_se_gate(p, tiles, 9, p, p, p, p, ops._ptr(gate), B, C, sq, ops._stream(None)))

    shape_msg = "se_gate: C a multiple of 8 from 8 to 4608, 1 <= sq <= 256"
    for call in (raw(16, 0, 1), wrapped(16, 257), wrapped(12, 4)):
        refused(ops, shape_msg, call, gate)
    refused(ops, "se_gate: B, tiles and hw must be positive", raw(16, 4, 0), gate)
    wrapped(16, 4)()
    torch.cuda.synchronize()
    assert bool((gate[:32] == 0.5).all()) and bool(torch.isnan(gate[32:]).all())  # sigmoid(0)


@pytest.mark.parametrize("prec", ["fp16", "fp32"])
def test_scale_channels_refusals(ops, prec):
    """C = 12, and a gate 4 bytes off its 16-byte alignment."""
    x = torch.zeros(2 * 5 * 16, dtype=dt(prec), device="cuda")
    g = torch.zeros(64, device="cuda")
    y = nan(2 * 5 * 16, dt(prec))
    refused(ops, "scale_channels: C a multiple of 8 from 8 to 4608",
            lambda: ops.scale_channels(prec, x[:2 * 5 * 12].view(2, 5, 12), g[:24].view(2, 12), y), y)
    assert g[1:].data_ptr() % 16 == 4
    refused(ops, "scale_channels: 16-byte aligned x, gate and y",
            lambda: ops.scale_channels(prec, x.view(2, 5, 16), g[1:33].view(2, 16), y), y)


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

"""Op-level tests of the HBM-bound kernels of elementwise.hip, pool.hip and layernorm.hip through
include/spi_ops.h: layout ingest,
the max and average pools (fp32, fp16 and the split layout), the BERT embedding (scalar and vector
kernels, with the fused mask bias), mask_to_bias, vit_assemble and gather_rows -- each against the
reference of op_refs.py, which test_op_refs.py holds to the torch op it restates.

Every output buffer carries 8 NaN guard rows that must survive the call.
"""
import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import op_refs as R

pytestmark = pytest.mark.gpu

GUARD = 8
NAN = float("nan")
# Normalised max error bars.  fp32 sums and means: the project's fp32 bar (test_ops_gpu.TOL).
TOL32 = 1e-5
# fp16 outputs of a row op: test_layernorm's fp16 bar (2^-11 output rounding and some).
TOL16 = 1e-3
# fp32 LayerNorm outputs: test_layernorm's fp32 bar.
TOL_LN32 = 2e-6

MEAN = np.float32([0.485, 0.456, 0.406])
STD = np.float32([0.229, 0.224, 0.225])
SCALE = np.float32(1) / (np.float32(255) * STD)
SHIFT = -MEAN / STD


@pytest.fixture(scope="module")
def ops(spi, gpu):
    return importlib.import_module("starpu-inference-server_amd.ops")


def guarded(rows, *tail, dtype=torch.float32):
    return torch.full((rows + GUARD, *tail), NAN, dtype=dtype, device="cuda")


def take(t, rows, what):
    """The first `rows` rows on the host, once the guard rows behind them are seen untouched."""
    torch.cuda.synchronize()
    assert bool(torch.isnan(t[rows:]).all()), f"{what}: rows past the output were written"
    return t[:rows].cpu()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


# ---- ingest -------------------------------------------------------------------------------------


@pytest.mark.parametrize("f16", [False, True], ids=["to_fp32", "to_fp16"])
@pytest.mark.parametrize("kind", ["fp32", "u8_nchw", "u8_nhwc"])
@pytest.mark.parametrize("B,H,W", [(1, 5, 7), (2, 33, 17), (3, 64, 64)])
def test_ingest(ops, B, H, W, kind, f16):
    """Bit-exact against permute + zero-pad; an 8-bit image enters under two fp32 roundings and sits at
    an odd byte address."""
    rng = np.random.default_rng(B * H * W)
    cpad = 8 if f16 else 4  # one 16-byte vector of the compute type, as the model pads the stem's input
    if kind == "fp32":
        img = rng.standard_normal((B, 3, H, W)).astype(np.float32)
        x = dev(img)
    else:
        nhwc = kind == "u8_nhwc"
        u8 = rng.integers(0, 256, (B, H, W, 3) if nhwc else (B, 3, H, W), dtype=np.uint8)
        img = R.xf_image(u8, nhwc, SCALE, SHIFT)
        buf = torch.empty(u8.size + 1, dtype=torch.uint8, device="cuda")
        x = buf[1:].view(u8.shape)
        x.copy_(torch.from_numpy(u8))
        assert x.data_ptr() % 2 == 1
    out = guarded(B * H * W, cpad, dtype=torch.float16 if f16 else torch.float32)
    ops.ingest(kind, x, B, 3, H, W, cpad, out, SCALE, SHIFT)
    got = take(out, B * H * W, "ingest").numpy().reshape(B, H, W, cpad)
    np.testing.assert_array_equal(got, R.ingest_ref(img, cpad, f16))


def test_ingest_more_channels(ops):
    """C > 3 (fp32 source only) and C == cpad: no padding lane."""
    img = np.random.default_rng(0).standard_normal((2, 8, 6, 5)).astype(np.float32)
    out = guarded(2 * 6 * 5, 8)
    ops.ingest("fp32", dev(img), 2, 8, 6, 5, 8, out)
    np.testing.assert_array_equal(take(out, 60, "ingest").numpy().reshape(2, 6, 5, 8), R.ingest_ref(img, 8, False))


# ---- max pool -----------------------------------------------------------------------------------

POOL_SHAPES = [(1, 5, 5, 8), (2, 9, 7, 64), (3, 112, 112, 64), (1, 113, 57, 32)]
POOL_GEO = [(3, 2, 1), (2, 2, 0)]


def pool_input(B, H, W, C):
    return torch.from_numpy(np.random.default_rng(B + H * W + C).standard_normal((B, H, W, C)).astype(np.float32))


def torch_maxpool(x_nhwc, k, stride, pad):
    return F.max_pool2d(x_nhwc.permute(0, 3, 1, 2), k, stride, pad).permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("k,stride,pad", POOL_GEO)
@pytest.mark.parametrize("B,H,W,C", POOL_SHAPES)
def test_maxpool(ops, B, H, W, C, k, stride, pad, prec):
    x = pool_input(B, H, W, C).to(ops.act_dtype(prec))
    ref = torch_maxpool(x.float(), k, stride, pad)  # a max is exact: equal in either type
    OH, OW = ops.pool_out(H, W, k, stride, pad)
    assert ref.shape == (B, OH, OW, C)
    out = guarded(B * OH * OW, C, dtype=x.dtype)
    ops.maxpool(prec, x.cuda(), B, H, W, C, k, stride, pad, out)
    got = take(out, B * OH * OW, "maxpool").float().reshape(B, OH, OW, C)
    assert torch.equal(got, ref)


@pytest.mark.parametrize("k,stride,pad", POOL_GEO)
@pytest.mark.parametrize("B,H,W,C", [s for s in POOL_SHAPES if s[3] % 32 == 0])
def test_maxpool_split(ops, B, H, W, C, k, stride, pad):
    """Raw comparison: the output bits are to_split(max of the values the split input holds)."""
    s = ops.to_split(pool_input(B, H, W, C) * 3)
    ref = ops.to_split(torch_maxpool(ops.from_split(s), k, stride, pad))
    OH, OW = ops.pool_out(H, W, k, stride, pad)
    out = guarded(B * OH * OW, C)
    ops.maxpool("fp16x3s", s.cuda(), B, H, W, C, k, stride, pad, out)
    got = take(out, B * OH * OW, "maxpool split").reshape(B, OH, OW, C)
    assert same_bits(got, ref)


# ---- average pool -------------------------------------------------------------------------------

# (2, 81, 2048) in fp32 is 512 16-byte channel vectors per pixel: avgpool_kernel's CV > 256 branch, one
# thread per vector looping over the pixels (C / 4 = 512 > 256; the fp16 forms have C / 8 = 256 and stay
# on the LDS branch).  (2, 100, 8): CV = 1 in fp16, 2 in fp32.  (5, 64, 96): 256 % CV != 0, idle threads.
AVG_SHAPES = [(1, 1, 32), (3, 49, 512), (2, 81, 2048), (5, 64, 96), (2, 100, 8)]


# the split layout holds whole 32-channel blocks: no split form of C = 8 (its rejection: test_pool_rejections)
AVG_CASES = [(*s, m) for s in AVG_SHAPES for m in ("fp32", "fp16", "fp16_to_fp32", "split") if m != "split" or s[2] % 32 == 0]


@pytest.mark.parametrize("B,HW,C,mode", AVG_CASES)
def test_avgpool(ops, B, HW, C, mode):
    x = torch.from_numpy(np.random.default_rng(B * HW + C).standard_normal((B, HW, C)).astype(np.float32)) + 0.5
    if mode == "split":
        xin = ops.to_split(x)
        held, prec, odt = ops.from_split(xin), "fp16x3s", torch.float32
    elif mode == "fp32":
        xin, held, prec, odt = x, x, "fp32", torch.float32
    else:
        xin = x.half()
        held, prec, odt = xin, "fp16", torch.float16 if mode == "fp16" else torch.float32
    ref = R.avgpool_ref(held.double().numpy())  # the float64 mean of the values the layout holds
    out = guarded(B, C, dtype=odt)
    ops.avgpool(prec, xin.cuda(), B, HW, C, out)
    e = R.nerr(take(out, B, "avgpool").double().numpy(), ref)
    print(f"avgpool {mode} {B}x{HW}x{C}: {e:.3e}")
    assert e < (TOL16 if mode == "fp16" else TOL32)


def test_pool_rejections(ops):
    """C not a multiple of the 16-byte vector: each pool refuses (it would drop the trailing channels)."""
    for prec, C, dt in (("fp32", 6, torch.float32), ("fp16", 12, torch.float16), ("fp16x3s", 48, torch.float32)):
        x = torch.zeros(2, 6, 6, C, dtype=dt, device="cuda")
        y = torch.zeros(2 * 36 + GUARD, C, dtype=torch.float32, device="cuda")  # room for either pool's output
        with pytest.raises(ops.OpError):
            ops.maxpool(prec, x, 2, 6, 6, C, 3, 2, 1, y)
        with pytest.raises(ops.OpError):
            ops.avgpool(prec, x, 2, 36, C, y)
    x = torch.zeros(2, 6, 6, 32, device="cuda")
    with pytest.raises(ops.OpError):
        ops.maxpool("fp32", x, 2, 6, 6, 32, 3, 2, 3, torch.zeros(2 * 36 + GUARD, 32, device="cuda"))  # pad >= k


# ---- BERT embedding -----------------------------------------------------------------------------

VOCAB, NPOS = 50, 128


def embed_tables(D):
    rng = np.random.default_rng(D)
    word = rng.standard_normal((VOCAB, D)).astype(np.float32)
    pos = (0.5 * rng.standard_normal((NPOS, D))).astype(np.float32)
    type0, beta = (0.3 * rng.standard_normal(D)).astype(np.float32), rng.standard_normal(D).astype(np.float32)
    gamma = (1 + 0.3 * rng.standard_normal(D)).astype(np.float32)
    return word, pos, type0, gamma, beta


def embed_ids(B, S):
    """Ids with both ends of the table and three that the kernel clamps: -1 -> 0, vocab and 2^40 -> vocab - 1."""
    ids = np.random.default_rng(B * S).integers(0, VOCAB, B * S)
    edge = np.int64([-1, VOCAB, 2 ** 40, 0, VOCAB - 1])[:B * S]
    ids[:edge.size] = edge
    return ids.astype(np.int64)


def run_embed(ops, prec, B, S, D, yt_offset=0, with_yt=True):
    word, pos, type0, gamma, beta = embed_tables(D)
    ids = embed_ids(B, S)
    M = B * S
    mask = (np.arange(M) % 3 != 1).astype(np.int64)  # zeros among the ones
    ref = R.bert_embed_ref(ids, word, pos, type0, gamma, beta, S, R.EPS)
    ydt = torch.float16 if prec == "fp16" else torch.float32
    yf, mb = guarded(M, D), guarded(M)
    flat = torch.full(((M + GUARD) * D + yt_offset,), NAN, dtype=ydt, device="cuda")
    yt = flat[yt_offset:].view(M + GUARD, D)
    ops.bert_embed(prec, dev(ids), dev(word), dev(pos), dev(type0), dev(gamma), dev(beta), yf, yt if with_yt else None,
                   B, S, D, R.EPS, mask=dev(mask), mask_bias=mb)
    what = f"bert_embed {prec} B{B} S{S} D{D}"
    ef = R.nerr(take(yf, M, what).numpy(), ref)
    print(f"{what}: yf {ef:.3e}")
    assert ef < TOL_LN32, f"{what}: yf {ef:.3e}"
    np.testing.assert_array_equal(take(mb, M, what).numpy(), R.mask_to_bias_ref(mask))
    if with_yt:
        et = R.nerr(take(yt, M, what).double().numpy(), ref)
        print(f"{what}: yt {et:.3e}")
        assert et < (TOL16 if prec == "fp16" else TOL_LN32), f"{what}: yt {et:.3e}"
    else:
        assert bool(torch.isnan(flat).all())


# D 64, 200, 256, 1000: the scalar kernel; 768 and 1024: the vector kernel (NV = 3 and 4).  (3, 7) is 21
# rows: a ragged last block of 4 rows.
@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("B,S", [(1, 1), (3, 7), (2, 128)])
@pytest.mark.parametrize("D", [64, 200, 256, 1000, 768, 1024])
def test_bert_embed(ops, D, B, S, prec):
    run_embed(ops, prec, B, S, D)


def test_bert_embed_unaligned_yt_takes_the_scalar_kernel(ops):
    """yt off 8-byte alignment at D = 768: the vector kernel's 8-byte stores cannot run; same bars."""
    run_embed(ops, "fp16", 3, 7, 768, yt_offset=2)


def test_bert_embed_without_yt(ops):
    run_embed(ops, "fp16", 3, 7, 768, with_yt=False)
    run_embed(ops, "fp32", 3, 7, 200, with_yt=False)


def test_bert_embed_rejections(ops):
    """yf is required -- both kernels store every row through it (the scalar one offsets the pointer before it
    tests it, the vector one never tests it), and the model always passes it -- as are D <= 1024 and
    S <= npos.  Buffers sized for the nominal shape."""
    def call(B, S, D, yf=True, npos=NPOS, mask=False, mask_bias=False):
        M = B * S
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device="cuda")  # noqa: E731
        with pytest.raises(ops.OpError):
            ops.bert_embed("fp16", z(M, dt=torch.int64), z(VOCAB, D), z(max(npos, S), D), z(D), z(D), z(D),
                           z(M, D) if yf else None, z(M, D, dt=torch.float16), B, S, D, R.EPS,
                           mask=z(M, dt=torch.int64) if mask else None, mask_bias=z(M) if mask_bias else None,
                           npos=npos)

    call(2, 8, 768, yf=False)   # the vector kernel's case
    call(2, 8, 200, yf=False)   # the scalar kernel's
    call(2, 8, 1088)            # D past the 16 values a lane holds
    call(1, 129, 64)            # S > npos
    call(2, 8, 64, mask=True)   # mask without mask_bias
    call(2, 8, 64, mask_bias=True)


# ---- mask_to_bias, vit_assemble, gather_rows ----------------------------------------------------


@pytest.mark.parametrize("n", [1, 21, 4099])
def test_mask_to_bias(ops, n):
    mask = np.random.default_rng(n).integers(-1, 3, n).astype(np.int64)  # any non-zero keeps the key
    out = guarded(n)
    ops.mask_to_bias(dev(mask), out, n)
    np.testing.assert_array_equal(take(out, n, "mask_to_bias").numpy(), R.mask_to_bias_ref(mask))


@pytest.mark.parametrize("B,P,D", [(1, 4, 64), (3, 196, 128), (2, 9, 1000)])
def test_vit_assemble(ops, B, P, D):
    rng = np.random.default_rng(B * P + D)
    patches, cls, pos = (rng.standard_normal(s).astype(np.float32) for s in ((B, P, D), (D,), (P + 1, D)))
    out = guarded(B * (P + 1), D)
    ops.vit_assemble(dev(patches), dev(cls), dev(pos), out, B, P, D)
    got = take(out, B * (P + 1), "vit_assemble").numpy().reshape(B, P + 1, D)
    np.testing.assert_array_equal(got, R.vit_assemble_ref(patches, cls, pos))


@pytest.mark.parametrize("f16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("rows,stride,D", [(7, 1, 200), (4, 5, 64), (3, 197, 768)])
def test_gather_rows(ops, rows, stride, D, f16):
    x = np.random.default_rng(rows * stride + D).standard_normal(((rows - 1) * stride + 1, D)).astype(np.float32)
    out = guarded(rows, D, dtype=torch.float16 if f16 else torch.float32)
    ops.gather_rows(dev(x), out, rows, stride, D)
    np.testing.assert_array_equal(take(out, rows, "gather_rows").numpy(), R.gather_rows_ref(x, rows, stride, f16))

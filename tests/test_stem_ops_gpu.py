"""Op-level parity of the fused stem (csrc/stem.hip) through spi_op_stem_pool / spi_op_stem_pool_u8: every
(PR, NW) form x precision code x source at small shapes, against a float64 conv + bias + ReLU + max pool on the
values the kernel multiplies (op_refs.stem_operands).

Bars: 1e-5 normalised max error into the split output (code 3), 1e-3 into fp16 (codes 1, 2, 4).  What a parity
bar cannot hold is held by equalities that follow from the code:
  * the three rows_per_block settings give the same bits -- a stem row's accumulation order does not depend on
    PR or NW and max is exact; on random data this pins the 4-wave carry across the 64-column boundary, the
    8-wave exchange through LDS and the short last workgroup against each other;
  * code 4 (fp16x3) stores the hi halves of code 3 (fp16x3s): the same arithmetic, another store;
  * the u8 NCHW / NHWC sources give the bits of the fp32 source on op_refs.xf_image of the pixels;
  * on the exact lattice (op_refs.stem_lattice_case) every instance gives the float64 value rounded once, bit
    for bit -- the lo-weight variant at fp16m shows a dropped lo MFMA, which 1e-3 cannot.
Every output has GUARD NaN rows behind it that must survive.  test_op_refs.test_stem_cases_discriminate shows on
these inputs that a kernel missing the group boundary's left neighbour, a workgroup's recomputed row, a lo half,
the kw = 6 tap, an odd W's last column, or padding with shift[c], sits more than 10x above the bar.

Which shape (B, H, W) reaches which edge (OW stem columns, PH x PW pooled; rows_per_block 0 runs PR = 2 on 8
waves when OW > 64, else PR = 1 on 4 waves; 1 / 2 run PR = 1 / 2 on 4 waves, two groups walked with the carry):
  (1, 1, 1)     one pixel: OW = PH = PW = 1; under PR = 2 the workgroup's five stem rows hold one inside the map
  (3, 9, 7)     OW 4; odd 3 H W: images 2 and 3 start off 16 bytes; PH 3: the last PR = 2 workgroup stores one row
  (1, 2, 8)     H 2: OH 1, PH 1 under PR = 2; W 8 even, OW 4
  (1, 10, 47)   OW 24, PW 12, one partial group
  (3, 11, 127)  OW 64: group 0 exactly full, odd image starts
  (1, 13, 128)  OW 64, PH 4 (even)
  (1, 2, 129)   OW 65: a second group of ONE column, PH 1 on the 8-wave PR = 2 form, PW 33 odd
  (3, 9, 131)   OW 66: a second group of two columns, PH 3 odd on the 8-wave form, odd image starts
  (1, 23, 130)  OW 65 with PH 6
  (1, 11, 132)  OW 66 even, PH 3
  (1, 13, 190)  OW 95 odd, PW 48 even
  (1, 10, 221)  OW 111, PW 56
  (3, 1, 223)   OW 112 (the widest) at H 1: every workgroup's rows but one outside the map; odd image starts
  (1, 40, 222)  the tall case: PH 10, five / ten workgroups per image
  (1, 23, 224)  the model's width, PH 6
Images are N(0, 1) or U[0, 1) by shape; the u8 images pass through the ImageNet transform (signed values).

Worst normalised max errors measured on an MI355X over test_stem_parity (each case prints its own): fp16 4.3e-4
((1, 2, 8), transformed pixels), fp16m 4.3e-4 ((3, 9, 131)), fp16x3 4.1e-4 ((1, 10, 221)) against the 1e-3 bar --
an fp16 output's half ulp is 2.4e-4 to 4.9e-4 of the largest element -- and fp16x3s 4.0e-7 ((3, 9, 7)) against 1e-5.
Every equality held at every shape.
"""
import importlib

import numpy as np
import pytest
import torch

import op_refs as R
from oracle.cpu_codelet import normalized_max_error

pytestmark = pytest.mark.gpu

GUARD = 8
NAN = float("nan")
PRECS = ("fp16", "fp16m", "fp16x3s", "fp16x3")
SOURCES = ("f32", "nchw", "nhwc")


@pytest.fixture(scope="module")
def ops(spi, gpu):
    return importlib.import_module("starpu-inference-server_amd.ops")


def bits(a):
    return np.ascontiguousarray(a).view(np.int16)


def values(code, o):
    return R.stem_from_split(o) if code == 3 else o.astype(np.float64)


def run(ops, prec, src, img, w, b_d, rows, shape, scale=None, shift=None):
    """One launch into a NaN buffer with GUARD rows behind the output; returns the fp16 array
    [B][PH][PW][64] ([..][128]: the split layout of code 3).  src "f32": img fp32 NCHW tensor; "nchw" /
    "nhwc": a uint8 device tensor."""
    B, H, W = shape
    _, _, PH, PW = R.stem_out_hw(H, W)
    n, width = B * PH * PW, 128 if prec == "fp16x3s" else 64
    buf = torch.full((n + GUARD, width), NAN, dtype=torch.float16, device="cuda")
    out = buf[:n].view(B, PH, PW, width)
    if src == "f32":
        ops.stem_pool(prec, img, w, b_d, rows_per_block=rows, out=out)
    else:
        ops.stem_pool_u8(prec, img, w, b_d, scale, shift, nhwc=src == "nhwc", rows_per_block=rows, out=out)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert np.isnan(got[n:]).all(), f"{prec} {src} rows={rows} {shape}: rows past the map were written"
    assert not np.isnan(got[:n]).any(), f"{prec} {src} rows={rows} {shape}: an output element was left unwritten"
    return got[:n].reshape(B, PH, PW, width)


def u8_tensors(u8):
    return {"nchw": torch.from_numpy(u8).cuda(),
            "nhwc": torch.from_numpy(np.ascontiguousarray(u8.transpose(0, 2, 3, 1))).cuda()}


def offset_by_one(t):
    """The same bytes on the device one byte past an aligned address."""
    buf = torch.empty(t.numel() + 1, dtype=torch.uint8, device="cuda")
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 1 and view.is_contiguous()
    return view


@pytest.mark.parametrize("B,H,W,kind", R.STEM_SHAPES, ids=[f"{s[0]}x{s[1]}x{s[2]}" for s in R.STEM_SHAPES])
def test_stem_parity(ops, B, H, W, kind):
    """Every precision x rows_per_block x source at one shape: parity with float64 on a signed fp32 image and on
    the transformed 8-bit one, the same bits from the three (PR, NW) forms and from the three sources, code 4 =
    the hi halves of code 3, guards intact."""
    shape = (B, H, W)
    OW = R.stem_out_hw(H, W)[1]
    x, u8, w, b = R.stem_case(B, H, W, kind)
    xu = R.xf_image(u8, False, R.STEM_SCALE, R.STEM_SHIFT)
    b_d = torch.from_numpy(b).cuda()
    imgs = {"x": torch.from_numpy(x).cuda(), "xu": torch.from_numpy(xu).cuda()}
    pix = u8_tensors(u8)
    assert {R.stem_form(r, OW) for r in (0, 1, 2)} == ({(2, 8), (1, 4), (2, 4)} if OW > 64 else {(1, 4), (2, 4)})
    refs, kept = {}, {}
    for prec in PRECS:
        code = R.STEM_CODES[prec]
        outs = {}
        for rows in (0, 1, 2):
            of = run(ops, prec, "f32", imgs["x"], w, b_d, rows, shape)
            ou = run(ops, prec, "f32", imgs["xu"], w, b_d, rows, shape)
            for src in ("nchw", "nhwc"):
                o8 = run(ops, prec, src, pix[src], w, b_d, rows, shape, scale=R.STEM_SCALE, shift=R.STEM_SHIFT)
                assert np.array_equal(bits(o8), bits(ou)), f"{prec} rows={rows} {shape}: u8 {src} != fp32 source"
            outs[rows] = (of, ou)
        for rows in (1, 2):
            for i, name in enumerate(("randn / rand image", "transformed pixels")):
                assert np.array_equal(bits(outs[rows][i]), bits(outs[0][i])), \
                    f"{prec} {shape} {name}: form {R.stem_form(rows, OW)} differs from {R.stem_form(0, OW)}"
        for i, (name, img) in enumerate((("x", x), ("xu", xu))):
            key = (name, min(code, 3))
            if key not in refs:
                refs[key] = R.stem_ref(*R.stem_operands(code, img, w), b)
            e = normalized_max_error(values(code, outs[0][i]), refs[key])
            print(f"stem {prec} {shape} {name}: {e:.3e}")
            assert e < R.STEM_BAR[code], f"stem {prec} {shape} {name}: {e:.3e}"
        kept[code] = outs[0]
    for i in range(2):
        assert np.array_equal(bits(R.stem_hi_of_split(kept[3][i])), bits(kept[4][i])), \
            f"{shape}: fp16x3 is not the hi half of fp16x3s"


@pytest.mark.parametrize("variant", ["mixed", "lowt"])
@pytest.mark.parametrize("B,H,W", R.STEM_LATTICE_SHAPES)
def test_stem_exact_lattice(ops, B, H, W, variant):
    """Every product and partial sum exact in fp32: each of the 36 instances gives the float64 value (from the
    three products the kernel forms) rounded once, bit for bit.  fp32 source: integers + a lo part; u8 sources:
    the integers under the default transform.  "lowt": hi weights summing to zero over a constant image, so
    the interior is bias + 4 sum(lo) -- at fp16m a dropped lo MFMA changes the stored bits."""
    shape = (B, H, W)
    xi, x, w, b = R.stem_lattice_case(B, H, W, variant)
    b_d = torch.from_numpy(b).cuda()
    x_d, pix = torch.from_numpy(x).cuda(), u8_tensors(xi)
    for prec in PRECS:
        code = R.STEM_CODES[prec]
        want = {"f32": R.stem_expected_bits(code, R.stem_lattice_ref(code, x, w, b))}
        want["nchw"] = want["nhwc"] = R.stem_expected_bits(code, R.stem_lattice_ref(code, xi.astype(np.float32), w, b))
        for rows in (0, 1, 2):
            for src in SOURCES:
                got = run(ops, prec, src, x_d if src == "f32" else pix[src], w, b_d, rows, shape)
                assert np.array_equal(bits(got), bits(want[src])), \
                    f"{variant} {prec} {src} rows={rows} {shape}: {(bits(got) != bits(want[src])).sum()} elements differ"


def test_stem_all_zero_under_a_very_negative_bias(ops):
    """bias = -1000: every pre-activation is negative, every output must be +0 (not -0, not a leftover)."""
    shape = (3, 9, 131)
    x, u8, w, _ = R.stem_case(*shape, "randn")
    b_d = torch.full((64,), -1000.0, device="cuda")
    x_d, pix = torch.from_numpy(x).cuda(), u8_tensors(u8)
    for prec in PRECS:
        for rows in (0, 1, 2):
            for src in SOURCES:
                got = run(ops, prec, src, x_d if src == "f32" else pix[src], w, b_d, rows, shape,
                          scale=R.STEM_SCALE, shift=R.STEM_SHIFT)
                assert not bits(got).any(), f"{prec} {src} rows={rows}: an output is not +0"


@pytest.mark.parametrize("src", ["nchw", "nhwc"])
def test_stem_u8_one_byte_past_alignment(ops, src):
    """The 8-bit image one byte past a 16-byte boundary, two groups wide, odd rows and image starts."""
    shape = (3, 9, 131)
    _, u8, w, b = R.stem_case(*shape, "randn")
    b_d = torch.from_numpy(b).cuda()
    pix = u8_tensors(u8)[src]
    for prec in PRECS:
        for rows in (0, 2):
            want = run(ops, prec, src, pix, w, b_d, rows, shape, scale=R.STEM_SCALE, shift=R.STEM_SHIFT)
            got = run(ops, prec, src, offset_by_one(pix), w, b_d, rows, shape, scale=R.STEM_SCALE, shift=R.STEM_SHIFT)
            assert np.array_equal(bits(got), bits(want)), f"{prec} {src} rows={rows}"


@pytest.mark.parametrize("W", R.STEM_REFUSED_W)
def test_stem_refuses_wider_than_224(ops, W):
    """OW = 113 is past the kernel's planes: refused with the message, before any launch (the buffer keeps its
    NaNs)."""
    H = 9
    _, _, PH, PW = R.stem_out_hw(H, W)
    b_d = torch.zeros(64, device="cuda")
    w = np.zeros((64, 3, 7, 7), np.float32)
    for src in SOURCES:
        img = torch.zeros(1, 3, H, W, device="cuda") if src == "f32" else \
            torch.zeros((1, H, W, 3) if src == "nhwc" else (1, 3, H, W), dtype=torch.uint8, device="cuda")
        buf = torch.full((PH * PW + GUARD, 64), NAN, dtype=torch.float16, device="cuda")
        with pytest.raises(ops.OpError, match="wider than 224"):
            if src == "f32":
                ops.stem_pool("fp16", img, w, b_d, out=buf)
            else:
                ops.stem_pool_u8("fp16", img, w, b_d, nhwc=src == "nhwc", out=buf)
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf).all())

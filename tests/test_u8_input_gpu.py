"""8-bit image tasks on the device: the kernels that read the task's buffer (fused stem, layout
ingest, ViT patchify) load bytes and apply the per-channel input transform at that load.

Everything downstream of that load is the code an fp32 task runs, so the checks are equalities:
a u8 input must give bit for bit what the same entry point gives on the "host image"
x_u8.astype(float32) * scale + shift (float32 numpy: one rounded multiply, one rounded add; NCHW,
after a transpose for NHWC inputs).  The ImageNet transform has three distinct non-zero shifts: a
swapped channel, a padding pixel entering as shift[c] instead of 0, or a multiply-add contracted
into an FMA (which changes about half of the values) all break the equality."""
import importlib

import numpy as np
import pytest
import torch

from oracle.cpu_codelet import cpu_inference, normalized_max_error

pytestmark = pytest.mark.gpu

MEAN = np.float32([0.485, 0.456, 0.406])
STD = np.float32([0.229, 0.224, 0.225])
SCALE = np.float32(1) / (np.float32(255) * STD)
SHIFT = -MEAN / STD
UNIT_SCALE = np.float32([1, 1, 1]) / np.float32(255)
ZERO = np.float32([0, 0, 0])


def host_image(x_u8, nhwc, scale=SCALE, shift=SHIFT):
    x = np.ascontiguousarray(x_u8.transpose(0, 3, 1, 2)) if nhwc else x_u8
    return x.astype(np.float32) * scale.reshape(1, 3, 1, 1) + shift.reshape(1, 3, 1, 1)


def pixels(seed, b, h, w, nhwc):
    shape = (b, h, w, 3) if nhwc else (b, 3, h, w)
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def offset_by_one(x_u8):
    """The same pixels on the device, starting one byte into their allocation (odd address)."""
    buf = torch.empty(x_u8.size + 1, dtype=torch.uint8, device="cuda")
    view = buf[1:].view(x_u8.shape)
    view.copy_(torch.from_numpy(x_u8))
    assert view.data_ptr() % 2 == 1 and view.is_contiguous()
    return view


def same_bits(a, b):
    """Raw equality (the split layout keeps fp16 pairs in float32 storage: compare the halves)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


@pytest.fixture(scope="module")
def ops(spi, gpu):
    return importlib.import_module("starpu-inference-server_amd.ops")


# ---- 1. the fused stem --------------------------------------------------------------------------

STEM_SHAPES = [(3, 64, 64, 0), (1, 65, 47, 0), (2, 33, 17, 2), (1, 9, 9, 0), (2, 223, 224, 1), (1, 224, 224, 0)]


def stem_weights(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(64, 3, 7, 7, generator=g) * 0.1, (torch.randn(64, generator=g) * 0.1).cuda()


@pytest.mark.parametrize("nhwc", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("prec", ["fp16", "fp16m", "fp16x3s", "fp16x3"])
@pytest.mark.parametrize("B,H,W,rows", STEM_SHAPES)
def test_stem_pool_u8_equals_fp32_on_host_image(ops, prec, B, H, W, rows, nhwc):
    """The fused-stem test's shapes (odd row starts at 65x47, odd image starts at 33x17, a last
    workgroup short of rows, the 8-wave two-group form at 224)."""
    w, b = stem_weights(B * 1000 + H * 10 + W + rows)
    x = pixels(H * W + B, B, H, W, nhwc)
    ref = ops.stem_pool(prec, torch.from_numpy(host_image(x, nhwc)).cuda(), w, b, rows_per_block=rows)
    got = ops.stem_pool_u8(prec, torch.from_numpy(x).cuda(), w, b, SCALE, SHIFT, nhwc=nhwc, rows_per_block=rows)
    torch.cuda.synchronize()
    assert ref.float().abs().max() > 0
    assert same_bits(got, ref)


@pytest.mark.parametrize("nhwc", [False, True], ids=["nchw", "nhwc"])
def test_stem_pool_u8_odd_base_address(ops, nhwc):
    w, b = stem_weights(7)
    x = pixels(8, 2, 64, 64, nhwc)
    ref = ops.stem_pool("fp16m", torch.from_numpy(host_image(x, nhwc)).cuda(), w, b)
    got = ops.stem_pool_u8("fp16m", offset_by_one(x), w, b, SCALE, SHIFT, nhwc=nhwc)
    torch.cuda.synchronize()
    assert same_bits(got, ref)


def test_stem_pool_u8_default_transform_is_a_cast(ops):
    w, b = stem_weights(9)
    x = torch.from_numpy(pixels(10, 2, 64, 64, False)).cuda()
    ref = ops.stem_pool("fp16x3", x.float(), w * 0.01, b)
    got = ops.stem_pool_u8("fp16x3", x, w * 0.01, b)
    torch.cuda.synchronize()
    assert same_bits(got, ref)


# ---- 2. patchify --------------------------------------------------------------------------------

def unfold(img, ps):
    """[B][3][H][W] -> [B GH GW][3 ps ps], column c ps ps + kh ps + kw."""
    B, C, H, W = img.shape
    return np.ascontiguousarray(img.reshape(B, C, H // ps, ps, W // ps, ps).transpose(0, 2, 4, 1, 3, 5)).reshape(
        B * (H // ps) * (W // ps), C * ps * ps)


@pytest.mark.parametrize("out_f16", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("B,H,W,ps,odd", [(2, 32, 32, 16, False), (1, 28, 42, 14, False), (3, 48, 32, 8, False),
                                          (3, 48, 32, 8, True)])
def test_patchify_u8(ops, B, H, W, ps, odd, out_f16):
    """Pure data movement: scalar (ps 14) and vector kernels, the 8-byte loads (aligned NCHW, W % 8 == 0)
    and their byte-load fallback (odd base), exact against the fp32 source and a numpy unfold."""
    for nhwc in (False, True):
        x = pixels(H + W + ps, B, H, W, nhwc)
        img = host_image(x, nhwc)
        want = unfold(img, ps).astype(np.float16 if out_f16 else np.float32)
        ref = ops.patchify("fp32", torch.from_numpy(img).cuda(), ps, out_f16=out_f16)
        xd = offset_by_one(x) if odd else torch.from_numpy(x).cuda()
        got = ops.patchify("u8_nhwc" if nhwc else "u8_nchw", xd, ps, SCALE, SHIFT, out_f16=out_f16)
        torch.cuda.synchronize()
        assert np.array_equal(ref.cpu().numpy(), want)
        assert np.array_equal(got.cpu().numpy(), want), f"nhwc={nhwc}"


# ---- 3. models: one replica, graphs on, u8 and fp32 tasks interleaved -----------------------------

_models = {}


def model(zoo, key):
    if key not in _models:
        kind, image, patch = key
        _models[key] = (zoo.resnet18(image=image) if kind == "resnet" else
                        zoo.vit(image=image, patch=patch, layers=2, heads=4, dim=256, mlp_dim=512))
    return _models[key]


def forward(spi, rep, x, batch, stream):
    out = torch.full((batch, 1000), float("nan"), device="cuda")
    spi.run_hip(rep, [x], out, stream=stream.cuda_stream)
    return out.cpu().numpy()


def interleaved(spi, rep, x_u8, nhwc, scale=SCALE, shift=SHIFT):
    """u8, fp32, u8, fp32 on one stream of one replica; returns (u8 output, fp32-input output)."""
    rep.set_input_transform(scale, shift)
    xu = torch.from_numpy(x_u8).cuda()
    xf = torch.from_numpy(host_image(x_u8, nhwc, scale, shift)).cuda()
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    outs = [forward(spi, rep, x, x_u8.shape[0], stream) for x in (xu, xf, xu, xf)]
    assert all(np.isfinite(o).all() for o in outs)
    assert np.array_equal(outs[0], outs[2]) and np.array_equal(outs[1], outs[3])
    return outs[0], outs[1]


@pytest.mark.parametrize("nhwc", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("prec,fused", [("fp32", True), ("fp16", True), ("fp16m", True), ("fp16x3", True),
                                        ("fp16", False)])
def test_resnet18_u8_equals_fp32_input(spi, zoo, gpu, monkeypatch, prec, fused, nhwc):
    """fp32 runs the layout ingest, the others the fused stem; SPI_STEM_FUSED=0 the ingest in fp16."""
    if not fused:
        monkeypatch.setenv("SPI_STEM_FUSED", "0")
    rep = spi.ModelReplica(model(zoo, ("resnet", 64, 0)), 0, prec, max_batch=3, image_size=64, graphs=True)
    u8, f32 = interleaved(spi, rep, pixels(11, 3, 64, 64, nhwc), nhwc)
    assert np.array_equal(u8, f32)


def test_resnet18_224_u8_equals_fp32_input(spi, zoo, gpu):
    rep = spi.ModelReplica(model(zoo, ("resnet", 224, 0)), 0, "fp16m", max_batch=1, graphs=True)
    u8, f32 = interleaved(spi, rep, pixels(12, 1, 224, 224, True), True)
    assert np.array_equal(u8, f32)


@pytest.mark.parametrize("nhwc", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("prec,image,patch", [("fp32", 160, 16), ("fp16", 160, 16), ("fp16", 224, 14)])
def test_vit_u8_equals_fp32_input(spi, zoo, gpu, prec, image, patch, nhwc):
    rep = spi.ModelReplica(model(zoo, ("vit", image, patch)), 0, prec, max_batch=2, image_size=image, graphs=True)
    u8, f32 = interleaved(spi, rep, pixels(13, 2, image, image, nhwc), nhwc)
    assert np.array_equal(u8, f32)


# ---- 4. against the CPU oracle ------------------------------------------------------------------

@pytest.mark.parametrize("kind,prec,image,batch", [("resnet", "fp16m", 224, 2), ("vit", "fp16", 160, 2)])
def test_u8_nhwc_oracle_parity(spi, zoo, gpu, kind, prec, image, batch):
    """Pixels scaled into [0, 1] (scale 1/255, shift 0: the range the project's bars were measured on)
    at the fp16 / fp16m bar of 1e-3 with top-1 agreement.  The ImageNet-normalised image is signed,
    a range the bars were never measured on: its error is printed, not gated."""
    m = model(zoo, (kind, image, 16 if kind == "vit" else 0))
    rep = spi.ModelReplica(m, 0, prec, max_batch=batch, image_size=image, graphs=True)
    x = pixels(0, batch, image, image, True)
    got, _ = interleaved(spi, rep, x, True, UNIT_SCALE, ZERO)
    ref = cpu_inference(m, [host_image(x, True, UNIT_SCALE, ZERO)])[0]
    err = normalized_max_error(got, ref)
    got_n, _ = interleaved(spi, rep, x, True)
    ref_n = cpu_inference(m, [host_image(x, True)])[0]
    err_n = normalized_max_error(got_n, ref_n)
    print(f"u8 nhwc {kind} {prec} @{image} bs{batch}: err [0,1] {err:.3e}, ImageNet-normalised {err_n:.3e} "
          f"(top-1 {'agrees' if (got_n.argmax(1) == ref_n.argmax(1)).all() else 'differs'})")
    assert err < 1e-3, err
    assert (got.argmax(1) == ref.argmax(1)).all()


# ---- 5. through the mini-runtime ----------------------------------------------------------------

@pytest.mark.parametrize("h2d", ["auto", "worker_sdma"])
def test_runtime_u8_jobs(spi, zoo, gpu, h2d):
    rtmod = importlib.import_module("starpu-inference-server_amd.runtime")
    rep = spi.ModelReplica(model(zoo, ("resnet", 64, 0)), 0, "fp16m", max_batch=8, image_size=64, graphs=True)
    rep.set_input_transform(SCALE, SHIFT)
    rt = rtmod.Runtime([rep], [((3, 64, 64), np.uint8)], [(1000, np.float32)], max_batch=8, workers_per_device=4,
                       pipeline_depth=2, h2d_mode=h2d, warmup_batches=-1)
    print(f"u8 runtime h2d_mode {h2d} -> {rt.h2d_mode}")
    jobs = []
    for rid in range(32):
        x = pixels(100 + rid, 8, 64, 64, False)
        y = np.full((8, 1000), np.nan, dtype=np.float32)
        rt.submit(rid, [x], [y])
        jobs.append((x, y))
    rt.drain()
    assert rt.stats() == (32, 0)
    rt.close()
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    for x, y in jobs:
        ref = forward(spi, rep, torch.from_numpy(host_image(x, False)).cuda(), 8, stream)
        assert np.array_equal(y, ref)

"""Resize + centre crop of 8-bit image tasks on the device (spi_model_set_input_resize, resample.hip).

The device op is held to ATen's float64 resample (resize_refs.py) within 255 (Kx + Ky + 4) 2^-24 pixel
levels.  Behind the resample a forward is the fp32-source code an fp32 task runs, so the model-level checks
are equalities: a resized task must give bit for bit what an fp32 task holding ops.resize_crop_u8's output
gives, and an S x S task at R = S what the plain 8-bit task of a replica without the resize gives."""
import importlib

import numpy as np
import pytest
import torch

import resize_refs as R
from oracle.cpu_codelet import cpu_inference, normalized_max_error

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(spi, gpu):
    return importlib.import_module("starpu-inference-server_amd.ops")


def offset_by_one(x_u8):
    """The same pixels on the device, starting one byte into their allocation (odd address)."""
    buf = torch.empty(x_u8.size + 1, dtype=torch.uint8, device="cuda")
    view = buf[1:].view(x_u8.shape)
    view.copy_(torch.from_numpy(x_u8))
    assert view.data_ptr() % 2 == 1 and view.is_contiguous()
    return view


def device_op(ops, x_u8, r, s, scale=None, shift=None, nhwc=False, odd=False):
    xd = offset_by_one(x_u8) if odd else torch.from_numpy(x_u8).cuda()
    y = ops.resize_crop_u8(xd, r, s, scale, shift, nhwc=nhwc)
    torch.cuda.synchronize()
    return y.cpu().numpy()


# ---- 1. the device op ---------------------------------------------------------------------------

@pytest.mark.parametrize("nhwc", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("H,W,r,s,odd", [c + (False,) for c in R.SHAPES + R.SHAPES_MANY_TAPS] +
                         [(37, 53, 24, 16, True), (257, 200, 36, 32, True), (400, 300, 20, 16, True)])
def test_device_op_within_bound_of_aten_float64(ops, H, W, r, s, odd, nhwc):
    x = R.pixels(H * 100 + W, 2, H, W, nhwc)
    got = device_op(ops, x, r, s, nhwc=nhwc, odd=odd)
    ref = R.reference64(x, nhwc, r, s)
    err, tol = np.abs(got.astype(np.float64) - ref).max(), R.bound(H, W, r, s)
    same = np.array_equal(got, ops.resize_crop_u8_host(x, r, s, nhwc=nhwc))
    print(f"device {H}x{W} -> {r} -> {s} {'nhwc' if nhwc else 'nchw'}{' odd base' if odd else ''}: max err {err:.3e}, "
          f"bound {tol:.3e}, bit-equal to the host reference: {same}")
    assert got.shape == ref.shape and err <= tol, (err, tol)


@pytest.mark.parametrize("nhwc", [False, True], ids=["nchw", "nhwc"])
def test_device_op_equalities(ops, nhwc):
    """Identity (H = W = R = S is a cast), the transform (two roundings), batch independence."""
    x = R.pixels(1, 2, 32, 32, nhwc)
    assert np.array_equal(device_op(ops, x, 32, 32, nhwc=nhwc), (x.transpose(0, 3, 1, 2) if nhwc else x).astype(np.float32))
    x = R.pixels(2, 3, 53, 37, nhwc)
    plain = device_op(ops, x, 24, 16, nhwc=nhwc)
    whole = device_op(ops, x, 24, 16, R.SCALE, R.SHIFT, nhwc=nhwc)
    assert np.array_equal(whole, plain * R.SCALE.reshape(1, 3, 1, 1) + R.SHIFT.reshape(1, 3, 1, 1))
    for b in range(3):
        assert np.array_equal(whole[b:b + 1], device_op(ops, x[b:b + 1], 24, 16, R.SCALE, R.SHIFT, nhwc=nhwc))


def test_device_op_more_than_one_tile_and_guards(ops):
    """A crop of several 32 x 8 tiles with ragged edges, written into a buffer with guard values around it."""
    x = R.pixels(3, 2, 97, 75, True)
    buf = torch.full((2 * 3 * 70 * 70 + 64,), 12345.0, device="cuda")
    out = buf[32:32 + 2 * 3 * 70 * 70].view(2, 3, 70, 70)
    ops.resize_crop_u8(torch.from_numpy(x).cuda(), 72, 70, nhwc=True, out=out)
    torch.cuda.synchronize()
    assert (buf[:32] == 12345.0).all() and (buf[-32:] == 12345.0).all()
    err = np.abs(out.cpu().numpy().astype(np.float64) - R.reference64(x, True, 72, 70)).max()
    assert err <= R.bound(97, 75, 72, 70), err


def test_device_op_arguments(ops):
    x = torch.zeros(1, 3, 8, 8, dtype=torch.uint8, device="cuda")
    for r, s in ((7, 8), (8, 0), (8193, 8)):
        with pytest.raises(ops.OpError):
            ops.resize_crop_u8(x, r, s)
    with pytest.raises(ops.OpError, match="long side"):
        ops.resize_crop_u8(torch.zeros(1, 3, 1, 40, dtype=torch.uint8, device="cuda"), 224, 224)


# ---- 2. models: resized, fp32 and plain 8-bit tasks alternated, graphs on --------------------------

_models = {}


def model(zoo, key):
    if key not in _models:
        kind, image = key
        _models[key] = (zoo.resnet18(image=image) if kind == "resnet" else
                        zoo.vit(image=image, patch=16, layers=2, heads=4, dim=256, mlp_dim=512))
    return _models[key]


def forward(spi, rep, x, stream):
    out = torch.full((x.shape[0], 1000), float("nan"), device="cuda")
    spi.run_hip(rep, [x], out, stream=stream.cuda_stream)
    return out.cpu().numpy()


@pytest.mark.parametrize("prec", ["fp32", "fp16", "fp16m", "fp16x3"])
def test_resnet18_resized_tasks_equal_fp32_tasks(spi, zoo, ops, prec):
    m = model(zoo, ("resnet", 64))
    rep = spi.ModelReplica(m, 0, prec, max_batch=2, image_size=64, graphs=True)
    rep.set_input_transform(R.SCALE, R.SHIFT)
    rep.set_input_resize(72)
    rep64 = spi.ModelReplica(m, 0, prec, max_batch=2, image_size=64, graphs=True)
    rep64.set_input_transform(R.SCALE, R.SHIFT)
    rep64.set_input_resize(64)
    plain = spi.ModelReplica(m, 0, prec, max_batch=2, image_size=64, graphs=True)
    plain.set_input_transform(R.SCALE, R.SHIFT)
    a, b, sq = R.pixels(20, 2, 80, 100, True), R.pixels(21, 2, 97, 75, False), R.pixels(22, 2, 64, 64, False)
    ad, bd, sqd = (torch.from_numpy(t).cuda() for t in (a, b, sq))
    ia = ops.resize_crop_u8(ad, 72, 64, R.SCALE, R.SHIFT, nhwc=True)
    ib = ops.resize_crop_u8(bd, 72, 64, R.SCALE, R.SHIFT, nhwc=False)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    outs = [[forward(spi, rep, ad, stream), forward(spi, rep, bd, stream), forward(spi, rep, ia, stream),
             forward(spi, rep64, sqd, stream)] for _ in range(2)]
    for o in outs[0] + outs[1]:
        assert np.isfinite(o).all()
    for k in range(4):  # the same bits in both rounds
        assert np.array_equal(outs[0][k], outs[1][k]), k
    assert np.array_equal(outs[0][0], outs[0][2])                      # u8 NHWC 80 x 100 == its fp32 task
    assert np.array_equal(outs[0][1], forward(spi, rep, ib, stream))   # u8 NCHW 97 x 75 == its fp32 task
    assert not np.array_equal(outs[0][0], outs[0][1])
    assert np.array_equal(outs[0][3], forward(spi, plain, sqd, stream))  # R = S = 64 == the plain 8-bit task
    # each image on its own, graphs off: the same rows
    eager = spi.ModelReplica(m, 0, prec, max_batch=2, image_size=64)
    eager.set_input_transform(R.SCALE, R.SHIFT)
    eager.set_input_resize(72)
    for i in range(2):
        assert np.array_equal(forward(spi, eager, ad[i:i + 1].contiguous(), stream), outs[0][0][i:i + 1])
    # the setter is refused once a stream workspace exists
    with pytest.raises(spi.InferenceExecutionException, match="stream workspace"):
        rep.set_input_resize(0)
    with pytest.raises(spi.InferenceExecutionException, match="stream workspace"):
        plain.set_input_resize(72)


def test_resnet18_both_ends_three_is_nchw(spi, zoo, ops):
    """[B,3,H,3] is read as NCHW -- H rows of 3 pixels -- not as 3 rows of H pixels with three channels."""
    rep = spi.ModelReplica(model(zoo, ("resnet", 64)), 0, "fp16m", max_batch=1, image_size=64, graphs=True)
    rep.set_input_resize(64)
    x = torch.from_numpy(R.pixels(23, 1, 200, 3, False)).cuda()  # [1,3,200,3]
    as_nchw, as_nhwc = ops.resize_crop_u8(x, 64, 64, nhwc=False), ops.resize_crop_u8(x, 64, 64, nhwc=True)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    got = forward(spi, rep, x, stream)
    assert np.array_equal(got, forward(spi, rep, as_nchw, stream))
    assert not np.array_equal(got, forward(spi, rep, as_nhwc, stream))


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_vit_resized_task_equals_fp32_task(spi, zoo, ops, prec):
    rep = spi.ModelReplica(model(zoo, ("vit", 160)), 0, prec, max_batch=2, image_size=160, graphs=True)
    rep.set_input_transform(R.SCALE, R.SHIFT)
    rep.set_input_resize(176)
    stream = torch.cuda.Stream()
    for nhwc in (True, False):
        x = torch.from_numpy(R.pixels(24, 2, 200, 170, nhwc)).cuda()
        img = ops.resize_crop_u8(x, 176, 160, R.SCALE, R.SHIFT, nhwc=nhwc)
        torch.cuda.synchronize()
        got, want = forward(spi, rep, x, stream), forward(spi, rep, img, stream)
        assert np.isfinite(want).all() and np.array_equal(got, want), nhwc
        assert np.array_equal(forward(spi, rep, x, stream), want)


# ---- 3. against the CPU oracle ------------------------------------------------------------------

def test_resized_nhwc_oracle_parity(spi, zoo):
    """ResNet-18 224 fp16m bs2, 300 x 260 NHWC source, R = 256, pixels scaled to [0, 1]: the existing 1e-3 bar
    with top-1 agreement against cpu_inference on the reference image (the resample's own error, at most
    1e-4 / 255 here, is far below the bar)."""
    m = model(zoo, ("resnet", 224))
    rep = spi.ModelReplica(m, 0, "fp16m", max_batch=2, graphs=True)
    rep.set_input_transform(R.UNIT_SCALE, R.ZERO)
    rep.set_input_resize(256)
    x = R.pixels(0, 2, 300, 260, True)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    got = forward(spi, rep, torch.from_numpy(x).cuda(), stream)
    ref = cpu_inference(m, [R.reference_image(x, True, 256, 224, R.UNIT_SCALE, R.ZERO)])[0]
    err = normalized_max_error(got, ref)
    print(f"resized u8 nhwc resnet18 fp16m @224 bs2 (300x260 -> 256 -> 224): err {err:.3e}")
    assert err < 1e-3, err
    assert (got.argmax(1) == ref.argmax(1)).all()


# ---- 4. through the mini-runtime ----------------------------------------------------------------

def test_runtime_resized_jobs(spi, zoo):
    """16 jobs of (48, 80, 3) uint8 samples: the runtime's per-sample dims are a source size."""
    rtmod = importlib.import_module("starpu-inference-server_amd.runtime")
    rep = spi.ModelReplica(model(zoo, ("resnet", 64)), 0, "fp16m", max_batch=8, image_size=64, graphs=True)
    rep.set_input_transform(R.SCALE, R.SHIFT)
    rep.set_input_resize(72)
    rt = rtmod.Runtime([rep], [((48, 80, 3), np.uint8)], [(1000, np.float32)], max_batch=8, workers_per_device=4,
                       pipeline_depth=2, warmup_batches=-1)
    jobs = []
    for rid in range(16):
        x = R.pixels(200 + rid, 8, 48, 80, True)
        y = np.full((8, 1000), np.nan, dtype=np.float32)
        rt.submit(rid, [x], [y])
        jobs.append((x, y))
    rt.drain()
    assert rt.stats() == (16, 0)
    rt.close()
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    for x, y in jobs:
        assert np.array_equal(y, forward(spi, rep, torch.from_numpy(x).cuda(), stream))

"""Resize + centre crop of 8-bit image tasks (spi_model_set_input_resize), host side: the shared
arithmetic (csrc/resample.hpp) run on the CPU by spi_op_resize_crop_u8_host against ATen's float64
resample; the contract checks (Model::check_io, the setter) on host-only replicas; the CPU codelets.

The reference (resize_refs.py) is torch.nn.functional.interpolate(x.double(), size=(RH, RW),
mode="bilinear", antialias=True, align_corners=False) followed by the crop rule; fp32 results are held
to 255 (Kx + Ky + 4) 2^-24 pixel levels (resize_refs.bound)."""
import importlib

import numpy as np
import pytest
import torch

import resize_refs as R


@pytest.fixture(scope="module")
def ops(spi):
    return importlib.import_module("starpu-inference-server_amd.ops")


# ---- 1. the shared arithmetic on the CPU --------------------------------------------------------

@pytest.mark.parametrize("nhwc", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("H,W,r,s", R.SHAPES + R.SHAPES_MANY_TAPS)
def test_host_reference_within_bound_of_aten_float64(ops, H, W, r, s, nhwc):
    x = R.pixels(H * 100 + W, 2, H, W, nhwc)
    got = ops.resize_crop_u8_host(x, r, s, nhwc=nhwc)
    ref = R.reference64(x, nhwc, r, s)
    assert got.shape == ref.shape == (2, 3, s, s) and got.dtype == np.float32
    err, tol = np.abs(got.astype(np.float64) - ref).max(), R.bound(H, W, r, s)
    print(f"host {H}x{W} -> {r} -> {s} {'nhwc' if nhwc else 'nchw'}: max err {err:.3e}, bound {tol:.3e}")
    assert ref.max() > ref.min()  # the reference is not a constant image
    assert err <= tol, (err, tol)


def test_crop_offsets_and_sizes():
    """The geometry the cases rely on: d = 3 rounds up to 2, d = 1 down to 0, the portrait's long side truncates."""
    assert R.geometry(33, 47, 32, 29) == (32, 45, 2, 8)  # d = 3 -> 2 (rows), d = 16 -> 8
    assert R.geometry(16, 17, 16, 15) == (16, 17, 0, 1)  # d = 1 -> 0 (rows), d = 2 -> 1
    assert R.geometry(53, 37, 24, 16) == (34, 24, 9, 4)  # 24 * 53 / 37 = 34.4 -> 34
    assert [R.geometry(10, 10, 10 + d, 10)[2] for d in range(6)] == [0, 0, 1, 2, 2, 2]


def test_package_geometry_matches_reference(spi):
    for (H, W, r, s) in R.SHAPES + [(500, 375, 256, 224), (300, 260, 256, 224), (97, 75, 72, 64)]:
        assert spi.resize_geometry(H, W, r, s) == R.geometry(H, W, r, s)


@pytest.mark.parametrize("nhwc", [False, True], ids=["nchw", "nhwc"])
def test_identity_is_a_cast(ops, nhwc):
    """H = W = R = S: the weights are exactly {1, 0}."""
    x = R.pixels(1, 2, 32, 32, nhwc)
    got = ops.resize_crop_u8_host(x, 32, 32, nhwc=nhwc)
    want = (x.transpose(0, 3, 1, 2) if nhwc else x).astype(np.float32)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("nhwc", [False, True], ids=["nchw", "nhwc"])
def test_transform_is_two_roundings(ops, nhwc):
    x = R.pixels(2, 2, 37, 53, nhwc)
    plain = ops.resize_crop_u8_host(x, 24, 16, nhwc=nhwc)
    got = ops.resize_crop_u8_host(x, 24, 16, R.SCALE, R.SHIFT, nhwc=nhwc)
    assert np.array_equal(got, plain * R.SCALE.reshape(1, 3, 1, 1) + R.SHIFT.reshape(1, 3, 1, 1))


@pytest.mark.parametrize("nhwc", [False, True], ids=["nchw", "nhwc"])
def test_batch_independence(ops, nhwc):
    x = R.pixels(3, 3, 53, 37, nhwc)
    whole = ops.resize_crop_u8_host(x, 24, 16, R.SCALE, R.SHIFT, nhwc=nhwc)
    for b in range(3):
        assert np.array_equal(whole[b:b + 1], ops.resize_crop_u8_host(x[b:b + 1], 24, 16, R.SCALE, R.SHIFT, nhwc=nhwc))


def test_host_op_arguments(ops):
    x = R.pixels(4, 1, 8, 8, False)
    for r, s in ((7, 8), (8, 0), (8193, 8)):
        with pytest.raises(ops.OpError):
            ops.resize_crop_u8_host(x, r, s)
    with pytest.raises(ops.OpError, match="long side"):
        ops.resize_crop_u8_host(R.pixels(5, 1, 1, 40, False), 224, 224)  # 224 * 40 = 8960 > 8192


# ---- 2. the GPU codelet's contract on host-only replicas (device -1) ------------------------------

def hip_call(spi, rep, dims, dtype, nbytes, classes=1000):
    """spi_hip_inference_func over host buffers of `nbytes` input bytes; returns the raised error text."""
    buf = np.zeros(max(nbytes, 1), np.uint8)
    out = np.zeros((dims[0], classes), np.float32)
    params = spi.make_params([list(dims)], [dtype], models_gpu=[rep])
    bufs = [spi.make_variable_interface(buf.ctypes.data, nbytes), spi.tensor_interface(torch.from_numpy(out))]
    with spi.worker_context(0, 0, None):  # replica index = device id
        with pytest.raises(spi.StarPUCodeletException) as e:
            spi.InferenceCodelet.hip_inference_func(bufs, params)
    return str(e.value)


def host_replica(spi, zoo, family):
    if family == "resnet":
        return spi.ModelReplica(zoo.resnet18(image=64), -1, "fp16", max_batch=4, image_size=64), 64
    return spi.ModelReplica(zoo.vit(image=32, patch=16, layers=1, heads=2, dim=128, mlp_dim=256), -1, "fp16",
                            max_batch=4, image_size=32), 32


@pytest.mark.parametrize("family", ["resnet", "vit"])
def test_check_io_resize_off_is_unchanged(spi, zoo, family):
    rep, s = host_replica(spi, zoo, family)
    msg = hip_call(spi, rep, [2, s + 16, s + 36, 3], torch.uint8, 2 * (s + 16) * (s + 36) * 3)
    assert f"Tensor layout mismatch: expected [B,3,{s},{s}] or [B,{s},{s},3]" in msg, msg
    rep.set_input_resize(s + 8)
    rep.set_input_resize(0)  # and switched off again
    msg = hip_call(spi, rep, [2, 3, s + 16, s + 36], torch.uint8, 2 * (s + 16) * (s + 36) * 3)
    assert f"Tensor layout mismatch: expected [B,3,{s},{s}] or [B,{s},{s},3]" in msg, msg
    assert "resize" not in rep.description


@pytest.mark.parametrize("family", ["resnet", "vit"])
def test_check_io_resize_on(spi, zoo, family):
    rep, s = host_replica(spi, zoo, family)
    rep.set_input_resize(s + 8)
    H, W = s + 16, s + 36
    n = 2 * 3 * H * W
    for dims in ([2, 3, H, W], [2, H, W, 3], [2, 3, s, s], [2, s, s, 3], [2, 3, 1, 5], [2, 3, H, 3], [1, 8192, 8192, 3]):
        nb = int(np.prod(dims))
        if nb > 1 << 24:  # no 200 MB buffer for the largest source: its size is checked first
            assert "Input buffer too small" in hip_call(spi, rep, dims, torch.uint8, 16)
            continue
        msg = hip_call(spi, rep, dims, torch.uint8, nb)  # accepted: the host-only replica's own error
        assert "host-only replica" in msg and "mismatch" not in msg, (dims, msg)
    # in_bytes at one byte per element, in both layouts
    assert "Input buffer too small" in hip_call(spi, rep, [2, 3, H, W], torch.uint8, n - 1)
    assert "Input buffer too small" in hip_call(spi, rep, [2, H, W, 3], torch.uint8, n - 1)
    # anything else names both accepted forms
    for dims in ([2, 4, H, W], [2, H, W, 4], [2, 3, H], [2, 3, 0, W], [2, 3, H, 8193], [2, 8193, W, 3]):
        msg = hip_call(spi, rep, dims, torch.uint8, max(1, int(np.prod(dims))))
        assert "Tensor layout mismatch: expected [B,3,H,W] or [B,H,W,3]" in msg, (dims, msg)
    # fp32 tasks keep the strict [B,3,S,S] check and four bytes per element
    msg = hip_call(spi, rep, [2, 3, H, W], torch.float32, 4 * n)
    assert f"Tensor layout mismatch: expected [B,3,{s},{s}]" in msg and "or [B" not in msg, msg
    assert "host-only replica" in hip_call(spi, rep, [2, 3, s, s], torch.float32, 4 * 2 * 3 * s * s)
    assert "Input buffer too small" in hip_call(spi, rep, [2, 3, s, s], torch.float32, 2 * 3 * s * s)
    # a resized long side above 8192 is refused: short side 1 -> s + 8, long side 300 (s + 8) >= 12000
    msg = hip_call(spi, rep, [1, 1, 300, 3], torch.uint8, 900)
    assert "long side" in msg and "8192" in msg, msg
    msg = hip_call(spi, rep, [1, 3, 300, 1], torch.uint8, 900)
    assert "long side" in msg and "8192" in msg, msg


def test_check_io_both_ends_three(spi, zoo):
    """[B,3,H,3] is NCHW: H rows of 3 pixels, not 3 rows of H pixels.  Both readings have the same byte count and
    the same resized long side, so check_io accepts it either way; which one the forward takes is checked on the
    device (test_resize_input_gpu.test_resnet18_both_ends_three_is_nchw)."""
    rep, s = host_replica(spi, zoo, "resnet")
    rep.set_input_resize(s)
    assert "host-only replica" in hip_call(spi, rep, [1, 3, 200, 3], torch.uint8, 1800)
    assert "Input buffer too small" in hip_call(spi, rep, [1, 3, 200, 3], torch.uint8, 1799)
    assert "long side" in hip_call(spi, rep, [1, 3, 2000, 3], torch.uint8, 18000)  # 64 * 2000 / 3 > 8192


def test_setter(spi, zoo):
    N = spi._native
    rep, s = host_replica(spi, zoo, "resnet")
    base = rep.description
    for bad in (s - 1, 1, 8193, -1, -256):
        assert spi.lib.spi_model_set_input_resize(rep.handle, bad) == N.SPI_ERR_INVALID_ARGUMENT
        assert "input resize" in N.last_error() and str(bad) in N.last_error()
        with pytest.raises(spi.InferenceExecutionException, match="set_input_resize failed"):
            rep.set_input_resize(bad)
        assert rep.description == base and rep.resize_short == 0
    assert spi.lib.spi_model_set_input_resize(None, 0) == N.SPI_ERR_INVALID_ARGUMENT
    for good in (s, s + 8, 8192):
        rep.set_input_resize(good)
        assert rep.description == f"{base} resize{good}" and rep.resize_short == good
    # the digest, weight bytes and FLOPs do not change
    plain, _ = host_replica(spi, zoo, "resnet")
    assert (rep.weight_digest, rep.weight_bytes, rep.flops(2)) == (plain.weight_digest, plain.weight_bytes, plain.flops(2))
    # beside the classification outputs
    rep.set_image_outputs("probs")
    assert rep.description == f"{base} out[logits,probs] resize8192"
    rep.set_image_outputs(0)
    rep.set_input_resize(0)  # 0 resets
    assert rep.description == base and rep.resize_short == 0


def test_setter_other_families(spi, zoo):
    N = spi._native
    bert = spi.ModelReplica(zoo.bert(layers=1, hidden=128, heads=2, intermediate=256), -1, "fp16", max_batch=2, seq_len=16)
    assert spi.lib.spi_model_set_input_resize(bert.handle, 256) == N.SPI_ERR_UNSUPPORTED
    assert "ResNet / ViT" in N.last_error()
    with pytest.raises(spi.InferenceExecutionException) as e:
        bert.set_input_resize(256)
    assert e.value.status == N.SPI_ERR_UNSUPPORTED
    affine = spi.ModelReplica(None, -1, "fp32", family="affine")
    assert spi.lib.spi_model_set_input_resize(affine.handle, 0) == N.SPI_ERR_UNSUPPORTED
    vit, s = host_replica(spi, zoo, "vit")
    vit.set_input_resize(s + 4)
    assert vit.description.endswith(f" resize{s + 4}")


# ---- 3. the CPU codelets -------------------------------------------------------------------------

def cpu_codelet(spi, model_cpu, x):
    out = np.full((x.shape[0], 1000), np.nan, dtype=np.float32)
    params = spi.make_params([list(x.shape)], [torch.from_numpy(x).dtype], num_outputs=1, model_cpu=model_cpu)
    bufs = [spi.tensor_interface(torch.from_numpy(x)), spi.tensor_interface(torch.from_numpy(out))]
    with spi.worker_context(3, -1, None):
        spi.InferenceCodelet.cpu_inference_func(bufs, params)
    return out


@pytest.fixture(scope="module")
def resnet18_32(zoo, tmp_path_factory):
    m = zoo.resnet18(image=32)
    path = str(tmp_path_factory.mktemp("resize") / "resnet18_32.pt")
    torch.jit.trace(m, torch.rand(1, 3, 32, 32)).save(path)
    return m, path


@pytest.mark.parametrize("xf", [False, True], ids=["cast", "imagenet"])
def test_python_cpu_forward_resizes(spi, resnet18_32, xf):
    """A u8 NHWC task at 40 x 52 with input_resize = (36, 32) == the module on the reference image."""
    m, _ = resnet18_32
    x = R.pixels(6, 2, 40, 52, True)
    scale, shift = (R.SCALE, R.SHIFT) if xf else (None, None)
    img = R.reference_image(x, True, 36, 32, scale, shift)
    with torch.inference_mode():
        want = m(torch.from_numpy(img))
    fwd = spi.TorchCpuForward(m, input_transform=(R.SCALE, R.SHIFT) if xf else None, input_resize=(36, 32))
    got = torch.from_numpy(cpu_codelet(spi, fwd, x))
    assert torch.isfinite(want).all() and torch.equal(got, want)
    # the NCHW form of the same pixels
    assert torch.equal(torch.from_numpy(cpu_codelet(spi, fwd, np.ascontiguousarray(x.transpose(0, 3, 1, 2)))), want)
    # fp32 tasks are untouched
    assert torch.equal(torch.from_numpy(cpu_codelet(spi, fwd, img)), want)
    with pytest.raises(spi.InferenceExecutionException):
        spi.TorchCpuForward(m, input_resize=(31, 32))
    with pytest.raises(spi.StarPUCodeletException, match="long side"):
        cpu_codelet(spi, fwd, np.zeros((1, 1, 300, 3), np.uint8))


def test_cpp_cpu_codelet_resizes(spi, resnet18_32):
    lt = importlib.import_module("starpu-inference-server_amd.libtorch")
    m, path = resnet18_32
    ts = lt.TorchScriptModule(path)
    x = R.pixels(7, 2, 40, 52, True)
    img = R.reference_image(x, True, 36, 32, R.SCALE, R.SHIFT)
    want = torch.from_numpy(cpu_codelet(spi, ts, img))
    ts.set_input_transform(R.SCALE, R.SHIFT)
    ts.set_input_resize(36, 32)
    assert torch.isfinite(want).all() and torch.equal(torch.from_numpy(cpu_codelet(spi, ts, x)), want)
    assert torch.equal(torch.from_numpy(cpu_codelet(spi, ts, np.ascontiguousarray(x.transpose(0, 3, 1, 2)))), want)
    assert torch.equal(torch.from_numpy(cpu_codelet(spi, ts, img)), want)  # fp32 tasks are untouched
    for r, s in ((31, 32), (8193, 32), (32, 0), (0, 32)):
        with pytest.raises(spi.InferenceExecutionException):
            ts.set_input_resize(r, s)
    with pytest.raises(spi.StarPUCodeletException, match="long side"):
        cpu_codelet(spi, ts, np.zeros((1, 1, 300, 3), np.uint8))
    ts.set_input_resize(0, 0)  # cleared: a 40 x 52 image reaches the 32 x 32 module's transform path again
    got = cpu_codelet(spi, ts, R.pixels(8, 2, 32, 32, True))
    assert np.isfinite(got).all()
    ts.close()

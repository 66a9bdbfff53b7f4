"""ResNeXt replicas on the GPU: the bottleneck conv2 as a grouped conv, on the grouped kernel (fp16 / fp16m)
and as the dense block-diagonal expansion on the existing kernels (fp32 / fp16x3, and fp16 under SPI_GCONV=0).

Models: zoo.resnet([1, 1, 1, 1], True, image=64, groups=32, width_per_group=4) -- cpg 4 / 8 / 16 / 32 on maps
16 / 8 / 4 / 2, stride 2 three times -- and the same with width_per_group=8 (cpg 8 .. 64); batch 2, input
np.random.default_rng(1).

Bars.  fp32 and fp16x3 against the oracle at the project's 1e-5: the existing kernels on expanded weights earn
it.  fp16 and fp16m below 3e-3, the project's bound for reduced-size nets (TOL_RESNET_PLAIN_FP16 of
test_parity_gpu.py).  That bound was checked for these models on the CPU with tools/prec_emulate.py's arithmetic
(which emulates the formats, not the kernel): fp16 1.35e-3 and 1.74e-3, fp16m 0.72e-3 and 0.90e-3 at this
input; worst over seeds 1-3 and a [1, 2, 2, 1] variant 2.0e-3 / 1.3e-3 -- the 1.5x headroom the bound has over
its own emulated 1.67e-3.  No top-1 assertion: the emulation flips it on one of three seeds in fp16m.
"""
import functools
import importlib

import numpy as np
import pytest
import torch

from oracle.cpu_codelet import cpu_inference, normalized_max_error

pytestmark = pytest.mark.gpu

TOL = 1e-5
TOL_RESNET_PLAIN_FP16 = 3e-3
WIDTHS = [4, 8]  # width_per_group of the 32x4d and the 32x8d model


def tol(prec):
    return TOL if prec in ("fp32", "fp16x3") else TOL_RESNET_PLAIN_FP16


@functools.lru_cache(maxsize=None)
def case(width_per_group, groups=32, batch=2):
    """(model, input, oracle output), built once."""
    zoo = importlib.import_module("starpu-inference-server_amd.zoo")
    m = zoo.resnet([1, 1, 1, 1], True, image=64, groups=groups, width_per_group=width_per_group)
    x = np.random.default_rng(1).random((batch, 3, 64, 64), dtype=np.float32)
    return m, x, cpu_inference(m, [x])[0]


def hip_forward(spi, replica, x, out_shape, graphs=False):
    xin = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    out = torch.full(out_shape, float("nan"), device="cuda", dtype=torch.float32)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    replica.set_graphs(graphs)
    spi.run_hip(replica, [xin], out, stream=stream.cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def op_names(rep, x, out_shape):
    xin = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    ops = rep.profile([xin], torch.empty(out_shape, device="cuda"), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return [o["name"] for o in ops]


@pytest.mark.parametrize("prec", ["fp32", "fp16x3", "fp16", "fp16m"])
@pytest.mark.parametrize("wpg", WIDTHS)
def test_resnext_against_oracle(spi, gpu, wpg, prec):
    """Parity at the precision's bar, and the captured graph gives the eager bits."""
    m, x, ref = case(wpg)
    rep = spi.ModelReplica(m, 0, prec, max_batch=2, image_size=64)
    assert " g32 " in rep.description
    got = hip_forward(spi, rep, x, ref.shape)
    got_g = hip_forward(spi, rep, x, ref.shape, graphs=True)
    err = normalized_max_error(got, ref)
    print(f"resnext 32x{wpg}d@64 {prec}: err {err:.3e}")
    assert np.isfinite(got).all()
    assert err < tol(prec)
    np.testing.assert_array_equal(got, got_g)


@pytest.mark.parametrize("wpg", WIDTHS)
def test_resnext_routing(spi, gpu, wpg, monkeypatch):
    """fp16 / fp16m run one gconv3x3_ op per block; fp32 and SPI_GCONV=0 none."""
    m, x, ref = case(wpg)
    for prec in ("fp16", "fp16m"):
        names = op_names(spi.ModelReplica(m, 0, prec, max_batch=2, image_size=64), x, ref.shape)
        g = [n for n in names if n.startswith("gconv3x3_")]
        assert len(g) == 4 and all("_g32_" in n for n in g), names
        widths = [128 * wpg // 4 << i for i in range(4)]
        assert [n.split("_")[1] for n in g] == [f"c{c}" for c in widths], g
        assert [n.split("_")[3] for n in g] == ["s1", "s2", "s2", "s2"], g
    names = op_names(spi.ModelReplica(m, 0, "fp32", max_batch=2, image_size=64), x, ref.shape)
    assert not any(n.startswith("gconv3x3_") for n in names), names
    monkeypatch.setenv("SPI_GCONV", "0")
    for prec in ("fp16", "fp16m"):
        names = op_names(spi.ModelReplica(m, 0, prec, max_batch=2, image_size=64), x, ref.shape)
        assert not any(n.startswith("gconv3x3_") for n in names), names


@pytest.mark.parametrize("wpg", WIDTHS)
def test_grouped_kernel_against_dense_expansion(spi, gpu, wpg, monkeypatch):
    """The same fp16 forward on both routes: each inside the bar, and within the bar of each other."""
    m, x, ref = case(wpg)
    new = hip_forward(spi, spi.ModelReplica(m, 0, "fp16", max_batch=2, image_size=64), x, ref.shape)
    monkeypatch.setenv("SPI_GCONV", "0")
    rep = spi.ModelReplica(m, 0, "fp16", max_batch=2, image_size=64)
    monkeypatch.delenv("SPI_GCONV")
    dense = hip_forward(spi, rep, x, ref.shape)
    e_new, e_dense = normalized_max_error(new, ref), normalized_max_error(dense, ref)
    diff = float(np.abs(new - dense).max() / np.abs(ref).max())
    print(f"resnext 32x{wpg}d@64 fp16: grouped kernel {e_new:.3e}, dense expansion {e_dense:.3e}, "
          f"between them {diff:.3e}")
    assert e_new < TOL_RESNET_PLAIN_FP16 and e_dense < TOL_RESNET_PLAIN_FP16
    assert diff < TOL_RESNET_PLAIN_FP16


@pytest.mark.parametrize("prec", ["fp16", "fp32"])
def test_resnext_batch_below_max_batch(spi, gpu, prec):
    m, x4, ref4 = case(4, batch=3)
    rep = spi.ModelReplica(m, 0, prec, max_batch=4, image_size=64)
    for b in (1, 3):
        got = hip_forward(spi, rep, x4[:b], (b,) + ref4.shape[1:])
        # the oracle's rows do not depend on the batch they were computed in beyond fp32 rounding
        ref = cpu_inference(m, [x4[:b]])[0]
        err = normalized_max_error(got, ref)
        print(f"resnext 32x4d@64 {prec} batch {b} of 4: err {err:.3e}")
        assert err < tol(prec)


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_wide_resnet(spi, gpu, prec):
    """wide_resnet50_2's block shape (width_per_group=128, dense): coverage of the doubled inner width."""
    m, x, ref = case(128, groups=1)
    rep = spi.ModelReplica(m, 0, prec, max_batch=2, image_size=64)
    assert " g" not in rep.description.split("]")[1].split("img")[0]
    err = normalized_max_error(hip_forward(spi, rep, x, ref.shape), ref)
    print(f"wide resnet [1,1,1,1]@64 {prec}: err {err:.3e}")
    assert err < tol(prec)

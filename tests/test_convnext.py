"""ConvNeXt replicas on the host (device -1): detection, description, plan walk, refusals, the two weight transforms."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch.utils.flop_counter import FlopCounterMode


def small(zoo, dims=(96, 192, 384, 768)):
    return zoo.convnext([1, 1, 2, 1], list(dims), image=64, num_classes=10)


def _named(d):
    class Named(torch.nn.Module):
        def named_parameters(self, *a, **k):
            return iter([])
        def named_buffers(self, *a, **k):
            return iter(d.items())
    return Named()


@pytest.mark.parametrize("prec,tag", [("fp16", "f16"), ("fp32", "f32")])
def test_detection_description_and_plan(spi, zoo, prec, tag):
    m = small(zoo)
    rep = spi.ModelReplica(m, -1, prec, max_batch=4, image_size=64)  # family left to the names
    assert rep.description == f"convnext[1,1,2,1] C96 img64 classes10 {tag} maxB4"
    wrapped = _named({"model." + k: v for k, v in m.state_dict().items()})
    assert spi.ModelReplica(wrapped, -1, prec, max_batch=4, image_size=64, family="convnext").weight_digest == rep.weight_digest
    steps = C.c_int32()
    for batch in (1, 4):
        assert spi.lib.spi_model_plan_check(rep.handle, batch, 0, C.byref(steps)) == 0
        assert steps.value == 1 + 3 + 2 * 5 + 1  # stem, downsamples, two Linears per block, FC
    assert spi.lib.spi_model_plan_check(rep.handle, 5, 0, C.byref(steps)) != 0
    with torch.no_grad(), FlopCounterMode(display=False) as fc:
        m(torch.zeros(1, 3, 64, 64))
    assert rep.flops(1) == float(fc.get_total_flops()) and rep.flops(4) == 4 * rep.flops(1)


def test_refusals(spi, zoo):
    m = small(zoo)
    full = spi.ModelReplica(zoo.build("convnext_tiny"), -1, "fp16")
    assert full.description == "convnext[3,3,9,3] C96 img224 classes1000 f16 maxB8"

    def refused(module, match, prec="fp16", image=64):
        with pytest.raises(spi.InferenceExecutionException, match=match):
            spi.ModelReplica(module, -1, prec, image_size=image)

    for prec in ("fp16x3", "fp16m"):
        refused(m, "SPI_PREC_F16 or SPI_PREC_F32", prec)
    refused(m, "image size 72 must be a multiple of 32", image=72)
    sd = dict(m.state_dict())
    sd["features.1.0.block.0.weight"] = torch.zeros(96, 1, 3, 3)
    refused(_named(sd), r"features\.1\.0\.block\.0\.weight must be a depthwise \[C\]\[1\]\[7\]\[7\]")
    refused(small(zoo, dims=(96, 160, 320, 640)), "stage 1 has 160 channels: a downsample must double the 96")
    refused(small(zoo, dims=(80, 160, 320, 640)), "stage width 80 must be a multiple of 32")
    five = zoo.convnext([1] * 5, [32, 64, 128, 256, 512], image=32, num_classes=10)  # maps 8, 4, 2, 1, then none
    refused(five, "before stage 4 would halve a map of odd side 1", image=32)


def test_layer_scale_is_folded_into_block5(spi, zoo):
    """Packed block.5 is diag(gamma) W (and gamma b) in fp32: a model that carries the product in block.5 and
    layer_scale = 1 packs to the same bytes."""
    m = small(zoo)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    for k in [k for k in sd if k.endswith("layer_scale")]:
        pre = k[:-len("layer_scale")]
        g = sd[k].reshape(-1)
        sd[pre + "block.5.weight"] = g[:, None] * sd[pre + "block.5.weight"]
        sd[pre + "block.5.bias"] = g * sd[pre + "block.5.bias"]
        sd[k] = torch.ones_like(sd[k])
    for prec in ("fp16", "fp32"):
        a, b = (spi.ModelReplica(mod, -1, prec, image_size=64) for mod in (m, _named(sd)))
        assert a.weight_digest == b.weight_digest and a.weight_bytes == b.weight_bytes
    sd["features.1.0.layer_scale"] *= 2
    assert spi.ModelReplica(_named(sd), -1, "fp16", image_size=64).weight_digest != a.weight_digest


def test_space_to_depth_weight_order(spi):
    """The packed downsample weight over space-to-depth rows equals the 2x2 / stride 2 conv."""
    ops = importlib.import_module("starpu-inference-server_amd.ops")
    rng = np.random.default_rng(3)
    Cin, N = 32, 64
    w = rng.standard_normal((N, Cin, 2, 2)).astype(np.float32)
    x = rng.standard_normal((1, Cin, 4, 4))
    wp = ops.s2d_weight(w).astype(np.float64)
    rows = torch.from_numpy(x).permute(0, 2, 3, 1).reshape(1, 2, 2, 2, 2, Cin).permute(0, 1, 3, 2, 4, 5).reshape(4, 4 * Cin)
    got = rows.numpy() @ wp.T
    ref = F.conv2d(torch.from_numpy(x), torch.from_numpy(w.astype(np.float64)), stride=2).permute(0, 2, 3, 1).reshape(4, N)
    np.testing.assert_allclose(got, ref.numpy(), rtol=0, atol=1e-12)

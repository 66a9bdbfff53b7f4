"""EfficientNet replicas on the host (device -1): the zoo's models, detection, description, plan walk, FLOPs, the
depthwise weight layout, refusals."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch
from torch.utils.flop_counter import FlopCounterMode


def small(zoo):
    return zoo.efficientnet(1.0, 1.0, image=64, num_classes=10)


def _named(d):
    class Named(torch.nn.Module):
        def named_parameters(self, *a, **k):
            return iter([])
        def named_buffers(self, *a, **k):
            return iter(d.items())
    return Named()


@pytest.mark.parametrize("name,params,blocks", [("efficientnet_b0", 5288548, 16), ("efficientnet_b7", 66347960, 55)])
def test_zoo_matches_torchvision(zoo, name, params, blocks):
    """torchvision's published parameter counts, and its state_dict names."""
    m = zoo.build(name)
    assert sum(p.numel() for p in m.parameters()) == params
    keys = set(m.state_dict())
    assert sum(k.endswith("fc1.weight") for k in keys) == blocks
    last = {"efficientnet_b0": "features.7.0", "efficientnet_b7": "features.7.3"}[name]
    assert {"features.0.0.weight", "features.1.0.block.0.0.weight", "features.1.0.block.1.fc1.bias", "features.1.0.block.2.1.running_var",
            "features.2.0.block.1.0.weight", "features.2.0.block.2.fc2.weight", last + ".block.3.0.weight",
            "features.8.1.weight", "classifier.1.bias"} <= keys


@pytest.mark.parametrize("prec,tag", [("fp16", "f16"), ("fp32", "f32")])
def test_detection_description_plan_and_flops(spi, zoo, prec, tag):
    m = small(zoo)
    rep = spi.ModelReplica(m, -1, prec, max_batch=4, image_size=64)  # family left to the names
    assert rep.description == f"efficientnet[1,2,2,3,3,4,1] C32 img64 classes10 {tag} maxB4"
    wrapped = _named({"model." + k: v for k, v in m.state_dict().items()})
    assert spi.ModelReplica(wrapped, -1, prec, max_batch=4, image_size=64, family="efficientnet").weight_digest == rep.weight_digest
    steps = C.c_int32()
    for batch in (1, 4):
        assert spi.lib.spi_model_plan_check(rep.handle, batch, 0, C.byref(steps)) == 0
        assert steps.value == 1 + 15 + 16 + 1 + 1  # stem, expands (none in stage 1), projects, head, pooled FC
    assert spi.lib.spi_model_plan_check(rep.handle, 5, 0, C.byref(steps)) != 0
    with torch.no_grad(), FlopCounterMode(display=False) as fc:
        m(torch.zeros(2, 3, 64, 64))
    assert rep.flops(2) == float(fc.get_total_flops())


@pytest.mark.parametrize("prec", ["fp16", "fp32"])
def test_depthwise_weight_is_bn_folded_tap_major(spi, zoo, prec):
    """[k k][C] of the compute type: BatchNorm folded in fp32, one rounding.  A model that carries the folded weight
    under an identity BatchNorm packs to the same bytes as the original."""
    ops = importlib.import_module("starpu-inference-server_amd.ops")
    m = small(zoo)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    conv, bn = "features.3.0.block.1.0.weight", "features.3.0.block.1.1."  # stage 3's 5x5 / stride 2
    s = sd[bn + "weight"].double() / torch.sqrt(sd[bn + "running_var"].double() + 1e-5)
    w = (sd[conv].double() * s[:, None, None, None]).float().numpy()
    got = ops.pack_weight_dwconv(prec, w, device="cpu").numpy()
    want = w.reshape(w.shape[0], 25).T.astype(np.float16 if prec == "fp16" else np.float32)
    assert got.shape == (25, 144) and np.array_equal(got, want)
    # (x - 0) / sqrt(1 - eps + eps) * 1 + b: the fold of this BatchNorm leaves w and sets the bias
    sd[conv] = torch.from_numpy(w)
    sd[bn + "bias"] = (sd[bn + "bias"].double() - sd[bn + "running_mean"].double() * s).float()
    sd[bn + "weight"], sd[bn + "running_mean"] = torch.ones(144), torch.zeros(144)
    sd[bn + "running_var"] = torch.full((144,), 1.0 - 1e-5, dtype=torch.float64).float()
    a, b = (spi.ModelReplica(mod, -1, prec, image_size=64) for mod in (m, _named(sd)))
    assert a.weight_bytes == b.weight_bytes and a.weight_digest == b.weight_digest


def test_efficientnet_routes_are_covered(spi, zoo):
    """Every GEMM of efficientnet_b0 at image 224 and batch 1, 8 and 32 -- listed from torchvision's block table,
    its (N, K) sequence checked against the zoo's module -- plans, at fp16 and fp32, onto a route that
    test_silu_routes_ops_gpu.py launches with the SiLU epilogue (op_refs.SILU_GEMM_ROUTES)."""
    import op_refs as R

    net = zoo.EfficientNet(1.0, 1.0)
    convs = []
    for stage in list(net.features)[1:-1]:
        for blk in stage:
            seq = list(blk.block)
            convs += [seq[0][0]] * (len(seq) == 4) + [seq[-1][0]]
    convs.append(net.features[-1][0])
    gemms = R.effnet_b0_gemms(1)
    assert [(c.out_channels, c.in_channels) for c in convs] == [(N, K) for _, N, K, _, _ in gemms]
    assert all(c.kernel_size == (1, 1) and c.groups == 1 for c in convs)
    assert len(gemms) == 15 + 16 + 1 and sum(res for *_, res in gemms) == 9 and gemms[-1][0] == 49
    ks = {K for _, _, K, _, _ in gemms}
    assert ks == {16, 24, 32, 40, 80, 96, 112, 144, 192, 240, 320, 480, 672, 1152}
    found = set()
    with R.gemm_knobs(spi.lib, {}):
        for B in (1, 8, 32):
            for M, N, K, act, _ in R.effnet_b0_gemms(B):
                for prec in ("fp16", "fp32"):  # the model's descs: outputs and residuals of the compute type
                    route = R.gemm_route(R.query_gemm_plan(spi.lib, prec, M, N, K, K, R.F_ACT if act else 0))
                    assert route in R.SILU_GEMM_ROUTES, (B, prec, M, N, K, act, route)
                    found.add(route)
    assert ("gemm256", 128, 256, False) in found and ("gemm", 64, 64, True) in found  # the head at batch 32; split-K


def test_refusals(spi, zoo):
    m = small(zoo)

    def refused(module, match, prec="fp16", image=64):
        with pytest.raises(spi.InferenceExecutionException, match=match):
            spi.ModelReplica(module, -1, prec, image_size=image)

    for prec in ("fp16x3", "fp16m"):
        refused(m, "efficientnet: SPI_PREC_F16X3 and SPI_PREC_F16M are not served", prec)
    refused(m, "image size 72 must be a multiple of 32", image=72)
    sd = dict(m.state_dict())
    sd["features.2.0.block.1.0.weight"] = torch.zeros(96, 1, 7, 7)
    refused(_named(sd), r"features\.2\.0\.block\.1\.0\.weight must be a depthwise \[C\]\[1\]\[3\|5\]\[3\|5\] weight with C = 96")
    sd = dict(m.state_dict())
    sd["features.2.0.block.0.0.weight"] = torch.zeros(92, 16, 1, 1)
    for k in ("weight", "bias", "running_mean", "running_var"):
        sd["features.2.0.block.0.1." + k] = torch.ones(92)
    refused(_named(sd), "expanded map has 92 channels: a multiple of 8 from 8 to 4608 is served")
    sd = dict(m.state_dict())
    sd["features.1.0.block.0.0.weight"] = torch.zeros(32, 32, 3, 3)  # a dense 3x3 in the depthwise conv's place
    refused(_named(sd), "EfficientNetV2's fused-MBConv blocks are not served")
    sd = dict(m.state_dict())
    del sd["features.2.0.block.2.fc1.weight"]
    refused(_named(sd), "without squeeze-and-excitation")

"""ResNeXt replicas on the host (device_id = -1: recognised and packed, never uploaded): the full-size
models of the reference's export script, a TorchScript round trip, and what the packer refuses."""
import os
import tempfile

import pytest
import torch
from torch.utils.flop_counter import FlopCounterMode


def _named(d):
    class Named(torch.nn.Module):
        def named_parameters(self, *a, **k):
            return iter([])

        def named_buffers(self, *a, **k):
            return iter(d.items())
    return Named()


def module_flops(m, image):
    """Conv and linear FLOPs (2 per multiply-add) of one forward at batch 1, the way SURVEY.md 8 counted."""
    with torch.no_grad(), FlopCounterMode(display=False) as fc:
        m(torch.zeros(1, 3, image, image))
    return float(fc.get_total_flops())


@pytest.mark.parametrize("name", ["resnext50_32x4d", "resnext101_32x8d"])
def test_fullsize_resnext_replica(spi, zoo, name, monkeypatch):
    m = getattr(zoo, name)(calibrate=False)
    rep = spi.ModelReplica(m, -1, "fp16")
    depth = "[3,4,6,3]" if name == "resnext50_32x4d" else "[3,4,23,3]"
    assert rep.description.startswith(f"resnet-bottleneck{depth} g32 img224 classes1000 f16"), rep.description
    again = spi.ModelReplica(m, -1, "fp16")
    assert rep.weight_digest == again.weight_digest and rep.weight_bytes == again.weight_bytes
    want = module_flops(m, 224)
    assert abs(rep.flops(1) - want) <= 1e-6 * want, (rep.flops(1), want)
    assert abs(rep.flops(8) - 8 * want) <= 1e-6 * 8 * want
    monkeypatch.setenv("SPI_GCONV", "0")
    dense = spi.ModelReplica(m, -1, "fp16")
    print(f"{name}: {rep.weight_bytes / 2**20:.1f} MiB grouped, {dense.weight_bytes / 2**20:.1f} MiB dense expansion")
    assert dense.weight_bytes > rep.weight_bytes
    assert " g32 " in dense.description
    assert abs(dense.flops(1) - want) <= 1e-6 * want  # the conv's own FLOPs on either route


def test_zoo_names_and_wide_resnets(spi, zoo):
    for name in ("resnext50_32x4d", "resnext101_32x8d", "wide_resnet50_2", "wide_resnet101_2"):
        assert callable(getattr(zoo, name))
    m = zoo.build("wide_resnet50_2", calibrate=False)
    assert m.layer1[0].conv2.weight.shape == (128, 128, 3, 3) and m.layer4[0].conv3.weight.shape == (2048, 1024, 1, 1)
    rep = spi.ModelReplica(m, -1, "fp16")
    assert rep.description.startswith("resnet-bottleneck[3,4,6,3] img224"), rep.description
    want = module_flops(m, 224)
    assert abs(rep.flops(1) - want) <= 1e-6 * want
    m = zoo.build("resnext50_32x4d", calibrate=False)
    assert m.layer1[0].conv2.weight.shape == (128, 4, 3, 3) and m.layer4[2].conv2.groups == 32


def test_existing_models_draw_the_same_numbers(zoo):
    """The new keywords at their defaults construct the same modules in the same order."""
    a = zoo.resnet([1, 1, 1, 1], True, image=64, calibrate=False)
    b = zoo.resnet([1, 1, 1, 1], True, image=64, calibrate=False, groups=1, width_per_group=64)
    for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert ka == kb and torch.equal(va, vb)


def test_torchscript_resnext(spi, zoo):
    codelet = __import__("importlib").import_module("starpu-inference-server_amd.codelet")
    m = zoo.resnet([1, 1, 1, 1], True, image=64, groups=32, width_per_group=4)
    want = spi.ModelReplica(m, -1, "fp16", image_size=64)
    ts = torch.jit.trace(m, torch.zeros(1, 3, 64, 64))
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "resnext.pt")
        ts.save(path)
        got = spi.ModelReplica(codelet.load_model(path), -1, "fp16", image_size=64)
    assert got.weight_digest == want.weight_digest and got.description == want.description
    assert " g32 " in got.description


REJECT = "grouped/unsupported conv"


@pytest.mark.parametrize("prec", ["fp16", "fp32"])
def test_unsupported_grouped_convs_are_rejected(spi, zoo, prec):
    def small(**kw):
        return zoo.resnet([1, 1, 1, 1], True, image=64, calibrate=False, **kw)

    def refused(module, what):
        with pytest.raises(spi.InferenceExecutionException, match=REJECT):
            spi.ModelReplica(module, -1, prec, image_size=64)
        print(f"refused: {what}")

    # groups 32 on widths that are no multiple of 128: 64 .. 512 (cpg 2 ..) and 192 .. (cpg 6 ..)
    refused(small(groups=32, width_per_group=2), "32 groups on width 64")
    refused(small(groups=32, width_per_group=6), "32 groups on width 192")
    # channels per group outside {4, 8, 16, 32, 64} on a width that is a multiple of 128
    refused(small(groups=64, width_per_group=2), "cpg 2 on width 128")
    refused(small(groups=2, width_per_group=128), "cpg 128 on width 256")
    # a grouped conv1
    sd = dict(small(groups=32, width_per_group=4).state_dict())
    sd["layer2.0.conv1.weight"] = sd["layer2.0.conv1.weight"][:, :8].clone()
    refused(_named(sd), "grouped conv1")
    # two blocks with different group counts: 32 and 16, 32 and 1
    two = zoo.resnet([2, 1, 1, 1], True, image=64, calibrate=False, groups=32, width_per_group=4)
    sd = dict(two.state_dict())
    sd["layer1.1.conv2.weight"] = torch.zeros(128, 8, 3, 3)
    refused(_named(sd), "32 and 16 groups")
    sd["layer1.1.conv2.weight"] = torch.zeros(128, 128, 3, 3)
    refused(_named(sd), "32 groups and a dense conv2")
    # a grouped conv in a BasicBlock net
    sd = dict(zoo.resnet([1, 1, 1, 1], False, image=64, calibrate=False).state_dict())
    sd["layer2.0.conv2.weight"] = sd["layer2.0.conv2.weight"][:, :4].clone()
    refused(_named(sd), "grouped conv in a BasicBlock net")
    # and the supported model loads
    assert " g32 " in spi.ModelReplica(small(groups=32, width_per_group=4), -1, prec, image_size=64).description

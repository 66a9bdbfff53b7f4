"""Swin v2 on the host: the zoo modules against torchvision's parameter counts and the installed transformers
Swinv2ForImageClassification, the host cpb bias table, and replicas of device -1: generation detection, description,
digest, plan walk, FLOPs and refusals."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch
from torch.utils.flop_counter import FlopCounterMode

import swin_v2_refs as V
from test_convnext import _named  # a module whose named tensors are a given dict


def small(zoo, heads=(2, 4), embed=64, image=64):
    return zoo.swin_v2((2, 2), heads, embed, window=8, image=image, num_classes=10)


@pytest.mark.parametrize("name,count", [("swin_v2_t", 28_351_570), ("swin_v2_s", 49_737_442), ("swin_v2_b", 87_930_848)])
def test_parameter_counts_are_torchvisions(zoo, name, count):
    assert sum(p.numel() for p in zoo.build(name).parameters()) == count


def test_zoo_forward_agrees_with_transformers(zoo):
    """Every weight copied into Swinv2ForImageClassification, whose key projection has no bias (the zeroed K third);
    image 64, maps 16 and 8: block 1 of stage 0 is shifted and masked.  fp32 on both sides, the project's 1e-5."""
    from transformers import Swinv2Config, Swinv2ForImageClassification
    m = small(zoo)
    hf = Swinv2ForImageClassification(Swinv2Config(image_size=64, patch_size=4, num_channels=3, embed_dim=64, depths=[2, 2],
                                                   num_heads=[2, 4], window_size=8, num_labels=10, layer_norm_eps=1e-5)).eval()
    sd = m.state_dict()
    new = {"swinv2.embeddings.patch_embeddings.projection": "features.0.0", "swinv2.embeddings.norm": "features.0.2",
           "swinv2.layernorm": "norm", "classifier": "head", "swinv2.encoder.layers.0.downsample.reduction": "features.2.reduction",
           "swinv2.encoder.layers.0.downsample.norm": "features.2.norm"}
    for st in range(2):
        for b in range(2):
            src, dst = f"features.{2 * st + 1}.{b}.", f"swinv2.encoder.layers.{st}.blocks.{b}."
            new.update({dst + "layernorm_before": src + "norm1", dst + "layernorm_after": src + "norm2",
                        dst + "attention.output.dense": src + "attn.proj", dst + "intermediate.dense": src + "mlp.0",
                        dst + "output.dense": src + "mlp.3", dst + "attention.self.continuous_position_bias_mlp.0": src + "attn.cpb_mlp.0",
                        dst + "attention.self.continuous_position_bias_mlp.2": src + "attn.cpb_mlp.2"})
    want = {}
    for k in hf.state_dict():
        mod, leaf = k.rsplit(".", 1)
        parts = k.split(".")
        blk = f"features.{2 * int(parts[3]) + 1}.{parts[5]}.attn." if ".blocks." in k else ""
        if mod in new:
            want[k] = sd[new[mod] + "." + leaf]
        elif leaf == "logit_scale":
            want[k] = sd[blk + leaf]
        else:
            assert parts[-2] in ("query", "key", "value"), k
            want[k] = sd[blk + "qkv." + leaf].chunk(3)[("query", "key", "value").index(parts[-2])]
    hf.load_state_dict(want, strict=True)
    x = torch.from_numpy(np.random.default_rng(1).random((2, 3, 64, 64), dtype=np.float32))
    with torch.no_grad():
        a, b = m(x), hf(pixel_values=x).logits
    err = float((a - b).abs().max() / a.abs().max())
    print(f"zoo.swin_v2 against transformers: {err:.3e}")
    assert err < 1e-5


@pytest.mark.parametrize("ws", [2, 7, 8])
def test_host_cpb_table(zoo, ws):
    ops = importlib.import_module("starpu-inference-server_amd.ops")
    attn = zoo.swin_v2((1,), (3,), 96, window=ws, image=4 * ws).features[1][0].attn
    w0, b0, w2 = (t.detach().numpy() for t in (attn.cpb_mlp[0].weight, attn.cpb_mlp[0].bias, attn.cpb_mlp[2].weight))
    got, ref = ops.window_cpb_table(w0, b0, w2, ws), V.cpb_table_ref(w0, b0, w2, ws)
    assert got.shape == ref.shape and np.abs(got - ref).max() / np.abs(ref).max() < 1e-6
    assert ref.max() - ref.min() > 2.0, "the zoo's bias should vary over the window"
    N, packed = ws * ws, ops.window_cpb_bias(w0, b0, w2, ws, device="cpu").numpy()  # [head][key / 4][query slot][key % 4]
    full = packed.transpose(0, 2, 1, 3).reshape(3, 64, 64)[:, :N, :N]
    with torch.no_grad():
        own = attn.position_bias().numpy()
    assert np.abs(full - own).max() / np.abs(own).max() < 1e-6


@pytest.mark.parametrize("prec,tag", [("fp16", "f16"), ("fp32", "f32")])
def test_detection_description_and_plan(spi, zoo, prec, tag):
    m = small(zoo)
    rep = spi.ModelReplica(m, -1, prec, max_batch=4, image_size=64)  # family, generation, window, heads left to the tensors
    assert rep.description == f"swin_v2[2,2] C64 ws8 img64 classes10 {tag} maxB4"
    wrapped = _named({"model." + k: v for k, v in m.state_dict().items() if not k.endswith("relative_position_index")})
    assert spi.ModelReplica(wrapped, -1, prec, max_batch=4, image_size=64, family="swin").weight_digest == rep.weight_digest
    bare = _named({k: v for k, v in m.state_dict().items() if "relative_" not in k})  # no buffer: the config states the window
    assert spi.ModelReplica(bare, -1, prec, max_batch=4, image_size=64, window_size=8).weight_digest == rep.weight_digest
    steps = C.c_int32()
    for batch in (1, 4):
        assert spi.lib.spi_model_plan_check(rep.handle, batch, 0, C.byref(steps)) == 0
        assert steps.value == 1 + 1 + 4 * 4 + 1  # stem, merge, four GEMMs per block, avgpool + FC
    assert spi.lib.spi_model_plan_check(rep.handle, 5, 0, C.byref(steps)) != 0
    with torch.no_grad(), FlopCounterMode(display=False) as fc:
        m(torch.zeros(1, 3, 64, 64))
    cpb = sum(2 * 15 * 15 * 512 * (2 + h) for h in (2, 2, 4, 4))  # cpb_mlp runs once, on the host
    assert rep.flops(1) == float(fc.get_total_flops() - cpb) and rep.flops(4) == 4 * rep.flops(1)
    full = spi.ModelReplica(zoo.build("swin_v2_t"), -1, prec)
    assert full.description == f"swin_v2[2,2,6,2] C96 ws8 img256 classes1000 {tag} maxB8"


def test_refusals(spi, zoo):
    m, v1 = small(zoo), zoo.swin((2, 2), (2, 4), 64, window=7, image=56, num_classes=10)

    def refused(module, match, prec="fp16", image=64, **kw):
        with pytest.raises(spi.InferenceExecutionException, match=match):
            spi.ModelReplica(module, -1, prec, image_size=image, **kw)

    refused(m, "swin: SPI_PREC_F16X3 and SPI_PREC_F16M are not served", "fp16x3")
    refused(m, "map of side 12 .image 96. is no multiple of the window 8", image=96)
    sd = dict(m.state_dict())
    sd["features.1.0.attn.relative_position_bias_table"] = v1.state_dict()["features.1.0.attn.relative_position_bias_table"]
    refused(_named(sd), "Swin-v2.*one generation")  # the two generations mixed
    sd = dict(v1.state_dict())
    sd.update({k: v for k, v in m.state_dict().items() if k.startswith("features.1.1.attn.") and "relative_position" not in k})
    refused(_named(sd), "Swin-v2", image=56)
    sd = {k: v for k, v in m.state_dict().items() if k != "features.3.1.attn.cpb_mlp.0.bias"}
    refused(_named(sd), "Swin-v2: 'features.3.1.attn.cpb_mlp.0.bias' is missing")  # a partial v2 set
    refused(_named({k: v for k, v in m.state_dict().items() if "relative_" not in k}), "Swin-v2: no tensor states the window")

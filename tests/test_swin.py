"""Swin on the host: the zoo module against torchvision's parameter counts and against the installed transformers
implementation, and replicas of device -1: detection, what the packer reads from the tensors, the plan walk, the
refusals, the host bias expansion."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch
from torch.utils.flop_counter import FlopCounterMode

from test_convnext import _named  # a module whose named tensors are a given dict


def small(zoo, heads=(2, 4), embed=64, image=56):
    return zoo.swin((2, 2), heads, embed, window=7, image=image, num_classes=10)


@pytest.mark.parametrize("name,count", [("swin_t", 28_288_354), ("swin_s", 49_606_258), ("swin_b", 87_768_224)])
def test_parameter_counts_are_torchvisions(zoo, name, count):
    assert sum(p.numel() for p in zoo.build(name).parameters()) == count


def test_zoo_forward_agrees_with_transformers(zoo):
    """The restated graph against an independent implementation (roll direction, mask, bias index, merge order):
    every weight copied into SwinForImageClassification, qkv split into its three projections; image 56, maps 14
    and 7, so block 1 of stage 0 is shifted and masked.  fp32 on both sides: agreement to fp32 rounding."""
    from transformers import SwinConfig, SwinForImageClassification
    m = small(zoo)
    hf = SwinForImageClassification(SwinConfig(image_size=56, patch_size=4, num_channels=3, embed_dim=64, depths=[2, 2],
                                               num_heads=[2, 4], window_size=7, num_labels=10, layer_norm_eps=1e-5)).eval()
    sd = m.state_dict()
    new = {"swin.embeddings.patch_embeddings.projection": "features.0.0", "swin.embeddings.norm": "features.0.2",
           "swin.layernorm": "norm", "classifier": "head"}
    for st in range(2):
        if st == 0:
            new["swin.encoder.layers.0.downsample.reduction"] = "features.2.reduction"
            new["swin.encoder.layers.0.downsample.norm"] = "features.2.norm"
        for b in range(2):
            src, dst = f"features.{2 * st + 1}.{b}.", f"swin.encoder.layers.{st}.blocks.{b}."
            new.update({dst + "layernorm_before": src + "norm1", dst + "layernorm_after": src + "norm2",
                        dst + "attention.o_proj": src + "attn.proj", dst + "mlp.fc1": src + "mlp.0", dst + "mlp.fc2": src + "mlp.3"})
    want = {}
    for k, v in hf.state_dict().items():
        mod, leaf = k.rsplit(".", 1)
        parts = k.split(".")
        blk = f"features.{2 * int(parts[3]) + 1}.{parts[5]}.attn." if ".blocks." in k else ""
        if mod in new:
            want[k] = sd[new[mod] + "." + leaf]
        elif leaf == "relative_position_bias_table":
            want[k] = sd[blk + leaf]
        elif parts[-2] in ("q_proj", "k_proj", "v_proj"):
            want[k] = sd[blk + "qkv." + leaf].chunk(3)["qkv".index(parts[-2][0])]
        else:
            assert leaf == "relative_position_index", k
            want[k] = v
    hf.load_state_dict(want, strict=True)
    x = torch.from_numpy(np.random.default_rng(1).random((2, 3, 56, 56), dtype=np.float32))
    with torch.no_grad():
        a, b = m(x), hf(pixel_values=x).logits
    err = float((a - b).abs().max() / a.abs().max())
    print(f"zoo.swin against transformers: {err:.3e}")
    assert err < 2e-6


@pytest.mark.parametrize("prec,tag", [("fp16", "f16"), ("fp32", "f32")])
def test_detection_description_and_plan(spi, zoo, prec, tag):
    m = small(zoo)
    rep = spi.ModelReplica(m, -1, prec, max_batch=4, image_size=56)  # family, window, depths, heads left to the tensors
    assert rep.description == f"swin[2,2] C64 ws7 img56 classes10 {tag} maxB4"
    wrapped = _named({"model." + k: v for k, v in m.state_dict().items() if not k.endswith("relative_position_index")})
    assert spi.ModelReplica(wrapped, -1, prec, max_batch=4, image_size=56, family="swin").weight_digest == rep.weight_digest
    assert spi.ModelReplica(small(zoo, heads=(1, 2), embed=32), -1, prec, image_size=56).description.startswith("swin[2,2] C32 ws7")
    steps = C.c_int32()
    for batch in (1, 4):  # the planned workspace covers the walk at every batch up to max_batch
        assert spi.lib.spi_model_plan_check(rep.handle, batch, 0, C.byref(steps)) == 0
        assert steps.value == 1 + 1 + 4 * 4 + 1  # stem, merge, four GEMMs per block, avgpool + FC
    assert spi.lib.spi_model_plan_check(rep.handle, 5, 0, C.byref(steps)) != 0
    with torch.no_grad(), FlopCounterMode(display=False) as fc:
        m(torch.zeros(1, 3, 56, 56))
    assert rep.flops(1) == float(fc.get_total_flops()) and rep.flops(4) == 4 * rep.flops(1)
    full = spi.ModelReplica(zoo.build("swin_t"), -1, prec)
    assert full.description == f"swin[2,2,6,2] C96 ws7 img224 classes1000 {tag} maxB8"


def test_refusals(spi, zoo):
    m = small(zoo)

    def refused(module, match, prec="fp16", image=56):
        with pytest.raises(spi.InferenceExecutionException, match=match):
            spi.ModelReplica(module, -1, prec, image_size=image)

    for prec in ("fp16x3", "fp16m"):
        refused(m, "swin: SPI_PREC_F16X3 and SPI_PREC_F16M are not served", prec)
    refused(small(zoo, heads=(1, 2)), "64 channels over 1 heads: head_dim must be 32")
    refused(m, "map of side 16 .image 64. is no multiple of the window 7", image=64)
    refused(small(zoo, heads=(1, 2), embed=48), "stage width 48 must be a multiple of 32")
    sd = dict(m.state_dict())
    sd["features.2.reduction.weight"] = torch.zeros(192, 256)
    refused(_named(sd), "stage 1 has 192 channels: a merge must double the 64")
    sd = dict(m.state_dict())
    sd["features.1.0.attn.relative_position_bias_table"] = torch.zeros(17 * 17, 2)
    refused(_named(sd), r"289 rows: \(2 ws - 1\)\^2 for a window ws of 2 \.\. 8")
    for v2 in ("features.1.0.attn.logit_scale", "features.1.0.attn.cpb_mlp.0.weight"):
        sd = dict(m.state_dict())
        sd[v2] = torch.zeros(2, 1, 1)
        refused(_named(sd), "Swin-v2")
    wide = zoo.swin((1, 1, 1), (16, 32, 64), 512, window=7, image=112, num_classes=10)  # the second merge: 4 C = 4096
    refused(wide, "rows of 4096 columns: at most 2048", image=112)


@pytest.mark.parametrize("ws", [2, 7, 8])
def test_host_bias_expansion_is_table_of_index(zoo, ws):
    ops = importlib.import_module("starpu-inference-server_amd.ops")
    heads, N = 3, ws * ws
    attn = zoo.ShiftedWindowAttention(96, ws, 0, heads)
    table = torch.randn((2 * ws - 1) ** 2, heads)
    want = table[attn.relative_position_index].view(N, N, heads).permute(2, 0, 1).numpy()  # [head][query][key]
    packed = ops.window_bias(table, ws, device="cpu").numpy()  # [head][key / 4][query slot][key % 4]
    full = packed.transpose(0, 2, 1, 3).reshape(heads, 64, 64)
    np.testing.assert_array_equal(full[:, :N, :N], want)
    assert np.isneginf(full[:, :, N:]).all() and (full[:, N:, :N] == 0).all()

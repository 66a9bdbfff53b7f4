#!/usr/bin/env python3
"""CPU emulation of the fp16 number formats of an EfficientNet replica (tools/prec_emulate.py's method: it emulates
the formats, not the kernels): BatchNorm folded into the conv weights in fp32 and rounded once to fp16, fp16-rounded
activations, fp32 accumulation and fp32 SiLU / sigmoid arithmetic (--acc f64: float64 instead, to see how far the
figure moves with the summation alone), one fp16 rounding where a launch stores -- the ingested image, the stem,
each expand conv, each depthwise conv, the gated map, each project conv with its residual, the head conv.  The
squeeze-and-excitation branch stays fp32 from the un-rounded depthwise activations, and so do the pooled features
and the logits.  Prints the normalised max error against the float64 forward of the same module: the figure the
fp16 parity bar of tests/test_efficientnet_gpu.py is 1.5x of.  Needs torch only (zoo.py is loaded by path).

  python tools/prec_emulate_efficientnet.py [--width 1.0 1.1] [--seeds 1 2 3]
"""
import argparse
import copy
import importlib.util
import os

import numpy as np
import torch
import torch.nn.functional as F

_spec = importlib.util.spec_from_file_location("spi_zoo", os.path.join(
    os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "starpu-inference-server_amd", "zoo.py"))
zoo = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(zoo)


def h(t):
    return t.half().to(t.dtype)


def folded(seq, dt):
    """Conv + BatchNorm of a Conv2dNormActivation as the packer folds them: scale in float64, then fp32."""
    conv, bn = seq[0], seq[1]
    s = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
    w = (conv.weight.double() * s[:, None, None, None]).float()
    b = (bn.bias.double() - bn.running_mean.double() * s).float()
    return h(w).to(dt), b.to(dt), conv


def forward(model, x, dt):
    def cba(seq, v, act=True):
        w, b, conv = folded(seq, dt)
        y = F.conv2d(v, w, b, conv.stride, conv.padding, groups=conv.groups)
        return F.silu(y) if act else y

    f = list(model.features)
    y = h(cba(f[0], h(x.to(dt))))
    for stage in f[1:-1]:
        for blk in stage:
            layers = list(blk.block)
            a = h(cba(layers[0], y)) if len(layers) == 4 else y
            d = cba(layers[-3], a)  # fp32: the pool sums are taken before the store's rounding
            se = layers[-2]
            g = torch.sigmoid(se.fc2.to(dt)(F.silu(se.fc1.to(dt)(d.mean((2, 3), keepdim=True)))))
            o = cba(layers[-1], h(h(d) * g), act=False)
            y = h(o + y) if blk.use_res else h(o)
    p = h(cba(f[-1], y)).mean((2, 3))
    fc = model.classifier[1]
    return (p @ h(fc.weight.detach().float()).to(dt).T + fc.bias.detach().to(dt)).double()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, nargs="*", default=[1])
    ap.add_argument("--width", type=float, nargs="*", default=[1.0, 1.1])
    ap.add_argument("--acc", choices=["f32", "f64"], default="f32")
    a = ap.parse_args()
    for width in a.width:
        model = zoo.efficientnet(width, 1.0, image=64, num_classes=10)
        for seed in a.seeds:
            x = torch.from_numpy(np.random.default_rng(seed).random((2, 3, 64, 64), dtype=np.float32))
            with torch.no_grad():
                ref = copy.deepcopy(model).double()(x.double())
                emu = forward(copy.deepcopy(model), x, torch.float32 if a.acc == "f32" else torch.float64)
            per_image = ((emu - ref).abs().amax(1) / ref.abs().max()).tolist()
            print(f"width {width} input seed {seed} acc {a.acc}: fp16 emulation {max(per_image):.3e} (per image "
                  + ", ".join(f"{e:.3e}" for e in per_image) + ")")


if __name__ == "__main__":
    main()

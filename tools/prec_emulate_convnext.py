#!/usr/bin/env python3
"""CPU emulation of the fp16 number formats of a ConvNeXt replica (tools/prec_emulate.py's method: it emulates
the formats, not the kernels): fp16-rounded weights and activations, fp32 accumulation and fp32 LayerNorm / GELU
arithmetic (--acc f64: float64 instead, to see how far the figure moves with the summation alone), one fp16
rounding where a launch stores -- the stem's LayerNorm, dwconv + LayerNorm, each Linear, each block's residual
sum, LayerNorm + space to depth, each downsample, pool + LayerNorm; the stem GEMM and the logits stay fp32.
Prints the normalised max error against the float64 forward of the same module: the figure the fp16 parity
bar of tests/test_convnext_gpu.py is 1.5x of.  Needs torch only (zoo.py is loaded by path, not the package).

  python tools/prec_emulate_convnext.py [--seeds 1 2 3]
"""
import argparse
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


def forward(model, x, r, dt):
    """r = h, dt = float32: the fp16 emulation with fp32 arithmetic; r = identity, dt = float64: the reference."""
    c = lambda t: t.detach().to(dt)  # noqa: E731
    ln = lambda v, m: F.layer_norm(v, m.normalized_shape, c(m.weight), c(m.bias), m.eps)  # noqa: E731
    f = model.features
    y = F.conv2d(r(c(x)), r(c(f[0][0].weight)), c(f[0][0].bias), stride=4).float().to(dt)
    y = r(ln(y.permute(0, 2, 3, 1), f[0][1]))  # NHWC from here on
    for layer in list(f)[1:]:
        if isinstance(layer[0], zoo.CNBlock):
            for blk in layer:
                dw, _, norm, fc1, _, fc2, _ = blk.block
                a = F.conv2d(y.permute(0, 3, 1, 2), r(c(dw.weight)), c(dw.bias), padding=3, groups=y.shape[-1])
                a = r(ln(a.permute(0, 2, 3, 1), norm))
                a = r(F.gelu(a @ r(c(fc1.weight)).T + c(fc1.bias)))
                g = blk.layer_scale.detach().float().reshape(-1)  # the packer folds layer_scale in fp32
                y = r(a @ r(c(g[:, None] * fc2.weight.detach().float())).T + c(g * fc2.bias.detach().float()) + y)
        else:
            a = r(ln(y, layer[0])).permute(0, 3, 1, 2)
            y = r(F.conv2d(a, r(c(layer[1].weight)), c(layer[1].bias), stride=2).permute(0, 2, 3, 1))
    p = r(ln(y.mean((1, 2)), model.classifier[0]))
    return (p @ r(c(model.classifier[2].weight)).T + c(model.classifier[2].bias)).double()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, nargs="*", default=[1])
    ap.add_argument("--depths", type=int, nargs=4, default=[1, 1, 2, 1])
    ap.add_argument("--dims", type=int, nargs=4, default=[96, 192, 384, 768])
    ap.add_argument("--acc", choices=["f32", "f64"], default="f32")
    a = ap.parse_args()
    model = zoo.convnext(a.depths, a.dims, image=64, num_classes=10)
    for seed in a.seeds:
        x = torch.from_numpy(np.random.default_rng(seed).random((2, 3, 64, 64), dtype=np.float32))
        with torch.no_grad():
            ref = forward(model, x, lambda t: t, torch.float64)
            emu = forward(model, x, h, torch.float32 if a.acc == "f32" else torch.float64)
        per_image = ((emu - ref).abs().amax(1) / ref.abs().max()).tolist()
        print(f"dims {a.dims} input seed {seed} acc {a.acc}: fp16 emulation {max(per_image):.3e} (per image "
              + ", ".join(f"{e:.3e}" for e in per_image) + ")")


if __name__ == "__main__":
    main()

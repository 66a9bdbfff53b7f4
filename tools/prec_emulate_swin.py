#!/usr/bin/env python3
"""CPU emulation of the fp16 number formats of a Swin replica (tools/prec_emulate.py's method: it emulates the
formats, not the kernels): fp16-rounded weights and GEMM / attention operands, fp32 accumulation and fp32
LayerNorm / GELU / softmax arithmetic (--acc f64: float64 instead), one fp16 rounding where a launch stores -- each
LayerNorm, the QKV rows, the attention's P (its PV operand) and context, each Linear with its residual sum, the
merge's gathered + normalised rows and its Linear; the stem GEMM, the relative-position bias and the logits stay
fp32.  Prints the normalised max error against the float64 forward of the same module: the figure the fp16 parity
bar of tests/test_swin_gpu.py is 1.5x of.  Needs torch only (zoo.py is loaded by path, not the package).

  python tools/prec_emulate_swin.py [--seeds 1 2 3] [--embed 64 --heads 2 4 8] [--v2 --image 128]
--v2: zoo.swin_v2 (cosine attention with the norms in the fp32 score epilogue, post-norm blocks, PatchMergingV2).
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


def window_attention(a, qkv, r, c):
    """zoo.ShiftedWindowAttention.forward on given qkv rows [B, H, W, 3C], without proj; P rounded by r."""
    B, H, W, C3 = qkv.shape
    C, ws, N = C3 // 3, a.window, a.window ** 2
    s = 0 if ws >= H else a.shift
    x = torch.roll(qkv, (-s, -s), (1, 2)) if s else qkv
    nw = (H // ws) * (W // ws)
    x = x.view(B, H // ws, ws, W // ws, ws, C3).permute(0, 1, 3, 2, 4, 5).reshape(B * nw, N, 3, a.heads, C // a.heads)
    q, k, v = x.permute(2, 0, 3, 1, 4)
    if isinstance(a, zoo.ShiftedWindowAttentionV2):  # raw operands to the MFMA, the norms and tau in the fp32 epilogue
        qn, kn = (t.norm(dim=-1, keepdim=True).clamp_min(1e-12) for t in (q, k))
        attn = (q @ k.transpose(-2, -1)) / kn.transpose(-2, -1) / qn * c(a.logit_scale).clamp(max=np.log(100.0)).exp()
        attn = attn + c(a.position_bias())
    else:
        attn = (q @ k.transpose(-2, -1)) * (C // a.heads) ** -0.5
        attn = attn + c(a.relative_position_bias_table)[a.relative_position_index].view(N, N, -1).permute(2, 0, 1)
    if s:
        lab = torch.zeros(H, W, dtype=attn.dtype)
        for i, hs in enumerate((slice(0, -ws), slice(-ws, -s), slice(-s, None))):
            for j, wsl in enumerate((slice(0, -ws), slice(-ws, -s), slice(-s, None))):
                lab[hs, wsl] = 3 * i + j
        lab = lab.view(H // ws, ws, W // ws, ws).permute(0, 2, 1, 3).reshape(nw, N)
        mask = (lab[:, :, None] != lab[:, None, :]).to(attn.dtype) * -100.0
        attn = (attn.view(B, nw, a.heads, N, N) + mask[None, :, None]).view(-1, a.heads, N, N)
    p = torch.exp(attn - attn.amax(-1, keepdim=True))
    o = (r(p) @ v) / p.sum(-1, keepdim=True)
    o = o.transpose(1, 2).reshape(B, H // ws, W // ws, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, C)
    return torch.roll(o, (s, s), (1, 2)) if s else o


def forward(model, x, r, dt):
    """r = h, dt = float32: the fp16 emulation with fp32 arithmetic; r = identity, dt = float64: the reference."""
    c = lambda t: t.detach().to(dt)  # noqa: E731
    ln = lambda v, m: F.layer_norm(v, m.normalized_shape, c(m.weight), c(m.bias), m.eps)  # noqa: E731
    lin = lambda v, m: v @ r(c(m.weight)).T + (c(m.bias) if m.bias is not None else 0)  # noqa: E731
    f = model.features
    y = F.conv2d(r(c(x)), r(c(f[0][0].weight)), c(f[0][0].bias), stride=4).permute(0, 2, 3, 1)
    y = r(ln(y, f[0][2]))
    for layer in list(f)[1:]:
        if isinstance(layer, zoo.PatchMerging):
            g = torch.cat([y[:, 0::2, 0::2], y[:, 1::2, 0::2], y[:, 0::2, 1::2], y[:, 1::2, 1::2]], -1)
            y = r(lin(r(ln(g, layer.norm)), layer.reduction))
            continue
        if isinstance(layer, zoo.PatchMergingV2):  # gather, Linear, then the LayerNorm
            g = torch.cat([y[:, 0::2, 0::2], y[:, 1::2, 0::2], y[:, 0::2, 1::2], y[:, 1::2, 1::2]], -1)
            y = r(ln(r(lin(g, layer.reduction)), layer.norm))
            continue
        for blk in layer:
            if isinstance(blk, zoo.SwinTransformerBlockV2):  # post-norm; the K third of the QKV bias is zero
                kb = torch.cat([torch.ones(y.shape[-1]), torch.zeros(y.shape[-1]), torch.ones(y.shape[-1])]).to(dt)
                qkv = r(y @ r(c(blk.attn.qkv.weight)).T + c(blk.attn.qkv.bias) * kb)
                y = r(y + ln(r(lin(r(window_attention(blk.attn, qkv, r, c)), blk.attn.proj)), blk.norm1))
                hid = r(F.gelu(lin(y, blk.mlp[0])))
                y = r(y + ln(r(lin(hid, blk.mlp[3])), blk.norm2))
                continue
            qkv = r(lin(r(ln(y, blk.norm1)), blk.attn.qkv))
            y = r(lin(r(window_attention(blk.attn, qkv, r, c)), blk.attn.proj) + y)
            hid = r(F.gelu(lin(r(ln(y, blk.norm2)), blk.mlp[0])))
            y = r(lin(hid, blk.mlp[3]) + y)
    p = r(ln(y, model.norm))  # avgpool + FC: one GEMM on the normalised rows, the mean in its fp32 epilogue
    return (p @ r(c(model.head.weight)).T).mean((1, 2)).double() + model.head.bias.detach().double()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, nargs="*", default=[1])
    ap.add_argument("--depths", type=int, nargs="*", default=[2, 2, 2])
    ap.add_argument("--heads", type=int, nargs="*", default=[2, 4, 8])
    ap.add_argument("--embed", type=int, default=64)
    ap.add_argument("--image", type=int, default=112)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--acc", choices=["f32", "f64"], default="f32")
    ap.add_argument("--v2", action="store_true", help="zoo.swin_v2 at window 8 (tests/test_swin_v2_gpu.py: --v2 --image 128)")
    a = ap.parse_args()
    model = (zoo.swin_v2(a.depths, a.heads, a.embed, window=8, image=a.image, num_classes=10) if a.v2 else
             zoo.swin(a.depths, a.heads, a.embed, window=7, image=a.image, num_classes=10))
    for seed in a.seeds:
        x = torch.from_numpy(np.random.default_rng(seed).random((a.batch, 3, a.image, a.image), dtype=np.float32))
        with torch.no_grad():
            ref = forward(model, x, lambda t: t, torch.float64)
            emu = forward(model, x, h, torch.float32 if a.acc == "f32" else torch.float64)
            direct = model.double()(x.double())
            model.float()
        per_image = ((emu - ref).abs().amax(1) / ref.abs().max()).tolist()
        print(f"embed {a.embed} heads {a.heads} input seed {seed} acc {a.acc}: fp16 emulation {max(per_image):.3e} (per image "
              + ", ".join(f"{e:.3e}" for e in per_image) + f"); restated forward vs module {float((ref - direct).abs().max()):.1e}")


if __name__ == "__main__":
    main()

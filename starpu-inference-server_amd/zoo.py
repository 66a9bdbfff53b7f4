"""Model zoo: the architectures the reference serves, with seeded random weights.

The reference exports TorchScript files from torchvision / HF
(models/import_resnet.py:25-73, models/import_vit.py:10-62,
models/import_bert-base-uncased.py:8-39).  torchvision is not installed and
nothing can be downloaded, so the ResNet and ViT graphs are re-declared here in
plain ``torch.nn`` with torchvision's parameter names and forward, and BERT is
HF ``transformers.BertModel`` built from a local ``BertConfig`` (bert-base
defaults: 768/12/12/3072/30522, LN eps 1e-12, erf-GELU), wrapped exactly like
the reference's ``BertWrapper`` (returns ``last_hidden_state``).

Weights are random (no checkpoints offline) but deterministic: ``torch`` CPU RNG
seeded per model, then BatchNorm running statistics are calibrated on a seeded
synthetic batch so activations stay O(1) through 150+ layers (as with trained
statistics).  These modules are what the host loads into the HIP replicas and
what the CPU codelet (and the test oracle) runs.
"""
from __future__ import annotations

import math
from collections import OrderedDict
from typing import Sequence

import torch
from torch import nn
from torch.nn import functional as F


# ---------------------------------------------------------------------------
# ResNet (torchvision.models.resnet naming)
# ---------------------------------------------------------------------------
class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes: int, planes: int, stride: int = 1, downsample: nn.Module | None = None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        identity = x
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        if self.downsample is not None:
            identity = self.downsample(x)
        return self.relu(out + identity)


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes: int, planes: int, stride: int = 1, downsample: nn.Module | None = None,
                 groups: int = 1, width_per_group: int = 64):
        super().__init__()
        width = int(planes * width_per_group / 64) * groups  # torchvision's formula (ResNeXt, wide ResNet)
        self.conv1 = nn.Conv2d(inplanes, width, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(width)
        self.conv2 = nn.Conv2d(width, width, 3, stride, 1, groups=groups, bias=False)
        self.bn2 = nn.BatchNorm2d(width)
        self.conv3 = nn.Conv2d(width, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        identity = x
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        if self.downsample is not None:
            identity = self.downsample(x)
        return self.relu(out + identity)


class ResNet(nn.Module):
    def __init__(self, block, layers: Sequence[int], num_classes: int = 1000, width: int = 64, groups: int = 1,
                 width_per_group: int = 64):
        super().__init__()
        self.inplanes = width
        self.groups, self.width_per_group = groups, width_per_group
        self.conv1 = nn.Conv2d(3, width, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(width)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        self.layer1 = self._make_layer(block, width, layers[0])
        self.layer2 = self._make_layer(block, width * 2, layers[1], 2)
        self.layer3 = self._make_layer(block, width * 4, layers[2], 2)
        self.layer4 = self._make_layer(block, width * 8, layers[3], 2)
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(width * 8 * block.expansion, num_classes)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")

    def _make_layer(self, block, planes, blocks, stride=1):
        downsample = None
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(
                nn.Conv2d(self.inplanes, planes * block.expansion, 1, stride, bias=False),
                nn.BatchNorm2d(planes * block.expansion))
        # bottleneck-only keywords; a BasicBlock net takes neither (torchvision raises too)
        kw = {} if (self.groups, self.width_per_group) == (1, 64) else dict(
            groups=self.groups, width_per_group=self.width_per_group)
        layers = [block(self.inplanes, planes, stride, downsample, **kw)]
        self.inplanes = planes * block.expansion
        for _ in range(1, blocks):
            layers.append(block(self.inplanes, planes, **kw))
        return nn.Sequential(*layers)

    def forward(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return self.fc(torch.flatten(self.avgpool(x), 1))


def _randomize_bn_and_calibrate(model: nn.Module, image: int, seed: int, calib_batch: int = 4,
                                normalised_half: bool = False) -> None:
    g = torch.Generator().manual_seed(seed + 1)
    # The last BN of each residual branch gets a small gamma, as in trained
    # ResNets (torchvision's zero_init_residual idea, kept non-zero): with unit
    # gammas a random 50-block ResNet-152 amplifies fp32 rounding to ~5e-4
    # (fp32 vs fp64 on CPU), which would make any parity check meaningless.
    last_bn = set()
    for blk in model.modules():
        if isinstance(blk, Bottleneck):
            last_bn.add(id(blk.bn3))
        elif isinstance(blk, BasicBlock):
            last_bn.add(id(blk.bn2))
        elif isinstance(blk, MBConv) and blk.use_res:
            last_bn.add(id(blk.block[-1][1]))
    for m in model.modules():
        if isinstance(m, nn.BatchNorm2d):
            with torch.no_grad():
                if id(m) in last_bn:
                    m.weight.copy_(0.1 + 0.3 * torch.rand(m.num_features, generator=g))
                else:
                    m.weight.copy_(0.75 + 0.5 * torch.rand(m.num_features, generator=g))
                m.bias.copy_(0.2 * torch.rand(m.num_features, generator=g) - 0.1)
            m.momentum = None  # cumulative average: one pass = that batch's statistics
            m.reset_running_stats()
    x = torch.rand(calib_batch, 3, image, image, generator=g)
    if normalised_half:  # the second half under the ImageNet mean / std: pixels in -2.1 .. 2.6
        mean, std = torch.tensor([0.485, 0.456, 0.406]).view(3, 1, 1), torch.tensor([0.229, 0.224, 0.225]).view(3, 1, 1)
        x[calib_batch // 2:] = (x[calib_batch // 2:] - mean) / std
    model.train()
    with torch.no_grad():
        model(x)
    model.eval()


def resnet(layers: Sequence[int], bottleneck: bool, seed: int = 0, image: int = 224,
           num_classes: int = 1000, calibrate: bool = True, groups: int = 1, width_per_group: int = 64) -> ResNet:
    torch.manual_seed(seed)
    model = ResNet(Bottleneck if bottleneck else BasicBlock, layers, num_classes, groups=groups,
                   width_per_group=width_per_group)
    if calibrate:
        _randomize_bn_and_calibrate(model, image, seed)
    return model.eval()


def resnet18(seed: int = 0, image: int = 224, **kw) -> ResNet:
    return resnet([2, 2, 2, 2], False, seed, image, **kw)


def resnet152(seed: int = 0, image: int = 224, **kw) -> ResNet:
    return resnet([3, 8, 36, 3], True, seed, image, **kw)


# The grouped and wide variants of the reference's export script (models/import_resnet.py).
def resnext50_32x4d(seed: int = 0, image: int = 224, **kw) -> ResNet:
    return resnet([3, 4, 6, 3], True, seed, image, groups=32, width_per_group=4, **kw)


def resnext101_32x8d(seed: int = 0, image: int = 224, **kw) -> ResNet:
    return resnet([3, 4, 23, 3], True, seed, image, groups=32, width_per_group=8, **kw)


def wide_resnet50_2(seed: int = 0, image: int = 224, **kw) -> ResNet:
    return resnet([3, 4, 6, 3], True, seed, image, width_per_group=128, **kw)


def wide_resnet101_2(seed: int = 0, image: int = 224, **kw) -> ResNet:
    return resnet([3, 4, 23, 3], True, seed, image, width_per_group=128, **kw)


# ---------------------------------------------------------------------------
# Vision Transformer (torchvision.models.vision_transformer naming)
# ---------------------------------------------------------------------------
class MLPBlock(nn.Sequential):
    def __init__(self, dim: int, mlp_dim: int):
        super().__init__(nn.Linear(dim, mlp_dim), nn.GELU(), nn.Dropout(0.0), nn.Linear(mlp_dim, dim),
                         nn.Dropout(0.0))


class EncoderBlock(nn.Module):
    def __init__(self, heads: int, dim: int, mlp_dim: int):
        super().__init__()
        self.ln_1 = nn.LayerNorm(dim, eps=1e-6)
        self.self_attention = nn.MultiheadAttention(dim, heads, dropout=0.0, batch_first=True)
        self.dropout = nn.Dropout(0.0)
        self.ln_2 = nn.LayerNorm(dim, eps=1e-6)
        self.mlp = MLPBlock(dim, mlp_dim)

    def forward(self, inp):
        x = self.ln_1(inp)
        x, _ = self.self_attention(x, x, x, need_weights=False)
        x = self.dropout(x) + inp
        y = self.mlp(self.ln_2(x))
        return x + y


class Encoder(nn.Module):
    def __init__(self, seq: int, layers: int, heads: int, dim: int, mlp_dim: int):
        super().__init__()
        self.pos_embedding = nn.Parameter(torch.empty(1, seq, dim).normal_(std=0.02))
        self.dropout = nn.Dropout(0.0)
        self.layers = nn.Sequential(OrderedDict(
            (f"encoder_layer_{i}", EncoderBlock(heads, dim, mlp_dim)) for i in range(layers)))
        self.ln = nn.LayerNorm(dim, eps=1e-6)

    def forward(self, x):
        return self.ln(self.layers(self.dropout(x + self.pos_embedding)))


class VisionTransformer(nn.Module):
    def __init__(self, image: int, patch: int, layers: int, heads: int, dim: int, mlp_dim: int,
                 num_classes: int = 1000):
        super().__init__()
        self.image_size, self.patch_size, self.hidden_dim = image, patch, dim
        self.conv_proj = nn.Conv2d(3, dim, patch, patch)
        self.class_token = nn.Parameter(torch.zeros(1, 1, dim))
        seq = (image // patch) ** 2 + 1
        self.encoder = Encoder(seq, layers, heads, dim, mlp_dim)
        self.heads = nn.Sequential(OrderedDict(head=nn.Linear(dim, num_classes)))

    def _process_input(self, x):
        n = x.shape[0]
        x = self.conv_proj(x)
        x = x.reshape(n, self.hidden_dim, -1)
        return x.permute(0, 2, 1)

    def forward(self, x):
        x = self._process_input(x)
        cls = self.class_token.expand(x.shape[0], -1, -1)
        x = self.encoder(torch.cat([cls, x], dim=1))
        return self.heads(x[:, 0])


def vit(image: int = 224, patch: int = 16, layers: int = 24, heads: int = 16, dim: int = 1024,
        mlp_dim: int = 4096, num_classes: int = 1000, seed: int = 0) -> VisionTransformer:
    torch.manual_seed(seed)
    model = VisionTransformer(image, patch, layers, heads, dim, mlp_dim, num_classes)
    with torch.no_grad():
        # torchvision zero-initialises class_token and the head, which would make
        # every logit equal; random values keep the parity check meaningful.
        model.class_token.normal_(std=0.02)
        model.heads.head.weight.normal_(std=0.02)
        model.heads.head.bias.normal_(std=0.02)
        for m in model.modules():
            if isinstance(m, nn.LayerNorm):
                m.weight.copy_(1.0 + 0.1 * torch.randn_like(m.weight))
                m.bias.copy_(0.05 * torch.randn_like(m.bias))
    return model.eval()


def vit_l_16(seed: int = 0, image: int = 224, **kw) -> VisionTransformer:
    return vit(image, 16, 24, 16, 1024, 4096, seed=seed, **kw)


# ---------------------------------------------------------------------------
# ConvNeXt (torchvision.models.convnext naming)
# ---------------------------------------------------------------------------
class LayerNorm2d(nn.LayerNorm):
    def forward(self, x):
        x = x.permute(0, 2, 3, 1)
        x = nn.functional.layer_norm(x, self.normalized_shape, self.weight, self.bias, self.eps)
        return x.permute(0, 3, 1, 2)


class Permute(nn.Module):
    def __init__(self, dims):
        super().__init__()
        self.dims = list(dims)

    def forward(self, x):
        return torch.permute(x, self.dims)


class CNBlock(nn.Module):
    def __init__(self, dim: int, layer_scale: float = 1e-6):
        super().__init__()
        self.block = nn.Sequential(
            nn.Conv2d(dim, dim, 7, padding=3, groups=dim, bias=True), Permute([0, 2, 3, 1]),
            nn.LayerNorm(dim, eps=1e-6), nn.Linear(dim, 4 * dim), nn.GELU(), nn.Linear(4 * dim, dim),
            Permute([0, 3, 1, 2]))
        self.layer_scale = nn.Parameter(torch.ones(dim, 1, 1) * layer_scale)

    def forward(self, x):  # eval: stochastic depth is the identity
        return x + self.layer_scale * self.block(x)


class ConvNeXt(nn.Module):
    def __init__(self, depths: Sequence[int], dims: Sequence[int], num_classes: int = 1000):
        super().__init__()
        layers = [nn.Sequential(nn.Conv2d(3, dims[0], 4, 4), LayerNorm2d(dims[0], eps=1e-6))]
        for i, (depth, dim) in enumerate(zip(depths, dims)):
            if i > 0:
                layers.append(nn.Sequential(LayerNorm2d(dims[i - 1], eps=1e-6), nn.Conv2d(dims[i - 1], dim, 2, 2)))
            layers.append(nn.Sequential(*[CNBlock(dim) for _ in range(depth)]))
        self.features = nn.Sequential(*layers)
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.classifier = nn.Sequential(LayerNorm2d(dims[-1], eps=1e-6), nn.Flatten(1), nn.Linear(dims[-1], num_classes))

    def forward(self, x):
        return self.classifier(self.avgpool(self.features(x)))


def convnext(depths: Sequence[int], dims: Sequence[int], image: int = 224, num_classes: int = 1000,
             seed: int = 0) -> ConvNeXt:
    """ConvNeXt with seeded random weights (image only documents the size the model is meant for).
    torchvision initialises layer_scale to 1e-6 and the weights to N(0, 0.02^2), which would hide every
    block behind its residual: here layer_scale is drawn from U(0.05, 0.3), conv and linear weights from
    N(0, 1 / fan_in) with biases N(0, 0.05^2), and the LayerNorm gains and biases are re-drawn as vit()
    does, so that a wrong block shows in the logits."""
    torch.manual_seed(seed)
    model = ConvNeXt(depths, dims, num_classes)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                fan_in = m.weight[0].numel()
                m.weight.normal_(std=fan_in ** -0.5)
                m.bias.normal_(std=0.05)
            elif isinstance(m, nn.LayerNorm):
                m.weight.copy_(1.0 + 0.1 * torch.randn_like(m.weight))
                m.bias.copy_(0.05 * torch.randn_like(m.bias))
            elif isinstance(m, CNBlock):
                m.layer_scale.uniform_(0.05, 0.3)
    return model.eval()


def convnext_tiny(seed: int = 0, image: int = 224, **kw) -> ConvNeXt:
    return convnext([3, 3, 9, 3], [96, 192, 384, 768], image, seed=seed, **kw)


def convnext_small(seed: int = 0, image: int = 224, **kw) -> ConvNeXt:
    return convnext([3, 3, 27, 3], [96, 192, 384, 768], image, seed=seed, **kw)


def convnext_base(seed: int = 0, image: int = 224, **kw) -> ConvNeXt:
    return convnext([3, 3, 27, 3], [128, 256, 512, 1024], image, seed=seed, **kw)


def convnext_large(seed: int = 0, image: int = 224, **kw) -> ConvNeXt:
    return convnext([3, 3, 27, 3], [192, 384, 768, 1536], image, seed=seed, **kw)


# ---------------------------------------------------------------------------
# Swin Transformer (torchvision.models.swin_transformer naming, v1 and v2 blocks)
# ---------------------------------------------------------------------------
class ShiftedWindowAttention(nn.Module):
    def __init__(self, dim: int, window: int, shift: int, heads: int):
        super().__init__()
        self.window, self.shift, self.heads = window, shift, heads
        self.qkv = nn.Linear(dim, 3 * dim)
        self.proj = nn.Linear(dim, dim)
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * window - 1) ** 2, heads))
        coords = torch.stack(torch.meshgrid(torch.arange(window), torch.arange(window), indexing="ij")).flatten(1)
        rel = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0) + (window - 1)
        self.register_buffer("relative_position_index", (rel[:, :, 0] * (2 * window - 1) + rel[:, :, 1]).flatten())

    def forward(self, x):  # [B, H, W, C]; H and W multiples of the window (torchvision pads otherwise)
        B, H, W, C = x.shape
        ws, N = self.window, self.window ** 2
        sy, sx = (0 if ws >= H else self.shift), (0 if ws >= W else self.shift)
        if sy or sx:
            x = torch.roll(x, shifts=(-sy, -sx), dims=(1, 2))
        nw = (H // ws) * (W // ws)
        x = x.view(B, H // ws, ws, W // ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B * nw, N, C)
        qkv = self.project_qkv(x).reshape(B * nw, N, 3, self.heads, C // self.heads).permute(2, 0, 3, 1, 4)
        v = qkv[2]
        attn = self.logits(qkv[0], qkv[1]) + self.position_bias().unsqueeze(0)
        if sy or sx:
            mask = x.new_zeros((H, W))
            count = 0
            for h in ((0, -ws), (-ws, -sy), (-sy, None)):
                for w in ((0, -ws), (-ws, -sx), (-sx, None)):
                    mask[h[0]:h[1], w[0]:w[1]] = count
                    count += 1
            mask = mask.view(H // ws, ws, W // ws, ws).permute(0, 2, 1, 3).reshape(nw, N)
            mask = mask.unsqueeze(1) - mask.unsqueeze(2)
            mask = mask.masked_fill(mask != 0, -100.0)
            attn = attn.view(B, nw, self.heads, N, N) + mask.unsqueeze(1).unsqueeze(0)
            attn = attn.view(-1, self.heads, N, N)
        x = (attn.softmax(-1) @ v).transpose(1, 2).reshape(B * nw, N, C)
        x = self.proj(x)
        x = x.view(B, H // ws, W // ws, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, C)
        if sy or sx:
            x = torch.roll(x, shifts=(sy, sx), dims=(1, 2))
        return x


    def project_qkv(self, x):
        return self.qkv(x)

    def logits(self, q, k):
        return (q * q.shape[-1] ** -0.5) @ k.transpose(-2, -1)

    def position_bias(self):  # [heads, N, N]
        N = self.window ** 2
        return self.relative_position_bias_table[self.relative_position_index].view(N, N, -1).permute(2, 0, 1)


class ShiftedWindowAttentionV2(ShiftedWindowAttention):
    """torchvision's v2 attention: cosine scores under a learnt per-head temperature clamped at 100, the bias
    16 sigmoid(cpb_mlp(log-spaced relative coordinates)), and a K projection without bias (zeroed on every call)."""

    def __init__(self, dim: int, window: int, shift: int, heads: int):
        super().__init__(dim, window, shift, heads)
        del self.relative_position_bias_table
        self.logit_scale = nn.Parameter(torch.log(10 * torch.ones((heads, 1, 1))))
        self.cpb_mlp = nn.Sequential(nn.Linear(2, 512, bias=True), nn.ReLU(inplace=True), nn.Linear(512, heads, bias=False))
        r = torch.arange(-(window - 1), window, dtype=torch.float32)
        table = torch.stack(torch.meshgrid([r, r], indexing="ij")).permute(1, 2, 0).contiguous().unsqueeze(0)
        table = table / (window - 1) * 8
        self.register_buffer("relative_coords_table", torch.sign(table) * torch.log2(torch.abs(table) + 1.0) / 3.0)

    def project_qkv(self, x):
        bias, n = self.qkv.bias.clone(), self.qkv.bias.numel() // 3
        bias[n:2 * n].zero_()
        return F.linear(x, self.qkv.weight, bias)

    def logits(self, q, k):
        attn = F.normalize(q, dim=-1) @ F.normalize(k, dim=-1).transpose(-2, -1)
        return attn * torch.clamp(self.logit_scale, max=math.log(100.0)).exp()

    def position_bias(self):
        N = self.window ** 2
        table = self.cpb_mlp(self.relative_coords_table).view(-1, self.heads)
        return 16 * torch.sigmoid(table[self.relative_position_index].view(N, N, -1).permute(2, 0, 1))


class SwinTransformerBlock(nn.Module):
    attention = ShiftedWindowAttention

    def __init__(self, dim: int, heads: int, window: int, shift: int):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=1e-5)
        self.attn = self.attention(dim, window, shift, heads)
        self.norm2 = nn.LayerNorm(dim, eps=1e-5)
        self.mlp = nn.Sequential(nn.Linear(dim, 4 * dim), nn.GELU(), nn.Dropout(0.0), nn.Linear(4 * dim, dim), nn.Dropout(0.0))

    def forward(self, x):  # eval: stochastic depth is the identity
        x = x + self.attn(self.norm1(x))
        return x + self.mlp(self.norm2(x))


class SwinTransformerBlockV2(SwinTransformerBlock):  # residual-post-norm
    attention = ShiftedWindowAttentionV2

    def forward(self, x):
        x = x + self.norm1(self.attn(x))
        return x + self.norm2(self.mlp(x))


class PatchMerging(nn.Module):
    def __init__(self, dim: int):
        super().__init__()
        self.reduction = nn.Linear(4 * dim, 2 * dim, bias=False)
        self.norm = nn.LayerNorm(4 * dim, eps=1e-5)

    def forward(self, x):  # [B, H, W, C] -> [B, H/2, W/2, 2C]
        x = torch.cat([x[..., 0::2, 0::2, :], x[..., 1::2, 0::2, :], x[..., 0::2, 1::2, :], x[..., 1::2, 1::2, :]], -1)
        return self.reduction(self.norm(x))


class PatchMergingV2(nn.Module):
    def __init__(self, dim: int):
        super().__init__()
        self.reduction = nn.Linear(4 * dim, 2 * dim, bias=False)
        self.norm = nn.LayerNorm(2 * dim, eps=1e-5)

    def forward(self, x):  # the LayerNorm behind the Linear
        x = torch.cat([x[..., 0::2, 0::2, :], x[..., 1::2, 0::2, :], x[..., 0::2, 1::2, :], x[..., 1::2, 1::2, :]], -1)
        return self.norm(self.reduction(x))


class SwinTransformer(nn.Module):
    def __init__(self, depths: Sequence[int], heads: Sequence[int], embed: int, window: int = 7, num_classes: int = 1000,
                 v2: bool = False):
        super().__init__()
        block, merge = (SwinTransformerBlockV2, PatchMergingV2) if v2 else (SwinTransformerBlock, PatchMerging)
        layers = [nn.Sequential(nn.Conv2d(3, embed, 4, 4), Permute([0, 2, 3, 1]), nn.LayerNorm(embed, eps=1e-5))]
        for i, (depth, nh) in enumerate(zip(depths, heads)):
            dim = embed * 2 ** i
            if i > 0:
                layers.append(merge(dim // 2))
            layers.append(nn.Sequential(*[block(dim, nh, window, 0 if j % 2 == 0 else window // 2)
                                          for j in range(depth)]))
        self.features = nn.Sequential(*layers)
        feat = embed * 2 ** (len(depths) - 1)
        self.norm = nn.LayerNorm(feat, eps=1e-5)
        self.permute = Permute([0, 3, 1, 2])
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.flatten = nn.Flatten(1)
        self.head = nn.Linear(feat, num_classes)

    def forward(self, x):
        return self.head(self.flatten(self.avgpool(self.permute(self.norm(self.features(x))))))


def swin(depths: Sequence[int], heads: Sequence[int], embed: int, window: int = 7, image: int = 224,
         num_classes: int = 1000, seed: int = 0) -> SwinTransformer:
    """Swin Transformer (v1) with seeded random weights (image only documents the size the model is meant for).
    torchvision's trunc_normal(0.02) init would leave the relative-position bias and every block's branch far
    below the residual stream (the ConvNeXt note above): here conv and linear weights are N(0, 1 / fan_in) with
    biases N(0, 0.05^2), LayerNorm gains and biases are re-drawn as vit() does, and the bias tables are N(0, 1),
    the size of the scaled q k^T scores, so that a wrong bias index, mask or block shows in the logits."""
    torch.manual_seed(seed)
    model = SwinTransformer(depths, heads, embed, window, num_classes)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                m.weight.normal_(std=m.weight[0].numel() ** -0.5)
                if m.bias is not None:
                    m.bias.normal_(std=0.05)
            elif isinstance(m, nn.LayerNorm):
                m.weight.copy_(1.0 + 0.1 * torch.randn_like(m.weight))
                m.bias.copy_(0.05 * torch.randn_like(m.bias))
            elif isinstance(m, ShiftedWindowAttention):
                m.relative_position_bias_table.normal_()
    return model.eval()


def swin_v2(depths: Sequence[int], heads: Sequence[int], embed: int, window: int = 8, image: int = 256,
            num_classes: int = 1000, seed: int = 0) -> SwinTransformer:
    """Swin Transformer v2 (torchvision's swin_v2_* naming and forward) with seeded random weights, initialised
    in the spirit of swin(): N(0, 1 / fan_in) weights, re-drawn LayerNorms.  logit_scale is uniform in
    log 3 .. log 200, so the heads' temperatures span 3 .. 100 and about a sixth of them sit at the clamp;
    cpb_mlp's second layer is four times N(0, 1 / 512) and its first bias N(0, 0.5^2), so the bias
    16 sigmoid(.) ranges over several units inside a window.  The post-norm branches are LayerNorm outputs
    (unit size) beside a residual stream that starts at unit size: none is negligible."""
    torch.manual_seed(seed)
    model = SwinTransformer(depths, heads, embed, window, num_classes, v2=True)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                m.weight.normal_(std=m.weight[0].numel() ** -0.5)
                if m.bias is not None:
                    m.bias.normal_(std=0.05)
            elif isinstance(m, nn.LayerNorm):
                m.weight.copy_(1.0 + 0.1 * torch.randn_like(m.weight))
                m.bias.copy_(0.05 * torch.randn_like(m.bias))
        for m in model.modules():
            if isinstance(m, ShiftedWindowAttentionV2):
                m.logit_scale.uniform_(math.log(3.0), math.log(200.0))
                m.cpb_mlp[0].bias.normal_(std=0.5)
                m.cpb_mlp[2].weight.mul_(4.0)
    return model.eval()


def swin_v2_t(seed: int = 0, image: int = 256, **kw) -> SwinTransformer:
    return swin_v2([2, 2, 6, 2], [3, 6, 12, 24], 96, image=image, seed=seed, **kw)


def swin_v2_s(seed: int = 0, image: int = 256, **kw) -> SwinTransformer:
    return swin_v2([2, 2, 18, 2], [3, 6, 12, 24], 96, image=image, seed=seed, **kw)


def swin_v2_b(seed: int = 0, image: int = 256, **kw) -> SwinTransformer:
    return swin_v2([2, 2, 18, 2], [4, 8, 16, 32], 128, image=image, seed=seed, **kw)


def swin_t(seed: int = 0, image: int = 224, **kw) -> SwinTransformer:
    return swin([2, 2, 6, 2], [3, 6, 12, 24], 96, image=image, seed=seed, **kw)


def swin_s(seed: int = 0, image: int = 224, **kw) -> SwinTransformer:
    return swin([2, 2, 18, 2], [3, 6, 12, 24], 96, image=image, seed=seed, **kw)


def swin_b(seed: int = 0, image: int = 224, **kw) -> SwinTransformer:
    return swin([2, 2, 18, 2], [4, 8, 16, 32], 128, image=image, seed=seed, **kw)


# ---------------------------------------------------------------------------
# EfficientNet (torchvision.models.efficientnet naming, b0 .. b7)
# ---------------------------------------------------------------------------
def _make_divisible(v: float, divisor: int = 8) -> int:
    new_v = max(divisor, int(v + divisor / 2) // divisor * divisor)
    return new_v + divisor if new_v < 0.9 * v else new_v


def _conv_bn_act(cin: int, cout: int, k: int, stride: int = 1, groups: int = 1, act: bool = True) -> nn.Sequential:
    layers = [nn.Conv2d(cin, cout, k, stride, (k - 1) // 2, groups=groups, bias=False), nn.BatchNorm2d(cout, eps=1e-5)]
    return nn.Sequential(*layers, nn.SiLU()) if act else nn.Sequential(*layers)


class SqueezeExcitation(nn.Module):
    def __init__(self, channels: int, squeeze: int):
        super().__init__()
        self.fc1 = nn.Conv2d(channels, squeeze, 1)
        self.fc2 = nn.Conv2d(squeeze, channels, 1)

    def forward(self, x):
        s = nn.functional.silu(self.fc1(x.mean((2, 3), keepdim=True)))
        return x * torch.sigmoid(self.fc2(s))


class MBConv(nn.Module):
    def __init__(self, expand: int, k: int, stride: int, cin: int, cout: int):
        super().__init__()
        self.use_res = stride == 1 and cin == cout
        mid = _make_divisible(cin * expand)
        layers = [_conv_bn_act(cin, mid, 1)] if mid != cin else []
        layers += [_conv_bn_act(mid, mid, k, stride, groups=mid), SqueezeExcitation(mid, max(1, cin // 4)),
                   _conv_bn_act(mid, cout, 1, act=False)]
        self.block = nn.Sequential(*layers)

    def forward(self, x):  # eval: stochastic depth is the identity
        return x + self.block(x) if self.use_res else self.block(x)


# (expand, kernel, stride, in, out, layers) of efficientnet_b0; width_mult scales in / out, depth_mult the layers
_MBCONV_SETTINGS = [(1, 3, 1, 32, 16, 1), (6, 3, 2, 16, 24, 2), (6, 5, 2, 24, 40, 2), (6, 3, 2, 40, 80, 3),
                    (6, 5, 1, 80, 112, 3), (6, 5, 2, 112, 192, 4), (6, 3, 1, 192, 320, 1)]


class EfficientNet(nn.Module):
    def __init__(self, width_mult: float, depth_mult: float, num_classes: int = 1000):
        super().__init__()
        ch = lambda c: _make_divisible(c * width_mult)  # noqa: E731
        layers = [_conv_bn_act(3, ch(_MBCONV_SETTINGS[0][3]), 3, 2)]
        for expand, k, stride, cin, cout, n in _MBCONV_SETTINGS:
            stage = [MBConv(expand, k, stride if i == 0 else 1, ch(cin) if i == 0 else ch(cout), ch(cout))
                     for i in range(int(math.ceil(n * depth_mult)))]
            layers.append(nn.Sequential(*stage))
        last = ch(_MBCONV_SETTINGS[-1][4])
        layers.append(_conv_bn_act(last, 4 * last, 1))
        self.features = nn.Sequential(*layers)
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.classifier = nn.Sequential(nn.Dropout(0.2), nn.Linear(4 * last, num_classes))

    def forward(self, x):
        return self.classifier(torch.flatten(self.avgpool(self.features(x)), 1))


def efficientnet(width_mult: float = 1.0, depth_mult: float = 1.0, image: int = 224, num_classes: int = 1000,
                 seed: int = 0) -> EfficientNet:
    """EfficientNet with seeded random weights: conv and linear weights N(0, 1 / fan_in), the squeeze-and-
    excitation biases N(0, 0.5^2) so that the gates spread over (0, 1), BatchNorm gains and biases as resnet() sets
    them: a wrong block, gate or stride shows in the logits.  The running statistics come from one calibration pass
    over 32 images at 64 pixels (fewer as the image grows, 4 at the least), half of them uniform in [0, 1] and half
    under the ImageNet mean / std, so that the net stays inside its calibrated range for both kinds of input.
    Calibrated on 4 uniform images alone, the BatchNorms behind near-constant SiLU channels amplified a rounding
    60-fold (fp32 against float64: 3.5e-6, and 4.2e-5 on a normalised image); this recipe gives 5e-7 and 2e-6."""
    torch.manual_seed(seed)
    model = EfficientNet(width_mult, depth_mult, num_classes)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                m.weight.normal_(std=m.weight[0].numel() ** -0.5)
                if m.bias is not None:
                    m.bias.normal_(std=0.5 if isinstance(m, nn.Conv2d) else 0.05)
    calib = max(4, min(32, 32 * 64 * 64 // (image * image) // 2 * 2))
    _randomize_bn_and_calibrate(model, image, seed, calib_batch=calib, normalised_half=True)
    return model.eval()


# (width_mult, depth_mult, image) of torchvision's efficientnet_b0 .. _b7
_EFFICIENTNETS = {"efficientnet_b0": (1.0, 1.0, 224), "efficientnet_b1": (1.0, 1.1, 240), "efficientnet_b2": (1.1, 1.2, 288),
                  "efficientnet_b3": (1.2, 1.4, 320), "efficientnet_b4": (1.4, 1.8, 384), "efficientnet_b5": (1.6, 2.2, 456),
                  "efficientnet_b6": (1.8, 2.6, 528), "efficientnet_b7": (2.0, 3.1, 600)}


def _efficientnet_named(name: str):
    def make(seed: int = 0, image: int | None = None, **kw) -> EfficientNet:
        w, d, size = _EFFICIENTNETS[name]
        return efficientnet(w, d, size if image is None else image, seed=seed, **kw)
    return make


(efficientnet_b0, efficientnet_b1, efficientnet_b2, efficientnet_b3, efficientnet_b4, efficientnet_b5, efficientnet_b6,
 efficientnet_b7) = (_efficientnet_named(_n) for _n in sorted(_EFFICIENTNETS))


# ---------------------------------------------------------------------------
# BERT (HF transformers BertModel, wrapped like models/import_bert-base-uncased.py)
# ---------------------------------------------------------------------------
class BertWrapper(nn.Module):
    def __init__(self, bert: nn.Module):
        super().__init__()
        self.bert = bert

    def forward(self, input_ids: torch.Tensor, attention_mask: torch.Tensor) -> torch.Tensor:
        return self.bert(input_ids=input_ids, attention_mask=attention_mask, return_dict=False)[0]


class BertTupleWrapper(nn.Module):
    """HF's own output: (last_hidden_state, pooler_output), what a replica with bert_io "pooler" serves."""

    def __init__(self, bert: nn.Module):
        super().__init__()
        self.bert = bert

    def forward(self, input_ids: torch.Tensor, attention_mask: torch.Tensor):
        out = self.bert(input_ids=input_ids, attention_mask=attention_mask, return_dict=False)
        return out[0], out[1]


class BertSegmentsWrapper(nn.Module):
    """BertWrapper with the third input of sentence-pair tasks (bert_io "token_types")."""

    def __init__(self, bert: nn.Module):
        super().__init__()
        self.bert = bert

    def forward(self, input_ids: torch.Tensor, attention_mask: torch.Tensor,
                token_type_ids: torch.Tensor) -> torch.Tensor:
        return self.bert(input_ids=input_ids, attention_mask=attention_mask, token_type_ids=token_type_ids,
                         return_dict=False)[0]


class BertHeadWrapper(nn.Module):
    """A fine-tuned HF head model (BertForSequenceClassification, BertForTokenClassification or
    BertForQuestionAnswering, eval) returning HF's tuple as a replica with a task head serves it:
    last_hidden_state and pooler_output first, where `outputs` names them ("hidden", "pooler"), then the
    logits -- [B,L] ("sequence"), [B,S,L] ("token"), or start and end logits [B,S] each ("qa").  The
    parameters are model.bert.* beside model.classifier.* / model.qa_outputs.*, as HF names them.
    A RoBERTa head model (model.roberta.*) is wrapped the same way; its sequence head has no pooler and is
    the two-layer model.classifier(last_hidden_state) (classifier.dense + tanh, classifier.out_proj)."""

    def __init__(self, model: nn.Module, head: str, outputs=("hidden",)):
        super().__init__()
        if head not in ("sequence", "token", "qa"):
            raise ValueError(f"unknown BERT head {head!r}; known: 'sequence', 'token', 'qa'")
        if "pooler" in outputs and (head != "sequence" or not hasattr(model, "bert")):
            raise ValueError("HF's token and QA head models, and RoBERTa's, have no pooler (add_pooling_layer=False)")
        self.model = model
        self.head = head
        self.outputs = tuple(outputs)

    @property
    def bert(self) -> nn.Module:
        for name in ("bert", "roberta", "mpnet"):  # HF's attribute for the encoder of a head model
            if hasattr(self.model, name):
                return getattr(self.model, name)
        raise AttributeError("BertHeadWrapper: the head model has no .bert, .roberta or .mpnet")

    def forward(self, input_ids: torch.Tensor, attention_mask: torch.Tensor):
        out = self.bert(input_ids=input_ids, attention_mask=attention_mask, return_dict=False)
        hidden = out[0]
        res = []
        if "hidden" in self.outputs:
            res.append(hidden)
        if "pooler" in self.outputs:
            res.append(out[1])
        if self.head == "sequence" and not hasattr(self.model, "bert"):
            res.append(self.model.classifier(hidden))
        elif self.head == "sequence":
            res.append(self.model.classifier(self.model.dropout(out[1])))
        elif self.head == "token":
            res.append(self.model.classifier(self.model.dropout(hidden)))
        else:
            start, end = self.model.qa_outputs(hidden).split(1, dim=-1)
            res += [start.squeeze(-1).contiguous(), end.squeeze(-1).contiguous()]
        return tuple(res)


def bert(layers: int = 12, hidden: int = 768, heads: int = 12, intermediate: int = 3072,
         vocab: int = 30522, max_position: int = 512, seed: int = 0, init_std: float = 0.02,
         head: str | None = None, num_labels: int = 2, outputs=("hidden",)) -> nn.Module:
    """BertModel in BertWrapper; with head = "sequence" | "token" | "qa" the HF head model of num_labels
    labels (QA: 2) in BertHeadWrapper, which returns the `outputs` it names, then the logits."""
    import logging

    from transformers import (BertConfig, BertForQuestionAnswering, BertForSequenceClassification,
                              BertForTokenClassification, BertModel)
    from transformers.utils import logging as hf_logging

    hf_logging.set_verbosity_error()
    logging.getLogger("transformers").setLevel(logging.ERROR)
    torch.manual_seed(seed)
    cfg = BertConfig(num_hidden_layers=layers, hidden_size=hidden, num_attention_heads=heads,
                     intermediate_size=intermediate, vocab_size=vocab, max_position_embeddings=max_position,
                     initializer_range=init_std, torchscript=True)
    if head is None:
        model = BertWrapper(BertModel(cfg))
    else:
        cfg.num_labels = 2 if head == "qa" else num_labels
        hf = {"sequence": BertForSequenceClassification, "token": BertForTokenClassification,
              "qa": BertForQuestionAnswering}
        if head not in hf:
            raise ValueError(f"unknown BERT head {head!r}; known: {sorted(hf)}")
        model = BertHeadWrapper(hf[head](cfg), head, outputs)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, nn.LayerNorm):
                m.weight.copy_(1.0 + 0.1 * torch.randn_like(m.weight))
                m.bias.copy_(0.05 * torch.randn_like(m.bias))
        if head is not None:
            # HF's 0.02 init gives logits too small for a normalised comparison to mean anything (the
            # reason vit() re-draws its head): weights from N(0, 1/D), bias from N(0, 0.1^2)
            dense = model.model.qa_outputs if head == "qa" else model.model.classifier
            dense.weight.copy_(torch.randn_like(dense.weight) / hidden ** 0.5)
            dense.bias.copy_(0.1 * torch.randn_like(dense.bias))
    return model.eval()


def bert_base(seed: int = 0, **kw) -> BertWrapper:
    return bert(seed=seed, **kw)


def minilm_l6(seed: int = 0, **kw) -> BertWrapper:
    """all-MiniLM-L6-H384's graph: 6 layers, hidden 384 over 12 heads of 32, FFN 1536."""
    return bert(**{**dict(layers=6, hidden=384, heads=12, intermediate=1536), **kw}, seed=seed)


def minilm_l12(seed: int = 0, **kw) -> BertWrapper:
    """all-MiniLM-L12-H384's graph: minilm_l6 with 12 layers."""
    return bert(**{**dict(layers=12, hidden=384, heads=12, intermediate=1536), **kw}, seed=seed)


def roberta(layers: int = 12, hidden: int = 768, heads: int = 12, intermediate: int = 3072,
            vocab: int = 50265, max_position: int = 514, seed: int = 0, init_std: float = 0.02,
            head: str | None = None, num_labels: int = 2, outputs=("hidden",)) -> nn.Module:
    """HF RobertaModel in BertWrapper (type_vocab_size 1, pad_token_id 1, layer_norm_eps 1e-5: the published
    checkpoints' values); with head = "sequence" | "token" | "qa" the HF head model in BertHeadWrapper.  A
    replica serves it with bert_io "roberta_positions", which ModelReplica sets by itself from the config.
    max_position counts the table's rows: the longest sequence is max_position - 2.  Position row 1, the
    pad token's, is drawn like the others (HF zeroes it), so a kernel that skipped it would show."""
    import logging

    from transformers import (RobertaConfig, RobertaForQuestionAnswering, RobertaForSequenceClassification,
                              RobertaForTokenClassification, RobertaModel)
    from transformers.utils import logging as hf_logging

    hf_logging.set_verbosity_error()
    logging.getLogger("transformers").setLevel(logging.ERROR)
    torch.manual_seed(seed)
    cfg = RobertaConfig(num_hidden_layers=layers, hidden_size=hidden, num_attention_heads=heads,
                        intermediate_size=intermediate, vocab_size=vocab, max_position_embeddings=max_position,
                        type_vocab_size=1, pad_token_id=1, bos_token_id=0, eos_token_id=2, layer_norm_eps=1e-5,
                        initializer_range=init_std, torchscript=True)
    if head is None:
        model = BertWrapper(RobertaModel(cfg))
    else:
        cfg.num_labels = 2 if head == "qa" else num_labels
        hf = {"sequence": RobertaForSequenceClassification, "token": RobertaForTokenClassification,
              "qa": RobertaForQuestionAnswering}
        if head not in hf:
            raise ValueError(f"unknown BERT head {head!r}; known: {sorted(hf)}")
        model = BertHeadWrapper(hf[head](cfg), head, outputs)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, nn.LayerNorm):
                m.weight.copy_(1.0 + 0.1 * torch.randn_like(m.weight))
                m.bias.copy_(0.05 * torch.randn_like(m.bias))
        pos = model.bert.embeddings.position_embeddings.weight
        pos[1].copy_(init_std * torch.randn_like(pos[1]))
        if head is not None:  # bert()'s re-draw, for the same reason; the two-layer head's first layer too
            inner = model.model
            dense = [inner.qa_outputs] if head == "qa" else \
                [inner.classifier.dense, inner.classifier.out_proj] if head == "sequence" else [inner.classifier]
            for d in dense:
                d.weight.copy_(torch.randn_like(d.weight) / hidden ** 0.5)
                d.bias.copy_(0.1 * torch.randn_like(d.bias))
    return model.eval()


def roberta_base(seed: int = 0, **kw) -> nn.Module:
    return roberta(seed=seed, **kw)


def xlm_roberta_base(seed: int = 0, **kw) -> nn.Module:
    """xlm-roberta-base's graph: roberta_base over a 250002-row vocabulary (pass vocab= for a smaller table)."""
    return roberta(**{**dict(vocab=250002), **kw}, seed=seed)


def xlm_roberta_large(seed: int = 0, **kw) -> nn.Module:
    """xlm-roberta-large's graph: 24 layers, hidden 1024 over 16 heads, FFN 4096, vocabulary 250002."""
    return roberta(**{**dict(layers=24, hidden=1024, heads=16, intermediate=4096, vocab=250002), **kw}, seed=seed)


def mpnet(layers: int = 12, hidden: int = 768, heads: int = 12, intermediate: int = 3072,
          vocab: int = 30527, max_position: int = 514, seed: int = 0, init_std: float = 0.02,
          head: str | None = None, num_labels: int = 2, outputs=("hidden",), buckets: int = 32) -> nn.Module:
    """HF MPNetModel in BertWrapper (pad_token_id 1, layer_norm_eps 1e-5: the sentence-transformers checkpoints'
    values); with head = "sequence" | "token" | "qa" the HF head model in BertHeadWrapper.  A replica recognises it
    by its names (encoder.relative_attention_bias.weight, attention.attn.q) and serves it through the
    relative-bias attention kernel; positions follow RoBERTa's rule, so the longest sequence is
    max_position - 2, at most 512.  LayerNorms, position row 1 and the heads are re-drawn as roberta() does;
    the bucket table is re-drawn from N(0, 1.5^2): real checkpoints hold values of several units, and HF's
    0.02 init would hide a wrong bucket.  HF's encoder looks up 32 buckets whatever the config says, so
    `buckets` other than 32 builds a table the module itself cannot run (packer tests only)."""
    import logging

    from transformers import (MPNetConfig, MPNetForQuestionAnswering, MPNetForSequenceClassification,
                              MPNetForTokenClassification, MPNetModel)
    from transformers.utils import logging as hf_logging

    hf_logging.set_verbosity_error()
    logging.getLogger("transformers").setLevel(logging.ERROR)
    torch.manual_seed(seed)
    cfg = MPNetConfig(num_hidden_layers=layers, hidden_size=hidden, num_attention_heads=heads,
                      intermediate_size=intermediate, vocab_size=vocab, max_position_embeddings=max_position,
                      relative_attention_num_buckets=buckets, pad_token_id=1, bos_token_id=0, eos_token_id=2,
                      layer_norm_eps=1e-5, initializer_range=init_std, torchscript=True)
    if head is None:
        model = BertWrapper(MPNetModel(cfg))
    else:
        cfg.num_labels = 2 if head == "qa" else num_labels
        hf = {"sequence": MPNetForSequenceClassification, "token": MPNetForTokenClassification,
              "qa": MPNetForQuestionAnswering}
        if head not in hf:
            raise ValueError(f"unknown BERT head {head!r}; known: {sorted(hf)}")
        model = BertHeadWrapper(hf[head](cfg), head, outputs)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, nn.LayerNorm):
                m.weight.copy_(1.0 + 0.1 * torch.randn_like(m.weight))
                m.bias.copy_(0.05 * torch.randn_like(m.bias))
        pos = model.bert.embeddings.position_embeddings.weight
        pos[1].copy_(init_std * torch.randn_like(pos[1]))
        table = model.bert.encoder.relative_attention_bias.weight
        table.copy_(1.5 * torch.randn_like(table))
        if head is not None:
            inner = model.model
            dense = [inner.qa_outputs] if head == "qa" else \
                [inner.classifier.dense, inner.classifier.out_proj] if head == "sequence" else [inner.classifier]
            for d in dense:
                d.weight.copy_(torch.randn_like(d.weight) / hidden ** 0.5)
                d.bias.copy_(0.1 * torch.randn_like(d.bias))
    return model.eval()


def mpnet_base(seed: int = 0, **kw) -> nn.Module:
    """all-mpnet-base-v2's graph: 12 layers, hidden 768 over 12 heads, FFN 3072, 32 buckets."""
    return mpnet(seed=seed, **kw)


class AddConstant(nn.Module):
    """The reference's toy TorchScript models (tests/e2e/fixtures/simple_model.ts: x + 1)."""

    def __init__(self, value: float = 1.0):
        super().__init__()
        self.value = value

    def forward(self, x):
        return x + self.value


def build(name: str, seed: int = 0, **kw) -> nn.Module:
    """Named constructors for the BASELINE.json configs."""
    table = {
        "resnet18": resnet18,
        "resnet152": resnet152,
        "resnext50_32x4d": resnext50_32x4d,
        "resnext101_32x8d": resnext101_32x8d,
        "wide_resnet50_2": wide_resnet50_2,
        "wide_resnet101_2": wide_resnet101_2,
        "vit_l_16": vit_l_16,
        "convnext_tiny": convnext_tiny,
        "convnext_small": convnext_small,
        "convnext_base": convnext_base,
        "convnext_large": convnext_large,
        "swin_t": swin_t,
        "swin_s": swin_s,
        "swin_b": swin_b,
        "swin_v2_t": swin_v2_t,
        "swin_v2_s": swin_v2_s,
        "swin_v2_b": swin_v2_b,
        "bert-base-uncased": bert_base,
        "bert_base": bert_base,
        "minilm_l6": minilm_l6,
        "minilm_l12": minilm_l12,
        "roberta_base": roberta_base,
        "xlm_roberta_base": xlm_roberta_base,
        "xlm_roberta_large": xlm_roberta_large,
        "mpnet_base": mpnet_base,
        **{name: _efficientnet_named(name) for name in _EFFICIENTNETS},
    }
    if name not in table:
        raise KeyError(f"unknown model {name!r}; known: {sorted(table)}")
    return table[name](seed=seed, **kw)


# TorchScript names a class by its Python module path; this package's directory
# name is not an identifier, so give the zoo's modules a loadable qualified name
# (a traced/scripted model must round-trip through .pt like the reference's).
for _cls in (BasicBlock, Bottleneck, ResNet, MLPBlock, EncoderBlock, Encoder, VisionTransformer, LayerNorm2d, Permute,
             CNBlock, ConvNeXt, ShiftedWindowAttention, ShiftedWindowAttentionV2, SwinTransformerBlock, SwinTransformerBlockV2,
             PatchMerging, PatchMergingV2, SwinTransformer, SqueezeExcitation, MBConv, EfficientNet, BertWrapper,
             BertTupleWrapper, BertSegmentsWrapper, BertHeadWrapper, AddConstant):
    _cls.__module__ = "spi_zoo"

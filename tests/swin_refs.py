"""References of the Swin op tests, plain numpy in float64: shifted-window attention written the way torchvision
writes it (roll, window partition, softmax with bias and the labelled-slices mask, reverse, unroll) and the
relative-position index.  The qkv operand is drawn like hd_refs.attn_case: 1.5 N(0, 1)."""
import numpy as np

HD = 32


def rel_index(ws):
    """torchvision's relative_position_index, [N][N]."""
    c = np.stack(np.meshgrid(np.arange(ws), np.arange(ws), indexing="ij")).reshape(2, -1)
    rel = c[:, :, None] - c[:, None, :] + ws - 1
    return rel[0] * (2 * ws - 1) + rel[1]


def window_case(B, Hh, W, heads, ws, seed=0):
    """qkv fp32 [B H W][3 C] and a bias table [(2 ws - 1)^2][heads] ~ N(0, 1)."""
    qkv = (1.5 * np.random.default_rng(B * Hh * W + heads).standard_normal((B * Hh * W, 3 * heads * HD))).astype(np.float32)
    table = np.random.default_rng(100 + seed).standard_normal(((2 * ws - 1) ** 2, heads)).astype(np.float32)
    return qkv, table


def window_attention_ref(qkv, table, B, Hh, W, heads, ws, shift, scale):
    """float64 ctx [B H W][C]."""
    C, N = heads * HD, ws * ws
    x = np.asarray(qkv, np.float64).reshape(B, Hh, W, 3 * C)
    x = np.roll(x, (-shift, -shift), (1, 2))
    x = x.reshape(B, Hh // ws, ws, W // ws, ws, 3, heads, HD).transpose(5, 0, 1, 3, 6, 2, 4, 7)
    q, k, v = x.reshape(3, B, (Hh // ws) * (W // ws), heads, N, HD)
    s = (q * scale) @ k.swapaxes(-1, -2) + np.asarray(table, np.float64)[rel_index(ws)].transpose(2, 0, 1)
    if shift:
        label = np.zeros((Hh, W))
        for i, hs in enumerate((slice(0, -ws), slice(-ws, -shift), slice(-shift, None))):
            for j, wsl in enumerate((slice(0, -ws), slice(-ws, -shift), slice(-shift, None))):
                label[hs, wsl] = 3 * i + j
        label = label.reshape(Hh // ws, ws, W // ws, ws).transpose(0, 2, 1, 3).reshape(-1, N)
        s = s + np.where(label[:, :, None] != label[:, None, :], -100.0, 0.0)[None, :, None]
    p = np.exp(s - s.max(-1, keepdims=True))
    o = (p @ v) / p.sum(-1, keepdims=True)  # [B][windows][heads][N][HD]
    o = o.reshape(B, Hh // ws, W // ws, heads, ws, ws, HD).transpose(0, 1, 4, 2, 5, 3, 6).reshape(B, Hh, W, C)
    return np.roll(o, (shift, shift), (1, 2)).reshape(B * Hh * W, C)

"""References of the Swin v2 op tests, plain numpy in float64, in torchvision's order of operations: the cosine
window attention (normalise q and k, multiply by the temperature, add bias and mask, softmax) on swin_refs'
partition, and the continuous-position-bias table 16 sigmoid(cpb_mlp(log-spaced coordinates))."""
import numpy as np

from swin_refs import HD, rel_index


def cpb_table_ref(w0, b0, w2, ws):
    """[(2 ws - 1)^2][heads] from cpb_mlp.0.weight [hidden][2], cpb_mlp.0.bias [hidden], cpb_mlp.2.weight [heads][hidden]."""
    r = np.arange(-(ws - 1), ws, dtype=np.float64)
    t = np.stack(np.meshgrid(r, r, indexing="ij"), -1) / (ws - 1) * 8
    t = (np.sign(t) * np.log2(np.abs(t) + 1.0) / 3.0).reshape(-1, 2)
    hidden = np.maximum(t @ np.asarray(w0, np.float64).T + np.asarray(b0, np.float64), 0.0)
    return 16.0 / (1.0 + np.exp(-(hidden @ np.asarray(w2, np.float64).T)))


def cos_window_attention_ref(qkv, table, tau, B, Hh, W, heads, ws, shift):
    """float64 ctx [B H W][C]; tau [heads], table [(2 ws - 1)^2][heads]."""
    C, N = heads * HD, ws * ws
    x = np.asarray(qkv, np.float64).reshape(B, Hh, W, 3 * C)
    x = np.roll(x, (-shift, -shift), (1, 2))
    x = x.reshape(B, Hh // ws, ws, W // ws, ws, 3, heads, HD).transpose(5, 0, 1, 3, 6, 2, 4, 7)
    q, k, v = x.reshape(3, B, (Hh // ws) * (W // ws), heads, N, HD)
    q = q / np.maximum(np.linalg.norm(q, axis=-1, keepdims=True), 1e-12)
    k = k / np.maximum(np.linalg.norm(k, axis=-1, keepdims=True), 1e-12)
    s = (q @ k.swapaxes(-1, -2)) * np.asarray(tau, np.float64)[:, None, None]
    s = s + np.asarray(table, np.float64)[rel_index(ws)].transpose(2, 0, 1)
    if shift:
        label = np.zeros((Hh, W))
        for i, hs in enumerate((slice(0, -ws), slice(-ws, -shift), slice(-shift, None))):
            for j, wsl in enumerate((slice(0, -ws), slice(-ws, -shift), slice(-shift, None))):
                label[hs, wsl] = 3 * i + j
        label = label.reshape(Hh // ws, ws, W // ws, ws).transpose(0, 2, 1, 3).reshape(-1, N)
        s = s + np.where(label[:, :, None] != label[:, None, :], -100.0, 0.0)[None, :, None]
    p = np.exp(s - s.max(-1, keepdims=True))
    o = (p @ v) / p.sum(-1, keepdims=True)
    o = o.reshape(B, Hh // ws, W // ws, heads, ws, ws, HD).transpose(0, 1, 4, 2, 5, 3, 6).reshape(B, Hh, W, C)
    return np.roll(o, (shift, shift), (1, 2)).reshape(B * Hh * W, C)

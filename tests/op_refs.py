"""Plain float64 / bit-exact references of the ops behind include/spi_ops.h that the GPU op tests
(test_qkv_attention_ops_gpu.py, test_elementwise_ops_gpu.py) compare the HIP kernels with, plus the
inputs those tests share.  Nothing here touches a GPU; test_op_refs.py checks every reference
against the torch op it restates, so the GPU bars rest on checked ground.
"""
import numpy as np
import torch

FMIN = float(torch.finfo(torch.float32).min)
EPS = 1e-5


def nerr(got, ref):
    """Normalised max error: max|got - ref| / max|ref|."""
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max())


def make_rows(rng, M, D):
    """test_ln_fold_ops_gpu.make_rows: per-row sigma in [0.5, 2], per-row mean in {0, +2, -3} sigma and a
    +-0.5 sigma shift per 64-column chunk, so a wrong-row or wrong-chunk statistic shows."""
    ch = -(-D // 64)
    sigma = rng.uniform(0.5, 2.0, (M, 1))
    mean = sigma * rng.choice([0.0, 2.0, -3.0], (M, 1))
    shift = 0.5 * sigma * rng.choice([-1.0, 1.0], (M, ch))
    return (rng.standard_normal((M, D)) * sigma + mean + np.repeat(shift, 64, axis=1)[:, :D]).astype(np.float32)


# ---------------------------------------------------------------------------------------------
# fused QKV projection + attention

# (B, S, heads): S = 1, S % 16 != 0, both sides of the 128-row tile and the end of the 256-row one,
# the minimum of two heads, odd head counts, D = 1024 (16 statistics chunks) and BERT-base width
QKV_SHAPES = [(2, 128, 2), (3, 80, 4), (1, 1, 2), (2, 17, 3), (2, 127, 2), (1, 129, 2), (2, 197, 3), (1, 255, 2),
              (1, 256, 2), (1, 33, 16), (2, 64, 12)]
QKV_CASES = [(B, S, h, fold, masked) for (B, S, h) in QKV_SHAPES for fold in (False, True) for masked in (False, True)]


def qkv_mask(B, S):
    """The last sequence padded from S / 2 on, the first sequence's first min(3, S - 1) keys masked."""
    m = np.zeros((B, S), np.float32)
    m[-1, S // 2:] = FMIN
    m[0, :min(3, S - 1)] = FMIN
    return m


def qkv_case(ops, B, S, heads, fold, masked, seed=None):
    """Inputs of one parity case.  W at 1.5 / sqrt(D) and the bias at 0.5 give q / k / v of sigma about
    1.5 (test_attention's).  Unfolded: rows N(0, 1).  Folded: make_rows behind a LayerNorm of
    gamma = 1 + 0.3 N, beta = 0.1 N folded by ops.fold_linear; the statistics are those of the fp32 rows
    (as in the model), not of their fp16 copy.
    Returns a dict: A16 [B S][D] float16, W (fp32, to pack), W16 (its fp16 rounding), bias, stats / c1
    (None without the fold), mask (fp32 [B][S] or None)."""
    D = heads * 64
    rng = np.random.default_rng(B * S + heads if seed is None else seed)
    W = (rng.standard_normal((3 * D, D)) * 1.5 / np.sqrt(D)).astype(np.float32)
    b = (rng.standard_normal(3 * D) * 0.5).astype(np.float32)
    c = {"B": B, "S": S, "heads": heads, "mask": qkv_mask(B, S) if masked else None, "stats": None, "c1": None}
    if fold:
        x = make_rows(rng, B * S, D)
        gamma = (1 + 0.3 * rng.standard_normal(D)).astype(np.float32)
        beta = (0.1 * rng.standard_normal(D)).astype(np.float32)
        W, b, c["c1"] = ops.fold_linear("fp16", W, b, gamma, beta)
        c["stats"] = ops.chunk_stats(x.astype(np.float64)).astype(np.float32)
        c.update(x=x, gamma=gamma, beta=beta)
    else:
        x = rng.standard_normal((B * S, D)).astype(np.float32)
    c.update(A16=x.astype(np.float16), W=W, W16=W.astype(np.float16), bias=b)
    return c


def _heads(qkv, B, S, heads):
    """[B S][3 D] tensor -> q, k, v [B][heads][S][64]."""
    t = qkv.view(B, S, 3, heads, 64).permute(2, 0, 3, 1, 4)
    return t[0], t[1], t[2]


def combine_stats64(stats, eps):
    """ops.combine_stats (Chan's formula in float64) restated, so this module needs no library."""
    s = np.asarray(stats, np.float64)
    mean = s[..., 0].mean(-1)
    m2 = (s[..., 1] + 64.0 * (s[..., 0] - mean[:, None]) ** 2).sum(-1)
    return mean, 1.0 / np.sqrt(m2 / (64.0 * s.shape[1]) + eps)


def qkv_attention_ref(A16, W16, bias, mask_bias, B, S, heads, scale, stats=None, c1=None, eps=None, round16=True):
    """float64 reference on the operands as given (A16 / W16 are normally fp16 arrays): q | k | v =
    A W^T + bias, or with the fold rstd (A W^T - mean c1) + bias with (mean, rstd) combined from the chunk
    statistics; rounded to fp16 where the kernel rounds (round16); softmax(q k^T scale + mask) v in
    float64.  Returns float64 [B S][64 heads]."""
    D = heads * 64
    acc = np.asarray(A16, np.float64) @ np.asarray(W16, np.float64).T
    if stats is not None:
        mean, rstd = combine_stats64(stats, eps)
        acc = rstd[:, None] * (acc - mean[:, None] * np.asarray(c1, np.float64))
    qkv = acc + np.asarray(bias, np.float64)
    if round16:
        qkv = qkv.astype(np.float16).astype(np.float64)
    q, k, v = _heads(torch.from_numpy(qkv), B, S, heads)
    s = (q @ k.transpose(-1, -2)) * scale
    if mask_bias is not None:
        s = s + torch.from_numpy(np.asarray(mask_bias, np.float64).reshape(B, S))[:, None, None, :]
    p = torch.exp(s - s.max(-1, keepdim=True).values)
    o = (p @ v) / p.sum(-1, keepdim=True)
    return o.permute(0, 2, 1, 3).reshape(B * S, D).numpy()


def emulate_qkv_attention(A16, W16, bias, mask_bias, B, S, heads, scale, stats=None, c1=None, eps=None):
    """qkv_attn.hip's arithmetic in torch on the CPU: fp32 accumulation of the fp16 products, the fold's
    epilogue in fp32, fp16 q / k / v, fp32 scores and softmax with the row sum taken from the fp32
    probabilities, fp16 P against fp16 V accumulated in fp32, fp16 output.  (The kernel's summation
    order, its online rescaling and __expf are what the GPU bar's slack over this is for.)"""
    D = heads * 64
    acc = torch.from_numpy(np.asarray(A16, np.float16)).float() @ torch.from_numpy(np.asarray(W16, np.float16)).float().T
    if stats is not None:
        mean, rstd = combine_stats64(stats, eps)
        mean32, rstd32 = torch.from_numpy(mean.astype(np.float32)), torch.from_numpy(rstd.astype(np.float32))
        acc = rstd32[:, None] * (acc - mean32[:, None] * torch.from_numpy(np.asarray(c1, np.float32)))
    qkv = (acc + torch.from_numpy(np.asarray(bias, np.float32))).half().float()
    q, k, v = _heads(qkv, B, S, heads)
    s = (q @ k.transpose(-1, -2)) * np.float32(scale)
    if mask_bias is not None:
        s = s + torch.from_numpy(np.asarray(mask_bias, np.float32).reshape(B, S))[:, None, None, :]
    p = torch.exp(s - s.max(-1, keepdim=True).values)
    o = (p.half().float() @ v) / p.sum(-1, keepdim=True)
    return o.permute(0, 2, 1, 3).reshape(B * S, D).half().numpy()


# ---------------------------------------------------------------------------------------------
# the HBM-bound kernels


def xf_image(x_u8, nhwc, scale, shift):
    """8-bit pixels -> the fp32 NCHW image that enters the network: float32(p) * scale[c] + shift[c], one
    rounded fp32 multiply and one rounded fp32 add (test_u8_input_gpu.host_image)."""
    x = np.ascontiguousarray(x_u8.transpose(0, 3, 1, 2)) if nhwc else x_u8
    scale, shift = np.float32(scale).reshape(1, 3, 1, 1), np.float32(shift).reshape(1, 3, 1, 1)
    return x.astype(np.float32) * scale + shift


def ingest_ref(x_nchw, cpad, f16):
    """fp32 [B][C][H][W] -> NHWC [B][H][W][cpad], channels zero-padded, rounded to fp16 when f16."""
    B, C, H, W = x_nchw.shape
    y = np.zeros((B, H, W, cpad), np.float32)
    y[..., :C] = x_nchw.transpose(0, 2, 3, 1)
    return y.astype(np.float16) if f16 else y


def maxpool_ref(x_nhwc, k, stride, pad):
    """k x k max pool of [B][H][W][C]; padding never wins (-inf).  Keeps the dtype: a max is exact."""
    x = np.asarray(x_nhwc)
    B, H, W, C = x.shape
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    xp = np.full((B, H + 2 * pad + stride, W + 2 * pad + stride, C), -np.inf, x.dtype)
    xp[:, pad:pad + H, pad:pad + W] = x
    out = np.full((B, OH, OW, C), -np.inf, x.dtype)
    for kh in range(k):
        for kw in range(k):
            out = np.maximum(out, xp[:, kh:kh + stride * OH:stride, kw:kw + stride * OW:stride][:, :OH, :OW])
    return out


def avgpool_ref(x):
    """float64 mean over HW of [B][HW][C] values."""
    return np.asarray(x, np.float64).mean(axis=1)


def bert_embed_ref(ids, word, pos, type0, gamma, beta, S, eps):
    """The embedding sum as the kernels take it, (word[clamp(id)] + type0) + pos[s] in fp32, then the
    LayerNorm in float64.  ids int64 [B S]; returns float64 [B S][D]."""
    ids = np.clip(np.asarray(ids, np.int64).reshape(-1), 0, word.shape[0] - 1)
    s = np.arange(ids.size) % S
    v = ((word[ids] + type0[None, :]).astype(np.float32) + pos[s]).astype(np.float32).astype(np.float64)
    mean = v.mean(-1, keepdims=True)
    var = ((v - mean) ** 2).mean(-1, keepdims=True)
    return (v - mean) / np.sqrt(var + eps) * gamma.astype(np.float64) + beta.astype(np.float64)


def mask_to_bias_ref(mask):
    return np.where(np.asarray(mask) != 0, np.float32(0), np.float32(FMIN)).astype(np.float32)


def vit_assemble_ref(patches, cls, pos):
    """patches fp32 [B][P][D], cls [D], pos [P + 1][D] -> fp32 [B][P + 1][D] (one rounded fp32 add each)."""
    B, P, D = patches.shape
    x = np.empty((B, P + 1, D), np.float32)
    x[:, 0] = cls
    x[:, 1:] = patches
    return (x + pos[None]).astype(np.float32)


def gather_rows_ref(x, rows, stride_rows, f16):
    y = np.asarray(x, np.float32)[:rows * stride_rows:stride_rows]
    return y.astype(np.float16) if f16 else y.copy()

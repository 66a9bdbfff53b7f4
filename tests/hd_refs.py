"""References, emulation and generators of the standalone attention tests with the head width stated (head_dim
32 beside op_refs' 64), pure numpy / torch on the CPU.  op_refs' case list is reused with the head count doubled
at the same D: a (B, S, h) entry there is h 64-wide heads, here 2 h heads of 32 on the very same operand."""
import numpy as np
import torch

import op_refs as R

HD = 32
SCALE = 1.0 / np.sqrt(HD)
# (B, S, heads, mask kind): op_refs' list, D unchanged
ATTN_CASES = [(B, S, 2 * h, kind) for (B, S, h, kind) in R.ATTN_CASES]
# emulate_attention_f16's normalised max error against attention_ref over ATTN_CASES at width 32, scale
# 1 / sqrt(32): the worst measured on a CPU is 4.49e-4 ((1, 257, 4) "head"); test_head_dim holds every case to
# ATTN_EMU_WORST and the worst to within a tenth of it.  The fp16 GPU bar is 3x this.
ATTN_EMU_WORST = 4.5e-4


def _heads(qkv, B, S, heads, hd):
    """[B S][3 D] tensor -> q, k, v [B][heads][S][hd]."""
    t = qkv.view(B, S, 3, heads, hd).permute(2, 0, 3, 1, 4)
    return t[0], t[1], t[2]


def attention_ref(qkv, mask_bias, B, S, heads, scale, hd=HD):
    """op_refs.attention_ref with the head width stated: float64 [B S][heads hd]."""
    q, k, v = _heads(torch.from_numpy(np.ascontiguousarray(qkv, np.float64)), B, S, heads, hd)
    s = (q @ k.transpose(-1, -2)) * scale
    if mask_bias is not None:
        s = s + torch.from_numpy(np.asarray(mask_bias, np.float64).reshape(B, S))[:, None, None, :]
    p = torch.exp(s - s.max(-1, keepdim=True).values)
    o = (p @ v) / p.sum(-1, keepdim=True)
    return o.permute(0, 2, 1, 3).reshape(B * S, heads * hd).numpy()


def emulate_attention_f16(qkv16, mask_bias, B, S, heads, scale, hd=HD):
    """op_refs.emulate_attention_f16 with the head width stated (the kernels' arithmetic does not depend on it:
    fp32 scores and softmax, fp16 P and V, fp32 accumulation, fp16 output)."""
    q, k, v = _heads(torch.from_numpy(np.ascontiguousarray(qkv16, np.float16)).float(), B, S, heads, hd)
    s = (q @ k.transpose(-1, -2)) * np.float32(scale)
    if mask_bias is not None:
        s = s + torch.from_numpy(np.asarray(mask_bias, np.float32).reshape(B, S))[:, None, None, :]
    p = torch.exp(s - s.max(-1, keepdim=True).values)
    o = (p.half().float() @ v) / p.sum(-1, keepdim=True)
    return o.permute(0, 2, 1, 3).reshape(B * S, heads * hd).half().numpy()


def attn_case(B, S, heads):
    """op_refs.attn_case's operand of the same D: packed qkv fp32 [B S][3 D], D = 32 heads."""
    return R.attn_case(B, S, heads // 2)


def attn_exact_case(S, variant, heads=4, hd=HD):
    """op_refs.attn_exact_case's recipe rebuilt for four 32-wide heads, B = 2: q = 0, k random, v random but for
    column 0 of each head, which holds SIGN[h] on a key that counts and -7 SIGN[h] on a masked one, SIGN = +1 on
    even heads and -1 on odd ones: ctx[:, 0] of head h is SIGN[h] times a known quotient, and a V column (or a
    ctx column) taken from the neighbouring sub-head comes out with the wrong sign.
    Returns (qkv fp32 [2 S][3 heads hd], exact in fp16; mask [2][S] or None; want float64 [2][S][heads])."""
    B = 2
    rng = np.random.default_rng(2000 + S)
    qkv = (1.5 * rng.standard_normal((B, S, 3, heads, hd))).astype(np.float16).astype(np.float32)
    qkv[:, :, 0] = 0
    want = np.ones((B, S), np.float64)
    if variant == "all":
        mask = np.zeros((B, S), np.float32)
        mask[1, :] = R.FMIN
        v0 = np.ones((B, S), np.float32)
        v0[1] = np.where(rng.random(S) < 0.4, -7, 1)
        if v0[1].sum() == 0:
            v0[1, 0] = -v0[1, 0] - 6  # 1 <-> -7
        want[1, :] = v0[1].astype(np.float64).mean()
    else:
        mask = R.attn_mask(B, S, {"ones": None, "head": "head", "tile": "middle"}[variant])
        v0 = np.ones((B, S), np.float32) if mask is None else np.where(mask != 0, -7, 1).astype(np.float32)
    sign = np.where(np.arange(heads) % 2 == 0, 1.0, -1.0)
    qkv[:, :, 2, :, 0] = v0[:, :, None] * sign.astype(np.float32)
    return qkv.reshape(B * S, 3 * heads * hd), mask, want[:, :, None] * sign

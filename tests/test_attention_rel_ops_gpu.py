"""spi_op_attention_rel (the REL instances of attention.hip) against float64 softmax(q k^T scale + bias + mask) v,
bias[h][q][k] = table[bucket(k - q)][h] through HF's own bucket function, at test_attention_ops_gpu's metric and bars;
the table is N(0, 2^2) with independent halves, so a transposed or mis-centred row is an O(1) error.  Measured on an
MI355X, worst over the cases: fp32 1.17e-6 (bar 1e-5), fp16 3.80e-4 (bar 1.23e-3)."""
import importlib

import numpy as np
import pytest
import torch

import op_refs as R
from test_attention_ops_gpu import DT, GUARD, NAN, TOL, dev, rounded

pytestmark = pytest.mark.gpu

# (B, S, heads, masked, P): one partial tile; a second query tile (the slice starts off the row's centre); 4 waves full;
# whole-sequence staging; 8-wave tiles over several key tiles; both ends of the row; rows packed for S (half == S - 1)
CASES = [(2, 17, 2, True, 512), (1, 65, 3, False, 512), (2, 128, 2, True, 512), (1, 197, 2, True, 512),
         (1, 300, 2, False, 512), (1, 512, 2, True, 512), (1, 65, 3, False, 65)]


def reference(qkv, mask, table, B, S, heads):
    from transformers.models.mpnet.modeling_mpnet import MPNetEncoder
    bucket = MPNetEncoder.relative_position_bucket(torch.arange(S)[None] - torch.arange(S)[:, None], num_buckets=32)
    bias = torch.from_numpy(table.astype(np.float64))[bucket].permute(2, 0, 1)                  # [heads][q][k]
    q, k, v = torch.from_numpy(qkv.astype(np.float64)).view(B, S, 3, heads, 64).permute(2, 0, 3, 1, 4)
    s = q @ k.transpose(-1, -2) * 0.125 + bias
    if mask is not None:
        s = s + torch.from_numpy(mask.astype(np.float64))[:, None, None, :]
    return (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(B * S, heads * 64).numpy()


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("B,S,heads,masked,P", CASES)
def test_parity(spi, gpu, B, S, heads, masked, P, prec):
    ops = importlib.import_module("starpu-inference-server_amd.ops")
    qkv, mask = rounded(R.attn_case(B, S, heads), prec), R.qkv_mask(B, S) if masked else None
    table = (2.0 * np.random.default_rng(heads).standard_normal((32, heads))).astype(np.float32)
    ctx = torch.full((B * S + GUARD, heads * 64), NAN, dtype=DT[prec], device="cuda")
    ops.attention_rel(prec, dev(qkv, DT[prec]), dev(ops.rel_bias_rows(table, P)), P - 1, B, S, heads,
                      mask_bias=dev(mask), out=ctx)
    assert bool(torch.isnan(ctx[B * S:]).all()), "rows past B S were written"
    e = R.nerr(ctx[:B * S].cpu().numpy(), reference(qkv, mask, table, B, S, heads))
    print(f"attention_rel {prec} B{B} S{S} H{heads} masked{int(masked)} P{P}: {e:.3e}")
    assert e < TOL[prec]


def test_rejections(spi, gpu):  # decided on the host before any launch: the NaN-filled ctx comes back untouched
    ops = importlib.import_module("starpu-inference-server_amd.ops")
    qkv, rows = torch.zeros(16, 3 * 128, dtype=torch.float16, device="cuda"), torch.zeros(2 * 32 + 4, device="cuda")
    ctx = torch.full((16, 128), NAN, dtype=torch.float16, device="cuda")
    for match, r, half, kw in [("head_dim", rows, 15, dict(head_dim=32)), ("S - 1 <= half", rows, 14, {}),
                               ("ld >= 2 half", rows, 15, dict(ld=30)), ("non-null", None, 15, {}),
                               ("16-byte aligned", rows[1:], 15, {})]:
        with pytest.raises(ops.OpError, match=match):
            ops.attention_rel("fp16", qkv, r, half, 1, 16, 2, out=ctx, **{**dict(ld=32), **kw})
    assert bool(torch.isnan(ctx).all())

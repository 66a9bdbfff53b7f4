"""Plain float64 / bit-exact references of the ops behind include/spi_ops.h that the GPU op tests
(test_qkv_attention_ops_gpu.py, test_attention_ops_gpu.py, test_elementwise_ops_gpu.py, test_conv_pair_ops_gpu.py,
test_hilo_weight_ops_gpu.py, the hi + lo consumer of test_ln_fold_ops_gpu.py) compare the HIP kernels with,
plus the inputs and case lists those tests share.  Nothing here touches a GPU; test_op_refs.py checks every reference
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


def attention_ref(qkv, mask_bias, B, S, heads, scale):
    """float64 softmax(q k^T scale + mask) v on the packed [B S][3 D] operand as given (mask_bias [B][S]
    or None, added to every query's scores).  Returns float64 [B S][64 heads]."""
    q, k, v = _heads(torch.from_numpy(np.ascontiguousarray(qkv, np.float64)), B, S, heads)
    s = (q @ k.transpose(-1, -2)) * scale
    if mask_bias is not None:
        s = s + torch.from_numpy(np.asarray(mask_bias, np.float64).reshape(B, S))[:, None, None, :]
    p = torch.exp(s - s.max(-1, keepdim=True).values)
    o = (p @ v) / p.sum(-1, keepdim=True)
    return o.permute(0, 2, 1, 3).reshape(B * S, heads * 64).numpy()


def emulate_attention_f16(qkv16, mask_bias, B, S, heads, scale):
    """The fp16 attention kernels' arithmetic (attention.hip, the tail of qkv_attn.hip) in torch on the CPU:
    fp32 scores and softmax on the fp16 q / k, the row sum taken from the fp32 probabilities, fp16 P against
    fp16 V accumulated in fp32, fp16 output.  (The kernels' summation order, their online rescaling and
    __expf are what the GPU bar's slack over this is for.)"""
    q, k, v = _heads(torch.from_numpy(np.ascontiguousarray(qkv16, np.float16)).float(), B, S, heads)
    s = (q @ k.transpose(-1, -2)) * np.float32(scale)
    if mask_bias is not None:
        s = s + torch.from_numpy(np.asarray(mask_bias, np.float32).reshape(B, S))[:, None, None, :]
    p = torch.exp(s - s.max(-1, keepdim=True).values)
    o = (p.half().float() @ v) / p.sum(-1, keepdim=True)
    return o.permute(0, 2, 1, 3).reshape(B * S, heads * 64).half().numpy()


def qkv_attention_ref(A16, W16, bias, mask_bias, B, S, heads, scale, stats=None, c1=None, eps=None, round16=True):
    """float64 reference on the operands as given (A16 / W16 are normally fp16 arrays): q | k | v =
    A W^T + bias, or with the fold rstd (A W^T - mean c1) + bias with (mean, rstd) combined from the chunk
    statistics; rounded to fp16 where the kernel rounds (round16); softmax(q k^T scale + mask) v in
    float64.  Returns float64 [B S][64 heads]."""
    acc = np.asarray(A16, np.float64) @ np.asarray(W16, np.float64).T
    if stats is not None:
        mean, rstd = combine_stats64(stats, eps)
        acc = rstd[:, None] * (acc - mean[:, None] * np.asarray(c1, np.float64))
    qkv = acc + np.asarray(bias, np.float64)
    if round16:
        qkv = qkv.astype(np.float16).astype(np.float64)
    return attention_ref(qkv, mask_bias, B, S, heads, scale)


def emulate_qkv_attention(A16, W16, bias, mask_bias, B, S, heads, scale, stats=None, c1=None, eps=None):
    """qkv_attn.hip's arithmetic in torch on the CPU: fp32 accumulation of the fp16 products, the fold's
    epilogue in fp32, fp16 q / k / v, fp32 scores and softmax with the row sum taken from the fp32
    probabilities, fp16 P against fp16 V accumulated in fp32, fp16 output.  (The kernel's summation
    order, its online rescaling and __expf are what the GPU bar's slack over this is for.)"""
    acc = torch.from_numpy(np.asarray(A16, np.float16)).float() @ torch.from_numpy(np.asarray(W16, np.float16)).float().T
    if stats is not None:
        mean, rstd = combine_stats64(stats, eps)
        mean32, rstd32 = torch.from_numpy(mean.astype(np.float32)), torch.from_numpy(rstd.astype(np.float32))
        acc = rstd32[:, None] * (acc - mean32[:, None] * torch.from_numpy(np.asarray(c1, np.float32)))
    qkv = (acc + torch.from_numpy(np.asarray(bias, np.float32))).half().float()
    return emulate_attention_f16(qkv.numpy(), mask_bias, B, S, heads, scale)


# ---------------------------------------------------------------------------------------------
# the standalone attention kernels (attention.hip): what the model runs on the default ViT path, for every
# fp32 transformer and for every sequence the fused kernel refuses (S > 256)

# (B, S, heads): both sides of each kernel boundary (fp16: 4 waves up to 128 keys, the whole sequence staged
# for 129..224, 64-key tiles from 225 on; fp32: 64-query x 64-key tiles throughout), up to 5 query blocks x
# 10 key tiles
ATTN_SHAPES = [(1, 1, 2), (2, 17, 3), (2, 127, 2), (2, 128, 2), (1, 129, 2), (2, 197, 3), (1, 224, 2), (1, 225, 2),
               (1, 257, 2), (2, 384, 2), (1, 512, 3), (1, 577, 2)]
ATTN_MASKS = [None, "head", "middle", "tail"]
ATTN_CASES = [(B, S, h, kind) for (B, S, h) in ATTN_SHAPES for kind in ATTN_MASKS if kind is None or S > 1]
# the near-exact cases (B = 2, heads = 2): each side of every multiple of 64 up to 256, then long sequences
ATTN_EXACT_S = [1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193, 223, 224, 225, 255, 256, 257, 320, 385, 512,
                577]
ATTN_EXACT_VARIANTS = ["ones", "head", "tile", "all"]
ATTN_EXACT_CASES = [(S, v) for S in ATTN_EXACT_S for v in ATTN_EXACT_VARIANTS
                    if not (v == "head" and S == 1) and not (v == "tile" and S < 193)]
# emulate_attention_f16's normalised max error against attention_ref over ATTN_CASES: the worst measured on
# a CPU is 4.04e-4 ((1, 129, 2) "head"; 1.6e-4 .. 4.0e-4 over the list), and
# test_op_refs.test_attention_emulation_within_bar holds every case to ATTN_EMU_TOL.  The fp16 GPU bar is 3x
# the measured worst case.
ATTN_EMU_WORST = 4.1e-4
ATTN_EMU_TOL = 5e-4


def attn_mask(B, S, kind):
    """fp32 additive mask [B][S] (FMIN on a masked key) on the last sequence, or None.  "head": keys
    0 .. min(69, S - 2), a whole first 64-key tile and the next one's edge (and, with B > 1, the first three
    keys of sequence 0); "middle": keys 123 .. 196 clipped to S - 1, a whole interior tile and both
    neighbours' edges (nothing for S <= 123: an all-zero mask); "tail": from S / 2 on."""
    if kind is None:
        return None
    m = np.zeros((B, S), np.float32)
    if kind == "head":
        m[-1, :min(69, S - 2) + 1] = FMIN
        if B > 1:
            m[0, :min(3, S - 1)] = FMIN
    elif kind == "middle":
        m[-1, 123:min(197, S)] = FMIN
    elif kind == "tail":
        m[-1, S // 2:] = FMIN
    else:
        raise ValueError(kind)
    return m


def attn_case(B, S, heads):
    """The parity operand: packed qkv fp32 [B S][3 D] of 1.5 N(0, 1) (scores of sigma about 2.25 at scale 1/8)."""
    rng = np.random.default_rng(B * S + heads)
    return (1.5 * rng.standard_normal((B * S, 3 * heads * 64))).astype(np.float32)


def attn_exact_case(S, variant):
    """A near-exact case, B = 2, heads = 2: q = 0, so every score is 0 and every probability 1 or 0; k random;
    v random but for column 0 of each head, which holds 1 on a key that counts and -7 on a masked one.
    ctx[:, 0] of each head is then a known quotient.  "ones": no mask, 1; "head" / "tile": attn_mask's "head"
    / "middle" keys masked, still 1; "all": every key of the last sequence masked and its values drawn from
    {1, -7}: their mean (kept off zero, the bar is relative).
    Returns (qkv fp32 [2 S][384], exact in fp16; mask [2][S] or None; want float64 [2][S])."""
    B, heads, D = 2, 2, 128
    rng = np.random.default_rng(1000 + S)
    qkv = (1.5 * rng.standard_normal((B, S, 3, heads, 64))).astype(np.float16).astype(np.float32)
    qkv[:, :, 0] = 0
    want = np.ones((B, S), np.float64)
    if variant == "all":
        mask = np.zeros((B, S), np.float32)
        mask[1, :] = FMIN
        v0 = np.ones((B, S), np.float32)
        v0[1] = np.where(rng.random(S) < 0.4, -7, 1)
        if v0[1].sum() == 0:
            v0[1, 0] = -v0[1, 0] - 6  # 1 <-> -7
        want[1, :] = v0[1].astype(np.float64).mean()
    else:
        mask = attn_mask(B, S, {"ones": None, "head": "head", "tile": "middle"}[variant])
        v0 = np.ones((B, S), np.float32) if mask is None else np.where(mask != 0, -7, 1).astype(np.float32)
    qkv[:, :, 2, :, 0] = v0[:, :, None]
    return qkv.reshape(B * S, 3 * D), mask, want


# ---------------------------------------------------------------------------------------------
# hi + lo fp16 weights (GemmDesc::krep = 2) and the grouped conv pair
#
# Every krep reference multiplies hilo_values(w): exactly the two fp16 numbers the kernel multiplies, summed.
# What is left between the kernel and the float64 reference is the fp32 accumulation alone, so the fp32
# output bar (1e-5) applies, and a kernel that dropped or misplaced the lo half sits above 1e-4
# (test_op_refs.test_krep_cases_discriminate checks both sides for every case below).


def hi_values(w):
    """float64 fp16(w): what a plain fp16 pack holds."""
    return np.asarray(w, np.float32).astype(np.float16).astype(np.float64)


def hilo_values(w):
    """float64 fp16(w) + fp16(w - fp16(w)): the weight a hi + lo pack holds."""
    w = np.asarray(w, np.float32)
    hi = w.astype(np.float16)
    return hi.astype(np.float64) + (w - hi.astype(np.float32)).astype(np.float16).astype(np.float64)


def hilo_layout(w):
    """numpy construction of the hi + lo packed image of a [N][K] fp32 matrix: fp16 [Npad][Kpad], Npad =
    round_up(N, 128), Kpad = 2 round_up(K, 64); logical k = 64 blk + j has hi at blk 128 + j, lo 64 further."""
    w = np.asarray(w, np.float32)
    n, k = w.shape
    npad, kblk = -(-n // 128) * 128, -(-k // 64)
    hi = np.zeros((npad, kblk * 64), np.float16)
    lo = np.zeros((npad, kblk * 64), np.float16)
    hi[:n, :k] = w.astype(np.float16)
    lo[:n, :k] = (w - hi[:n, :k].astype(np.float32)).astype(np.float16)
    img = np.stack([hi.reshape(npad, kblk, 64), lo.reshape(npad, kblk, 64)], axis=2)  # [Npad][blk][hi | lo][64]
    return np.ascontiguousarray(img.reshape(npad, kblk * 128))


# dense: (M, N, K); the chooser splits the last three into 4 to 6 slices
KREP_DENSE = [(64, 64, 192), (100, 96, 160), (50, 1000, 96), (8, 128, 768), (197, 128, 1024), (64, 64, 1152)]
KREP_FORMS = ["plain", "res32", "relu"]
KREP_GELU = (100, 96, 160)  # fp16 output
# SPI_GEMM_PLAN = "bm,bn,stages,splits" forced on one shape each; the first: 14 packed steps, and a 5-way
# split has to round to whole (hi, lo) pairs -- 4 slices
KREP_FORCED = [("64,64,2,5", (100, 96, 448)), ("64,64,3,3", (64, 64, 1152)), ("128,64,3,2", (197, 128, 1024)),
               ("128,128,2,1", (50, 1000, 96))]
# conv: (B, H, Cin, Cout, k, stride, pad)
KREP_CONV = [(1, 12, 64, 128, 1, 2, 0), (1, 28, 128, 256, 1, 2, 0), (3, 11, 128, 256, 1, 2, 0),
             (2, 13, 64, 128, 3, 2, 1)]
KREP_CONV_RES = (1, 28, 128, 256, 1, 2, 0)  # fp32 residual, fp16 output
# folded consumer: (M, N, K)
KREP_FOLD = [(M, N, K) for M in (1, 100) for (N, K) in ((128, 64), (256, 192), (384, 640), (256, 1024))]

# conv pairs: (B, H, Cin, (Cout0, k0, stride0, pad0), (Cout1, k1, stride1, pad1)) -> precisions
_ALL = ("fp32", "fp16", "fp16x3", "fp16x3s")
PAIR_CASES = [
    ((1, 12, 64, (128, 3, 2, 1), (128, 1, 2, 0)), _ALL),
    ((2, 13, 64, (128, 3, 2, 1), (128, 1, 2, 0)), _ALL),
    ((1, 28, 128, (256, 3, 2, 1), (256, 1, 2, 0)), _ALL),
    ((1, 14, 256, (512, 3, 2, 1), (512, 1, 2, 0)), _ALL),
    ((4, 28, 128, (256, 3, 2, 1), (256, 1, 2, 0)), _ALL),
    ((3, 11, 128, (64, 1, 1, 0), (256, 1, 2, 0)), _ALL),
    ((1, 10, 512, (256, 1, 1, 0), (1024, 1, 2, 0)), _ALL),
    ((1, 14, 1024, (512, 1, 1, 0), (2048, 1, 2, 0)), _ALL),
    ((8, 56, 64, (128, 3, 2, 1), (128, 1, 2, 0)), ("fp16", "fp16x3s")),
    ((6, 56, 256, (128, 1, 1, 0), (512, 1, 2, 0)), ("fp16", "fp16x3s")),
    ((1, 9, 32, (64, 3, 2, 1), (64, 1, 2, 0)), ("fp16",)),
    ((1, 28, 128, (128, 3, 1, 1), (256, 1, 1, 0)), ("fp16",)),
]
PAIR_PARAMS = [(c, p) for c, precs in PAIR_CASES for p in precs]
# the fp16 cases whose conv 1 can carry hi + lo weights (Cin >= 64)
PAIR_HILO_CASES = [c for c, precs in PAIR_CASES if "fp16" in precs and c[2] >= 64]


def pair_id(case):
    B, H, cin, c0, c1 = case
    return f"{B}x{H}x{cin}-{c0[0]}k{c0[1]}s{c0[2]}-{c1[0]}k{c1[1]}s{c1[2]}"


def krep_dense_case(M, N, K):
    """Inputs shared by every form of a dense shape: fp16-exact A of N(0, 1), W of N(0, 1 / K), bias and an
    fp32 residual at a quarter of the output's sigma (so they shift the normalisation by little)."""
    rng = np.random.default_rng(M * 7 + N * 3 + K)
    A16 = rng.standard_normal((M, K)).astype(np.float16)
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    b = (0.25 * rng.standard_normal(N)).astype(np.float32)
    R = (0.25 * rng.standard_normal((M, N))).astype(np.float32)
    return A16, W, b, R


def gelu64(x):
    t = torch.from_numpy(np.asarray(x, np.float64))
    return (0.5 * t * (1 + torch.erf(t / 2 ** 0.5))).numpy()


def epilogue64(acc, bias=None, res=None, act=None):
    y = np.asarray(acc, np.float64)
    if bias is not None:
        y = y + np.asarray(bias, np.float64)
    if res is not None:
        y = y + np.asarray(res, np.float64)
    return {None: y, "relu": np.maximum(y, 0), "gelu": gelu64(y)}[act]


def dense_acc64(A, Wv):
    """float64 A . Wv^T on the values as given."""
    return np.asarray(A, np.float64) @ np.asarray(Wv, np.float64).T


def dense_acc32_hilo(A16, W):
    """The krep = 2 k-loop's arithmetic in torch on the CPU: fp32 accumulation of A . hi^T and A . lo^T."""
    a = torch.from_numpy(np.asarray(A16, np.float32))
    w = np.asarray(W, np.float32)
    hi = w.astype(np.float16)
    lo = (w - hi.astype(np.float32)).astype(np.float16)
    return (a @ torch.from_numpy(hi.astype(np.float32)).T + a @ torch.from_numpy(lo.astype(np.float32)).T).numpy()


def conv_case(B, H, cin, convs, seed=None):
    """Inputs of convs on one NHWC input: x fp32 [B][H][H][cin] of N(0, 1) and per conv (cout, k, stride, pad)
    the weight [cout][k][k][cin] of He scale (its reshape to [cout][k k cin] is the matrix to pack) and a
    bias of N(0, 1)."""
    rng = np.random.default_rng(B * 1000 + H * 10 + cin if seed is None else seed)
    x = rng.standard_normal((B, H, H, cin)).astype(np.float32)
    ws = []
    for cout, k, _, _ in convs:
        w = (rng.standard_normal((cout, k, k, cin)) * np.sqrt(2.0 / (cin * k * k))).astype(np.float32)
        ws.append((w, rng.standard_normal(cout).astype(np.float32)))
    return x, ws


def conv_acc(x_vals, w_vals, stride, pad, dtype=torch.float64):
    """NHWC conv of x_vals [B][H][W][C] with w_vals [cout][k][k][C] on the values as given, in dtype
    (float64: the reference; float32: an fp32-accumulated emulation) -> numpy [B][OH][OW][cout]."""
    x = torch.from_numpy(np.ascontiguousarray(x_vals)).to(dtype).permute(0, 3, 1, 2)
    w = torch.from_numpy(np.ascontiguousarray(w_vals)).to(dtype).permute(0, 3, 1, 2)
    return torch.nn.functional.conv2d(x, w, None, stride, pad).permute(0, 2, 3, 1).contiguous().numpy()


def conv_acc32_hilo(x16, w, stride, pad):
    """fp32 accumulation of the conv against fp16(w) and against the lo half, summed (the krep = 2 loop)."""
    w = np.asarray(w, np.float32)
    hi = w.astype(np.float16)
    lo = (w - hi.astype(np.float32)).astype(np.float16)
    x = np.asarray(x16, np.float32)
    return conv_acc(x, hi.astype(np.float32), stride, pad, torch.float32) + \
        conv_acc(x, lo.astype(np.float32), stride, pad, torch.float32)


def krep_fold_case(ops, M, N, K):
    """A LayerNorm + linear layer folded for hi + lo weights: rows of make_rows behind gamma = 1 + 0.3 N with
    three gains of 8, beta = 0.1 N with three of +-3 (test_ln_fold_ops_gpu.make_ln).  Returns A16, the
    statistics of the fp32 rows (fp32), W' (fp32, to pack hi + lo), bias', c1."""
    rng = np.random.default_rng(N * 11 + K)
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    gamma = (1 + 0.3 * rng.standard_normal(K)).astype(np.float32)
    beta = (0.1 * rng.standard_normal(K)).astype(np.float32)
    gamma[[1, K // 2, K - 3]] = 8.0
    beta[[2, K // 3, K - 1]] = [3.0, -3.0, 3.0]
    wf, bias, c1 = ops.fold_linear("fp16", W, b, gamma, beta, hilo=True)
    x = make_rows(np.random.default_rng(M * 13 + N + K), M, K)
    stats = ops.chunk_stats(x.astype(np.float64)).astype(np.float32)
    return x.astype(np.float16), stats, wf, bias, c1


def fold_consumer64(acc, stats, c1, bias, eps=EPS):
    """The consumer epilogue rstd (acc - mean c1) + bias' in float64."""
    mean, rstd = combine_stats64(stats, eps)
    return rstd[:, None] * (np.asarray(acc, np.float64) - mean[:, None] * np.asarray(c1, np.float64)) + \
        np.asarray(bias, np.float64)


def fold_consumer32(acc32, stats, c1, bias, eps=EPS):
    """The same epilogue in fp32 on an fp32 accumulator."""
    mean, rstd = combine_stats64(stats, eps)
    mean, rstd = mean.astype(np.float32), rstd.astype(np.float32)
    return rstd[:, None] * (np.asarray(acc32, np.float32) - mean[:, None] * np.asarray(c1, np.float32)) + \
        np.asarray(bias, np.float32)


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

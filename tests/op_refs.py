"""Plain float64 / bit-exact references of the ops behind include/spi_ops.h that the GPU op tests
(test_qkv_attention_ops_gpu.py, test_attention_ops_gpu.py, test_elementwise_ops_gpu.py, test_conv_pair_ops_gpu.py,
test_hilo_weight_ops_gpu.py, test_conv_kinds_ops_gpu.py, test_stem_ops_gpu.py, test_fc_ops_gpu.py, the hi + lo
consumer of test_ln_fold_ops_gpu.py) compare the HIP kernels with,
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


def conv_case(B, H, cin, convs, seed=None, W=None):
    """Inputs of convs on one NHWC input: x fp32 [B][H][W][cin] of N(0, 1) (W defaults to H) and per conv
    (cout, k, stride, pad), k an integer or (kh, kw), the weight [cout][kh][kw][cin] of He scale (its reshape
    to [cout][kh kw cin] is the matrix to pack) and a bias of N(0, 1)."""
    rng = np.random.default_rng(B * 1000 + H * 10 + cin if seed is None else seed)
    x = rng.standard_normal((B, H, H if W is None else W, cin)).astype(np.float32)
    ws = []
    for cout, k, _, _ in convs:
        kh, kw = (k, k) if isinstance(k, int) else k
        w = (rng.standard_normal((cout, kh, kw, cin)) * np.sqrt(2.0 / (cin * kh * kw))).astype(np.float32)
        ws.append((w, rng.standard_normal(cout).astype(np.float32)))
    return x, ws


def conv_acc(x_vals, w_vals, stride, pad, dtype=torch.float64):
    """NHWC conv of x_vals [B][H][W][C] with w_vals [cout][kh][kw][C] on the values as given, in dtype
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


# ---------------------------------------------------------------------------------------------
# the conv kinds behind spi_op_conv2d (test_conv_kinds_ops_gpu.py): kConvGen, kConvTap, the three kConvTapW
# forms, kConvHalo / kConvHaloS and the weight-resident 64 -> 64 conv, on non-square maps and filters
#
# A shape is always the 9-tuple (B, H, W, Cin, Cout, KH, KW, stride, pad).

# 3x3 / stride 1 / pad 1, (B, H, W, Cin, Cout): the smallest at which each kind still does all it can do
CONV3_SHAPES = {
    "S1": (1, 5, 9, 64, 64),       # one ragged tile; eligible for the weight-resident kernel
    "S2": (2, 13, 3, 128, 64),     # W = 3: every pixel on a side border, the image seam inside a tile
    "S3": (3, 7, 20, 64, 128),     # three images, M = 420, two column tiles
    "S4": (2, 14, 9, 128, 128),    # the default rule's 64-row halo (OH >= 14)
    "S5": (1, 9, 30, 64, 64),      # short and wide
    "S6": (3, 6, 17, 64, 64),      # kConvHaloS
    "S7": (1, 20, 50, 64, 64),     # the default rule's 128-row halo (OW > 32); no 64-row candidate fits
    "S8": (2, 3, 61, 64, 64),      # H = 3; no 64-row candidate fits
    "S9": (1, 30, 9, 256, 64),     # tall and narrow; 4 (fp16) or 8 channel blocks: the deepest split-K
    "S10": (2, 40, 52, 64, 256),   # the 128 x 64 window tile: 132 tiles, M = 4160 = 32.5 tile rows
}
# the weight-resident kernel (fp16, 64 -> 64), (B, H, W): the widest map whose halo fits (th = 1), one pixel
# wider (must not take the kernel), one 16-row band per image, 2-row bands with a partial last one, 61 rows,
# an odd band count
WRES_SHAPES = [(1, 3, 83), (1, 3, 84), (2, 16, 8), (3, 13, 56), (2, 61, 30), (19, 28, 28)]
WRES_REFUSED = (1, 3, 84)
# geometry no model uses, for the tap walk and the gather
CONV_GEO_SHAPES = [
    (1, 9, 13, 64, 96, 5, 5, 1, 2),    # 25 taps (K = Kpad = 1600), ragged Cout, 4 to 8 slices
    (2, 9, 14, 64, 64, 1, 7, 1, 0),    # KH != KW
    (1, 11, 7, 32, 64, 3, 1, 2, 1),    # KH != KW at stride 2, K = 96 of Kpad = 128: the gather in fp16, the
                                       # tap walk with a Kpad tail step elsewhere
    (1, 10, 12, 64, 64, 7, 7, 2, 3),   # 49 taps: the gather at wide Cin; the split layout rejects it
    (1, 9, 11, 16, 24, 3, 3, 1, 1),    # the gather with k-steps straddling filter rows
    (1, 12, 10, 64, 64, 3, 3, 3, 0),   # stride 3, no padding, the last columns unused
    (2, 8, 15, 128, 64, 1, 1, 1, 1),   # the output's outer ring lies wholly in the padding: act(bias)
    (1, 6, 10, 64, 64, 3, 3, 1, 2),    # pad > k // 2
]
CONV_RING = (2, 8, 15, 128, 64, 1, 1, 1, 1)
CONV_PRECS = ("fp32", "fp16", "fp16x3", "fp16x3s")
PREC_ID = {"fp32": 0, "fp16": 1, "fp16x3": 2, "fp16x3s": 3}
KIND_KNOBS = ("SPI_GEMM_WIN", "SPI_GEMM_HALO_CFG", "SPI_CONV_WRES", "SPI_GEMM_MAXSPLIT", "SPI_GEMM_PLAN")
_NO_FAST = {"SPI_GEMM_HALO_CFG": "0", "SPI_CONV_WRES": "0"}
KIND_SETTINGS = {
    **{f"win{v}": {**_NO_FAST, "SPI_GEMM_WIN": str(v)} for v in range(4)},
    **{f"halo{rows}{m}": {"SPI_GEMM_HALO_CFG": f"{rows},{m}", "SPI_CONV_WRES": "0"}
       for rows in (64, 128, 256) for m in "as"},
    "rule": {"SPI_CONV_WRES": "0"},
    "rule-max3": {"SPI_CONV_WRES": "0", "SPI_GEMM_MAXSPLIT": "3"},
    "wres2": {"SPI_CONV_WRES": "2"},
    "wres0": {"SPI_CONV_WRES": "0"},
    "default": {},
    "plan64": {"SPI_GEMM_PLAN": "64,64,3,2"},
    "plan128x64": {"SPI_GEMM_PLAN": "128,64,2,1"},
    "plan128": {"SPI_GEMM_PLAN": "128,128,2,1"},
}
HALO_SETTINGS = [f"halo{rows}{m}" for rows in (64, 128, 256) for m in "as"] + ["rule"]
PLAN_FIELDS = ("bm", "bn", "stages", "splits", "halo", "win", "nw", "k_per_split")


def shape9(s):
    """(B, H, W) of a weight-resident shape or (B, H, W, Cin, Cout) of a 3x3 one -> the 9-tuple."""
    s = tuple(s)
    if len(s) == 3:
        s += (64, 64)
    return s + (3, 3, 1, 1) if len(s) == 5 else s


def conv_accepts(prec, shape):
    """Whether spi_op_conv2d takes the shape at the precision (include/spi_ops.h)."""
    _, H, W, cin, cout, kh, kw, _, pad = shape
    if H + 2 * pad < kh or W + 2 * pad < kw or cin & (cin - 1) or cin < (8 if prec == "fp16" else 4):
        return False
    return prec != "fp16x3s" or (cin >= 32 and cout % 32 == 0 and kh * kw <= 31)


def conv_kind_runs():
    """Every (group, setting, precision, shape) the GPU tests launch, in the order they run: the smallest
    maps first within a group.  test_exact_integer_cases runs the same list."""
    runs = []
    s3 = {k: shape9(v) for k, v in CONV3_SHAPES.items()}
    for name in sorted(s3, key=lambda n: s3[n][0] * s3[n][1] * s3[n][2] * s3[n][3]):
        for prec in ("fp16", "fp16x3s"):
            runs += [("window", f"win{v}", prec, s3[name]) for v in (1, 0, 2, 3)]
        if name != "S10":
            for prec in ("fp32", "fp16", "fp16x3s"):
                runs += [("halo", st, prec, s3[name]) for st in HALO_SETTINGS]
                if name == "S9":
                    runs.append(("halo", "rule-max3", prec, s3[name]))
    for s in sorted(WRES_SHAPES, key=lambda s: s[0] * s[1] * s[2]):
        runs += [("wres", st, "fp16", shape9(s)) for st in ("wres2", "wres0")]
    for i, s in enumerate(CONV_GEO_SHAPES):
        for prec in CONV_PRECS:
            if conv_accepts(prec, s):
                runs += [("geo", st, prec, s) for st in ("default", ("plan64", "plan128x64", "plan128")[i % 3])]
    return runs


def kind_key(setting, prec, shape):
    return f"{setting}|{prec}|" + ",".join(map(str, shape))


def query_conv_plan(lib, prec, shape):
    """spi_debug_conv_plan under the knobs in force, as a list of the 8 PLAN_FIELDS."""
    import ctypes as C
    out = (C.c_int * 8)()
    assert lib.spi_debug_conv_plan(PREC_ID[prec], *shape, out) == 0
    return [int(v) for v in out]


def query_conv_route(lib, prec, shape, res, act):
    """spi_debug_conv_route: 1 when the weight-resident kernel would run (aligned operands, a whole pack)."""
    return int(lib.spi_debug_conv_route(PREC_ID[prec], *shape, int(bool(res)), {None: 0, "relu": 1}[act]))


class kind_knobs:
    """with kind_knobs(lib, setting): the five knobs set to the setting's values (the others unset), re-read
    by the library, and put back on the way out."""

    def __init__(self, lib, setting):
        self.lib, self.env = lib, KIND_SETTINGS[setting]

    def __enter__(self):
        import os
        self.saved = {k: os.environ.pop(k, None) for k in KIND_KNOBS}
        os.environ.update(self.env)
        self.lib.spi_debug_gemm_reload_env()

    def __exit__(self, *exc):
        import os
        for k, v in self.saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
        self.lib.spi_debug_gemm_reload_env()


def conv_kind_name(prec, shape, plan, route=0):
    """The device path a plan means, as gemm() / dispatch() / launch_tile() choose it: wres, halo<rows> /
    haloS64, win<rows>x<waves>, gen (several taps per k-step: Cin below the k-step, or more than 31 taps) or
    tap; "-k<slices>" appended under split-K."""
    pl = dict(zip(PLAN_FIELDS, plan))
    if route:
        return "wres"
    cin, taps = shape[3], shape[5] * shape[6]
    if pl["halo"]:
        name = ("haloS" if pl["halo"] == 2 else "halo") + str(pl["bm"])
    elif pl["win"]:
        name = f"win{pl['bm']}x{pl['nw']}"
    elif cin < (64 if prec == "fp16" else 32) or taps > 31:
        name = f"gen{pl['bm']}x{pl['bn']}"
    else:
        name = f"tap{pl['bm']}x{pl['bn']}"
    return name + (f"-k{pl['splits']}" if pl["splits"] > 1 else "")


def split_values(x):
    """float64 hi + lo of the split layout: fp16(x) + fp16(x - fp16(x)) (ops.from_split(ops.to_split(x)))."""
    x = np.asarray(x, np.float32)
    hi = x.astype(np.float16)
    return hi.astype(np.float64) + (x - hi.astype(np.float32)).astype(np.float16).astype(np.float64)


def operand_values(prec, x, w=None):
    """float64 values the kernel multiplies / adds for fp32 data at a precision: fp16-rounded for fp16 (the
    weight too), the split layout's hi + lo for fp16x3s activations against the fp32 weight, the fp32
    values for fp32 and fp16x3."""
    def act(a):
        a = np.asarray(a, np.float32)
        return a.astype(np.float16).astype(np.float64) if prec == "fp16" else \
            split_values(a) if prec == "fp16x3s" else a.astype(np.float64)
    if w is None:
        return act(x)
    w = np.asarray(w, np.float32)
    return act(x), (w.astype(np.float16) if prec == "fp16" else w).astype(np.float64)


def conv_out_hw(shape):
    _, H, W, _, _, kh, kw, stride, pad = shape
    return (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1


def conv_kind_case(shape):
    """fp32 inputs of one shape, shared by every precision, kind and form: x [B][H][W][Cin] of N(0, 1), the
    weight [Cout][KH][KW][Cin] of He scale, bias and residual [B][OH][OW][Cout] of N(0, 1)."""
    B, H, W, cin, cout, kh, kw, stride, pad = shape
    x, [(w, b)] = conv_case(B, H, cin, [(cout, (kh, kw), stride, pad)], seed=sum(v * 31 ** i for i, v in enumerate(shape)),
                            W=W)
    oh, ow = conv_out_hw(shape)
    r = np.random.default_rng(H * 100 + W + cout).standard_normal((B, oh, ow, cout)).astype(np.float32)
    return x, w, b, r


EXACT_MAX = 2048  # every integer up to 2048 is an fp16 number


def conv_exact_case(shape):
    """An integer case: x in [-2, 2], w in {-1, 0, 1}, bias and residual in [-4, 4], ReLU.  Every product and
    partial sum is an integer far below 2^24: exact in fp32 in any order, under any split-K; the reference
    stays within EXACT_MAX, so an fp16 or split output holds it exactly as well.  Returns x, w, b, r (fp32,
    the same for every precision) and the float64 reference [B][OH][OW][Cout]."""
    B, H, W, cin, cout, kh, kw, stride, pad = shape
    rng = np.random.default_rng(7 + sum(v * 29 ** i for i, v in enumerate(shape)))
    x = rng.integers(-2, 3, (B, H, W, cin)).astype(np.float32)
    w = rng.integers(-1, 2, (cout, kh, kw, cin)).astype(np.float32)
    b = rng.integers(-4, 5, cout).astype(np.float32)
    oh, ow = conv_out_hw(shape)
    r = rng.integers(-4, 5, (B, oh, ow, cout)).astype(np.float32)
    ref = epilogue64(conv_acc(x, w, stride, pad), b, r, "relu")
    assert np.abs(conv_acc(x, w, stride, pad)).max() + 8 <= EXACT_MAX and np.abs(ref).max() <= EXACT_MAX, shape
    assert np.array_equal(ref, np.rint(ref)) and ref.max() > 0
    return x, w, b, r, ref


# the wrong 3x3 / s1 / p1 convs a kernel with a slipped index computes (test_op_refs holds each at least
# 10x above the bar, for every CONV3_SHAPES entry)
def conv3_flat_unmasked(xv, wv, shape):
    """No column, row or image mask: tap (kh, kw) of pixel m reads pixel m + (kh - 1) W + kw - 1 of the flat
    pixel list whenever that lies in [0, M)."""
    B, H, W, cin, cout = shape[:5]
    M = B * H * W
    xf = np.asarray(xv, np.float64).reshape(M, cin)
    out = np.zeros((M, cout))
    for kh in range(3):
        for kw in range(3):
            off = (kh - 1) * W + kw - 1
            lo, hi = max(0, -off), min(M, M - off)
            out[lo:hi] += xf[lo + off:hi + off] @ np.asarray(wv, np.float64)[:, kh, kw].T
    return out.reshape(B, H, W, cout)


def conv3_hw_exchanged(xv, wv, shape):
    """The same pixel list walked as [B][W][H]."""
    B, H, W, cin, cout = shape[:5]
    return conv_acc(np.asarray(xv).reshape(B, W, H, cin), wv, 1, 1).reshape(B, H, W, cout)


def conv3_images_joined(xv, wv, shape):
    """The B images as one tall image: rows leak across the seams."""
    B, H, W, cin, cout = shape[:5]
    return conv_acc(np.asarray(xv).reshape(1, B * H, W, cin), wv, 1, 1).reshape(B, H, W, cout)


def conv3_window_walk(xv, wv, shape, bm=64, col_mask=True, pitch=None):
    """The kw-window kind's indexing (gemm.hip kConvTapW, as test_window_indexing.py restates it) on an
    H x W map: per tile of bm output pixels from m0 and filter row kh, the bm + 2 pixels from
    m0 + (kh - 1) pitch - 1 on (zeros outside [0, M)), tap kw of tile row r from window row r + kw, taps
    outside the image zeroed by the per-row mask.  pitch = W and col_mask give the conv; col_mask=False
    drops the mask's column terms, pitch = H is issue_win with d.H written for d.W."""
    B, H, W, cin, cout = shape[:5]
    pitch = W if pitch is None else pitch
    M = B * H * W
    xf, w = np.asarray(xv, np.float64).reshape(M, cin), np.asarray(wv, np.float64)
    out = np.zeros((M, cout))
    rows = np.arange(bm)
    for m0 in range(0, M, bm):
        m = m0 + rows
        valid = m < M
        rem = np.where(valid, m, 0) % (H * W)
        oh, ow = rem // W, rem % W
        left, right = ((ow > 0), (ow + 1 < W)) if col_mask else (np.ones(bm, bool), np.ones(bm, bool))
        acc = np.zeros((bm, cout))
        for kh in range(3):
            row_ok = valid & (oh + kh - 1 >= 0) & (oh + kh - 1 < H)
            pix = m0 + (kh - 1) * pitch - 1 + np.arange(bm + 2)
            win = np.where(((pix >= 0) & (pix < M))[:, None], xf[np.clip(pix, 0, M - 1)], 0.0)
            for kw, col_ok in enumerate((left, np.ones(bm, bool), right)):
                acc += np.where((row_ok & col_ok)[:, None], win[rows + kw], 0.0) @ w[:, kh, kw].T
        out[m[valid]] = acc[valid]
    return out.reshape(B, H, W, cout)


# ---------------------------------------------------------------------------------------------
# the fused stem (stem.hip; test_stem_ops_gpu.py): 7x7/s2/p3 conv over 3 channels + bias + ReLU + 3x3/s2/p1 max
# pool, NCHW image -> NHWC [B][PH][PW][64]
#
# A precision code is spi_op_stem_pool's: 1 fp16 image x fp16 weights, 2 fp16 image x hi + lo weights (fp16m),
# 3 split image x hi + lo weights into the split layout, 4 the same arithmetic into fp16.

STEM_CODES = {"fp16": 1, "fp16m": 2, "fp16x3s": 3, "fp16x3": 4}
STEM_BAR = {1: 1e-3, 2: 1e-3, 3: 1e-5, 4: 1e-3}
# (B, H, W, image kind).  OW = (W - 1) // 2 + 1 stem columns in groups of 64, PH / PW pooled rows / columns; a
# workgroup takes PR pooled rows (rows_per_block 1 / 2: PR = 1 / 2 on 4 waves; 0: PR = 2 on 8 waves when
# OW > 64, else PR = 1 on 4).  test_stem_ops_gpu's docstring says which shape reaches which edge.
STEM_SHAPES = [
    (1, 1, 1, "randn"), (3, 9, 7, "rand"), (1, 2, 8, "randn"), (1, 10, 47, "rand"), (3, 11, 127, "randn"),
    (1, 13, 128, "rand"), (1, 2, 129, "randn"), (3, 9, 131, "randn"), (1, 23, 130, "rand"), (1, 11, 132, "randn"),
    (1, 13, 190, "rand"), (1, 10, 221, "randn"), (3, 1, 223, "rand"), (1, 40, 222, "randn"), (1, 23, 224, "randn"),
]
STEM_REFUSED_W = (225, 226)
# the ImageNet transform: three distinct scales and non-zero shifts, signed images
STEM_SCALE = (np.float32(1) / (np.float32(255) * np.float32([0.229, 0.224, 0.225]))).astype(np.float32)
STEM_SHIFT = (-np.float32([0.485, 0.456, 0.406]) / np.float32([0.229, 0.224, 0.225])).astype(np.float32)


def stem_out_hw(H, W):
    """(OH, OW, PH, PW) of an H x W image."""
    oh, ow = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    return oh, ow, (oh - 1) // 2 + 1, (ow - 1) // 2 + 1


def stem_form(rows_per_block, OW):
    """(PR, NW) of the instance stem_pool() launches (stem.hip): 2 -> (2, 4); 1, or a one-group map -> (1, 4);
    else two pooled rows on 8 waves."""
    return (2, 4) if rows_per_block == 2 else (1, 4) if rows_per_block == 1 or OW <= 64 else (2, 8)


def stem_case(B, H, W, kind):
    """One shape's inputs: x fp32 [B][3][H][W] (N(0, 1), or U[0, 1) for "rand"), 8-bit pixels u8 [B][3][H][W]
    (their NHWC form is a transpose), the weight [64][3][7][7] and bias [64] of sigma 0.1 (test_ops_gpu's)."""
    rng = np.random.default_rng(B * 100000 + H * 1000 + W)
    x = (rng.standard_normal((B, 3, H, W)) if kind == "randn" else rng.random((B, 3, H, W))).astype(np.float32)
    u8 = rng.integers(0, 256, (B, 3, H, W), dtype=np.uint8)
    w = (0.1 * rng.standard_normal((64, 3, 7, 7))).astype(np.float32)
    b = (0.1 * rng.standard_normal(64)).astype(np.float32)
    return x, u8, w, b


def stem_operands(code, x, w):
    """float64 (image, weight) values a precision code multiplies: fp16(x) for codes 1 and 2, hi + lo for 3 and 4;
    fp16(w) for code 1, hi + lo otherwise.  (The kernel leaves out the lo x lo products, about 2^-22 of a term:
    stem_lattice_ref models that where a bit depends on it.)"""
    xv = hi_values(x) if code <= 2 else split_values(x)
    return xv, (hi_values(w) if code == 1 else hilo_values(w))


def stem_conv64(xv, wv, pad_value=None):
    """float64 7x7/s2/p3 conv of [B][3][H][W] values -> NHWC [B][OH][OW][64]; the padding is 0, or with
    pad_value [3] that constant per channel (a mutant)."""
    x = torch.from_numpy(np.ascontiguousarray(xv, np.float64))
    if pad_value is not None:
        p = torch.from_numpy(np.asarray(pad_value, np.float64)).view(1, 3, 1, 1)
        x = torch.nn.functional.pad(x - p, (3, 3, 3, 3)) + p
    else:
        x = torch.nn.functional.pad(x, (3, 3, 3, 3))
    y = torch.nn.functional.conv2d(x, torch.from_numpy(np.ascontiguousarray(wv, np.float64)), None, 2, 0)
    return y.permute(0, 2, 3, 1).contiguous().numpy()


def stem_pool64(s, no_left_at=None, no_row_above=None):
    """3x3/s2/p1 max pool of the ReLU'd stem map s [B][OH][OW][64] (>= 0, so padding may enter as 0).
    Mutants: no_left_at = pc: pooled column pc misses its left stem column 2 pc - 1 (the column a 64-column
    group takes from the group before: pc = 32); no_row_above = PR: every pooled row pr > 0 that starts a
    workgroup of PR rows misses stem row 2 pr - 1 (the row the workgroup recomputes)."""
    B, OH, OW, C = s.shape
    PH, PW = (OH - 1) // 2 + 1, (OW - 1) // 2 + 1
    sp = np.zeros((B, 2 * PH + 2, 2 * PW + 2, C))
    sp[:, 1:OH + 1, 1:OW + 1] = s
    out = np.zeros((B, PH, PW, C))
    for dr in range(3):
        for dc in range(3):
            t = sp[:, dr:dr + 2 * PH:2, dc:dc + 2 * PW:2].copy()
            if dc == 0 and no_left_at is not None and no_left_at < PW:
                t[:, :, no_left_at] = 0
            if dr == 0 and no_row_above:
                t[:, no_row_above::no_row_above] = 0
            out = np.maximum(out, t)
    return out


def stem_ref(xv, wv, bias, **mutant):
    """float64 pooled stem output [B][PH][PW][64] on the operand values as given."""
    pad = mutant.pop("pad_value", None)
    return stem_pool64(np.maximum(stem_conv64(xv, wv, pad) + np.asarray(bias, np.float64), 0), **mutant)


def stem_split_bits(ref):
    """The split layout of a float64 [..][64] reference as fp16 [..][128]: per pixel [32 hi | 32 lo] x 2."""
    r = np.asarray(ref, np.float64).astype(np.float32)
    hi = r.astype(np.float16)
    lo = (r - hi.astype(np.float32)).astype(np.float16)
    sh = r.shape[:-1]
    return np.concatenate([hi.reshape(*sh, 2, 32), lo.reshape(*sh, 2, 32)], axis=-1).reshape(*sh, 128)


def stem_from_split(bits16):
    """fp16 [..][128] split layout -> float64 hi + lo [..][64]."""
    h = np.asarray(bits16, np.float16).astype(np.float64)
    sh = h.shape[:-1]
    h = h.reshape(*sh, 2, 64)
    return (h[..., :32] + h[..., 32:]).reshape(*sh, 64)


def stem_hi_of_split(bits16):
    """The hi halves of an fp16 [..][128] split output as fp16 [..][64]."""
    sh = bits16.shape[:-1]
    return np.ascontiguousarray(np.asarray(bits16).reshape(*sh, 2, 64)[..., :32]).reshape(*sh, 64)


# the exact-lattice cases, (B, H, W): one group (tall enough for pooled pixels clear of the border), a second
# group of two columns with an odd PH and odd image starts, the widest map
STEM_LATTICE_SHAPES = [(1, 15, 47), (3, 9, 131), (1, 11, 224)]


def stem_lattice_case(B, H, W, variant="mixed"):
    """Inputs whose every product and partial sum is exact in fp32 in any order: the image integers in [0, 7]
    (xi; what a u8 source feeds under the default transform) plus, for the fp32 source, a lo part of +-2^-10 on
    the pixels >= 4 (a quarter of an fp16 ulp there: fp16(x) is the integer and the lo plane +-2^-10); weights
    hi in {-1, 0, 1} plus lo in {-2 .. 2} x 2^-13 where hi != 0, another pattern per tap and channel; bias
    multiples of 2^-13.  Every term is a multiple of 2^-13 (the lo x lo products, 2^-23, are the ones the
    kernel omits) and every sum stays below 147 x 7 (1 + 2^-11) + 8 < 2^11.
    variant "lowt" (the lo-weight case at fp16m): a constant image of 4s, and hi weights that sum to zero per
    channel, so an interior output is bias + 4 sum(lo) -- a kernel without the lo MFMA gives bias.
    Returns xi uint8 [B][3][H][W], x fp32 (xi + lo), w fp32 [64][3][7][7], bias fp32 [64]."""
    rng = np.random.default_rng(5000 + B * 100000 + H * 1000 + W + (variant == "lowt"))
    n, c, kh, kw = np.meshgrid(np.arange(64), np.arange(3), np.arange(7), np.arange(7), indexing="ij")
    tap = (c * 7 + kh) * 7 + kw
    if variant == "lowt":
        xi = np.full((B, 3, H, W), 4, np.uint8)
        hi = np.where(tap == (n % 147), 0, np.where((tap + (tap > n % 147) + n) % 2, 1, -1))  # 73 of each sign
        assert (hi.reshape(64, -1).sum(1) == 0).all()
        bias = 1 + rng.integers(0, 64, 64) * 2.0 ** -13
    else:
        xi = rng.integers(0, 8, (B, 3, H, W)).astype(np.uint8)
        hi = (n * 5 + tap * 3 + (tap // 7)) % 3 - 1
        bias = rng.integers(-8 * 2 ** 13, 8 * 2 ** 13, 64) * 2.0 ** -13
    lo = np.where(hi != 0, (n * 7 + tap * 11 + kw * 3) % 5 - 2, 0) * 2.0 ** -13
    xlo = np.where(xi >= 4, rng.integers(-1, 2, xi.shape), 0) * 2.0 ** -10
    x = (xi + xlo).astype(np.float32)
    w = (hi + lo).astype(np.float32)
    assert np.array_equal(x.astype(np.float16).astype(np.float64), xi) and np.array_equal(split_values(x), xi + xlo)
    assert np.array_equal(hi_values(w), hi) and np.array_equal(hilo_values(w), hi + lo)
    return xi, x, w, bias.astype(np.float32)


def stem_lattice_ref(code, x, w, bias, drop_lo_w=False, drop_lo_x=False):
    """The exact float64 output of a lattice case from the products the kernel forms: hi x hi, then hi x lo
    (weights; codes >= 2) and lo x hi (image; codes 3 and 4), never lo x lo."""
    xh, wh = hi_values(x), hi_values(w)
    xl, wl = split_values(x) - xh, hilo_values(w) - wh
    acc = stem_conv64(xh, wh)
    if code >= 2 and not drop_lo_w:
        acc = acc + stem_conv64(xh, wl)
    if code >= 3 and not drop_lo_x:
        acc = acc + stem_conv64(xl, wh)
    assert np.abs(acc).max() + 8 < 2048 and np.array_equal(acc * 2 ** 13, np.rint(acc * 2 ** 13))
    return stem_pool64(np.maximum(acc + np.asarray(bias, np.float64), 0))


def stem_expected_bits(code, ref):
    """A float64 reference rounded once as the kernel stores it: fp16 [..][64], or for code 3 the split
    layout fp16 [..][128]."""
    return stem_split_bits(ref) if code == 3 else np.asarray(ref, np.float64).astype(np.float32).astype(np.float16)


# ---------------------------------------------------------------------------------------------
# fused avgpool + FC (GemmDesc::pool_rows; test_fc_ops_gpu.py): x [B][HW][C] -> act(mean_HW(x) W^T + bias) [B][N]

# (B, HW, C, N, bias, act): HW = 1, 2, 3, 5 leave some of the four row parts empty; 63 / 64 fill the tile;
# B = 65 is more than a tile's rows; N = 1, 64 / 65 (one tile to the column, one column into the next), 70, 1000;
# C = 2048 is 32 (fp16) or 64 k-steps: the 3-stage ring; C = 32 one k-step or half of one
FC_CASES = [
    (1, 1, 32, 1, True, None), (65, 2, 96, 64, False, "relu"), (3, 3, 32, 65, True, "relu"),
    (65, 4, 32, 70, True, None), (3, 5, 96, 64, False, None), (3, 7, 512, 70, True, "relu"),
    (1, 16, 2048, 65, True, None), (3, 49, 512, 1000, True, None), (3, 49, 512, 1000, False, "relu"),
    (3, 63, 96, 65, False, None), (3, 64, 32, 1, True, None), (1, 64, 96, 1000, True, None),
]
FC_EXACT = [(3, HW, 96, 70) for HW in (1, 2, 4, 16, 64)]
FC_BAR = 1e-5
# SPI_GEMM_PLAN forced on one pooled case: every dense tile compiles the pooled epilogue (gemm_tile.hpp)
FC_FORCED = ["128,128,2,1", "128,64,2,1", "128,64,3,1", "64,64,2,1", "64,64,4,1", "64,64,3,2"]
FC_FORCED_CASE = (3, 7, 512, 70, True, "relu")


def fc_case(B, HW, C, N):
    """x fp32 [B][HW][C] of N(0, 1) + 0.5 (a mean that does not vanish), W [N][C] of N(0, 1 / C), bias N(0, 1)."""
    rng = np.random.default_rng(B * 1000003 + HW * 10007 + C * 13 + N)
    x = (rng.standard_normal((B, HW, C)) + 0.5).astype(np.float32)
    W = (rng.standard_normal((N, C)) / np.sqrt(C)).astype(np.float32)
    return x, W, rng.standard_normal(N).astype(np.float32)


def fc_exact_case(B, HW, C, N):
    """Integers: x in [-4, 4], W in {-1, 0, 1}, bias multiples of 1 / 4 -- with HW a power of two every sum,
    the division and the bias add are exact in fp32 (|sum| <= 64 C 4 < 2^24), in every precision's operands."""
    rng = np.random.default_rng(77 + HW)
    x = rng.integers(-4, 5, (B, HW, C)).astype(np.float32)
    W = rng.integers(-1, 2, (N, C)).astype(np.float32)
    return x, W, (rng.integers(-16, 17, N) / 4).astype(np.float32)


def fc_ref(xv, wv, bias, act, mutant=None):
    """float64 act(mean over HW of (x W^T) + bias) on the operand values.  Mutants (what a slipped index in the
    pooled epilogue computes): "next": the tile's 64 rows summed, the next images' included, where they
    exist; "div64": divided by 64; "part3": the rows r = 3 mod 4 (one of the four partial sums) dropped."""
    xv = np.asarray(xv, np.float64)
    B, HW, _ = xv.shape
    rows = xv.reshape(B * HW, -1) @ np.asarray(wv, np.float64).T
    if mutant == "next":
        tot = np.stack([rows[b * HW:b * HW + 64].sum(0) for b in range(B)])
    elif mutant == "part3":
        tot = (rows.reshape(B, HW, -1) * (np.arange(HW) % 4 != 3)[None, :, None]).sum(1)
    else:
        tot = rows.reshape(B, HW, -1).sum(1)
    return epilogue64(tot / (64 if mutant == "div64" else HW), bias, None, act)


# ---------------------------------------------------------------------------------------------
# dense GEMM at fp32 / fp16x3 / fp16x3s (spi_op_gemm, precisions 0, 2, 3): the k-step is 32

DENSE32_PRECS = ("fp32", "fp16x3", "fp16x3s")
# KREP_DENSE's pattern: ragged M and N, K tails of half a step (176 = 160 + 16, 40); the default plan splits the
# last three
DENSE32_SHAPES = [(64, 64, 96), (100, 96, 176), (50, 1000, 40), (8, 128, 768), (197, 128, 1024), (64, 64, 1152)]
DENSE32_FORMS = ["plain", "res", "relu", "gelu"]
DENSE32_FORCED = [("128,128,2,1", (50, 1000, 96)), ("128,64,2,1", (197, 128, 176)), ("128,64,3,2", (197, 128, 1024)),
                  ("64,64,2,5", (100, 96, 448)), ("64,64,3,3", (64, 64, 1152)), ("64,64,4,2", (100, 96, 448))]
DENSE32_XCD = (300, 320, 64)  # under "64,64,2,1": 5 x 5 tiles


def dense32_shape(prec, M, N, K):
    """The split layout keeps its multiples of 32 (K and N rounded down)."""
    return (M, N // 32 * 32, K // 32 * 32) if prec == "fp16x3s" else (M, N, K)


def dense32_case(M, N, K):
    """fp32 A of N(0, 1), W of N(0, 1 / K), bias and residual at a quarter of the output's sigma."""
    rng = np.random.default_rng(M * 7 + N * 3 + K + 1)
    A = rng.standard_normal((M, K)).astype(np.float32)
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    return A, W, (0.25 * rng.standard_normal(N)).astype(np.float32), (0.25 * rng.standard_normal((M, N))).astype(np.float32)


def dense32_ksteps(K):
    """k-steps of 32 in the packed K (padded to a multiple of 64)."""
    return -(-K // 64) * 2


def forced_splits(ksteps, splits, max_split=8):
    """finish_plan's slice count for a 64-column tile: slices of ceil(ksteps / splits) steps."""
    s = max(1, min(splits, max_split, ksteps))
    kt = -(-ksteps // s)
    return -(-ksteps // kt), kt

"""Op-level wrappers over include/spi_ops.h (kernel parity tests, micro-benchmarks).

Every call goes to libspi_hip.so; tensors are torch device tensors used as
plain HBM buffers (torch shares the process's HIP runtime, see _native.py).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _native as N
from ._native import lib

PREC = {"fp32": 0, "fp16": 1, "fp16x3": 2, "fp16x3s": 3}  # fp16x3s: split activation layout
ACT = {None: 0, "none": 0, "relu": 1, "gelu": 2}


class OpError(RuntimeError):
    pass


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _check(rc):
    if rc != 0:
        raise OpError(N.last_error())


def act_dtype(prec: str) -> torch.dtype:
    return torch.float16 if prec == "fp16" else torch.float32


def to_split(x: torch.Tensor) -> torch.Tensor:
    """fp32 [..., C] (C % 32 == 0) -> the split layout (fp16x3s operands), stored in a
    float32 tensor of the same shape: per 32-channel block [32 hi fp16 | 32 lo fp16]."""
    x = x.float().contiguous()
    hi = x.half()
    lo = (x - hi.float()).half()
    blk = x.shape[-1] // 32
    s = torch.cat([hi.reshape(*x.shape[:-1], blk, 32), lo.reshape(*x.shape[:-1], blk, 32)], dim=-1)
    return s.contiguous().view(torch.float32).reshape(x.shape)


def from_split(s: torch.Tensor) -> torch.Tensor:
    """Inverse of to_split: hi + lo in fp32."""
    blk = s.shape[-1] // 32
    h = s.contiguous().view(torch.float16).reshape(*s.shape[:-1], blk, 64)
    return (h[..., :32].float() + h[..., 32:].float()).reshape(s.shape)


def pack_weight(prec: str, w: np.ndarray | torch.Tensor, device="cuda") -> torch.Tensor:
    """[N][K] fp32 -> packed device buffer (uint8 tensor)."""
    w = np.ascontiguousarray(np.asarray(w.cpu() if isinstance(w, torch.Tensor) else w, dtype=np.float32))
    n, k = w.shape
    npad, kpad = C.c_int32(), C.c_int32()
    nbytes = lib.spi_op_packed_bytes(PREC[prec], n, k, C.byref(npad), C.byref(kpad))
    host = np.empty(nbytes, dtype=np.uint8)
    _check(lib.spi_op_pack_weight(PREC[prec], w.ctypes.data, n, k, host.ctypes.data))
    return torch.from_numpy(host).to(device)


def conv_weight_matrix(w: torch.Tensor, cin_pad: int) -> np.ndarray:
    """torch conv weight [Cout][Cin][KH][KW] -> [Cout][KH*KW*cin_pad] (k = (kh*KW+kw)*cin_pad + c)."""
    cout, cin, kh, kw = w.shape
    m = torch.zeros(cout, kh, kw, cin_pad)
    m[..., :cin] = w.permute(0, 2, 3, 1)
    return m.reshape(cout, kh * kw * cin_pad).numpy()


def workspace(device="cuda") -> torch.Tensor:
    return torch.zeros(lib.spi_op_workspace_bytes(), dtype=torch.uint8, device=device)


def gemm(prec, A, W_packed, N_, bias=None, residual=None, out=None, out_f32=True, act=None, ws=None,
         stream=None, res_f32=None):
    M, K = A.shape
    if out is None:
        out = torch.empty(M, N_, device=A.device, dtype=torch.float32 if out_f32 else act_dtype(prec))
    split = prec == "fp16x3s"  # float32-storage tensors holding the split layout, not fp32 values
    if res_f32 is None:
        res_f32 = residual is not None and residual.dtype == torch.float32 and not split
    ws = workspace(A.device) if ws is None else ws
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    _check(lib.spi_op_gemm(PREC[prec], _ptr(A), M, K, A.stride(0), _ptr(W_packed), N_, _ptr(bias), _ptr(residual),
                           int(res_f32), residual.stride(0) if residual is not None else 0, _ptr(out),
                           int(out.dtype == torch.float32 and not split), out.stride(0), ACT[act], _ptr(ws), C.c_void_p(s)))
    return out


def conv2d(prec, x_nhwc, W_packed, cout, kh, kw, stride, pad, bias=None, residual=None, act=None, ws=None,
           stream=None, out=None):
    B, H, W_, cin = x_nhwc.shape
    oh, ow = (H + 2 * pad - kh) // stride + 1, (W_ + 2 * pad - kw) // stride + 1
    if out is None:
        out = torch.empty(B, oh, ow, cout, device=x_nhwc.device, dtype=x_nhwc.dtype)
    ws = workspace(x_nhwc.device) if ws is None else ws
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    _check(lib.spi_op_conv2d(PREC[prec], _ptr(x_nhwc), B, H, W_, cin, _ptr(W_packed), cout, kh, kw, stride, pad,
                             _ptr(bias), _ptr(residual), _ptr(out), ACT[act], _ptr(ws), C.c_void_p(s)))
    return out


# ---- hi + lo fp16 weights (the fp16m layers, GemmDesc::krep = 2) and the grouped conv pair ----


def pack_weight_hilo_host(w: np.ndarray | torch.Tensor) -> np.ndarray:
    """[N][K] fp32 -> the hi + lo packed image as a host fp16 array [Npad][Kpad] (Kpad = 2 round_up(K, 64):
    per 64 logical k a block [64 hi | 64 lo])."""
    w = np.ascontiguousarray(np.asarray(w.cpu() if isinstance(w, torch.Tensor) else w, dtype=np.float32))
    n, k = w.shape
    npad, kpad = C.c_int32(), C.c_int32()
    nbytes = lib.spi_op_packed_bytes_hilo(n, k, C.byref(npad), C.byref(kpad))
    host = np.empty(nbytes, dtype=np.uint8)
    _check(lib.spi_op_pack_weight_hilo(w.ctypes.data, n, k, host.ctypes.data))
    return host.view(np.float16).reshape(npad.value, kpad.value)


def pack_weight_hilo(w: np.ndarray | torch.Tensor, device="cuda") -> torch.Tensor:
    """[N][K] fp32 -> hi + lo packed device buffer (uint8 tensor)."""
    return torch.from_numpy(pack_weight_hilo_host(w).reshape(-1).view(np.uint8)).to(device)


def gemm_hilo(A, W_packed, N_, bias=None, residual=None, out=None, out_f32=True, act=None, ws=None, stream=None):
    """gemm("fp16", ...) on hi + lo weights (pack_weight_hilo): A fp16; the residual's and out's dtype say
    whether they are fp32."""
    M, K = A.shape
    if out is None:
        out = torch.empty(M, N_, device=A.device, dtype=torch.float32 if out_f32 else torch.float16)
    ws = workspace(A.device) if ws is None else ws
    _check(lib.spi_op_gemm_hilo(_ptr(A), M, K, A.stride(0), _ptr(W_packed), N_, _ptr(bias), _ptr(residual),
                                int(residual is not None and residual.dtype == torch.float32),
                                residual.stride(0) if residual is not None else 0, _ptr(out),
                                int(out.dtype == torch.float32), out.stride(0), ACT[act], _ptr(ws), _stream(stream)))
    return out


def conv2d_hilo(x_nhwc, W_packed, cout, kh, kw, stride, pad, bias=None, residual=None, act=None, ws=None,
                stream=None, out=None, out_f32=False):
    """conv2d("fp16", ...) on hi + lo weights: x fp16 NHWC, Cin >= 64; fp32 residual / output by dtype."""
    B, H, W_, cin = x_nhwc.shape
    oh, ow = (H + 2 * pad - kh) // stride + 1, (W_ + 2 * pad - kw) // stride + 1
    if out is None:
        out = torch.empty(B, oh, ow, cout, device=x_nhwc.device, dtype=torch.float32 if out_f32 else torch.float16)
    ws = workspace(x_nhwc.device) if ws is None else ws
    _check(lib.spi_op_conv2d_hilo(_ptr(x_nhwc), B, H, W_, cin, _ptr(W_packed), cout, kh, kw, stride, pad, _ptr(bias),
                                  _ptr(residual), int(residual is not None and residual.dtype == torch.float32),
                                  _ptr(out), int(out.dtype == torch.float32), ACT[act], _ptr(ws), _stream(stream)))
    return out


PAIR_PLAN_FIELDS = ("bm", "bn", "stages", "splits", "halo", "win", "nw", "k_per_split")


def conv_spec(W_packed, cout, k, stride, pad, y, bias=None, act=None, hilo=False, out_f32=False):
    """One conv of conv_pair (spi_op_conv_spec): a k x k filter, output buffer y."""
    return N.ConvSpec(W_packed.data_ptr(), cout, k, k, stride, pad, None if bias is None else bias.data_ptr(),
                      ACT[act], int(hilo), int(out_f32), y.data_ptr())


def conv_pair(prec, x_nhwc, spec0, spec1, ws, stream=None):
    """Two convs on one input as the ResNet forward runs a block's conv1 and downsample conv (grouped into
    one launch when their plans allow).  spec0 / spec1: conv_spec(); the tensors they were built from must
    stay alive until the call returns.  Returns the plan that ran: {"q0", "q1" (dicts of
    PAIR_PLAN_FIELDS), "grouped", "wgs", "slab_off", "ticket_off", "partial_floats", "counter_slots"}."""
    B, H, W_, cin = x_nhwc.shape
    plan = (C.c_int64 * 22)()
    _check(lib.spi_op_conv_pair(PREC[prec], _ptr(x_nhwc), B, H, W_, cin, None if spec0 is None else C.byref(spec0),
                                None if spec1 is None else C.byref(spec1), _ptr(ws), _stream(stream), plan))
    v = [int(t) for t in plan]
    return {"q0": dict(zip(PAIR_PLAN_FIELDS, v[:8])), "q1": dict(zip(PAIR_PLAN_FIELDS, v[8:16])),
            "grouped": bool(v[16]), "wgs": v[17], "slab_off": v[18], "ticket_off": v[19], "partial_floats": v[20],
            "counter_slots": v[21]}


# ---- grouped 3x3 conv (a ResNeXt bottleneck's conv2; spi_ops.h: spi_op_conv2d_grouped) ----


def pack_weight_grouped(w: np.ndarray | torch.Tensor, groups: int, device="cuda") -> torch.Tensor:
    """torch conv weight [C][C / groups][3][3] fp32 -> the grouped kernel's packed device buffer (uint8 tensor)."""
    w = np.ascontiguousarray(np.asarray(w.cpu() if isinstance(w, torch.Tensor) else w, dtype=np.float32))
    if w.ndim != 4 or groups < 1 or w.shape[0] != w.shape[1] * groups:
        raise OpError("pack_weight_grouped: a [C][C / groups][KH][KW] weight")
    c, _, kh, kw = w.shape
    nbytes = lib.spi_op_gconv_packed_bytes(c, groups, kh, kw)
    host = np.empty(max(nbytes, 16), dtype=np.uint8)
    _check(lib.spi_op_gconv_pack_weight(w.ctypes.data, c, groups, kh, kw, host.ctypes.data))
    return torch.from_numpy(host).to(device)


def conv2d_grouped(x_nhwc, W_packed, groups, stride, bias=None, act=None, out=None, k=3, pad=1, stream=None):
    """Grouped 3x3 / pad 1 conv, fp16 NHWC, Cin == Cout: x [B][H][W][C] -> out [B][OH][OW][C] (default: a
    fresh tensor); W_packed from pack_weight_grouped, bias fp32 [C] or None, act None / "relu"; act may also
    be the integer code itself."""
    B, H, W_, c = x_nhwc.shape
    if out is None:
        out = torch.empty(B, (H + 2 * pad - k) // stride + 1, (W_ + 2 * pad - k) // stride + 1, c,
                          device=x_nhwc.device, dtype=torch.float16)
    _check(lib.spi_op_conv2d_grouped(_ptr(x_nhwc), B, H, W_, c, _ptr(W_packed), groups, k, k, stride, pad, _ptr(bias),
                                     _ptr(out), ACT.get(act, act), _stream(stream)))
    return out


def attention(prec, qkv, B, S, heads, mask_bias=None, scale=0.125, stream=None, out=None, head_dim=64):
    """ctx [B S][D] of packed qkv [B S][3 D], D = heads * head_dim (32 or 64); out: the buffer to write
    (default: a fresh one).  prec may be the integer precision code itself."""
    D = heads * head_dim
    ctx = torch.empty(B * S, D, device=qkv.device, dtype=qkv.dtype) if out is None else out
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    _check(lib.spi_op_attention_hd(PREC.get(prec, prec), _ptr(qkv), _ptr(mask_bias), _ptr(ctx), B, S, heads, head_dim,
                                   scale, C.c_void_p(s)))
    return ctx


def layernorm(prec, x, gamma, beta, eps, stream=None):
    rows, D = x.shape
    yf = torch.empty_like(x)
    yt = torch.empty(rows, D, device=x.device, dtype=torch.float16) if prec == "fp16" else None
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    _check(lib.spi_op_layernorm(PREC[prec], _ptr(x), _ptr(gamma), _ptr(beta), _ptr(yf), _ptr(yt), rows, D, eps,
                                C.c_void_p(s)))
    return yf, yt


def avgpool_fc(prec, x, W_packed, N_, bias=None, act=None, ws=None, stream=None, out=None):
    """Fused global average pool + linear layer: x [B][HW][C] -> fp32 [B][N] (one launch); out: the contiguous
    buffer to write (default: a fresh one)."""
    B, HW, Cc = x.shape
    if out is None:
        out = torch.empty(B, N_, device=x.device, dtype=torch.float32)
    ws = workspace(x.device) if ws is None else ws
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    _check(lib.spi_op_avgpool_fc(PREC[prec], _ptr(x), B, HW, Cc, _ptr(W_packed), N_, _ptr(bias), _ptr(out), ACT[act],
                                 _ptr(ws), C.c_void_p(s)))
    return out


# fp16 operands / fp16 image x hi+lo weights (the model's fp16m stem) / hi+lo image x hi+lo weights, split out
# (fp16x3s) or fp16 out (fp16x3)
STEM_PREC = {"fp16": 1, "fp16m": 2, "fp16x3s": 3, "fp16x3": 4}


def stem_pool(prec, x_nchw, w_folded, bias, rows_per_block=0, stream=None, out=None):
    """Fused ResNet stem (7x7/s2 conv over 3 channels, 64 out, folded BN bias, ReLU, 3x3/s2 max pool)
    on the NCHW fp32 image, one launch.  Returns NHWC [B][PH][PW][64]: fp16, or for fp16x3s the split
    layout in a float32-storage tensor; out: the contiguous buffer of that shape and type to write
    (default: a fresh one)."""
    B, _, H, W_ = x_nchw.shape
    oh, ow = (H - 1) // 2 + 1, (W_ - 1) // 2 + 1
    ph, pw = (oh - 1) // 2 + 1, (ow - 1) // 2 + 1
    w = np.ascontiguousarray(np.asarray(w_folded.cpu() if isinstance(w_folded, torch.Tensor) else w_folded,
                                        dtype=np.float32))
    host = np.empty(lib.spi_op_stem_pool_bytes(), dtype=np.uint8)
    _check(lib.spi_op_stem_pool_pack(w.ctypes.data, host.ctypes.data))
    wp = torch.from_numpy(host).to(x_nchw.device)
    if out is None:
        out = torch.empty(B, ph, pw, 64, device=x_nchw.device,
                          dtype=torch.float32 if prec == "fp16x3s" else torch.float16)
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    _check(lib.spi_op_stem_pool(STEM_PREC[prec], _ptr(x_nchw), B, H, W_, _ptr(wp), _ptr(bias), _ptr(out),
                                rows_per_block, C.c_void_p(s)))
    return out


def stem_pool_u8(prec, x_u8, w_folded, bias, scale=None, shift=None, nhwc=False, rows_per_block=0, stream=None,
                 out=None):
    """stem_pool on 8-bit pixels: x_u8 uint8 [B][3][H][W], or [B][H][W][3] with nhwc; a pixel p of
    channel c enters as float32(p) * scale[c] + shift[c] (default 1, 0).  x_u8 may start at any byte
    address (a slice of a larger buffer), but must be contiguous.  out as stem_pool's."""
    if x_u8.dtype != torch.uint8 or not x_u8.is_contiguous():
        raise OpError("stem_pool_u8: a contiguous uint8 tensor")
    if nhwc:
        B, H, W_, _ = x_u8.shape
    else:
        B, _, H, W_ = x_u8.shape
    oh, ow = (H - 1) // 2 + 1, (W_ - 1) // 2 + 1
    ph, pw = (oh - 1) // 2 + 1, (ow - 1) // 2 + 1
    w = np.ascontiguousarray(np.asarray(w_folded.cpu() if isinstance(w_folded, torch.Tensor) else w_folded,
                                        dtype=np.float32))
    host = np.empty(lib.spi_op_stem_pool_bytes(), dtype=np.uint8)
    _check(lib.spi_op_stem_pool_pack(w.ctypes.data, host.ctypes.data))
    wp = torch.from_numpy(host).to(x_u8.device)
    if out is None:
        out = torch.empty(B, ph, pw, 64, device=x_u8.device, dtype=torch.float32 if prec == "fp16x3s" else torch.float16)
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    _check(lib.spi_op_stem_pool_u8(STEM_PREC[prec], _ptr(x_u8), int(nhwc), B, H, W_, _ptr(wp), _ptr(bias),
                                   N.float3(scale), N.float3(shift), _ptr(out), rows_per_block, C.c_void_p(s)))
    return out


SRC_KIND = {"fp32": 0, "u8_nchw": 1, "u8_nhwc": 2}


def patchify(src_kind, x, ps, scale=None, shift=None, out_f16=False, stream=None):
    """ViT patchify of a 3-channel image: fp32 [B][3][H][W] ("fp32"), uint8 [B][3][H][W] ("u8_nchw") or
    uint8 [B][H][W][3] ("u8_nhwc", both under the scale / shift transform) -> [B (H/ps) (W/ps)][3 ps ps]
    fp32 or fp16, column c ps ps + kh ps + kw."""
    if not x.is_contiguous() or x.dtype != (torch.float32 if src_kind == "fp32" else torch.uint8):
        raise OpError("patchify: a contiguous tensor of the source kind's element type")
    if src_kind == "u8_nhwc":
        B, H, W_, _ = x.shape
    else:
        B, _, H, W_ = x.shape
    out = torch.empty(B * (H // ps) * (W_ // ps), 3 * ps * ps, device=x.device,
                      dtype=torch.float16 if out_f16 else torch.float32)
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    _check(lib.spi_op_patchify(SRC_KIND[src_kind], _ptr(x), B, H, W_, ps, N.float3(scale), N.float3(shift),
                               _ptr(out), int(out_f16), C.c_void_p(s)))
    return out


def resize_crop_u8(x_u8, resize_short, crop, scale=None, shift=None, nhwc=False, out=None, stream=None):
    """Resize + centre crop of 8-bit pixels on the device (spi_op_resize_crop_u8): x_u8 uint8 [B][3][H][W], or
    [B][H][W][3] with nhwc, contiguous, at any byte address -> float32 [B][3][crop][crop]: the antialiased
    bilinear resample to short side resize_short, centre crop, then float32(v) * scale[c] + shift[c]."""
    if x_u8.dtype != torch.uint8 or not x_u8.is_contiguous() or x_u8.dim() != 4 or x_u8.shape[3 if nhwc else 1] != 3:
        raise OpError("resize_crop_u8: a contiguous uint8 tensor, [B][3][H][W] or with nhwc [B][H][W][3]")
    B, H, W_ = (x_u8.shape[0], x_u8.shape[1], x_u8.shape[2]) if nhwc else (x_u8.shape[0], x_u8.shape[2], x_u8.shape[3])
    if out is None:
        out = torch.empty(B, 3, crop, crop, device=x_u8.device, dtype=torch.float32)
    _check(lib.spi_op_resize_crop_u8(_ptr(x_u8), int(nhwc), B, H, W_, resize_short, crop, N.float3(scale),
                                     N.float3(shift), _ptr(out), _stream(stream)))
    return out


def resize_crop_u8_host(x_u8: np.ndarray, resize_short, crop, scale=None, shift=None, nhwc=False) -> np.ndarray:
    """resize_crop_u8's arithmetic on the CPU (spi_op_resize_crop_u8_host; the header the kernel shares):
    a uint8 numpy array in, float32 [B][3][crop][crop] out.  Needs no device."""
    x = np.ascontiguousarray(x_u8)
    if x.dtype != np.uint8 or x.ndim != 4 or x.shape[3 if nhwc else 1] != 3:
        raise OpError("resize_crop_u8_host: a uint8 array, [B][3][H][W] or with nhwc [B][H][W][3]")
    B, H, W_ = (x.shape[0], x.shape[1], x.shape[2]) if nhwc else (x.shape[0], x.shape[2], x.shape[3])
    out = np.empty((B, 3, crop, crop), np.float32)
    _check(lib.spi_op_resize_crop_u8_host(x.ctypes.data, int(nhwc), B, H, W_, resize_short, crop, N.float3(scale),
                                          N.float3(shift), out.ctypes.data, None))
    return out


# ---- LayerNorm folded across GEMMs (spi_ops.h: spi_op_fold_linear / spi_op_gemm_ln / ..._planes) ----

KIND = {None: 0, "none": 0, "fp16": 1, "fp32": 2, "planes": 3}  # SPI_KIND_*


def to_planes(x: torch.Tensor, plane: int | None = None) -> torch.Tensor:
    """fp32 tensor -> its two-plane form in one flat fp16 buffer of 2 * plane elements:
    hi = fp16(x) from element 0, lo = fp16(x - hi) from element `plane` (default x.numel());
    elements past x.numel() in either plane are zero."""
    x = x.float().contiguous()
    n = x.numel()
    plane = n if plane is None else plane
    if plane < n:
        raise ValueError("plane shorter than the tensor")
    hi = x.half()
    buf = torch.zeros(2 * plane, dtype=torch.float16, device=x.device)
    buf[:n] = hi.reshape(-1)
    buf[plane:plane + n] = (x - hi.float()).half().reshape(-1)
    return buf


def from_planes(buf: torch.Tensor, plane: int, shape=None) -> torch.Tensor:
    """Inverse of to_planes: hi + lo in fp32, the first prod(shape) elements (default: the whole plane)."""
    n = plane if shape is None else int(np.prod(shape))
    flat = buf.reshape(-1)
    x = flat[:n].float() + flat[plane:plane + n].float()
    return x if shape is None else x.reshape(*shape)


def chunk_stats(x64: np.ndarray) -> np.ndarray:
    """float64 rows [rows][D] (D % 64 == 0) -> [rows][D / 64][2] of each 64-column chunk's
    (mean, M2 = sum of squared deviations from that mean), float64."""
    x64 = np.asarray(x64, dtype=np.float64)
    rows, D = x64.shape
    c = x64.reshape(rows, D // 64, 64)
    mean = c.mean(-1)
    return np.stack([mean, ((c - mean[..., None]) ** 2).sum(-1)], axis=-1)


def combine_stats(stats: np.ndarray, eps: float):
    """Chan's formula over [rows][chunks][2] chunk statistics, in float64 -> (row mean, row rstd)."""
    s = np.asarray(stats, dtype=np.float64)
    chunks = s.shape[1]
    mean = s[..., 0].mean(-1)
    m2 = (s[..., 1] + 64.0 * (s[..., 0] - mean[:, None]) ** 2).sum(-1)
    return mean, 1.0 / np.sqrt(m2 / (64.0 * chunks) + eps)


def fold_linear(prec, w, b, gamma, beta, hilo=False):
    """Host arithmetic of the fold for y = LN(x) W^T + b: (W diag(gamma), b + W beta, c1) as fp32 numpy."""
    f32 = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.float32))  # noqa: E731
    w, b, gamma, beta = f32(w), f32(b), f32(gamma), f32(beta)
    n, k = w.shape
    wf, bias, c1 = np.empty((n, k), np.float32), np.empty(n, np.float32), np.empty(n, np.float32)
    _check(lib.spi_op_fold_linear(PREC[prec], w.ctypes.data, None if b is None else b.ctypes.data, n, k,
                                  gamma.ctypes.data, beta.ctypes.data, int(hilo), wf.ctypes.data, bias.ctypes.data,
                                  c1.ctypes.data))
    return wf, bias, c1


def gemm_ln(A, W_packed, N_, out, out_kind, M=None, K=None, lda=None, bias=None, in_stats=None, c1=None,
            residual=None, res_kind=None, ldr=None, res_stats=None, res_g=None, res_b=None, eps=1e-5, ldc=None,
            plane=0, out_stats=None, c16=None, ld16=None, act=None, ws=None, stream=None, hilo=False):
    """spi_op_gemm_ln on caller-owned buffers (tensors used as plain HBM; strides default to N / K).
    c1 may be a tensor or a raw device address (int).  hilo: W_packed holds hi + lo weights
    (pack_weight_hilo of fold_linear(hilo=True)'s), spi_op_gemm_ln_hilo."""
    M = A.shape[0] if M is None else M
    K = A.shape[1] if K is None else K
    ws = workspace(A.device) if ws is None else ws
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    c1p = C.c_void_p(c1) if isinstance(c1, int) else _ptr(c1)
    fn = lib.spi_op_gemm_ln_hilo if hilo else lib.spi_op_gemm_ln
    _check(fn(_ptr(A), M, K, K if lda is None else lda, _ptr(W_packed), N_, _ptr(bias),
                              _ptr(in_stats), c1p, _ptr(residual), KIND[res_kind], N_ if ldr is None else ldr,
                              _ptr(res_stats), _ptr(res_g), _ptr(res_b), eps, _ptr(out), KIND[out_kind],
                              N_ if ldc is None else ldc, plane, _ptr(out_stats), _ptr(c16),
                              N_ if ld16 is None else ld16, ACT[act], _ptr(ws), C.c_void_p(s)))
    return out


def layernorm_planes(prec, xh, plane, ldx, gamma, beta, rows, D, eps, yf=None, yt=None, ldy=None, stream=None):
    """Row LayerNorm of rows held in two fp16 planes; yt is fp16 for prec fp16, else fp32."""
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    _check(lib.spi_op_layernorm_planes(PREC[prec], _ptr(xh), plane, ldx, _ptr(gamma), _ptr(beta), _ptr(yf), _ptr(yt),
                                       D if ldy is None else ldy, rows, D, eps, C.c_void_p(s)))
    return yf, yt


def vit_assemble_planes(patches, cls, pos, xh, plane, stats, B, P, D, stream=None):
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    _check(lib.spi_op_vit_assemble_planes(_ptr(patches), _ptr(cls), _ptr(pos), _ptr(xh), plane, _ptr(stats), B, P, D,
                                          C.c_void_p(s)))
    return xh


# ---- fused QKV projection + attention, and the HBM-bound kernels (spi_ops.h) ----
# All on caller-owned buffers, so a test can put guard rows behind every output.


def _stream(stream):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream if stream is None else stream)


def qkv_attention(A, W_packed, heads, bias, ctx, B, S, lda=None, in_stats=None, c1=None, eps=1e-5, mask_bias=None,
                  scale=0.125, stream=None):
    """Fused QKV GEMM + attention: A fp16 [B S][lda] (default lda: A's row stride), W_packed from
    pack_weight("fp16", [3 D][D]), bias fp32 [3 D]; with in_stats / c1 the LayerNorm fold's consumer.
    Writes ctx fp16 [B S][64 heads]."""
    _check(lib.spi_op_qkv_attention(_ptr(A), A.stride(0) if lda is None else lda, _ptr(W_packed), heads, _ptr(bias),
                                    _ptr(in_stats), _ptr(c1), eps, _ptr(mask_bias), _ptr(ctx), B, S, scale,
                                    _stream(stream)))
    return ctx


def ingest(src_kind, x, B, Cc, H, W_, cpad, out, scale=None, shift=None, stream=None):
    """Image ("fp32" [B][C][H][W], "u8_nchw", "u8_nhwc") -> out NHWC [B][H][W][cpad], fp16 or fp32 by out.dtype."""
    _check(lib.spi_op_ingest(SRC_KIND[src_kind], _ptr(x), B, Cc, H, W_, cpad, N.float3(scale), N.float3(shift),
                             _ptr(out), int(out.dtype == torch.float16), _stream(stream)))
    return out


def pool_out(H, W_, k, stride, pad):
    return (H + 2 * pad - k) // stride + 1, (W_ + 2 * pad - k) // stride + 1


def maxpool(prec, x, B, H, W_, Cc, k, stride, pad, out, stream=None):
    """NHWC max pool; prec "fp32", "fp16" or "fp16x3s" (split in, split out)."""
    _check(lib.spi_op_maxpool(PREC[prec], _ptr(x), B, H, W_, Cc, k, stride, pad, _ptr(out), _stream(stream)))
    return out


def avgpool(prec, x, B, HW, Cc, out, stream=None):
    """Global average pool [B][HW][C] -> out [B][C]; fp16 input writes fp32 when out is a float32 tensor."""
    _check(lib.spi_op_avgpool(PREC[prec], _ptr(x), B, HW, Cc, _ptr(out),
                              int(prec == "fp16" and out.dtype == torch.float32), _stream(stream)))
    return out


def bert_embed(prec, ids, word, pos, type0, gamma, beta, yf, yt, B, S, D, eps, mask=None, mask_bias=None,
               vocab=None, npos=None, stream=None):
    _check(lib.spi_op_bert_embed(PREC[prec], _ptr(ids), _ptr(word), _ptr(pos), _ptr(type0), _ptr(gamma), _ptr(beta),
                                 _ptr(yf), _ptr(yt), B, S, D, word.shape[0] if vocab is None else vocab,
                                 pos.shape[0] if npos is None else npos, eps, _ptr(mask), _ptr(mask_bias),
                                 _stream(stream)))
    return yf, yt


def bert_embed_types(prec, ids, word, pos, type_table, type_ids, gamma, beta, yf, yt, B, S, D, eps, mask=None,
                     mask_bias=None, stream=None):
    """bert_embed with segment ids: type_table fp32 [type_vocab][D], type_ids int64 [B S] or None (row 0)."""
    _check(lib.spi_op_bert_embed_types(PREC[prec], _ptr(ids), _ptr(word), _ptr(pos), _ptr(type_table),
                                       type_table.shape[0], _ptr(type_ids), _ptr(gamma), _ptr(beta), _ptr(yf), _ptr(yt),
                                       B, S, D, word.shape[0], pos.shape[0], eps, _ptr(mask), _ptr(mask_bias),
                                       _stream(stream)))
    return yf, yt


def bert_embed_posids(prec, ids, word, pos, type_table, type_ids, gamma, beta, yf, yt, B, S, D, eps, mask=None,
                      mask_bias=None, stream=None):
    """bert_embed_types with RoBERTa's position rule: row (b, s) reads pos[1 + #non-pad ids up to s], or pos[1]
    at a pad id (1), so pos needs S + 2 rows."""
    _check(lib.spi_op_bert_embed_posids(PREC[prec], _ptr(ids), _ptr(word), _ptr(pos), _ptr(type_table),
                                        type_table.shape[0], _ptr(type_ids), _ptr(gamma), _ptr(beta), _ptr(yf),
                                        _ptr(yt), B, S, D, word.shape[0], pos.shape[0], eps, _ptr(mask),
                                        _ptr(mask_bias), _stream(stream)))
    return yf, yt


def bert_pooler(h, ld, W, bias, out, B, D, stream=None):
    """out fp32 [B][D] = tanh(bias + h_rows W^T): row b of h starts ld floats after row b - 1 (fp32 throughout)."""
    _check(lib.spi_op_bert_pooler(_ptr(h), ld, _ptr(W), _ptr(bias), _ptr(out), B, D, _stream(stream)))
    return out


HEAD_SRC = {"rows": 0, "pre_ln": 1, "planes": 2}


def bert_token_head(src, x, W, bias, y0, T, D, L, y1=None, plane=0, gamma=None, beta=None, eps=0.0, stream=None):
    """Token-level head: y0 fp32 [T][L] = bias + h W^T, or with y1 (L == 2) label 0 into y0 [T] and label 1 into
    y1 [T].  src "rows": x fp32 [T][D], normalised; "pre_ln": x fp32 pre-LayerNorm rows, normalised in the kernel
    with gamma / beta / eps; "planes": the same rows as fp16 hi at x and lo `plane` elements after it."""
    _check(lib.spi_op_bert_token_head(HEAD_SRC[src], _ptr(x), plane, _ptr(gamma), _ptr(beta), eps, _ptr(W), _ptr(bias),
                                      _ptr(y0), _ptr(y1), T, D, L, _stream(stream)))
    return y0, y1


def bert_dense_rows(h, ld, W, bias, out, B, D, N, activation=None, stream=None):
    """out fp32 [B][N] = act(bias + h_rows W^T), W fp32 [N][D]; activation None or "tanh" (N = D: bert_pooler)."""
    act = {None: 0, "none": 0, "tanh": 1}[activation]
    _check(lib.spi_op_bert_dense_rows(_ptr(h), ld, _ptr(W), _ptr(bias), _ptr(out), B, D, N, act, _stream(stream)))
    return out


def masked_mean(h, mask, out, B, S, D, stream=None):
    """out fp32 [B][D] = masked mean over S of h fp32 [B][S][D]; mask int64 [B][S] or None (every token)."""
    _check(lib.spi_op_masked_mean(_ptr(h), _ptr(mask), _ptr(out), B, S, D, _stream(stream)))
    return out


def softmax_topk(x, ldx, probs, topv, topi, B, N, k=0, topk_probs=False, stream=None):
    """Softmax and / or top-k of B fp32 logits rows of N, ldx floats apart: probs fp32 [B][N] or None; topv fp32
    [B][k] and topi int64 [B][k], both or neither (then k = 0); topk_probs: topv holds probabilities."""
    _check(lib.spi_op_softmax_topk(_ptr(x), ldx, _ptr(probs), _ptr(topv), _ptr(topi), B, N, k, int(bool(topk_probs)),
                                   _stream(stream)))
    return probs, topv, topi


def mask_to_bias(mask, bias, n, stream=None):
    _check(lib.spi_op_mask_to_bias(_ptr(mask), _ptr(bias), n, _stream(stream)))
    return bias


def vit_assemble(patches, cls, pos, x, B, P, D, stream=None):
    _check(lib.spi_op_vit_assemble(_ptr(patches), _ptr(cls), _ptr(pos), _ptr(x), B, P, D, _stream(stream)))
    return x


def gather_rows(x, out, rows, stride_rows, D, stream=None):
    _check(lib.spi_op_gather_rows(_ptr(x), _ptr(out), rows, stride_rows, D, int(out.dtype == torch.float16),
                                  _stream(stream)))
    return out

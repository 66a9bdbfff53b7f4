#!/usr/bin/env python3
"""Fused stem (stem_pool) launch time: 200 back-to-back launches between two events,
per precision and rows-per-workgroup, ResNet bs8 @ 224.

--input picks what the kernel reads: the fp32 NCHW image (default), or 8-bit pixels NCHW / NHWC
under the ImageNet transform (spi_op_stem_pool_u8).  --repeats prints that many timings per
configuration (medians and spreads come from repeats, interleaved across builds by the caller)."""
import argparse
import ctypes as C
import importlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ops = importlib.import_module("starpu-inference-server_amd.ops")
lib = ops.lib

ap = argparse.ArgumentParser()
ap.add_argument("--input", choices=["fp32", "u8_nchw", "u8_nhwc"], default=os.environ.get("STEM_INPUT", "fp32"))
ap.add_argument("--repeats", type=int, default=1)
args = ap.parse_args()

B = int(os.environ.get("B", "8"))
if args.input == "fp32":
    x = torch.rand(B, 3, 224, 224, device="cuda")
else:
    shape = (B, 3, 224, 224) if args.input == "u8_nchw" else (B, 224, 224, 3)
    x = torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda")
mean, std = np.float32([0.485, 0.456, 0.406]), np.float32([0.229, 0.224, 0.225])
scale = (C.c_float * 3)(*(np.float32(1) / (np.float32(255) * std)))
shift = (C.c_float * 3)(*(-mean / std))
w = torch.randn(64, 3, 7, 7) * 0.1
b = torch.randn(64, device="cuda") * 0.1
host = np.empty(lib.spi_op_stem_pool_bytes(), dtype=np.uint8)
lib.spi_op_stem_pool_pack(np.ascontiguousarray(w.numpy()).ctypes.data, host.ctypes.data)
wp = torch.from_numpy(host).cuda()
y = torch.empty(B, 56, 56, 64 * 2, device="cuda", dtype=torch.float16)
s = torch.cuda.current_stream().cuda_stream
flops = 2.0 * B * 112 * 112 * 64 * 147
only = os.environ.get("STEM_ONLY")  # e.g. "fp16m:1"
for prec, name in [(1, "fp16"), (2, "fp16m"), (3, "fp16x3s")]:
    for rows in (0, 1, 2):
        if only and only != f"{name}:{rows}":
            continue
        if args.input == "fp32":
            call = lambda: lib.spi_op_stem_pool(prec, ops._ptr(x), B, 224, 224, ops._ptr(wp), ops._ptr(b),
                                                ops._ptr(y), rows, C.c_void_p(s))
        else:
            call = lambda: lib.spi_op_stem_pool_u8(prec, ops._ptr(x), int(args.input == "u8_nhwc"), B, 224, 224,
                                                   ops._ptr(wp), ops._ptr(b), scale, shift, ops._ptr(y), rows,
                                                   C.c_void_p(s))
        if call() != 0:
            raise SystemExit(f"stem_pool failed: {ops.N.last_error()}")
        for _ in range(args.repeats):
            for _ in range(10):
                call()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(200):
                call()
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) / 200 * 1e3
            print(f"stem_pool {args.input:8s} {name:8s} rows/wg {rows}: {us:7.2f} us  {flops / us / 1e6:7.1f} TF/s "
                  "(algorithmic)", flush=True)

#!/usr/bin/env python3
"""Resize + centre crop of 8-bit images (spi_op_resize_crop_u8): launch time on the device and what it
replaces on the host.

Device: --launches back-to-back launches between two events, --repeats times, per layout; beside the time,
the bytes the algorithm needs -- the source bytes inside the crop's footprint (the rows and columns its taps
touch) plus the fp32 bytes written -- over that time.  --cpu-seconds > 0 also runs the same resize with ATen
(antialiased bilinear on the uint8 tensor, what torchvision's Resize does, then the crop) on --cpu-threads
threads and prints images/s.  Default shape: bs8, 500 x 375 NHWC -> 256 -> 224."""
import argparse
import ctypes as C
import importlib
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
spi = importlib.import_module("starpu-inference-server_amd")
ops = importlib.import_module("starpu-inference-server_amd.ops")

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--height", type=int, default=500)
ap.add_argument("--width", type=int, default=375)
ap.add_argument("--resize", type=int, default=256)
ap.add_argument("--crop", type=int, default=224)
ap.add_argument("--layouts", default="nhwc,nchw")
ap.add_argument("--launches", type=int, default=200)
ap.add_argument("--repeats", type=int, default=6)
ap.add_argument("--cpu-seconds", type=float, default=0.0)
ap.add_argument("--cpu-threads", type=int, default=16)
args = ap.parse_args()

B, H, W, R, S = args.batch, args.height, args.width, args.resize, args.crop
RH, RW, top, left = spi.resize_geometry(H, W, R, S)


def footprint(n_in, n_out, first, count):
    """Source indices the taps of output indices first .. first + count - 1 touch (include/spi_codelet.h)."""
    m = max(n_in, n_out)
    lo = max(0, (n_in * (2 * first + 1) - 2 * m + n_out) // (2 * n_out))
    hi = min(n_in, (n_in * (2 * (first + count - 1) + 1) + 2 * m + n_out) // (2 * n_out))
    return hi - lo


rows, cols = footprint(H, RH, top, S), footprint(W, RW, left, S)
need = B * 3 * (rows * cols + S * S * 4)
print(f"bs{B} {H}x{W} -> {RH}x{RW} -> {S}x{S}: footprint {rows} rows x {cols} columns, {need / 1e6:.2f} MB read + written")

if args.launches > 0:
    if spi.lib.spi_device_count() < 1:
        raise SystemExit("no HIP device")
    mean, std = np.float32([0.485, 0.456, 0.406]), np.float32([0.229, 0.224, 0.225])
    scale, shift = np.float32(1) / (np.float32(255) * std), -mean / std
    out = torch.empty(B, 3, S, S, device="cuda")
    xs = {lay: torch.randint(0, 256, (B, H, W, 3) if lay == "nhwc" else (B, 3, H, W), dtype=torch.uint8, device="cuda")
          for lay in args.layouts.split(",")}
    sc, sh = ops.N.float3(scale), ops.N.float3(shift)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for rep in range(args.repeats):  # layouts interleaved across repeats
        for lay, x in xs.items():
            # the C entry point with prebuilt arguments: the Python wrapper costs more host time per call than
            # the kernel runs, and the events would then time the enqueue
            call = lambda: ops.lib.spi_op_resize_crop_u8(ops._ptr(x), int(lay == "nhwc"), B, H, W, R, S, sc, sh,
                                                         ops._ptr(out), stream)
            if call() != 0:
                raise SystemExit(f"resize_crop_u8 failed: {ops.N.last_error()}")
            for _ in range(10):
                call()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            for _ in range(args.launches):
                call()
            e1.record()
            host_us = (time.perf_counter() - t0) / args.launches * 1e6
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) / args.launches * 1e3
            print(f"resize_crop_u8 {lay} repeat {rep}: {us:7.2f} us per launch between events ({host_us:.2f} us of host "
                  f"enqueue each; the larger bounds the figure)  {need / us / 1e6:6.3f} TB/s (algorithmic bytes)", flush=True)

if args.cpu_seconds > 0:
    torch.set_num_threads(args.cpu_threads)
    x = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8).permute(0, 3, 1, 2)  # decoded NHWC pixels, NCHW view

    def resize(t):
        y = torch.nn.functional.interpolate(t, size=(RH, RW), mode="bilinear", antialias=True, align_corners=False)
        return y[:, :, top:top + S, left:left + S].contiguous()

    resize(x)
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < args.cpu_seconds:
        resize(x)
        n += B
    dt = time.perf_counter() - t0
    print(f"ATen uint8 antialiased bilinear + crop, {args.cpu_threads} threads, batches of {B}: {n / dt:8.1f} images/s "
          f"({dt / n * 1e6:.0f} us per image)")

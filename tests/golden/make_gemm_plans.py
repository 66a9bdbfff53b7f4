#!/usr/bin/env python3
"""Record the GEMM planner's decisions as data (run from the repo root, CPU only).

gemm_plans.json -- what spi_debug_conv_plan, spi_debug_gemm_plan and spi_debug_conv_pair_plan
                   return for the serving shapes and the GPU suite's shapes under every knob setting
                   the GPU suite uses.  tests/test_gemm_plan.py holds the planner to it, so a
                   refactor of the plan rule can be checked without a GPU.  Regenerate it only
                   together with a deliberate change of the rule.

Layout: {"commit": ..., "settings": [env dicts], "default": {case: ints},
         "overrides": {setting index: {case: ints}}} -- a setting lists only the cases whose answer
differs from the default's.  A case string is the export's argument list:
  c:precision,B,H,Cin,Cout,k,stride,pad           -> the 8 plan fields
  d:precision,M,N,K,lda,krep,pool_rows,flags      -> 14 fields (spi_debug_gemm_plan)
  p:precision,B,H,Cin,Cout0,k0,s0,p0,Cout1,k1,s1,p1 -> 22 fields (spi_debug_conv_pair_plan)
"""
import ctypes as C
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
HERE = os.path.dirname(os.path.abspath(__file__))

KNOBS = ("SPI_GEMM_HALO_CFG", "SPI_GEMM_WIN", "SPI_GEMM_MAXSPLIT", "SPI_GEMM_256_MIN", "SPI_GEMM_256_LONGK",
         "SPI_GEMM_256_ORDER", "SPI_GEMM_PLAN")
SETTINGS = [{}] + [{k: v} for k, vs in (
    ("SPI_GEMM_HALO_CFG", ["0", "64,a", "64,s", "128,a", "128,s", "256,a", "256,s", "56:128,a;28:64,s;0:0,a"]),
    ("SPI_GEMM_WIN", ["0", "2", "3"]),
    ("SPI_GEMM_MAXSPLIT", ["0", "1", "2", "3"]),
    ("SPI_GEMM_256_MIN", ["1", "0,1,3", "0,1,2"]),
    ("SPI_GEMM_256_LONGK", ["0", "48,1024,4"]),
    ("SPI_GEMM_256_ORDER", ["0", "1"]),
    ("SPI_GEMM_PLAN", ["64,64,4,2", "128,64,3,1", "128,128,2,1"]),
) for v in vs]

# flag word of spi_debug_gemm_plan
ACT, RES_F32, RES_PLANES, OUT_PLANES, OUT_F16, OUT_F32 = 1, 2, 4, 8, 16, 32


def conv_cases():
    shapes = []  # (B, H, Cin, Cout, k, stride, pad)
    for B in (1, 8, 32):
        for H, cin, cout in ((56, 64, 64), (28, 128, 128), (14, 256, 256), (7, 512, 512)):
            shapes.append((B, H, cin, cout, 3, 1, 1))
        for H, cin, cout in ((56, 64, 128), (28, 128, 256), (14, 256, 512)):
            shapes.append((B, H, cin, cout, 3, 2, 1))
            shapes.append((B, H, cin, cout, 1, 2, 0))
        for H, cin, cout in ((56, 64, 64), (56, 64, 256), (56, 256, 64), (28, 512, 128), (14, 1024, 256),
                             (7, 2048, 512)):
            shapes.append((B, H, cin, cout, 1, 1, 0))
        for cin in (4, 8):
            shapes.append((B, 224, cin, 64, 7, 2, 3))
    # tests/test_ops_gpu.py: test_conv3x3_window_kind, test_conv_halo_candidates_split_layout / _fp16
    for B, H, cin, cout in ((8, 28, 128, 128), (8, 14, 256, 256), (8, 7, 512, 512), (3, 5, 64, 64), (2, 13, 128, 64),
                            (1, 3, 64, 128), (5, 9, 64, 64), (32, 7, 512, 512), (1, 28, 128, 128), (32, 14, 256, 256),
                            (16, 28, 128, 128), (3, 7, 64, 64), (2, 14, 128, 128), (3, 28, 64, 128), (1, 56, 64, 64),
                            (5, 9, 32, 64), (4, 13, 64, 64), (2, 14, 256, 256)):
        shapes.append((B, H, cin, cout, 3, 1, 1))
    out = []
    for s in dict.fromkeys(shapes):
        B, H, cin, cout, k, stride, pad = s
        for prec in (0, 1, 2, 3):
            if prec == 1 and cin < 8:
                continue
            if prec == 3 and (cin < 32 or cout % 32 or k * k > 31):
                continue
            out.append("c:" + ",".join(map(str, (prec,) + s)))
    return out


def dense_cases():
    shapes = [(1024, 768, 768), (1024, 2304, 768), (1024, 3072, 768), (1024, 768, 3072),  # BERT-base bs8
              (3152, 1024, 1024), (3152, 3072, 1024), (3152, 4096, 1024), (3152, 1024, 4096),  # ViT-L bs16
              (16, 1000, 1024), (8, 1000, 512), (1, 1000, 2048),  # heads, FC
              # test_gemm256_tiles, test_gemm256_split_k
              (1, 256, 64), (100, 256, 64), (300, 512, 128), (256, 768, 192), (1000, 1024, 640), (129, 256, 320),
              (600, 512, 4096), (3152, 1024, 2048), (257, 256, 3072)]
    out = []

    def add(prec, M, N, K, lda, krep, pool, flags):
        out.append("d:" + ",".join(map(str, (prec, M, N, K, lda, krep, pool, flags))))

    for M, N, K in dict.fromkeys(shapes):
        for prec in (0, 1, 2, 3):
            if prec == 3 and (K % 32 or N % 32):
                continue
            add(prec, M, N, K, K, 1, 0, 0)
        add(1, M, N, K, K, 1, 0, RES_F32 | OUT_F32)
        add(1, M, N, K, K, 1, 0, RES_F32 | OUT_F32 | ACT)  # gemm256 must refuse
        add(1, M, N, K, K, 1, 0, RES_PLANES | OUT_PLANES)
        if N % 128 == 0:
            add(1, M, N, K, K, 1, 0, RES_F32 | OUT_F32 | (N // 64) << 16)  # res_ln_chunks: gemm256 must refuse
        if K // 64 in (12, 16):
            add(1, M, N, K, K, 1, 0, (K // 64) << 8)  # the LayerNorm consumer fold (D = 768, 1024)
        add(1, M, N, K, K, 2, 0, 0)
        add(1, M, N, K, K + 4, 1, 0, 0)
    for B in (1, 8, 32):  # pooled FC (ResNet-18 / 152)
        for K in (512, 2048):
            for prec in (0, 1, 2, 3):
                add(prec, B * 49, 1000, K, K, 1, 49, OUT_F32)
    return out


def pair_cases():
    pairs = []  # (B, H, Cin, Cout0, k0, s0, p0, Cout1, k1, s1, p1)
    for B in (1, 8):  # ResNet-18: c1 3x3/s2 + ds 1x1/s2
        for H, cin in ((56, 64), (28, 128), (14, 256)):
            pairs.append((B, H, cin, 2 * cin, 3, 2, 1, 2 * cin, 1, 2, 0))
    for B in (1, 32):  # ResNet-152: c1 1x1 + ds 1x1
        pairs.append((B, 56, 64, 64, 1, 1, 0, 256, 1, 1, 0))
        for H, cin in ((56, 256), (28, 512), (14, 1024)):
            pairs.append((B, H, cin, cin // 2, 1, 1, 0, 2 * cin, 1, 2, 0))
    pairs.append((8, 28, 128, 128, 3, 1, 1, 256, 1, 1, 0))  # window / halo plan + tap walk: two launches
    out = []
    for s in pairs:
        for prec in (0, 1, 2, 3):
            out.append("p:" + ",".join(map(str, (prec,) + s)))
    return out


def query(lib, case):
    """The ints an export returns for a case string."""
    kind, args = case.split(":")
    args = [int(a) for a in args.split(",")]
    if kind == "c":
        prec, B, H, cin, cout, k, stride, pad = args
        out = (C.c_int * 8)()
        rc = lib.spi_debug_conv_plan(prec, B, H, H, cin, cout, k, k, stride, pad, out)
    elif kind == "d":
        out = (C.c_longlong * 14)()
        rc = lib.spi_debug_gemm_plan(*args[:7], C.c_uint(args[7]), out)
    else:
        prec, B, H, cin, c0, k0, s0, p0, c1, k1, s1, p1 = args
        out = (C.c_longlong * 22)()
        rc = lib.spi_debug_conv_pair_plan(prec, B, H, H, cin, c0, k0, k0, s0, p0, c1, k1, k1, s1, p1, out)
    assert rc == 0, case
    return list(out)


def apply_setting(lib, env):
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)
    lib.spi_debug_gemm_reload_env()


def main():
    lib = importlib.import_module("starpu-inference-server_amd").lib
    cases = conv_cases() + dense_cases() + pair_cases()
    table = {"commit": subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT, text=True).strip(),
             "settings": SETTINGS, "default": {}, "overrides": {}}
    try:
        for i, env in enumerate(SETTINGS):
            apply_setting(lib, env)
            got = {c: query(lib, c) for c in cases}
            if i == 0:
                table["default"] = got
            else:
                table["overrides"][str(i)] = {c: v for c, v in got.items() if v != table["default"][c]}
    finally:
        apply_setting(lib, {})
    with open(os.path.join(HERE, "gemm_plans.json"), "w") as f:
        json.dump(table, f, separators=(",", ":"))
        f.write("\n")
    print(len(cases), "cases x", len(SETTINGS), "settings;",
          sum(len(v) for v in table["overrides"].values()), "override rows")


if __name__ == "__main__":
    main()

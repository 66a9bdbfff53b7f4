#!/usr/bin/env python3
"""Record the general GEMM kernel's launch arguments as data (run from the repo root, CPU only).

gemm_args.json -- per case of gemm_plans.json (tests/golden/make_gemm_plans.py) and per edge case
                  below, under the default knob setting: what spi_debug_conv_args,
                  spi_debug_gemm_args and spi_debug_conv_pair_args (csrc/gemm_args.cpp) return.
                  tests/test_gemm_args.py holds make_args to it.  The file was recorded from the
                  commit it names, whose make_args still lived in gemm.hip: regenerate it only
                  together with a deliberate change of the kernel arguments.

Layout: {"commit": ..., "cases": {case: [digest, digest with C off 16 bytes, info ints]}}.  A digest
is 16 hex digits over every field of the kernel arguments; the info ints are tiles_m, tiles_n,
splits, xg_m, xg_n -- for a pair (p:) both problems', then grouped, problem 0's workgroups, all
workgroups.  Case strings as make_gemm_plans.py.
"""
import ctypes as C
import importlib
import importlib.util
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
HERE = os.path.dirname(os.path.abspath(__file__))

_spec = importlib.util.spec_from_file_location("make_gemm_plans", os.path.join(HERE, "make_gemm_plans.py"))
plans = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(plans)


def edge_cases():
    """Small problems at the edges of the tile decode; each row names what the default plan gives
    (tests/test_gemm_args.py asserts it, so a plan change that loses an edge shows)."""
    return list(EDGES)


# case -> (tiles_m, tiles_n, splits, xg_m, xg_n) it is here for
EDGES = {
    "d:0,1,192,64,64,1,0,0": (1, 3, 1, 1, 3),  # fewer than 16 tiles: no XCD reorder
    "d:0,64,1000,64,64,1,0,0": (1, 16, 1, 1, 8),  # exactly 16 tiles
    "d:0,200,448,64,64,1,0,0": (4, 7, 1, 2, 4),  # 28 tiles: no multiple of 8
    "d:0,520,320,768,768,1,0,0": (9, 5, 3, 1, 5),  # 3 slices
    "d:0,200,320,2048,2048,1,0,0": (4, 5, 7, 1, 5),  # 7 slices
    "d:0,1300,64,2048,2048,1,0,0": (21, 1, 7, 1, 1),  # 7 slices of one tile column
    "c:0,3,7,512,512,3,1,1": (3, 8, 6, 1, 8),  # a split conv
    "d:0,520,1000,64,64,1,0,0": (9, 16, 1, 2, 4),  # xg_m 2, 4, 8 not dividing 9 tile rows
    "d:0,520,320,64,64,1,0,0": (9, 5, 1, 4, 2),
    "d:0,520,128,64,64,1,0,0": (9, 2, 1, 8, 1),
    "d:0,1100,64,64,64,1,0,0": (18, 1, 1, 8, 1),
}


def cases():
    return plans.conv_cases() + plans.dense_cases() + plans.pair_cases() + edge_cases()


def query(lib, case, unaligned_c=0, with_map=False):
    """(digest as 16 hex digits, info ints, workgroup map or None) of a case string."""
    kind, args = case.split(":")
    args = [int(a) for a in args.split(",")]
    digest = C.c_ulonglong()
    info = (C.c_int * (13 if kind == "p" else 5))()

    def call(m, cap):
        if kind == "c":
            prec, B, H, cin, cout, k, stride, pad = args
            return lib.spi_debug_conv_args(prec, B, H, H, cin, cout, k, k, stride, pad, unaligned_c, C.byref(digest),
                                           info, m, cap)
        if kind == "d":
            return lib.spi_debug_gemm_args(*args[:7], C.c_uint(args[7]), unaligned_c, C.byref(digest), info, m, cap)
        prec, B, H, cin, c0, k0, s0, p0, c1, k1, s1, p1 = args
        return lib.spi_debug_conv_pair_args(prec, B, H, H, cin, c0, k0, k0, s0, p0, c1, k1, k1, s1, p1, unaligned_c,
                                            C.byref(digest), info, m, cap)

    assert call(None, 0) == 0, case
    wmap = None
    if with_map:
        width = 4 if kind == "p" else 3
        wgs = info[12] if kind == "p" else info[0] * info[1] * info[2]
        buf = (C.c_int * (width * wgs))()
        assert call(buf, wgs) == 0, case
        wmap = [tuple(buf[width * i:width * (i + 1)]) for i in range(wgs)]
    return "%016x" % digest.value, list(info), wmap


def main(lib=None):
    lib = lib or importlib.import_module("starpu-inference-server_amd").lib
    plans.apply_setting(lib, {})
    table = {"commit": subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT, text=True).strip(), "cases": {}}
    for c in cases():
        d0, info, _ = query(lib, c)
        d1, info1, _ = query(lib, c, unaligned_c=1)
        assert info == info1
        table["cases"][c] = [d0, d1] + info
    with open(os.path.join(HERE, "gemm_args.json"), "w") as f:
        json.dump(table, f, separators=(",", ":"))
        f.write("\n")
    print(len(table["cases"]), "cases")


if __name__ == "__main__":
    main()

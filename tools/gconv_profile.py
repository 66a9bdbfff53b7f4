#!/usr/bin/env python3
"""Device time of a ResNeXt's grouped conv2 shapes on the grouped kernel and on the dense expansion.

For each (model, batch): two fp16 replicas of the same module, one packed for the grouped kernel and one
under SPI_GCONV=0 (the dense block-diagonal expansion on the implicit-GEMM kernels).  Per distinct conv2
shape the op is timed with Model::profile_op (the op launched `reps` times back to back between two device
events, inside an otherwise normal forward), the two routes alternating, `rounds` times; the whole forward is
the sum of the op times of Model::profile, median of `rounds`.  All figures are device-time sums of eagerly
launched ops, not serving rates.  The byte bound is (x + y + the conv's own weights) / 8 TB/s.

    python tools/gconv_profile.py --out profiles/gconv/resnext.json
"""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 8e12


def replica(spi, module, batch, gconv):
    if gconv:
        os.environ.pop("SPI_GCONV", None)
    else:
        os.environ["SPI_GCONV"] = "0"
    try:
        return spi.ModelReplica(module, 0, "fp16", max_batch=batch)
    finally:
        os.environ.pop("SPI_GCONV", None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="resnext50_32x4d:8,resnext50_32x4d:32,resnext101_32x8d:8")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    spi = importlib.import_module("starpu-inference-server_amd")
    zoo = importlib.import_module("starpu-inference-server_amd.zoo")
    if spi.lib.spi_device_count() < 1:
        raise SystemExit("gconv_profile: no HIP device")
    stream = torch.cuda.Stream()
    results = []
    modules = {}
    for cfg in a.configs.split(","):
        name, batch = cfg.split(":")
        batch = int(batch)
        if name not in modules:
            modules[name] = zoo.build(name)
        m = modules[name]
        x = torch.rand(batch, 3, 224, 224, generator=torch.Generator().manual_seed(1)).cuda()
        out = torch.empty(batch, 1000, device="cuda")
        reps = {"gconv": replica(spi, m, batch, True), "dense": replica(spi, m, batch, False)}
        ops = {k: r.profile([x], out, stream.cuda_stream) for k, r in reps.items()}  # also the warm-up
        shapes = []
        for o in ops["gconv"]:
            if o["name"].startswith("gconv3x3_") and o["name"] not in [s["gconv"] for s in shapes]:
                _, c, g, s, mm = o["name"].split("_")
                C, G, S, M = int(c[1:]), int(g[1:]), int(s[1:]), int(mm[1:])
                dense = f"conv3x3_c{C}_k{C}_s{S}_M{M}"
                assert any(d["name"] == dense for d in ops["dense"]), dense
                byt = (M * S * S * C + M * C + C * (C // G) * 9) * 2  # x (even maps: M S^2 pixels), y, weights
                shapes.append(dict(gconv=o["name"], dense=dense, C=C, groups=G, stride=S, M=M, flops=o["flops"],
                                   bytes=byt, bound_us=byt / HBM_BYTES_PER_S * 1e6, gconv_us=[], dense_us=[]))
        whole = {"gconv": [], "dense": []}
        for _ in range(a.rounds):
            for sh in shapes:
                for k in ("gconv", "dense"):
                    r = reps[k].profile_op([x], out, stream.cuda_stream, sh[k], a.reps)
                    sh[k + "_us"].append(r["ms"] * 1e3)
            for k in ("gconv", "dense"):
                whole[k].append(sum(o["ms"] for o in reps[k].profile([x], out, stream.cuda_stream)) * 1e3)
        for sh in shapes:
            sh["gconv_med_us"] = statistics.median(sh["gconv_us"])
            sh["dense_med_us"] = statistics.median(sh["dense_us"])
            print(f"{name} bs{batch} C{sh['C']} s{sh['stride']} M{sh['M']}: grouped {sh['gconv_med_us']:.1f} us "
                  f"{sh['gconv_us']}, dense {sh['dense_med_us']:.1f} us {sh['dense_us']}, bound {sh['bound_us']:.2f} us",
                  flush=True)
        res = dict(model=name, batch=batch, precision="fp16", reps=a.reps, rounds=a.rounds, shapes=shapes,
                   forward_op_sum_us={k: dict(median=statistics.median(v), all=v) for k, v in whole.items()},
                   weight_bytes={k: r.weight_bytes for k, r in reps.items()})
        print(f"{name} bs{batch} forward, sum of op device times: grouped "
              f"{res['forward_op_sum_us']['gconv']['median']:.0f} us, dense "
              f"{res['forward_op_sum_us']['dense']['median']:.0f} us", flush=True)
        results.append(res)
        del reps
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()

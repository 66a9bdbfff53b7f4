#!/usr/bin/env python3
"""Device time of a BERT's attention block on its two routes: the fused QKV + attention kernel against the QKV
GEMM + standalone attention pair -- the measurement behind a routing decision.  A model
whose head width the fused kernel does not serve runs the pair under both settings: that is reported and the
model skipped.  (profiles/hd32/ holds the run that decided the route of 32-wide heads, taken while a 32-wide
form of the fused kernel was compiled in; profiles/hd32/README.md says what that form was.)

Two fp16 replicas of one module on one device, one created under SPI_QKV_ATTN=1 and one under SPI_QKV_ATTN=0.
Each op is timed with Model::profile_op (launched `reps` times back to back between two device events, inside an
otherwise normal forward), the two routes alternating, `rounds` times; the whole forward is the sum of the op
times of Model::profile.  All figures are device-time sums of eagerly launched ops, not serving rates.

    python tools/qkv_route_profile.py --out profiles/qkv_route.json
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


def replica(spi, module, batch, seq, fused):
    os.environ["SPI_QKV_ATTN"] = "1" if fused else "0"
    try:
        return spi.ModelReplica(module, 0, "fp16", max_batch=batch, seq_len=seq)
    finally:
        os.environ.pop("SPI_QKV_ATTN", None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="bert_base:8:128", help="model:batch:seq, comma-separated")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    spi = importlib.import_module("starpu-inference-server_amd")
    zoo = importlib.import_module("starpu-inference-server_amd.zoo")
    if spi.lib.spi_device_count() < 1:
        raise SystemExit("qkv_route_profile: no HIP device")
    stream = torch.cuda.Stream()
    results = []
    for cfg in a.configs.split(","):
        name, batch, seq = cfg.split(":")
        batch, seq = int(batch), int(seq)
        m = zoo.build(name)
        c = m.bert.config
        D, heads = c.hidden_size, c.num_attention_heads
        g = torch.Generator().manual_seed(1)
        ids = torch.randint(0, c.vocab_size, (batch, seq), generator=g).cuda()
        mask = torch.ones(batch, seq, dtype=torch.int64).cuda()
        out = torch.empty(batch, seq, D, device="cuda")
        reps = {"fused": replica(spi, m, batch, seq, True), "pair": replica(spi, m, batch, seq, False)}
        names = {k: [o["name"] for o in r.profile([ids, mask], out, stream.cuda_stream)] for k, r in reps.items()}
        ops = {"fused": [f"qkv_attention_S{seq}"],
               "pair": [f"gemm_M{batch * seq}_N{3 * D}_K{D}", f"attention_S{seq}"]}
        if ops["fused"][0] not in names["fused"]:
            print(f"{name}: the fused kernel does not serve {heads} heads of {D // heads} at seq {seq}; skipped", flush=True)
            continue
        for op in ops["pair"]:
            assert op in names["pair"], (op, sorted(set(names["pair"])))
        us = {op: [] for k in ops for op in ops[k]}
        whole = {"fused": [], "pair": []}
        for _ in range(a.rounds):
            for k in ("fused", "pair"):
                for op in ops[k]:
                    us[op].append(reps[k].profile_op([ids, mask], out, stream.cuda_stream, op, a.reps)["ms"] * 1e3)
            for k in ("fused", "pair"):
                whole[k].append(sum(o["ms"] for o in reps[k].profile([ids, mask], out, stream.cuda_stream)) * 1e3)
        route = {k: [sum(us[op][i] for op in ops[k]) for i in range(a.rounds)] for k in ops}
        res = dict(model=name, batch=batch, seq=seq, hidden=D, heads=heads, head_dim=D // heads, precision="fp16",
                   reps=a.reps, rounds=a.rounds, op_us=us,
                   route_us={k: dict(median=statistics.median(v), min=min(v), max=max(v), all=v) for k, v in route.items()},
                   forward_op_sum_us={k: dict(median=statistics.median(v), all=v) for k, v in whole.items()})
        print(f"{name} bs{batch} seq{seq} (D {D}, {heads} heads of {D // heads}), per layer: fused "
              f"{res['route_us']['fused']['median']:.2f} us [{min(route['fused']):.2f} .. {max(route['fused']):.2f}], pair "
              f"{res['route_us']['pair']['median']:.2f} us [{min(route['pair']):.2f} .. {max(route['pair']):.2f}] "
              f"({', '.join(f'{op} {statistics.median(us[op]):.2f}' for op in ops['pair'])}); forward op sum fused "
              f"{res['forward_op_sum_us']['fused']['median']:.0f} us, pair {res['forward_op_sum_us']['pair']['median']:.0f} us",
              flush=True)
        results.append(res)
        del reps
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()

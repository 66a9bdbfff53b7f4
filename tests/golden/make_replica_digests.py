#!/usr/bin/env python3
"""Record what the weight packer (csrc/model_pack.cpp) produces, as data (run from the repo root,
CPU only).

replica_digests.json -- weight_digest, weight_bytes, description and flops(1) of host-only replicas
                        (device -1) of small and full-size models in every precision, with the
                        packing toggles on and off.  tests/test_model_pack.py holds the packer to it
                        exactly, so a refactor of recognition / folding / packing can be checked
                        without a GPU.  Regenerate it only together with a deliberate change of the
                        blob layout, on a build of the commit that defines the layout.

The weights depend on neither torch's RNG nor its CPU kernels: the zoo models supply names and
shapes only, and element i of tensor `name` is filled in closed form (fill()).

Layout: {"commit": ..., "cases": {"model|precision|env": [digest hex, bytes, description, flops(1)]}}
"""
import importlib
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
HERE = os.path.dirname(os.path.abspath(__file__))
PKG = "starpu-inference-server_amd"

KNOBS = ("SPI_LN_FOLD", "SPI_STEM_FUSED")
ENVS = ("", "SPI_LN_FOLD=0", "SPI_STEM_FUSED=0")
PRECISIONS = ("fp32", "fp16", "fp16x3", "fp16m")

# name -> (zoo constructor, ModelReplica keywords)
SMALL = {
    "resnet_basic": (lambda z: z.resnet([1, 1, 1, 1], False, image=64, calibrate=False), dict(image_size=64)),
    "resnet_bottleneck": (lambda z: z.resnet([1, 1, 1, 1], True, image=64, calibrate=False), dict(image_size=64)),
    "bert_d128": (lambda z: z.bert(layers=2, hidden=128, heads=2, intermediate=256, vocab=64, max_position=32),
                  dict(num_heads=2, seq_len=16)),  # LayerNorm fold eligible
    "bert_d64": (lambda z: z.bert(layers=2, hidden=64, heads=1, intermediate=192, vocab=64, max_position=32),
                 dict(num_heads=1, seq_len=16)),  # D % 128 != 0: never folded
    "vit_d128": (lambda z: z.vit(image=32, patch=16, layers=2, heads=2, dim=128, mlp_dim=256, num_classes=10),
                 dict(num_heads=2, image_size=32)),
}
FULL = {
    "resnet18": (lambda z: z.resnet18(calibrate=False), dict()),
    "resnet152": (lambda z: z.resnet152(calibrate=False), dict()),
    "bert_base": (lambda z: z.bert_base(), dict(num_heads=12, seq_len=128)),
    "vit_l_16": (lambda z: z.vit_l_16(), dict(num_heads=16)),
}
MODELS = {**SMALL, **FULL}


def cases():
    return ([f"{m}|{p}|{e}" for m in SMALL for p in PRECISIONS for e in ENVS] + [f"{m}|fp16|" for m in FULL])


def fill(name, shape):
    """h = (i * 2654435761 + crc32(name)) mod 2^32, v = (h >> 8) / 2^24 - 0.5 (exact in fp32), then
    + 1 for a running_var, * 0.25 + 1 for a norm gain (a 1-D .weight), * 0.125 otherwise; the
    last step is computed in double and rounded to fp32 once."""
    n = int(np.prod(shape, dtype=np.int64))
    h = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(zlib.crc32(name.encode()))) & np.uint64(
        0xFFFFFFFF)
    v = (h >> np.uint64(8)).astype(np.float64) / 16777216.0 - 0.5
    if name.endswith("running_var"):
        v = v + 1.0
    elif name.endswith(".weight") and len(shape) == 1:
        v = v * 0.25 + 1.0
    else:
        v = v * 0.125
    return v.astype(np.float32).reshape(shape)


def filled(spi, module):
    """A module that exposes the zoo model's floating tensors, by name, with the closed-form fill."""
    d = {name: torch.from_numpy(fill(name, a.shape)) for name, a in spi.named_tensors(module)}

    class Named(torch.nn.Module):
        def named_parameters(self, *a, **k):
            return iter([])

        def named_buffers(self, *a, **k):
            return iter(d.items())
    return Named()


def record(spi, module, case):
    """[digest, bytes, description, flops(1)] of one case's host-only replica."""
    model, prec, env = case.split("|")
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    try:
        if env:
            k, v = env.split("=")
            os.environ[k] = v
        r = spi.ModelReplica(module, -1, prec, **MODELS[model][1])
        return ["%016x" % r.weight_digest, r.weight_bytes, r.description, r.flops(1)]
    finally:
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in saved.items() if v is not None})


def record_all(spi, zoo, want=None):
    out = {}
    for model, (make, _) in MODELS.items():
        mine = [c for c in cases() if c.split("|")[0] == model and (want is None or c in want)]
        if not mine:
            continue
        module = filled(spi, make(zoo))
        for c in mine:
            out[c] = record(spi, module, c)
    return out


def main():
    spi = importlib.import_module(PKG)
    zoo = importlib.import_module(PKG + ".zoo")
    table = {"commit": subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT, text=True).strip(),
             "cases": record_all(spi, zoo)}
    dump(table, os.path.join(HERE, "replica_digests.json"))
    print(len(table["cases"]), "replicas recorded")


def dump(table, path):
    """One line per case."""
    rows = ",\n".join("  %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in table["cases"].items())
    with open(path, "w") as f:
        f.write('{"commit": %s,\n "cases": {\n%s\n }}\n' % (json.dumps(table["commit"]), rows))


if __name__ == "__main__":
    main()

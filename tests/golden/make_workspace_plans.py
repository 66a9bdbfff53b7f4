#!/usr/bin/env python3
"""Record what a replica's forward plan (csrc/model_plan.cpp) sizes and counts, as data (run from the
repo root, CPU only).

workspace_plans.json -- per host-only replica (device -1): the bytes of every workspace buffer, the
                        split-K slab floats, the slab floats the launches plan before the allocation's
                        floor (spi_model_workspace_plan) and flops(3).  tests/test_model_plan.py holds
                        the plan to it, so a change of the walk, the descs or the sizing can be checked
                        without a GPU.

The cases are make_replica_digests.py's (same models, precisions, environments and closed-form weights)
plus the ones that change sizes: the classification outputs without logits, an input resize, BERT
without the hidden output, SPI_LN_FOLD=1, and a small ResNeXt with the grouped kernel on and off
(SPI_GCONV=0).

The table was recorded from the commit BEFORE the forward plans moved into model_plan.cpp, whose
Model::workspace_sizes_* were the only sizing code then: a build of that commit with one added export
(spi_model_workspace_plan returning what those members compute), loaded through SPI_HIP_LIB.  Regenerate
it only together with a deliberate change of the sizes.

Layout: {"commit": ..., "cases": {"model|precision|env|options": [[bytes...], slab floats, planned floats, flops(3)]}}
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
_spec = importlib.util.spec_from_file_location("make_replica_digests", os.path.join(HERE, "make_replica_digests.py"))
base = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(base)

KNOBS = base.KNOBS + ("SPI_GCONV",)
MODELS = dict(base.MODELS)
MODELS["resnext_small"] = (lambda z: z.resnet([1, 1, 1, 1], True, image=64, calibrate=False, groups=32,
                                              width_per_group=4), dict(image_size=64))
IMAGE_MODELS = ("resnet_basic", "resnet_bottleneck", "vit_d128")
# options: name -> (ModelReplica keywords, calls after construction)
OPTIONS = {
    "": (dict(), lambda r: None),
    "no_logits": (dict(), lambda r: r.set_image_outputs(("probs", "topk", "no_logits"), 3)),
    "resize": (dict(), lambda r: r.set_input_resize(96)),
    "no_hidden": (dict(bert_io=("pooler", "no_hidden")), lambda r: None),
}


def cases():
    out = [c + "|" for c in base.cases()]
    out += [f"{m}|{p}||{o}" for m in IMAGE_MODELS for p in ("fp32", "fp16") for o in ("no_logits", "resize")]
    out += [f"bert_d128|{p}||no_hidden" for p in ("fp32", "fp16")]
    out += [f"{m}|{p}|SPI_LN_FOLD=1|" for m in ("bert_d128", "bert_d64", "vit_d128") for p in base.PRECISIONS]
    out += [f"resnext_small|{p}|{e}|" for p in ("fp32", "fp16", "fp16m") for e in ("", "SPI_GCONV=0", "SPI_STEM_FUSED=0")]
    return out


def plan_of(spi, rep):
    """[[bytes per buffer], slab floats, planned floats] of a replica (spi_model_workspace_plan)."""
    fn = spi.lib.spi_model_workspace_plan
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.POINTER(C.c_size_t), C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_size_t),
                   C.POINTER(C.c_size_t)]
    sizes = (C.c_size_t * 32)()
    n, partial, planned = C.c_int32(), C.c_size_t(), C.c_size_t()
    assert fn(rep.handle, sizes, 32, C.byref(n), C.byref(partial), C.byref(planned)) == 0
    return [list(sizes[:n.value]), partial.value, planned.value]


def replica(spi, module, case):
    """The host-only replica of one case; the environment is restored before returning."""
    model, prec, env, opt = case.split("|")
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    try:
        if env:
            k, v = env.split("=")
            os.environ[k] = v
        kw, after = OPTIONS[opt]
        r = spi.ModelReplica(module, -1, prec, **MODELS[model][1], **kw)
        after(r)
        return r
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
        module = base.filled(spi, make(zoo))
        for c in mine:
            r = replica(spi, module, c)
            out[c] = plan_of(spi, r) + [r.flops(3)]
    return out


def main():
    spi = importlib.import_module(base.PKG)
    zoo = importlib.import_module(base.PKG + ".zoo")
    table = {"commit": subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT, text=True).strip(),
             "cases": record_all(spi, zoo)}
    base.dump(table, os.path.join(HERE, "workspace_plans.json"))
    print(len(table["cases"]), "plans recorded")


if __name__ == "__main__":
    main()

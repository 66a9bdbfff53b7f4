#!/usr/bin/env python3
"""Record which device path every case of tests/test_conv_kinds_ops_gpu.py takes (run from the repo root,
CPU only).

conv_kind_plans.json -- for every (knob setting, precision, shape) of op_refs.conv_kind_runs():
  "plans":  op_refs.kind_key(...) -> the 8 integers of spi_debug_conv_plan under the setting's knobs
  "routes": the same key -> spi_debug_conv_route per (residual, ReLU) form "00", "01", "10", "11", for the
            fp16 64 -> 64 cases
tests/test_op_refs.py holds the planner to it, and the GPU tests read their case ids (which name the kind)
from it.  Regenerate it only together with a deliberate change of the plan rule or of the case list.
"""
import importlib
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.dirname(HERE)]

import op_refs as R  # noqa: E402

ROUTE_FORMS = [(res, act) for res in (False, True) for act in (None, "relu")]


def routed(prec, shape):
    return prec == "fp16" and shape[3:5] == (64, 64)


def record(lib):
    plans, routes = {}, {}
    for _, setting, prec, shape in R.conv_kind_runs():
        key = R.kind_key(setting, prec, shape)
        if key in plans:
            continue
        with R.kind_knobs(lib, setting):
            plans[key] = R.query_conv_plan(lib, prec, shape)
            if routed(prec, shape):
                routes[key] = {f"{int(res)}{int(act is not None)}": R.query_conv_route(lib, prec, shape, res, act)
                               for res, act in ROUTE_FORMS}
    return plans, routes


def main():
    lib = importlib.import_module("starpu-inference-server_amd").lib
    plans, routes = record(lib)
    table = {"commit": subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT, text=True).strip(),
             "settings": R.KIND_SETTINGS, "plans": plans, "routes": routes}
    with open(os.path.join(HERE, "conv_kind_plans.json"), "w") as f:
        json.dump(table, f, separators=(",", ":"))
        f.write("\n")
    print(len(plans), "plans,", len(routes), "routed cases")


if __name__ == "__main__":
    main()

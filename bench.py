#!/usr/bin/env python3
"""MI355X inference-codelet benchmark (BASELINE.json metric: inferences/sec + p50 latency).

Headline workload = BASELINE.json configs[1]: ResNet-18, batch 8 per task, fp16 MFMA, one
MI355X -- run in the fp16m mode: fp16 activations and fp16 MFMA operands, with the layers that
set the fp16 error (stem, downsample convs, FC) on split-fp16 weights; it holds the north_star
1e-3 bar at this config (plain fp16 operands alone miss it on this random-init network,
DESIGN.md 3.2).  The fp32-grade fp16x3 mode is reported beside it.  The `--workers` HIP worker streams
of a GPU (STARPU_NWORKER_PER_CUDA=4, models/resnet18.yml:6) each call the HIP codelet
(libspi_hip.so, through the C-ABI) on a synthetic batch already resident in HBM.  A *step* is
`--tasks-per-step` codelet calls on every worker stream (default 8: 32 tasks = 256 images per GPU).

`value` = inferences of all ranks / (max over ranks of the barrier + device-sync bracketed time of
exactly `--steps` steps), inputs resident in HBM.  Multi-GPU: one process per GPU
(torch.distributed.run), one weight replica per device, tasks sharded across devices with no
data-path collective ("scaling": "weak").

A plain run sets up, warms up, times the `--steps` steps and prints the result line;
`--dump-outputs DIR` also writes every worker's output buffer of the last timed step to
DIR/<name>.npy (seeded inputs: two builds can be compared output for output).

Also reported with `--full` (rank 0, single GPU):
* `e2e`: the SURVEY 8(d) serving metric -- the mini-runtime (pinned slot pools, H2D/D2H, pipelined
  workers) driven by the C++ client loop: inf/s = inferences / (last response - first request)
  (inference_client.cpp:259-270), p50/p95/p99 request latency incl. H2D + D2H
  (latency_statistics.hpp:52-93);
* the dominant kernel's roofline, measured under the same four-stream load (hipEvents on its
  launch stream) and isolated, with HBM traffic and MFMA-busy from the committed rocprofv3 PMC
  passes (profiles/r02/);
* the CPU codelet baseline: the C++ LibTorch CPU codelet (libspi_torch.so, the reference's
  cpu_inference_func restated) on a TorchScript export of the same model, on the host's cores;
* extras: plain fp16, ResNet-18 bs1, bs1 requests batched by the runtime (adaptive vs fixed),
  BERT-base seq128 bs8 (C3), ResNet-152 bs32 (C4), ViT-L/16 bs16 (C5).
"""
from __future__ import annotations

import argparse
import ctypes as C
import glob
import importlib
import json
import os
import socket
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

BASELINE_METRIC = "inferences/sec + p50 latency, ResNet-18 bs=1 & BERT-base seq=128, 1/2/4/8 GPU"
WORKLOADS = {
    "resnet18": "ResNet-18 bs=8 fp16, single MI355X HIP codelet (conv-as-implicit-GEMM MFMA)",
    "bert_base": "bert-base-uncased seq=128 bs=8 fp16, 1xMI355X (QKV GEMM + softmax + LayerNorm fused)",
    "resnet152": "ResNet-152 bs=32 fp16, HIP workers per MI355X (request-parallel, no RCCL)",
    "vit_l_16": "ViT-L/16 224^2 bs=16 fp16 (patch-embed GEMM + MFMA attention, LDS-tiled)",
}
PEAK_TFLOPS = {"fp16": 2500.0, "fp16m": 2500.0, "fp16x3": 2500.0, "fp32": 157.3}  # MI355X dense (MI355X_MICROARCH.md)
PEAK_HBM_GBS = 8000.0
PROFILE_ROUND = "r02"
# The fp16 configs' parity-grade modes (north_star 1e-3): fp16m holds it on ResNet-18 at 224,
# the deep bottleneck ResNet-152 needs fp16x3 (fp16m emulates at 6-7e-3), the transformers
# pass in plain fp16 (fp32 softmax / LayerNorm / residual stream).
DEFAULT_PRECISION = {"resnet18": "fp16m", "resnet152": "fp16x3", "bert_base": "fp16", "vit_l_16": "fp16"}


def percentile(samples, p):
    """Linear-interpolated percentile (latency_statistics.hpp:52-93)."""
    xs = sorted(samples)
    if not xs:
        return float("nan")
    if len(xs) == 1:
        return xs[0]
    pos = (p / 100.0) * (len(xs) - 1)
    lo = int(np.floor(pos))
    hi = min(lo + 1, len(xs) - 1)
    return xs[lo] + (xs[hi] - xs[lo]) * (pos - lo)


def reduce_max_elapsed(elapsed: float, world: int) -> float:
    """Max over ranks of the barrier-bracketed timed region (control plane only, gloo)."""
    if world <= 1:
        return elapsed
    import torch
    import torch.distributed as dist

    t = torch.tensor([elapsed], dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def shard_requests(n: int, rank: int, world: int) -> list:
    """Request-level sharding across independent per-GPU workers (no data-path collective):
    contiguous blocks, as an eager shared queue drained by per-device workers would end up."""
    base, extra = divmod(n, world)
    lo = rank * base + min(rank, extra)
    return list(range(lo, lo + base + (1 if rank < extra else 0)))


def make_inputs(name, batch, rng, seq=128):
    if name.startswith("bert"):
        ids = rng.integers(0, 30522, size=(batch, seq), dtype=np.int64)
        mask = np.ones((batch, seq), dtype=np.int64)  # all-ones mask
        return [ids, mask], (batch, seq, 768)
    return [rng.random((batch, 3, 224, 224), dtype=np.float32)], (batch, 1000)


class Harness:
    """Prebuilt codelet calls (cl_arg + buffers + stream) for `workers` workers of one device."""

    def __init__(self, spi, replica, name, dev, batch, workers, rng, streams=None):
        import torch

        self.spi, self.lib, self.N = spi, spi.lib, spi._native
        self.torch = torch
        self.dev = dev
        self.replica = replica
        self.batch = batch
        # Reuse the worker streams of an earlier harness when given: each new HIP
        # stream takes a hardware queue, and queues beyond GPU_MAX_HW_QUEUES are shared.
        self.streams = list(streams) if streams is not None else [torch.cuda.Stream(dev) for _ in range(workers)]
        self.host_inputs, self.out_shape = make_inputs(name, batch, rng)
        self.d_in = [[torch.from_numpy(x).to(dev) for x in self.host_inputs] for _ in range(workers)]
        self.d_out = [torch.empty(self.out_shape, device=dev, dtype=torch.float32) for _ in range(workers)]
        torch.cuda.synchronize(dev)
        self.calls = []
        for w in range(workers):
            params = spi.make_params([list(x.shape) for x in self.d_in[w]], [x.dtype for x in self.d_in[w]],
                                     models_gpu=[replica], device_ids=[dev])
            bufs = spi.buffer_array([spi.tensor_interface(x) for x in self.d_in[w]] +
                                    [spi.tensor_interface(self.d_out[w])])
            self.calls.append((params.to_args(), bufs, self.streams[w]))

    def task(self, w, ev=None):
        a, bufs, st = self.calls[w]
        self.lib.spi_set_worker_context(w, self.dev, C.c_void_p(st.cuda_stream))
        if ev is not None:
            ev[0].record(st)
        self.lib.spi_hip_inference_func(bufs, C.byref(a))
        if ev is not None:
            ev[1].record(st)
        if a.status != self.N.SPI_OK:
            raise RuntimeError(a.error.decode())

    def rounds(self, n):
        for _ in range(n):
            for w in range(len(self.calls)):
                self.task(w)

    def throughput(self, steps, warmup, tasks_per_step=1, world=1, dist=None):
        """Timed region: exactly `steps` steps of `tasks_per_step` tasks per worker, no
        instrumentation inside (timing events on every task cost ~25 % on ROCm)."""
        torch = self.torch
        self.rounds(warmup * tasks_per_step)
        torch.cuda.synchronize(self.dev)
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize(self.dev)
        t0 = time.perf_counter()
        self.rounds(steps * tasks_per_step)
        torch.cuda.synchronize(self.dev)
        t1 = time.perf_counter()
        if world > 1:
            dist.barrier()
        return reduce_max_elapsed(t1 - t0, world)

    def loaded_latency(self, rounds):
        """Device latency of each task (events on its worker stream) with every worker busy."""
        torch = self.torch
        W = len(self.calls)
        events = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(W)]
                  for _ in range(rounds)]
        for k in range(rounds):
            for w in range(W):
                self.task(w, events[k][w])
        torch.cuda.synchronize(self.dev)
        return [s.elapsed_time(e) for step in events for (s, e) in step]

    def serial_e2e(self, iters):
        """pinned host -> H2D -> codelet -> D2H -> sync, one task in flight."""
        torch = self.torch
        st = self.streams[0]
        pinned_in = [torch.from_numpy(x).pin_memory() for x in self.host_inputs]
        pinned_out = torch.empty(self.out_shape, dtype=torch.float32).pin_memory()
        out = []
        for i in range(iters + 3):
            ts = time.perf_counter()
            with torch.cuda.stream(st):
                for h, d in zip(pinned_in, self.d_in[0]):
                    d.copy_(h, non_blocking=True)
                self.task(0)
                pinned_out.copy_(self.d_out[0], non_blocking=True)
            st.synchronize()
            if i >= 3:
                out.append((time.perf_counter() - ts) * 1e3)
        return out

    def op_profile(self, loaded: bool, repeats: int = 5):
        """Per-op device time of one forward on worker 0's stream (every launch bracketed by
        hipEvents on that stream), averaged over `repeats` forwards.  loaded=True: the other
        workers run back-to-back tasks meanwhile -- the four-stream load `value` is measured under."""
        torch = self.torch
        W = len(self.calls)
        acc = {}
        for _ in range(repeats):
            if loaded:
                for _ in range(12):  # ~12 tasks per busy worker covers the profiled forward
                    for w in range(1, W):
                        self.task(w)
            ops = self.replica.profile(self.d_in[0], self.d_out[0], self.streams[0].cuda_stream)
            torch.cuda.synchronize(self.dev)
            for op in ops:
                a = acc.setdefault(op["name"], [0.0, 0, op["flops"], op["bytes"]])
                a[0] += op["ms"]
                a[1] += 1
        return {k: (v[0] / repeats, v[1] // repeats, v[2], v[3]) for k, v in acc.items()}


def committed_profile(kind, model, batch, precision):
    """profiles/<round>/<kind>_<model>_bs<batch>_<precision>.json (rocprofv3 PMC passes, tools/pmc_*.sh)."""
    hits = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*", f"{kind}_{model}_bs{batch}_{precision}.json")))
    if not hits:
        return {}, None
    with open(hits[-1]) as f:
        return json.load(f).get("ops", {}), os.path.relpath(hits[-1], ROOT)


def committed_rocprof(op):
    """The newest profiles/<round>/roofline_rocprof.json entry for `op` (tools/rocprof_roofline.py)."""
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*", "roofline_rocprof.json")), reverse=True):
        with open(path) as f:
            rec = json.load(f).get(op)
        if rec:
            return rec
    return None


def trace_ranking(model, batch, precision):
    """The committed rocprofv3 kernel trace of this config's graph-replayed timed loop, regrouped
    per op (profiles/<round>/trace_<model>_bs<B>_<prec>_ops.csv, tools/trace_round.sh +
    tools/trace_ops.py --launches): rows largest total device time first, and the file."""
    hits = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*", f"trace_{model}_bs{batch}_{precision}_ops.csv")))
    if not hits:
        return [], None
    import csv
    with open(hits[-1]) as f:
        rows = [r for r in csv.DictReader(f) if r.get("op")]
    rows.sort(key=lambda r: -float(r["total_us"]))
    return rows, os.path.relpath(hits[-1], ROOT)


def roofline(h, precision, model, reps=200, name=None):
    """The op that bounds the timed loop, and its roofline: algorithmic FLOPs (or bytes) per
    launch over its steady-state launch duration -- `reps` launches of that op back to back on
    worker 0's stream between one pair of hipEvents (Model::profile_op), the same launches a
    rocprofv3 kernel trace of `bench.py --roofline-only --roofline-op NAME` counts.
    Which op: the largest summed device time in the committed rocprofv3 trace of this config's
    graph-replayed timed loop (trace_ranking); without one, the largest device time per
    forward of an eager forward under the four-stream load.  `name` overrides the choice.  The
    per-launch event times under the four-stream load are reported beside it."""
    ranking, rsrc = trace_ranking(model, h.batch, precision)
    loaded = h.op_profile(True) if name is None else None
    selection = "given"
    if name is None and ranking:
        name = ranking[0]["op"].split("|")[0]
        selection = f"largest summed device time in the rocprofv3 trace of the graph-replayed timed loop ({rsrc})"
    elif name is None:
        name = max(loaded.items(), key=lambda kv: kv[1][0])[0]
        selection = "largest device time per forward, eager forward under the four-stream load (no committed trace)"
    micro = h.replica.profile_op(h.d_in[0], h.d_out[0], h.streams[0].cuda_stream, name, reps)
    ms, flops, nbytes = micro["ms"], micro["flops"], micro["bytes"]
    peak = PEAK_TFLOPS[precision]
    traffic, tsrc = committed_profile("traffic", model, h.batch, precision)
    mfma, msrc = committed_profile("mfma", model, h.batch, precision)
    t_bytes = traffic.get(name, {}).get("hbm_bytes_per_launch")
    common = {"kernel": name, "selection": selection, "avg_launch_ms": round(ms, 5), "reps": reps,
              "measured": f"hipEvents around {reps} back-to-back launches of the op on its stream "
                          "(Model::profile_op); rocprofv3 summary of the same launches in profiles/",
              "traffic": t_bytes, "traffic_source": tsrc,
              "hbm_gbs": round(t_bytes / (ms * 1e-3) / 1e9, 1) if t_bytes else None,
              "mfma_busy_pct": mfma.get(name, {}).get("mfma_busy_pct"), "mfma_source": msrc}
    rp = committed_rocprof(name)
    if rp:  # the committed rocprofv3 --kernel-trace --stats average of the same launches
        common["rocprof_avg_launch_ms"] = rp["avg_ms"]
        common["frac_rocprof"] = round((flops / (rp["avg_ms"] * 1e-3) / 1e12 / peak) if flops else
                                       (nbytes / (rp["avg_ms"] * 1e-3) / 1e9 / PEAK_HBM_GBS), 5)
        common["rocprof_source"] = rp["source"]
    tr = next((r for r in ranking if name in r["op"].split("|")), None)
    if tr is not None:  # the same op in the timed loop's trace (profiler-perturbed concurrency)
        common["timed_loop_trace"] = {
            "share_of_device_time": float(tr["share"]), "mean_us": float(tr["mean_us"]),
            "median_us": float(tr["median_us"]), "kernel": tr["kernel"],
            "grid": [int(tr["workgroups_x"]), int(tr["grid_y"])],
            "frac_at_trace_mean": round((flops / (float(tr["mean_us"]) * 1e-6) / 1e12 / peak) if flops else
                                        (nbytes / (float(tr["mean_us"]) * 1e-6) / 1e9 / PEAK_HBM_GBS), 5),
            "source": rsrc}
    if loaded is not None and name in loaded:
        tot, cnt = loaded[name][0], loaded[name][1]
        fwd_loaded = sum(v[0] for v in loaded.values())
        ms_l = tot / max(cnt, 1)
        common["under_load"] = {
            "launches_per_forward": cnt, "avg_launch_ms": round(ms_l, 5),
            "forward_share": round(tot / fwd_loaded, 4),
            "frac": round((flops / (ms_l * 1e-3) / 1e12 / peak) if flops else
                          (nbytes / (ms_l * 1e-3) / 1e9 / PEAK_HBM_GBS), 5),
            "measured": "hipEvents around each launch of one eager forward on worker 0 while the other "
                        "workers replay forwards (5 forwards)"}
    if flops == 0:
        ach = nbytes / (ms * 1e-3) / 1e9
        return {"bound": "hbm", "achieved": round(ach, 2), "peak": PEAK_HBM_GBS, "unit": "GB/s",
                "frac": round(ach / PEAK_HBM_GBS, 5), "algorithmic_bytes_per_launch": nbytes, **common}
    ach = flops / (ms * 1e-3) / 1e12
    return {"bound": "mfma", "achieved": round(ach, 3), "peak": peak, "unit": "TFLOP/s", "frac": round(ach / peak, 5),
            "algorithmic_flops_per_launch": flops, "mfma_issue_per_flop": 3 if precision == "fp16x3" else 1,
            **common}


def runtime_e2e(rtmod, replica, name, batch, requests, inflight, req_batch=None, workers=4, schedule=None,
                warmup=None, **kw):
    """The serving path: mini-runtime (pinned slots, H2D/D2H, pipelined workers) + C++ client loop."""
    rb = req_batch or batch
    host_inputs, out_shape = make_inputs(name, rb, np.random.default_rng(7))
    if name.startswith("bert"):
        in_specs = [((x.shape[1],), np.int64) for x in host_inputs]
    else:
        in_specs = [((3, 224, 224), np.float32)]
    out_elems = int(np.prod(out_shape[1:]))
    # every task is max_batch when requests are max_batch and nothing merges them: warm that size only
    if rb == batch and "warmup_batches" not in kw:
        kw["warmup_batches"] = -1
    rt = rtmod.Runtime([replica], in_specs, [(out_elems, np.float32)], max_batch=batch, workers_per_device=workers,
                       **kw)
    h2d = rt.h2d_mode
    r = rt.loadgen(host_inputs, requests=requests, inflight=inflight,
                   warmup=warmup if warmup is not None else max(8 * workers, 2 * inflight), schedule=schedule)
    target = rt.batch_target
    rt.close()
    out = {"value": round(r["inferences_per_s"], 2), "unit": "inferences/s", "p50_latency_ms": round(r["p50_ms"], 4),
           "p95_latency_ms": round(r["p95_ms"], 4), "p99_latency_ms": round(r["p99_ms"], 4),
           "requests": r["completed"], "request_batch": rb, "max_batch": batch, "inflight": inflight,
           "workers": workers, "mean_task_batch": round(r["mean_task_batch"], 2),
           "p50_queue_ms": round(r["p50_queue_ms"], 4), "failed": r["failed"], "rejected": r["rejected"],
           "breakdown_ms": {k: round(r[k], 4) for k in ("p99_queue_ms", "p50_stage_ms", "p99_stage_ms",
                                                        "p50_device_ms", "p99_device_ms", "max_ms")},
           "worst_request_at": round(r["worst_at_frac"], 3),
           "seconds": round(r["seconds"], 3), "h2d_mode": h2d}
    if r["error"]:
        out["first_error"] = r["error"]
    if kw.get("batching") is not None:
        out["final_batch_target"] = target
    return out


def aggregate_e2e(local: dict, world: int, dist) -> dict:
    """Whole-job serving figures over the ranks (one runtime per GPU, each rank's loop started
    behind a barrier): inferences of all ranks / the longest rank's (last response - first
    request); p50/p95/p99 the worst rank's (per-rank values listed)."""
    if world <= 1:
        return local
    per = [None] * world
    dist.all_gather_object(per, local)
    inf = sum(p["requests"] * p["request_batch"] for p in per)
    sec = max(p["seconds"] for p in per)
    out = dict(local)
    out.update({"value": round(inf / sec, 2) if sec > 0 else 0.0, "requests": sum(p["requests"] for p in per),
                "seconds": sec, "failed": sum(p["failed"] for p in per), "rejected": sum(p["rejected"] for p in per),
                "p50_latency_ms": max(p["p50_latency_ms"] for p in per),
                "p95_latency_ms": max(p["p95_latency_ms"] for p in per),
                "p99_latency_ms": max(p["p99_latency_ms"] for p in per),
                "per_rank": [{k: p[k] for k in ("value", "p50_latency_ms", "p99_latency_ms")} for p in per],
                "aggregation": "sum of inferences over ranks / longest rank window; worst rank's percentiles"})
    return out


def host_cores():
    """The host as this process sees it.  `threads_used`: the CPU share of the job -- the GPU box
    allots OMP_NUM_THREADS (16) CPUs per GPU and asks jobs to stay inside it -- else every
    affinity CPU."""
    nodes = glob.glob("/sys/devices/system/node/node[0-9]*")
    try:
        affinity = len(os.sched_getaffinity(0))
    except AttributeError:
        affinity = os.cpu_count()
    share = int(os.environ.get("OMP_NUM_THREADS", "0") or 0) or affinity
    return {"nproc": os.cpu_count(), "affinity_cpus": affinity, "numa_nodes": max(1, len(nodes)),
            "threads_used": min(share, affinity),
            "share_rule": "OMP_NUM_THREADS (the box's CPU share per GPU)" if share < affinity else "affinity CPUs"}


def cpu_baseline(model, name, batch, seconds):
    """The C++ LibTorch CPU codelet (spi_cpu_inference_func + spi_torch_cpu_forward) on a TorchScript
    export of the same model, in the reference's three CPU-worker layouts (starpu_setup.cpp:291-386):
    (i) one worker with every thread of the share as intra-op threads, (ii) one worker per NUMA
    node with the share's threads split evenly (group_cpu_by_numa), (iii) the default, one StarPU
    CPU worker per core with one intra-op thread each -- at bs8 (C2's task) and bs1 (C1), value =
    the best bs8 layout.  The threads are the box's CPU share for this GPU (threads_used, the
    OMP_NUM_THREADS the box sets): the GPU box asks every job to size its worker pools to that
    share, so the whole host (nproc, reported) is not used; the per-core rate of (iii) times the
    affinity CPUs is reported as an extrapolation."""
    import torch

    lt = importlib.import_module("starpu-inference-server_amd.libtorch")
    cores = host_cores()
    n = cores["threads_used"]
    numa = cores["numa_nodes"]
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, f"{name}.pt")
        torch.jit.trace(model, torch.rand(1, 3, 224, 224)).save(path)
        ts = lt.TorchScriptModule(path)
    rng = np.random.default_rng(0)
    x8 = rng.random((batch, 3, 224, 224), dtype=np.float32)
    x1 = x8[:1].copy()
    per = max(1, n // numa)
    layouts = {"i_one_worker_all_threads": (1, n), "ii_worker_per_numa_node": (numa, per),
               "iii_worker_per_core": (n, 1)}
    ts.bench([x1], [4000], workers=1, threads=n, seconds=0.5)  # warm-up
    slot = seconds / (2 * len(layouts))
    main, c1 = {}, {}
    for key, (w, t) in layouts.items():
        r = ts.bench([x8], [batch * 4000], workers=w, threads=t, seconds=slot)
        main[key] = {"value": round(r["inferences_per_s"], 3), "unit": "inferences/s", "p50_ms": round(r["p50_ms"], 3),
                     "workers": w, "threads_per_worker": t, "tasks": r["tasks"]}
    for key, (w, t) in layouts.items():
        r = ts.bench([x1], [4000], workers=w, threads=t, seconds=slot)
        c1[key] = {"value": round(r["inferences_per_s"], 3), "unit": "inferences/s",
                   "p50_ms": round(r["p50_ms"], 3), "workers": w, "threads_per_worker": t, "tasks": r["tasks"]}
    ts.close()
    best = max(main, key=lambda k: main[k]["value"])
    per_core = c1["iii_worker_per_core"]["value"] / max(1, n)
    c1["extrapolated_full_host_per_core_layout"] = {
        "value": round(per_core * cores["affinity_cpus"], 1), "unit": "inferences/s",
        "basis": f"layout (iii) per-core rate x {cores['affinity_cpus']} affinity CPUs (not measured: the box "
                 f"allots {n} CPUs to this job)"}
    tag = {"i_one_worker_all_threads": "i", "ii_worker_per_numa_node": "ii", "iii_worker_per_core": "iii"}
    summary = {f"bs{batch}_{tag[k]}": [v["value"], v["p50_ms"], v["workers"], v["threads_per_worker"]]
               for k, v in main.items()}
    summary.update({f"bs1_{tag[k]}": [v["value"], v["p50_ms"], v["workers"], v["threads_per_worker"]]
                    for k, v in c1.items() if k in tag})
    return {
        "value": main[best]["value"], "unit": "inferences/s", "cores": n, "kind": "port",
        "sample": f"CPU-codelet tasks ({name} bs{batch} and bs1 fp32, TorchScript, libspi_torch.so: InferenceMode "
                  f"forward + copy_output_to_buffer behind spi_cpu_inference_func), ~{slot:.1f} s per layout; value "
                  f"= best bs{batch} layout ({best}); {n} threads = the box's CPU share of {cores['nproc']} CPUs, "
                  f"{numa} NUMA nodes",
        "sample_short": f"{name} fp32 LibTorch CPU codelet, layouts (i)-(iii) on the {n}-CPU share at bs{batch} and "
                        f"bs1, ~{slot:.1f} s each, as [inf/s, p50 ms, workers, threads]; value = bs{batch} {tag[best]}",
        "p50_ms": main[best]["p50_ms"], "host": cores, "layouts_bs%d" % batch: main,
        "c1_resnet18_bs1_fp32": c1, "layouts_summary": summary,
    }


def config_line(spi, zoo, rtmod, name, batch, precision, workers, streams, steps, dev, rank, world, dist, seq=128,
                e2e_requests=400, tasks_per_step=1):
    """Device-resident inf/s (all ranks), loaded p50 task latency and roofline (rank 0), and the
    PCIe-inclusive e2e run (all ranks, aggregated) for one BASELINE config.  A step is
    `tasks_per_step` codelet calls per worker stream, as the headline's."""
    model = zoo.build(name, seed=0)
    rep = spi.ModelReplica(model, dev, precision, max_batch=batch, seq_len=seq if name.startswith("bert") else 0,
                           graphs=True)
    h = Harness(spi, rep, name, dev, batch, workers, np.random.default_rng(3 + rank), streams)
    el = h.throughput(steps, 2, tasks_per_step, world, dist)
    lat = h.loaded_latency(10)
    out = {"value": round(world * workers * tasks_per_step * batch * steps / el, 2), "steps": steps,
           "tasks_per_step": tasks_per_step,
           "unit": "sequences/s" if name.startswith("bert") else "inferences/s", "dtype": precision, "batch": batch,
           "n_gpus": world, "p50_task_latency_ms": round(percentile(lat, 50), 4),
           "gflop_per_inference": round(rep.flops(1) / 1e9, 3)}
    if rank == 0:
        out["roofline"] = roofline(h, precision, name)
    out["model_tflops_per_gpu"] = round(rep.flops(1) * out["value"] / world / 1e12, 2)
    if world > 1:
        dist.barrier()
    out["e2e"] = aggregate_e2e(runtime_e2e(rtmod, rep, name, batch, e2e_requests, inflight=4 * workers,
                                           workers=workers), world, dist)
    del rep, model, h
    return out


def single_process_e2e(spi, zoo, rtmod, args, model, replica, world):
    """One mini-runtime over replicas on devices 0..world-1 (this process), the same closed-loop
    bs8 workload as `e2e` at 8 in flight per worker per device."""
    reps = [replica] + [spi.ModelReplica(model, d, args.precision, max_batch=args.batch,
                                         seq_len=128 if args.model.startswith("bert") else 0, graphs=True)
                        for d in range(1, world)]
    host_inputs, out_shape = make_inputs(args.model, args.batch, np.random.default_rng(11))
    in_specs = ([((x.shape[1],), np.int64) for x in host_inputs] if args.model.startswith("bert")
                else [((3, 224, 224), np.float32)])
    rt = rtmod.Runtime(reps, in_specs, [(int(np.prod(out_shape[1:])), np.float32)], max_batch=args.batch,
                       workers_per_device=args.workers, warmup_batches=-1)
    inflight = 8 * args.workers * world
    r = rt.loadgen(host_inputs, requests=args.e2e_requests * world, inflight=inflight, warmup=2 * inflight)
    wt = rt.worker_times()  # workers are numbered device-major, args.workers per device
    tasks_per_device = [sum(w["tasks"] for w in wt[d * args.workers:(d + 1) * args.workers]) for d in range(world)]
    h2d = rt.h2d_mode
    rt.close()
    del reps[1:]
    return {"value": round(r["inferences_per_s"], 2), "unit": "inferences/s", "devices": world,
            "p50_latency_ms": round(r["p50_ms"], 4), "p99_latency_ms": round(r["p99_ms"], 4),
            "requests": r["completed"], "failed": r["failed"], "inflight": inflight, "h2d_mode": h2d,
            "tasks_per_device": tasks_per_device,
            "shape": "one process, one runtime: one eager queue + one batcher over every device's workers "
                     "(StarPU's single-process layout); value = inferences / (last response - first request)"}


def free_port() -> int:
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def spawn_ranks(n: int) -> int:
    """`bench.py --gpus N` without a launcher: start N rank processes (one per GPU, RANK /
    LOCAL_RANK / WORLD_SIZE set, as torch.distributed.run would) before this process touches any
    GPU, pass rank 0's JSON line through, and exit with the worst return code."""
    port = free_port()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=None if r == 0 else subprocess.DEVNULL))
    rcs = [p.wait() for p in procs]
    return max(abs(rc) for rc in rcs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--model", default="resnet18", choices=sorted(WORKLOADS))
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--precision", default=None, choices=["fp16", "fp16m", "fp16x3", "fp32"],
                    help="default: the parity-grade fp16 mode of the model (DEFAULT_PRECISION)")
    ap.add_argument("--workers", type=int, default=4, help="worker streams per GPU")
    ap.add_argument("--tasks-per-step", type=int, default=8, help="codelet calls per worker per step")
    ap.add_argument("--repeats", type=int, default=5,
                    help="re-time the same K-step region this many times after `value` (value_repeats)")
    ap.add_argument("--graphs", type=int, default=1, help="capture the forward body into hipGraphs")
    ap.add_argument("--hw-queues", type=int, default=0,
                    help="GPU_MAX_HW_QUEUES for this process (0: 2 x workers + 8, at least the environment's)")
    ap.add_argument("--cpu-seconds", type=float, default=18.0, help="CPU baseline budget over its layouts (0 = skip)")
    ap.add_argument("--e2e-requests", type=int, default=4000)
    ap.add_argument("--extras", type=int, default=1, help="extra measurements (0 = skip)")
    ap.add_argument("--ci-schedule", type=int, default=1,
                    help="the reference's CI perf workload (ResNet-152, bs1 requests, adaptive batching to 16, "
                         "ci_perf_resnet.csv at its real intervals: ~14 s)")
    ap.add_argument("--roofline-only", action="store_true",
                    help="only the dominant op's back-to-back launches (the rocprofv3 roofline command)")
    ap.add_argument("--roofline-op", default="", help="op name for --roofline-only (default: chosen under load)")
    ap.add_argument("--roofline-reps", type=int, default=200)
    ap.add_argument("--loop-only", action="store_true",
                    help="only the timed loop (the rocprofv3 trace command of tools/trace_round.sh)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also measure everything else: re-timed regions, loaded task "
                         "latency, roofline, the e2e serving legs, the CPU baseline and the extras (minutes)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="after the timed steps write each worker's output buffer of the last step to "
                         "DIR/<name>.npy (float32)")
    ap.add_argument("--detail-out", default=None,
                    help="rank 0 writes the full record here (the printed line is its compact summary); "
                         "default: bench_out/bench_detail.json with --full, none without")
    ap.add_argument("--launch-table", default="",
                    help="write one eager forward's kernel launches (op, kernel, grid) here as TSV (rank 0)")
    ap.add_argument("--control-plane-only", action="store_true",
                    help="test hook (tests/test_host.py): run the multi-rank control path -- rank spawn, gloo "
                         "rendezvous, barrier + max-over-ranks timing, e2e aggregation, the JSON line -- around "
                         "a host-side stand-in for the GPU work")
    args = ap.parse_args()
    args.precision = args.precision or DEFAULT_PRECISION[args.model]
    if args.detail_out is None:
        args.detail_out = os.path.join("bench_out", "bench_detail.json") if args.full else ""

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(spawn_ranks(args.gpus))

    # One HIP hardware queue per stream: HIP maps streams onto GPU_MAX_HW_QUEUES queues
    # round-robin (default 4, shared with torch's own streams), and streams that share a queue
    # run serially -- 28.4k -> 38.1k inf/s at 4 workers going from 4 to 8 queues.  Room for the
    # harness's worker streams plus the runtime's workers and copy stream.  Must be set before the
    # first HIP call.
    queues = min(32, args.hw_queues or max(int(os.environ.get("GPU_MAX_HW_QUEUES", "4")), 2 * args.workers + 8))
    os.environ["GPU_MAX_HW_QUEUES"] = str(queues)

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))

    import torch
    import torch.distributed as dist

    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo", rank=rank, world_size=world)
    if args.control_plane_only:
        control_plane_only(args, rank, world, dist)
        return

    spi = importlib.import_module("starpu-inference-server_amd")
    zoo = importlib.import_module("starpu-inference-server_amd.zoo")
    rtmod = importlib.import_module("starpu-inference-server_amd.runtime")
    # SPI_BENCH_SHARE_DEVICE=1: every rank on device 0 (multi-rank rehearsal on a 1-GPU box only).
    dev = 0 if os.environ.get("SPI_BENCH_SHARE_DEVICE") == "1" else local_rank
    torch.cuda.set_device(dev)

    seq = 128
    model = zoo.build(args.model, seed=0)
    replica = spi.ModelReplica(model, dev, args.precision, max_batch=args.batch,
                               seq_len=seq if args.model.startswith("bert") else 0, graphs=bool(args.graphs))
    h = Harness(spi, replica, args.model, dev, args.batch, args.workers, np.random.default_rng(rank))
    if args.launch_table and rank == 0:
        with open(args.launch_table, "w") as f:
            for r in replica.launch_table(h.d_in[0], h.d_out[0], h.streams[0].cuda_stream):
                f.write("\t".join(str(x) for x in (r["op_index"], r["op"], r["kernel"], *r["grid"], r["block"])) + "\n")
        torch.cuda.synchronize(dev)
    if args.loop_only:
        elapsed = h.throughput(args.steps, args.warmup, args.tasks_per_step, world, dist)
        per_step = args.workers * args.tasks_per_step * args.batch
        if rank == 0:
            print(json.dumps({"loop_only": True, "model": args.model, "batch": args.batch, "dtype": args.precision,
                              "value": round(world * per_step * args.steps / elapsed, 2),
                              "ms_per_step": round(elapsed * 1e3 / args.steps, 4)}), flush=True)
        return
    if args.roofline_only:
        h.rounds(1)
        torch.cuda.synchronize(dev)
        rl = roofline(h, args.precision, args.model, args.roofline_reps, args.roofline_op or None)
        if rank == 0:
            print(json.dumps({"roofline_only": True, "config": WORKLOADS[args.model], "batch": args.batch,
                              "dtype": args.precision, "roofline": rl}), flush=True)
        return
    elapsed = h.throughput(args.steps, args.warmup, args.tasks_per_step, world, dist)
    per_step = args.workers * args.tasks_per_step * args.batch
    value = world * per_step * args.steps / elapsed
    if args.dump_outputs:
        dump_outputs(h, args.dump_outputs, rank, world)

    result = {
        "metric": BASELINE_METRIC,
        "value": round(value, 2),
        "unit": "inferences/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(elapsed * 1e3 / args.steps, 4),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": args.precision,
        "data": "synthetic (seeded U[0,1) images / uniform token ids, all-ones mask); random-init weights "
                "of the reference architecture (no checkpoints offline)",
        "config": {
            "workload": WORKLOADS[args.model],
            "batch_per_task": args.batch,
            "workers_per_gpu": args.workers,
            "tasks_per_step": args.tasks_per_step,
            "step": f"{args.tasks_per_step} codelet calls on each of the {args.workers} worker streams "
                    f"({per_step} inferences per GPU)",
            "precision_mode": {"fp16x3": "split-fp16 MFMA (hi/lo fp16 operands, fp32 accumulate): fp32-grade parity",
                               "fp16m": "fp16 MFMA operands + fp16 activations, fp32 accumulate; the stem (fp16 image) "
                                        "and the downsample convs on hi + lo fp16 weights, FC on plain fp16 weights "
                                        "(normalised max error 0.60-0.69e-3 at this config)",
                               "fp16": "fp16 MFMA operands, fp32 accumulate", "fp32": "fp32 MFMA"}[args.precision],
            "inputs": "resident in HBM when the timed region starts (the bench contract's `value`); the "
                      "PCIe-inclusive serving rate -- submit -> outputs in host memory, SURVEY 8(d) -- is `e2e`, "
                      "measured at every N",
            "graphs": bool(args.graphs),
            "hip_hw_queues": queues,
            "parallelism": f"replicas x{world} (request sharding, no collective)",
        },
    }
    if args.full:
        full_measurements(args, spi, zoo, rtmod, dist, h, model, replica, result, value, per_step, dev, rank, world)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        emit(result, args.detail_out)


def full_measurements(args, spi, zoo, rtmod, dist, h, model, replica, result, value, per_step, dev, rank, world):
    """`--full`: everything the benchmark reports beside the headline figure, added to `result`."""
    # stability evidence: the same K-step region re-timed (not `value`, which is the first region)
    repeats = [world * per_step * args.steps / h.throughput(args.steps, 0, args.tasks_per_step, world, dist)
               for _ in range(args.repeats)]
    task_lat = h.loaded_latency(20)
    result["value_repeats"] = [round(v, 1) for v in repeats]
    result["p50_task_latency_ms"] = round(percentile(task_lat, 50), 4)
    result["p95_task_latency_ms"] = round(percentile(task_lat, 95), 4)
    if rank == 0:
        result["model_gflop_per_inference"] = round(replica.flops(1) / 1e9, 4)
        result["model_tflops_per_gpu"] = round(replica.flops(1) * value / world / 1e12, 3)
        result["roofline"] = roofline(h, args.precision, args.model, args.roofline_reps)
        # the next ops of the timed loop's trace, each timed the same way (e.g. the layer-1 conv)
        ranking, _ = trace_ranking(args.model, args.batch, args.precision)
        nxt = []
        for r in ranking[1:3]:
            rl = roofline(h, args.precision, args.model, args.roofline_reps, name=r["op"].split("|")[0])
            nxt.append({k: rl[k] for k in ("kernel", "avg_launch_ms", "achieved", "frac") if k in rl} |
                       {"share_of_device_time": float(r["share"])})
        if nxt:
            result["roofline_next_ops"] = nxt
    # submit -> outputs in host memory, incl. H2D and D2H, through the runtime
    # closed loop on every rank's GPU, 8 requests in flight per worker (the H2D link -- 51 GB/s
    # measured, 85k inf/s of fp32 NCHW bs8 input -- and the compute pipeline both stay busy), and
    # half that load
    if world > 1:
        dist.barrier()
    e2e = aggregate_e2e(runtime_e2e(rtmod, replica, args.model, args.batch, args.e2e_requests,
                                    inflight=8 * args.workers, workers=args.workers), world, dist)
    e2e["fraction_of_device_resident"] = round(e2e["value"] / value, 4)
    e2e["pipeline"] = (f"{args.workers} workers x depth 2 per GPU, H2D {e2e['h2d_mode']} (SPI_H2D_AUTO), pinned slot "
                       f"pool of {2 * args.workers}, 4 host copy threads, every batch size warmed up")
    result["e2e"] = e2e
    if world > 1:
        dist.barrier()
    half = aggregate_e2e(runtime_e2e(rtmod, replica, args.model, args.batch, args.e2e_requests,
                                     inflight=4 * args.workers, workers=args.workers), world, dist)
    result["e2e_half_load"] = {k: half[k] for k in ("value", "unit", "p50_latency_ms", "p95_latency_ms",
                                                    "p99_latency_ms", "requests", "inflight")}
    # The reference's single-process serving shape (starpu_setup.cpp:388-432, inference_runner.cpp:
    # 251-275): ONE runtime over every GPU's replica -- one eager queue, one batcher, the host staging
    # of all devices in one process -- driven by one client loop; rank 0 runs it over devices
    # 0..N-1 while the other ranks wait, so a SCALE run measures the shared-queue path too.
    if world > 1:
        dist.barrier()
    if rank == 0:
        result["e2e_single_process"] = single_process_e2e(spi, zoo, rtmod, args, model, replica, world)
    if world > 1:
        dist.barrier()
    e2e1 = h.serial_e2e(40)
    result["p50_serial_e2e_latency_ms"] = round(percentile(e2e1, 50), 4)

    if rank == 0 and args.cpu_seconds > 0 and args.model == "resnet18":
        result["cpu_baseline"] = cpu_baseline(model, args.model, args.batch, args.cpu_seconds)

    if args.extras and args.model == "resnet18":
        extras = {}
        if world == 1:
            extras.update(single_gpu_extras(spi, zoo, rtmod, args, model, replica, h, dev, per_step))
        # C3 BERT-base seq128 bs8 fp16; C4 ResNet-152 bs32 fp16x3; C5 ViT-L/16 bs16 fp16 -- at every N
        for key, name, b, prec in [("c3_bert_base_seq128_bs8_fp16", "bert_base", 8, "fp16"),
                                   ("c4_resnet152_bs32_fp16x3", "resnet152", 32, "fp16x3"),
                                   ("c5_vit_l_16_bs16_fp16", "vit_l_16", 16, "fp16")]:
            if world > 1:
                dist.barrier()
            extras[key] = config_line(spi, zoo, rtmod, name, b, prec, args.workers, h.streams,
                                      max(10, args.steps // 2), dev, rank, world, dist,
                                      e2e_requests=400 if name != "bert_base" else 1000,
                                      tasks_per_step=args.tasks_per_step)
        result["extras"] = extras


def dump_outputs(h, out_dir, rank, world):
    """What the timed path handed its callers in the last step: every worker's output buffer
    (the codelet's W buffer) as <out_dir>/output[_rank<r>]_worker<w>.npy, float32."""
    os.makedirs(out_dir, exist_ok=True)
    tag = f"_rank{rank}" if world > 1 else ""
    for w, out in enumerate(h.d_out):
        np.save(os.path.join(out_dir, f"output{tag}_worker{w}.npy"), out.float().cpu().numpy())


def _r(x, nd=4):
    return None if x is None else round(float(x), nd)


def compact_line(full: dict) -> dict:
    """The driver-parsed line: the bench contract's keys plus the metric's own shapes (ResNet-18
    bs=1 rate and p50, C3 BERT-base, C4, C5, the CI workload), short enough (< 2000 bytes) for
    the driver's tail to hold it whole.  Everything else is in the detail
    file (`detail`)."""
    out = {k: full[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
                                "higher_is_better", "scaling", "vs_baseline", "dtype") if k in full}
    out["data"] = "synthetic, random-init weights"
    cfg = full.get("config", {})
    out["config"] = {"workload": cfg.get("workload"), "batch_per_task": cfg.get("batch_per_task"),
                     "workers_per_gpu": cfg.get("workers_per_gpu"), "tasks_per_step": cfg.get("tasks_per_step"),
                     "parallelism": cfg.get("parallelism")}
    rl = full.get("roofline")
    if rl:
        out["roofline"] = {k: rl.get(k) for k in ("bound", "achieved", "peak", "unit", "frac")}
        out["roofline"].update({"traffic": rl.get("traffic"), "kernel": rl.get("kernel"),
                                "avg_launch_ms": rl.get("avg_launch_ms"), "frac_rocprof": rl.get("frac_rocprof"),
                                "mfma_busy_pct": rl.get("mfma_busy_pct")})
    cb = full.get("cpu_baseline")
    if cb:
        out["cpu_baseline"] = {k: cb.get(k) for k in ("value", "unit", "cores", "kind")}
        out["cpu_baseline"]["sample"] = cb.get("sample_short", cb.get("sample"))
        host = cb.get("host", {})
        out["cpu_baseline"].update({"nproc": host.get("nproc"), "numa_nodes": host.get("numa_nodes"),
                                    "layouts": cb.get("layouts_summary")})
    e2e = full.get("e2e")
    if e2e:
        out["e2e"] = {"value": e2e.get("value"), "p50_ms": e2e.get("p50_latency_ms"),
                      "p99_ms": e2e.get("p99_latency_ms")}
    if "p50_task_latency_ms" in full:
        out["p50_task_latency_ms"] = full["p50_task_latency_ms"]
    ex = full.get("extras", {})
    b1 = ex.get("resnet18_bs1_tasks")
    if b1:
        out["resnet18_bs1"] = {"value": b1.get("value"), "p50_task_ms": b1.get("p50_task_latency_ms"),
                               "p50_serial_e2e_ms": b1.get("p50_serial_e2e_latency_ms")}
    for key, short in (("c3_bert_base_seq128_bs8_fp16", "c3_bert"), ("c4_resnet152_bs32_fp16x3", "c4_resnet152"),
                       ("c5_vit_l_16_bs16_fp16", "c5_vit_l")):
        c = ex.get(key)
        if c:
            e = c.get("e2e", {})
            out[short] = {"value": c.get("value"), "dtype": c.get("dtype"),
                          "p50_task_ms": c.get("p50_task_latency_ms"), "e2e": e.get("value"),
                          "e2e_p50_ms": e.get("p50_latency_ms"), "frac": (c.get("roofline") or {}).get("frac")}
    ci = ex.get("ci_perf_resnet152_schedule")
    if ci:
        t = ci.get("mi355x_tuned", {})
        out["ci_perf"] = {"value": ci.get("value"), "p50_ms": ci.get("p50_latency_ms"),
                          "tuned_value": t.get("value"), "tuned_p50_ms": t.get("p50_latency_ms")}
    return out


def emit(full: dict, detail_path: str) -> None:
    """Rank 0: the full record to `detail_path`, then ONE compact JSON line on stdout."""
    line = compact_line(full)
    if detail_path:
        try:
            os.makedirs(os.path.dirname(os.path.abspath(detail_path)), exist_ok=True)
            with open(detail_path, "w") as f:
                json.dump(full, f)
            line["detail"] = detail_path
        except OSError as e:  # the line must still go out
            line["detail_error"] = str(e)
    print(json.dumps(line, separators=(",", ":")), flush=True)


def control_plane_only(args, rank, world, dist):
    """The multi-rank control path with the GPU work replaced by a sleep of (rank + 1) ms per
    step: value must come from the slowest rank's window, e2e from the aggregation."""
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    time.sleep(args.steps * (rank + 1) * 1e-3)
    elapsed = reduce_max_elapsed(time.perf_counter() - t0, world)
    if world > 1:
        dist.barrier()
    per_step = args.workers * args.tasks_per_step * args.batch
    local = {"value": 1000.0 * (rank + 1), "unit": "inferences/s", "requests": 100, "request_batch": args.batch,
             "seconds": 0.1 * (rank + 1), "failed": 0, "rejected": 0, "p50_latency_ms": 1.0 + rank,
             "p95_latency_ms": 2.0 + rank, "p99_latency_ms": 3.0 + rank}
    e2e = aggregate_e2e(local, world, dist)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps({"metric": BASELINE_METRIC, "value": round(world * per_step * args.steps / elapsed, 2),
                          "n_gpus": world, "steps": args.steps, "ms_per_step": round(elapsed * 1e3 / args.steps, 4),
                          "e2e": e2e, "control_plane_only": True}), flush=True)


def single_gpu_extras(spi, zoo, rtmod, args, model, replica, h, dev, per_step):
    """Rank 0 at N = 1: the headline workload in the other precision modes, ResNet-18 bs1, bs1
    requests batched by the runtime, and the reference's own CI perf workload."""
    extras = {}
    # the same workload in the other modes: fp16x3 (fp32-grade, ~2e-6) and plain fp16
    # operands everywhere (1.8e-3 .. 2.0e-3: misses the 1e-3 bar, never the C2 figure)
    for prec in [p for p in ("fp16x3", "fp16") if p != args.precision]:
        rp = spi.ModelReplica(model, dev, prec, max_batch=args.batch, graphs=True)
        hp = Harness(spi, rp, "resnet18", dev, args.batch, args.workers, np.random.default_rng(1), h.streams)
        el = hp.throughput(args.steps, 2, args.tasks_per_step)
        extras[f"resnet18_bs8_{prec}"] = {
            "value": round(per_step * args.steps / el, 2), "unit": "inferences/s",
            "p50_task_latency_ms": round(percentile(hp.loaded_latency(10), 50), 4),
            "parity": "fp32-grade (1.6e-6 .. 3.2e-6)" if prec == "fp16x3" else
                      "1.8e-3 .. 2.0e-3 normalised max error: misses the 1e-3 bar, not a C2 result"}
        del rp, hp
    # ResNet-18 bs=1 (the metric names it): device-resident tasks, and bs1 requests served
    r1 = spi.ModelReplica(model, dev, args.precision, max_batch=1, graphs=True)
    h1 = Harness(spi, r1, "resnet18", dev, 1, args.workers, np.random.default_rng(2), h.streams)
    el = h1.throughput(args.steps, 2, args.tasks_per_step)
    lat1 = h1.loaded_latency(20)
    ser1 = h1.serial_e2e(40)
    extras["resnet18_bs1_tasks"] = {
        "value": round(args.workers * args.tasks_per_step * args.steps / el, 2), "unit": "inferences/s",
        "p50_task_latency_ms": round(percentile(lat1, 50), 4),
        "p50_serial_e2e_latency_ms": round(percentile(ser1, 50), 4), "dtype": args.precision}
    del r1, h1
    # bs1 client requests batched server-side into codelet calls of <= 8: closed loop, and the
    # bursty open-loop schedule shaped like ci/perf/ci_perf_resnet.csv (delta_us x repeat, time
    # scaled by 1/10 for ResNet-18), fixed coalescer vs adaptive strategy
    # (round 4: 48000 requests after 4000 untimed ones -- ~0.7 s; the round-3 window of 6000 was
    # ~0.1 s, short enough for start-up transients to set its p99 and the spread across boxes)
    extras["resnet18_bs1_requests_closed_loop_adaptive"] = runtime_e2e(
        rtmod, replica, "resnet18", args.batch, 48000, inflight=64, req_batch=1, warmup=4000,
        batching=rtmod.batching_config("adaptive", 1, args.batch, coalesce_timeout_us=200, congestion=True,
                                       tick_us=500, entry_horizon_us=3000, exit_horizon_us=7000))
    sched = [(170, 3000), (30, 300), (300, 3000)]
    for label, kw in [("fixed", dict(coalesce_max_jobs=args.batch, coalesce_delay_us=500)),
                      ("adaptive", dict(batching=rtmod.batching_config(
                          "adaptive", 1, args.batch, coalesce_timeout_us=500, congestion=True, tick_us=500,
                          entry_horizon_us=3000, exit_horizon_us=7000)))]:
        key = f"resnet18_bs1_requests_bursty_schedule_{label}"
        extras[key] = runtime_e2e(rtmod, replica, "resnet18", args.batch, 0, inflight=256, req_batch=1,
                                  max_queue=256, schedule=sched, **kw)
        extras[key]["schedule_delta_us_repeat"] = sched
    if args.ci_schedule:
        extras["ci_perf_resnet152_schedule"] = ci_perf_workload(spi, zoo, rtmod, dev, args.workers)
    return extras


def ci_perf_workload(spi, zoo, rtmod, dev, workers):
    """The reference's own perf workload (.github/workflows/ci.yml:625-739 perf-smoke):
    ResNet-152, bs1 requests on the ci/perf/ci_perf_resnet.csv schedule at its real intervals
    (1700 us x 3000, 300 us x 300, 3000 us x 3000 = 6300 requests), served as
    ci/perf/resnet152_ci_perf_gpu_only.yml configures it: adaptive batching 1..16, congestion
    thresholds fill 0.85 / 0.65 with 3000 / 7000 ms horizons on a 500 ms tick, 10 ms coalesce
    timeout, queue 100, pool of 12 slots, STARPU_CUDA_PIPELINE 4, 4 workers.  Precision fp16x3
    (ResNet-152's parity-grade mode, C4)."""
    m = zoo.build("resnet152", seed=0)
    rep = spi.ModelReplica(m, dev, "fp16x3", max_batch=16, graphs=True)
    sched = [(1700, 3000), (300, 300), (3000, 3000)]
    b = rtmod.batching_config("adaptive", 1, 16, coalesce_timeout_us=10_000, congestion=True, tick_us=500_000,
                              entry_horizon_us=3_000_000, exit_horizon_us=7_000_000, fill_high=0.85, fill_low=0.65)
    out = runtime_e2e(rtmod, rep, "resnet152", 16, 0, inflight=256, req_batch=1, workers=workers, schedule=sched,
                      max_queue=100, slots_per_device=12, pipeline_depth=4, batching=b)
    out.update({"schedule_delta_us_repeat": sched, "expected_requests": 6300, "dtype": "fp16x3",
                "config": "ci/perf/resnet152_ci_perf_gpu_only.yml (adaptive 1..16, queue 100, pool 12, pipeline 4)"})
    # This build's MI355X tuning beside it: the same strategy and limits, but an idle worker
    # dispatches what is queued at once instead of waiting out the 10 ms coalescer
    # (spi_batching_config.idle_dispatch; batches still form while every worker is busy).
    bt = rtmod.batching_config("adaptive", 1, 16, coalesce_timeout_us=10_000, congestion=True, tick_us=500_000,
                               entry_horizon_us=3_000_000, exit_horizon_us=7_000_000, fill_high=0.85, fill_low=0.65,
                               idle_dispatch=True)
    tuned = runtime_e2e(rtmod, rep, "resnet152", 16, 0, inflight=256, req_batch=1, workers=workers, schedule=sched,
                        max_queue=100, slots_per_device=12, pipeline_depth=4, batching=bt)
    tuned["config"] = "as above + idle_dispatch (MI355X tuning: no coalescing wait on an idle worker)"
    out["mi355x_tuned"] = tuned
    del rep, m
    return out


if __name__ == "__main__":
    main()

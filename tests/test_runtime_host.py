"""The mini-runtime's host-only parts on the CPU: `make runtime_check` builds the stand-alone program
(copy pool, job queue and batch composition, configuration resolver, batching strategy, load-generator
statistics; csrc/runtime_check.cpp) under the address + undefined-behaviour sanitizers and under the
thread sanitizer, and runs both."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = ("copy_pool", "job_queue", "runtime_config", "batching", "loadgen_stats")


def test_make_runtime_check():
    csrc = os.path.join(ROOT, "starpu-inference-server_amd", "csrc")
    r = subprocess.run(["make", "-C", csrc, "runtime_check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    for build in ("asan+ubsan", "tsan"):
        for group in GROUPS:
            assert f"runtime_check {build} {group} ok" in lines, r.stdout[-2000:]
    assert "MISMATCH" not in r.stdout

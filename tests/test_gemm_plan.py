"""The GEMM planner (csrc/gemm_plan.cpp) without a GPU: its three debug exports against the
recorded table tests/golden/gemm_plans.json (tests/golden/make_gemm_plans.py), and the table's
own consistency."""
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_gemm_plans", os.path.join(HERE, "golden", "make_gemm_plans.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

PLAN = ("bm", "bn", "stages", "splits", "halo", "win", "nw", "k_per_split")


@pytest.fixture(scope="module")
def table():
    with open(os.path.join(HERE, "golden", "gemm_plans.json")) as f:
        return json.load(f)


def settings_of(table):
    """(env, {case: expected ints}) per knob setting: a setting records only what differs from the default."""
    for i, env in enumerate(table["settings"]):
        yield env, {**table["default"], **table["overrides"].get(str(i), {})}


def test_table_covers_the_generator_cases(table):
    assert table["settings"] == gen.SETTINGS
    assert sorted(table["default"]) == sorted(gen.conv_cases() + gen.dense_cases() + gen.pair_cases())
    assert not any("SPI_GEMM_PLAN_LONGK" in env for env in table["settings"])


def test_planner_matches_table(spi, table):
    """Every case under every knob setting the GPU suite uses: exactly the recorded integers."""
    saved = {k: os.environ.get(k) for k in gen.KNOBS}
    bad = []
    try:
        for env, want in settings_of(table):
            gen.apply_setting(spi.lib, env)
            for case, ints in want.items():
                got = gen.query(spi.lib, case)
                if got != ints:
                    bad.append((env, case, got, ints))
    finally:
        gen.apply_setting(spi.lib, {k: v for k, v in saved.items() if v is not None})
    assert not bad, f"{len(bad)} plans differ from the table, first (env, case, got, recorded): {bad[:5]}"


def plan_use(case_args, pl):
    """(tiles, slab floats, tickets) of a conv under one 8-field plan; halo plans tile by bands."""
    B, H, cout, k, stride, pad = case_args
    oh = (H + 2 * pad - k) // stride + 1
    tiles = -(-B * oh * oh // pl["bm"]) * -(-cout // pl["bn"])
    split = pl["splits"] > 1
    return tiles, (tiles * pl["splits"] * pl["bm"] * pl["bn"] if split else 0), (tiles if split else 0)


def test_table_is_consistent(table):
    """Workspace figures follow from the plans: slabs = tiles x slices x tile, one ticket per tile
    (gemm256 split-K: two), nothing without split-K; a pair's summed workspace holds its joint plans
    and problem 1 starts where problem 0's slabs and tickets end."""
    for env, want in settings_of(table):
        for case, v in want.items():
            kind, args = case.split(":")
            a = [int(x) for x in args.split(",")]
            if kind == "d":
                _, M, N, _, _, _, pool, _ = a
                g_bm, g_sp = v[0], v[1]
                pl = dict(zip(PLAN, v[4:12]))
                floats = slots = 0
                if pl["splits"] > 1:
                    assert not pl["halo"]
                    tiles = (M // pool if pool else -(-M // pl["bm"])) * -(-N // pl["bn"])
                    floats, slots = tiles * pl["splits"] * pl["bm"] * pl["bn"], tiles
                if g_bm and g_sp > 1:
                    tiles = -(-M // g_bm) * (N // 256)
                    floats, slots = max(floats, tiles * g_sp * g_bm * 256), max(slots, 2 * tiles)
                assert g_bm in (0, 128, 256) and (g_bm or g_sp == 1), (env, case, v)
                assert v[12:] == [floats, slots], (env, case, v)
            elif kind == "p":
                _, B, H, _, c0, k0, s0, p0, c1, k1, s1, p1 = a
                q0, q1 = dict(zip(PLAN, v[:8])), dict(zip(PLAN, v[8:16]))
                grouped, wgs, slab_off, ticket_off, floats, slots = v[16:]
                if q0["halo"] or q1["halo"]:
                    assert not grouped, (env, case, v)
                    continue
                t0, f0, n0 = plan_use((B, H, c0, k0, s0, p0), q0)
                t1, f1, n1 = plan_use((B, H, c1, k1, s1, p1), q1)
                assert wgs == t0 * q0["splits"] + t1 * q1["splits"], (env, case, v)
                if grouped:  # one launch: problem 1 behind problem 0 in one workspace
                    assert (slab_off, ticket_off) == (f0, n0), (env, case, v)
                    assert floats >= f0 + f1 and slots >= n0 + n1, (env, case, v)
                    assert (q0["bm"], q0["bn"], q0["stages"]) == (q1["bm"], q1["bn"], q1["stages"]), (env, case, v)
                    assert not q0["win"] and not q1["win"], (env, case, v)
                else:  # two launches, each from the start of the workspace
                    assert (slab_off, ticket_off) == (0, 0), (env, case, v)
                    assert floats >= max(f0, f1) and slots >= max(n0, n1), (env, case, v)


def test_pair_fallback_is_pinned(table):
    """A window-kind 3x3/s1 conv shares no kernel instance with a 1x1 tap walk: two launches."""
    assert table["default"]["p:1,8,28,128,128,3,1,1,256,1,1,0"][16] == 0
    assert table["default"]["p:1,8,28,128,256,3,2,1,256,1,2,0"][16] == 1


def test_gemm256_refuses_what_it_has_no_instance_for(table):
    """Under SPI_GEMM_256_MIN=1 every eligible desc routes to gemm256: an activation over an fp32
    residual, a residual LayerNorm, krep = 2 and an unaligned lda must stay on the general kernel."""
    i = table["settings"].index({"SPI_GEMM_256_MIN": "1"})
    want = {**table["default"], **table["overrides"][str(i)]}
    assert want["d:1,1024,3072,768,768,1,0,0"][0] == 256
    assert want["d:1,1024,3072,768,768,1,0,%d" % (gen.RES_F32 | gen.OUT_F32)][0] == 256
    assert want["d:1,1024,3072,768,768,1,0,%d" % (gen.RES_PLANES | gen.OUT_PLANES)][0] == 256
    assert want["d:1,1024,3072,768,768,1,0,%d" % (gen.RES_F32 | gen.OUT_F32 | gen.ACT)][0] == 0
    assert want["d:1,1024,3072,768,768,1,0,%d" % (gen.RES_F32 | gen.OUT_F32 | 48 << 16)][0] == 0
    assert want["d:1,1024,3072,768,768,2,0,0"][0] == 0
    assert want["d:1,1024,3072,768,772,1,0,0"][0] == 0


@pytest.mark.parametrize("chunks,bm", [(12, 256), (16, 256), (1, 0), (3, 0), (18, 0)])
def test_gemm256_ln_chunk_guard(spi, chunks, bm):
    """gemm256's LayerNorm consumer fold reads an even chunk count in 2..16 (D = 768: 12, D = 1024:
    16); a folded-consumer desc with any other count keeps the general kernel, which handles it."""
    saved = {k: os.environ.get(k) for k in gen.KNOBS}
    try:
        gen.apply_setting(spi.lib, {})
        K = 64 * chunks
        got = gen.query(spi.lib, f"d:1,32768,256,{K},{K},1,0,{chunks << 8}")  # 128 tiles of 256 x 256
        plain = gen.query(spi.lib, f"d:1,32768,256,{K},{K},1,0,0")
    finally:
        gen.apply_setting(spi.lib, {k: v for k, v in saved.items() if v is not None})
    assert plain[0] == 256 and got[0] == bm, (chunks, got, plain)


POOLED_FORCED = ["128,128,2,1", "128,64,2,1", "128,64,3,1", "64,64,2,1", "64,64,3,2", "64,64,4,1"]


@pytest.mark.parametrize("plan", POOLED_FORCED)
def test_forced_plan_on_a_pooled_gemm(spi, plan):
    """A pooled problem (avgpool + FC, pool_rows) under SPI_GEMM_PLAN takes the forced tile, ring depth and
    split: every dense instance compiles the pooled epilogue (gemm_tile.hpp's static_assert), so none falls
    through to the ordinary [M][N] store.  One image per tile row whatever the tile height: tiles = B x
    ceil(N / bn), and a forced split's slabs and tickets are sized from that."""
    bm, bn, stages, splits = (int(v) for v in plan.split(","))
    saved = {k: os.environ.get(k) for k in gen.KNOBS}
    try:
        gen.apply_setting(spi.lib, {"SPI_GEMM_PLAN": plan})
        for prec, ksteps in ((0, 16), (1, 8), (2, 16), (3, 16)):
            v = gen.query(spi.lib, f"d:{prec},21,70,512,512,1,7,{gen.OUT_F32}")  # B = 3, HW = 7, C = 512, N = 70
            pl = dict(zip(PLAN, v[4:12]))
            want = splits if bn == 64 else 1
            assert (v[0], pl["bm"], pl["bn"], pl["stages"], pl["splits"]) == (0, bm, bn, stages, want), (plan, v)
            assert pl["k_per_split"] * want == ksteps * (64 if prec == 1 else 32), (plan, v)
            tiles = 3 * -(-70 // bn)
            assert v[12:] == ([tiles * want * bm * bn, tiles] if want > 1 else [0, 0]), (plan, v)
    finally:
        gen.apply_setting(spi.lib, {k: v for k, v in saved.items() if v is not None})


def test_forced_split_of_a_pooled_gemm_must_fit_the_op_workspace(spi):
    """The plan rule never splits a pooled GEMM, so spi_op_avgpool_fc used to skip the workspace check; a forced
    8-way split of B = 65, N = 1000 needs 65 x 16 x 8 slabs of 64 x 64 floats, twice the op workspace's 16 Mi
    floats.  Refused before anything is launched (the pointers here are never dereferenced)."""
    import ctypes as C

    from importlib import import_module
    native = import_module("starpu-inference-server_amd._native")
    saved = {k: os.environ.get(k) for k in gen.KNOBS}
    fake = [C.c_void_p(0x10000000 * i) for i in range(1, 6)]
    try:
        gen.apply_setting(spi.lib, {"SPI_GEMM_PLAN": "64,64,2,8", "SPI_GEMM_MAXSPLIT": "0"})
        v = gen.query(spi.lib, f"d:0,260,1000,512,512,1,4,{gen.OUT_F32}")
        assert v[7] == 8 and v[12] == 65 * 16 * 8 * 64 * 64 > 16 << 20, v
        rc = spi.lib.spi_op_avgpool_fc(0, fake[0], 65, 4, 512, fake[1], 1000, fake[2], fake[3], 0, fake[4], None)
        assert rc != 0 and "too large for the op workspace" in native.last_error()
    finally:
        gen.apply_setting(spi.lib, {k: v for k, v in saved.items() if v is not None})

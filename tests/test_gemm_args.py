"""The host side of a general-kernel launch (csrc/gemm_args.cpp) without a GPU, through its debug
exports: the kernel arguments against tests/golden/gemm_args.json (recorded before make_args moved out
of the kernel file), the workgroup -> (tile, slice) map of every recorded case, walked through the
decode the kernels themselves call (csrc/gemm_args.hpp), and what validate_gemm refuses."""
import ctypes as C
import importlib.util
import itertools
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_gemm_args", os.path.join(HERE, "golden", "make_gemm_args.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def table():
    with open(os.path.join(HERE, "golden", "gemm_args.json")) as f:
        return json.load(f)["cases"]


@pytest.fixture(scope="module")
def lib(spi):
    """The library under the default knob setting."""
    saved = {k: os.environ.get(k) for k in gen.plans.KNOBS}
    gen.plans.apply_setting(spi.lib, {})
    yield spi.lib
    gen.plans.apply_setting(spi.lib, {k: v for k, v in saved.items() if v is not None})


def test_table_covers_the_generator_cases(table):
    assert sorted(table) == sorted(gen.cases())
    with open(os.path.join(HERE, "golden", "gemm_plans.json")) as f:
        assert set(json.load(f)["default"]) <= set(table)


def test_arguments_match_the_recorded_digests(lib, table):
    """Every field make_args fills, for aligned pointers and for a C that is not: exactly as recorded."""
    bad = []
    for case, want in table.items():
        d0, info, _ = gen.query(lib, case)
        d1, _, _ = gen.query(lib, case, unaligned_c=1)
        if [d0, d1] + info != want:
            bad.append((case, [d0, d1] + info, want))
    assert not bad, f"{len(bad)} cases differ from the table, first (case, got, recorded): {bad[:3]}"
    assert all(v[0] != v[1] for v in table.values()), "an unaligned C must flip vec_ok"


def test_edge_cases_reach_their_edges(table):
    """The hand cases are in the table for the grid they give; a plan change that moves one shows here."""
    for case, want in gen.EDGES.items():
        assert tuple(table[case][2:]) == want, case
    grids = list(gen.EDGES.values())
    assert any(tm * tn < 16 and s == 1 for tm, tn, s, _, _ in grids)
    assert any(tm * tn == 16 and s == 1 for tm, tn, s, _, _ in grids)
    assert any(tm * tn > 16 and tm * tn % 8 and s == 1 for tm, tn, s, _, _ in grids)
    assert {3, 7} <= {s for _, _, s, _, _ in grids}
    assert {2, 4, 8} <= {xm for tm, _, _, xm, _ in grids if tm % xm}


def full_grid(tm, tn, splits):
    return sorted(itertools.product(range(tm), range(tn), range(splits)))


def test_every_workgroup_decodes_to_its_own_tile(lib, table):
    """In launch order, the workgroups of a launch visit [0, tiles_m) x [0, tiles_n) x [0, splits)
    exactly once each: no tile is missed, no split-K ticket short of its slices.  A grouped pair's
    first wgs0 workgroups are problem 0, the rest problem 1; an ungrouped pair is two such launches."""
    for case in table:
        _, info, wmap = gen.query(lib, case, with_map=True)
        if not case.startswith("p:"):
            tm, tn, splits = info[:3]
            assert len(wmap) == tm * tn * splits and sorted(wmap) == full_grid(tm, tn, splits), case
            continue
        wgs0, wgs = info[11], info[12]
        assert len(wmap) == wgs, case
        assert all(w[0] == 0 for w in wmap[:wgs0]) and all(w[0] == 1 for w in wmap[wgs0:]), case
        assert sorted(w[1:] for w in wmap[:wgs0]) == full_grid(*info[0:3]), case
        assert sorted(w[1:] for w in wmap[wgs0:]) == full_grid(*info[5:8]), case


OUT_F32, OUT_PLANES, LN_IN_12 = gen.plans.OUT_F32, gen.plans.OUT_PLANES, 12 << 8


@pytest.mark.parametrize("case,message", [
    # precision, M, N, K, lda, krep, pool_rows, flags
    ((0, 64, 128, 768, 768, 2, 0, 0),
     "krep = 2 needs F16, a packed Kpad of whole step pairs and dense or one-tap-per-step A"),
    ((1, 100, 128, 768, 768, 1, 49, OUT_F32), "pooled GEMM: dense A, pool_rows <= 64 dividing M"),
    ((1, 64, 192, 768, 768, 1, 0, LN_IN_12), "LayerNorm fold: dense fp16 GEMM, N % 128 == 0, aligned vectors"),
    ((1, 64, 128, 768, 768, 1, 0, OUT_PLANES | OUT_F32),
     "two-plane residual / output: dense fp16 GEMM, plane offset a multiple of 8"),
])
def test_validate_gemm_refuses(lib, case, message):
    msg = C.create_string_buffer(256)
    assert lib.spi_debug_validate_gemm(*case[:7], C.c_uint(case[7]), msg, len(msg)) == 2
    assert msg.value.decode() == message


@pytest.mark.parametrize("case", [
    (1, 64, 128, 768, 768, 2, 0, 0), (1, 98, 128, 768, 768, 1, 49, OUT_F32), (1, 64, 256, 768, 768, 1, 0, LN_IN_12),
    (1, 64, 128, 768, 768, 1, 0, OUT_PLANES | gen.plans.RES_PLANES),
])
def test_validate_gemm_accepts_the_neighbouring_desc(lib, case):
    """The same four rules on a desc that meets them: the refusals above are the rule's, not the export's."""
    msg = C.create_string_buffer(256)
    assert lib.spi_debug_validate_gemm(*case[:7], C.c_uint(case[7]), msg, len(msg)) == 0, msg.value

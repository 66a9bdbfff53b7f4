"""A replica's host-only forward plan (csrc/model_plan.cpp) without a GPU: the workspace sizes and flops(3)
against the table recorded from the sizing code the plan replaced (tests/golden/workspace_plans.json,
tests/golden/make_workspace_plans.py), and the walk of every forward against the planned workspace
(spi_model_plan_check: the checks each launch makes, with no launch)."""
import ctypes as C
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_workspace_plans",
                                               os.path.join(HERE, "golden", "make_workspace_plans.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

# Cases whose slab floats before the floor may exceed the recorded ones, each with the GemmDesc field --
# on the sizing desc since it is the launched one -- that changes the planned route.  None does: the
# fields the launches add (act, out_f32, res_f32, the planes, the LayerNorm-fold chunks) move no small
# model onto a route with larger slabs.
LARGER_PLANNED = {}


@pytest.fixture(scope="module")
def table():
    with open(os.path.join(HERE, "golden", "workspace_plans.json")) as f:
        return json.load(f)


def test_table_covers_the_generator_cases(table):
    assert sorted(table["cases"]) == sorted(gen.cases())
    assert len(gen.cases()) == (5 * 4 * 3 + 4) + 3 * 2 * 2 + 2 + 3 * 4 + 3 * 3
    assert set(LARGER_PLANNED) <= set(table["cases"])


@pytest.mark.parametrize("model", list(gen.MODELS))
def test_plan_matches_table(spi, zoo, table, model):
    """Every case of one model: the bytes of every buffer, the slab floats and flops(3) exactly as recorded;
    the slab floats before the floor too, but for LARGER_PLANNED's cases, which may only be larger."""
    want = {c: v for c, v in table["cases"].items() if c.split("|")[0] == model}
    assert want
    got = gen.record_all(spi, zoo, want=set(want))
    bad = {}
    for c, (sizes, slabs, planned, flops3) in want.items():
        g = got.get(c)
        ok = g is not None and g[0] == sizes and g[1] == slabs and g[3] == flops3
        ok = ok and (g[2] >= planned if c in LARGER_PLANNED else g[2] == planned)
        if not ok:
            bad[c] = (g, want[c])
    assert not bad, f"{len(bad)} plans differ from the table, (got, recorded): {bad}"


def test_options_change_the_sizes_where_expected(table):
    """The table's own consistency: the logits scratch and the resampled image appear with their option
    only, SPI_BERT_NO_HIDDEN adds the class-token rows, and flops(3) is three times the digest table's
    flops(1) (every term scales with the batch)."""
    cases = table["cases"]
    with open(os.path.join(HERE, "golden", "replica_digests.json")) as f:
        flops1 = {c + "|": v[3] for c, v in json.load(f)["cases"].items()}
    for c, f1 in flops1.items():
        assert cases[c][3] == 3 * f1, c
    for m in gen.IMAGE_MODELS:
        for p in ("fp32", "fp16"):
            plain, nol, rsz = (cases[f"{m}|{p}||{o}"][0] for o in ("", "no_logits", "resize"))
            image = gen.MODELS[m][1]["image_size"]
            classes = 10 if m.startswith("vit") else 1000
            assert plain[-2:] == [0, 0] and nol[-2:] == [8 * classes * 4, 0], (m, p)
            assert rsz[-2:] == [0, 8 * 3 * image * image * 4] and rsz[:-2] == plain[:-2] == nol[:-2], (m, p)
    for p in ("fp32", "fp16"):
        plain, noh = cases[f"bert_d128|{p}||"][0], cases[f"bert_d128|{p}||no_hidden"][0]
        assert plain[-1] == 0 and noh[-1] == 8 * 128 * 4 and plain[:-1] == noh[:-1], p


def _steps(spi, rep, B, S):
    n = C.c_int32(-1)
    st = spi.lib.spi_model_plan_check(rep.handle, B, S, C.byref(n))
    return st, n.value, spi.lib.spi_last_error().decode()


@pytest.mark.parametrize("model", [m for m in gen.MODELS if m not in gen.base.FULL])
def test_workspace_holds_every_launch(spi, zoo, model):
    """Every case of one model at every batch 1 .. max_batch (BERT: sequence lengths 1, 17 and seq): each
    GEMM, conv and conv pair of the forward fits the planned split-K workspace.  The small BERTs serve
    at most seq = 16 tokens, so 17 is walked on the same weights packed for seq_len = 32 (their
    max_position)."""
    module = gen.base.filled(spi, gen.MODELS[model][0](zoo))
    bert = model.startswith("bert")
    bad = []
    for case in [c for c in gen.cases() if c.split("|")[0] == model]:
        reps = [gen.replica(spi, module, case)]
        if bert and gen.MODELS[model][1]["seq_len"] < 17:
            saved = gen.MODELS[model]
            gen.MODELS[model] = (saved[0], dict(saved[1], seq_len=32))
            try:
                reps.append(gen.replica(spi, module, case))
            finally:
                gen.MODELS[model] = saved
        for rep, seq in zip(reps, (gen.MODELS[model][1].get("seq_len", 0), 32)):
            lengths = sorted({s for s in (1, 17, seq) if s <= seq}) if bert else [0]
            for B in range(1, rep.max_batch + 1):
                for S in lengths:
                    st, n, err = _steps(spi, rep, B, S)
                    if st != 0 or n < 1:
                        bad.append((case, B, S, st, err))
    assert not bad, bad


def test_plan_check_refuses_what_no_forward_takes(spi, zoo):
    module = gen.base.filled(spi, gen.MODELS["bert_d128"][0](zoo))
    rep = gen.replica(spi, module, "bert_d128|fp16||")
    for B, S in ((0, 16), (9, 16), (1, 0), (1, 17)):
        st, n, err = _steps(spi, rep, B, S)
        assert st != 0 and "plan_check" in err, (B, S, st, err)
    assert spi.lib.spi_model_plan_check(None, 1, 1, C.byref(C.c_int32())) != 0

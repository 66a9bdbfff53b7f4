"""The weight packer (csrc/model_pack.cpp) without a GPU: host-only replicas against the recorded
table tests/golden/replica_digests.json (tests/golden/make_replica_digests.py), exactly, and the
table's own consistency.  The digest covers the blob's bytes, not the offset tables; the GPU parity
suite covers those."""
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_replica_digests",
                                               os.path.join(HERE, "golden", "make_replica_digests.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def table():
    with open(os.path.join(HERE, "golden", "replica_digests.json")) as f:
        return json.load(f)


def test_table_covers_the_generator_cases(table):
    assert sorted(table["cases"]) == sorted(gen.cases())
    assert len(gen.cases()) == 5 * 4 * 3 + 4


@pytest.mark.parametrize("model", list(gen.MODELS))
def test_packer_matches_table(spi, zoo, table, model):
    """Every case of one model: digest, bytes, description and flops(1) exactly as recorded."""
    want = {c: v for c, v in table["cases"].items() if c.split("|")[0] == model}
    assert want
    got = gen.record_all(spi, zoo, want=set(want))
    bad = {c: (got.get(c), v) for c, v in want.items() if got.get(c) != v}
    assert not bad, f"{len(bad)} replicas differ from the table, (got, recorded): {bad}"


def test_toggles_change_the_blob_where_expected(table):
    """SPI_STEM_FUSED=0 drops the fused stem's weights from the ResNet blobs that carry them (every
    precision but fp32); SPI_LN_FOLD=0 drops the folded copies from the fp16 / fp16m transformers
    with D % 128 == 0; nothing else moves."""
    cases = table["cases"]
    for model in gen.SMALL:
        for prec in gen.PRECISIONS:
            base, nofold, unfused = (cases[f"{model}|{prec}|{e}"][:2] for e in gen.ENVS)
            stem = model.startswith("resnet") and prec != "fp32"
            fold = model in ("bert_d128", "vit_d128") and prec in ("fp16", "fp16m")
            assert (unfused != base) == stem and (nofold != base) == fold, (model, prec)
            assert unfused[1] < base[1] if stem else True, (model, prec)
            assert nofold[1] < base[1] if fold else True, (model, prec)

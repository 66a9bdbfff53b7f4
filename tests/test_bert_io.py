"""BERT sentence outputs and segment ids (spi_model_config.bert_io), host side: what the packer appends
and refuses, and the codelet's I/O contract (Model::check_io) on host-only replicas (device -1), where
check_io runs and the forward cannot."""
import importlib.util
import json
import os
import subprocess

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_spec = importlib.util.spec_from_file_location("make_replica_digests",
                                               os.path.join(HERE, "golden", "make_replica_digests.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

D, S, KW = 128, 16, dict(num_heads=2, seq_len=16)
OUT_COUNT = {"": 1, "pooler": 2, "mean": 2, "pooler|mean": 3, "no_hidden|pooler": 1, "no_hidden|mean": 1,
             "no_hidden|pooler|mean": 2, "token_types": 1}


def bits(spec):
    return tuple(spec.split("|")) if spec else 0


@pytest.fixture(scope="module")
def small(spi, zoo):
    """bert_d128 of the digest table, with the table's closed-form weights."""
    return gen.filled(spi, gen.MODELS["bert_d128"][0](zoo))


def without(spi, module, prefix):
    """The module's tensors minus those whose name contains `prefix`."""
    d = {n: torch.from_numpy(a) for n, a in spi.named_tensors(module) if prefix not in n}

    class Named(torch.nn.Module):
        def named_parameters(self, *a, **k):
            return iter([])

        def named_buffers(self, *a, **k):
            return iter(d.items())
    return Named()


@pytest.mark.parametrize("prec", ["fp32", "fp16", "fp16m"])
def test_bert_io_zero_is_the_recorded_replica(spi, small, prec):
    with open(os.path.join(HERE, "golden", "replica_digests.json")) as f:
        want = json.load(f)["cases"][f"bert_d128|{prec}|"]
    for io in (0, (), None):
        r = spi.ModelReplica(small, -1, prec, bert_io=io, **KW)
        assert ["%016x" % r.weight_digest, r.weight_bytes, r.description, r.flops(1)] == want


def test_bert_io_names_and_ints(spi):
    cd = importlib.import_module("starpu-inference-server_amd.codelet")
    assert cd.bert_io_bits(("pooler", "mean", "no_hidden", "token_types")) == 15
    assert cd.bert_io_bits("mean") == 2 and cd.bert_io_bits(9) == 9 and cd.bert_io_bits(None) == 0
    with pytest.raises(spi.InferenceExecutionException, match="unknown bert_io name"):
        cd.bert_io_bits(("pooler", "cls"))


def test_packing_with_bits_appends(spi, small):
    base = spi.ModelReplica(small, -1, "fp16", **KW)
    pool_bytes, type_bytes = (D * D + D) * 4, 2 * D * 4
    seen = {base.weight_digest}
    for spec, grow, desc in [("pooler", pool_bytes, "out[hidden,pooler] in[ids,mask]"),
                             ("token_types", type_bytes, "out[hidden] in[ids,mask,types]"),
                             ("pooler|token_types", pool_bytes + type_bytes, "out[hidden,pooler] in[ids,mask,types]"),
                             ("no_hidden|pooler|mean", pool_bytes, "out[pooler,mean] in[ids,mask]")]:
        a = spi.ModelReplica(small, -1, "fp16", bert_io=bits(spec), **KW)
        b = spi.ModelReplica(small, -1, "fp16", bert_io=bits(spec), **KW)
        assert a.weight_bytes >= base.weight_bytes + grow, spec
        assert a.weight_bytes <= base.weight_bytes + grow + 3 * 256, spec  # 256-byte lines, nothing else
        assert a.weight_digest == b.weight_digest and a.weight_bytes == b.weight_bytes, spec
        assert a.description == base.description + " " + desc, spec
        pooled = "pooler" in spec
        assert a.flops(3) == base.flops(3) + (2.0 * 3 * D * D if pooled else 0.0), spec
        if spec != "no_hidden|pooler|mean":  # the same blob as "pooler": the outputs are not in it
            assert a.weight_digest not in seen, spec
        seen.add(a.weight_digest)
    # the mean alone appends nothing: the blob is the plain one, the description is not
    m = spi.ModelReplica(small, -1, "fp16", bert_io="mean", **KW)
    assert (m.weight_digest, m.weight_bytes) == (base.weight_digest, base.weight_bytes)
    assert m.description.endswith("out[hidden,mean] in[ids,mask]")


def test_rejected_combinations(spi, zoo, small):
    def refuses(module, io, match, **kw):
        with pytest.raises(spi.InferenceExecutionException, match=match):
            spi.ModelReplica(module, -1, "fp16", bert_io=io, **kw)
    refuses(small, "no_hidden", "SPI_BERT_NO_HIDDEN leaves no output", **KW)
    refuses(small, ("no_hidden", "token_types"), "SPI_BERT_NO_HIDDEN leaves no output", **KW)
    refuses(small, 16, "unknown bits 16", **KW)
    refuses(small, 1 | 32 | 64, "unknown bits 96", **KW)
    refuses(without(spi, small, "pooler.dense"), "pooler", r"needs parameter 'pooler\.dense\.weight'", **KW)
    refuses(without(spi, small, "pooler.dense.bias"), ("pooler", "mean"), r"needs parameter 'pooler\.dense\.bias'", **KW)
    # without the pooler's weights everything but the pooler output still packs
    spi.ModelReplica(without(spi, small, "pooler.dense"), -1, "fp16", bert_io=("mean", "token_types"), **KW)
    resnet = zoo.resnet([1, 1, 1, 1], False, image=64, calibrate=False)
    vit = zoo.vit(image=32, patch=16, layers=2, heads=2, dim=128, mlp_dim=256, num_classes=10)
    for io in ("pooler", "mean", "token_types", ("no_hidden", "mean")):
        refuses(resnet, io, "not a BERT", image_size=64)
        refuses(vit, io, "not a BERT", num_heads=2, image_size=32)
    with pytest.raises(spi.InferenceExecutionException, match="not a BERT"):
        spi.ModelReplica(None, -1, "fp32", family="affine", bert_io="mean")


def hip_call(spi, rep, n_in, out_elems, B=2, seq=S, in_dtypes=None, in_dims=None, out_types=None):
    """spi_hip_inference_func over host buffers; returns (status, message) of the raised error."""
    N = spi._native
    dims = in_dims or [[B, seq]] * n_in
    dts = in_dtypes or [torch.int64] * n_in
    ins = [torch.zeros(int(np.prod(d)), dtype=dt) for d, dt in zip(dims, dts)]
    outs = [torch.zeros(max(n, 1), dtype=torch.float32) for n in out_elems]
    params = spi.make_params([list(d) for d in dims], dts, num_outputs=len(outs), models_gpu=[rep],
                             output_types=out_types or [torch.float32] * len(outs))
    bufs = [spi.tensor_interface(t) for t in ins] + [spi.make_vector_interface(t.data_ptr(), n, 4)
                                                     for t, n in zip(outs, out_elems)]
    with spi.worker_context(0, 0, None):  # replica index = device id
        with pytest.raises(spi.StarPUCodeletException) as e:
            spi.InferenceCodelet.hip_inference_func(bufs, params)
    assert e.value.status in (N.SPI_ERR_INVALID_ARGUMENT, N.SPI_ERR_OUTPUT_MISMATCH, N.SPI_ERR_DEVICE)
    return e.value.status, str(e.value)


def expected_elems(spec, B, seq=S):
    e = [] if "no_hidden" in spec else [B * seq * D]
    return e + [B * D] * (("pooler" in spec) + ("mean" in spec))


@pytest.mark.parametrize("spec", list(OUT_COUNT))
def test_check_io_outputs(spi, small, spec):
    N = spi._native
    rep = spi.ModelReplica(small, -1, "fp16", max_batch=4, bert_io=bits(spec), **KW)
    B = 3
    good = expected_elems(spec, B)
    assert len(good) == OUT_COUNT[spec]
    st, msg = hip_call(spi, rep, 2, good, B=B)  # the contract holds: only the missing device stops it
    assert st == N.SPI_ERR_DEVICE and "host-only replica" in msg, msg
    for wrong in (good + [B * D], good[:-1]):  # one output too many, one too few
        st, msg = hip_call(spi, rep, 2, wrong, B=B)
        assert st == N.SPI_ERR_INVALID_ARGUMENT and "Mismatch between model outputs and StarPU buffers" in msg, msg
    for i in range(len(good)):
        for delta in (-1, 1, B * D):
            wrong = list(good)
            wrong[i] += delta
            st, msg = hip_call(spi, rep, 2, wrong, B=B)
            assert st == N.SPI_ERR_OUTPUT_MISMATCH and "Output buffer size mismatch in bytes" in msg, (i, delta, msg)
        types = [torch.float32] * len(good)
        types[i] = torch.float16
        st, msg = hip_call(spi, rep, 2, good, B=B, out_types=types)
        assert st == N.SPI_ERR_INVALID_ARGUMENT and "Output type mismatch" in msg, msg
    if len(good) > 1 and "no_hidden" not in spec:  # hidden and a pooled output swapped
        st, msg = hip_call(spi, rep, 2, good[::-1], B=B)
        assert st == N.SPI_ERR_OUTPUT_MISMATCH, msg


def test_check_io_third_input(spi, small):
    N = spi._native
    plain = spi.ModelReplica(small, -1, "fp16", max_batch=4, **KW)
    pooled = spi.ModelReplica(small, -1, "fp16", max_batch=4, bert_io="pooler", **KW)
    typed = spi.ModelReplica(small, -1, "fp16", max_batch=4, bert_io="token_types", **KW)
    B, hidden = 2, [2 * S * D]
    for rep, outs in ((plain, hidden), (pooled, hidden + [B * D])):  # refused without the flag
        st, msg = hip_call(spi, rep, 3, outs)
        assert st == N.SPI_ERR_INVALID_ARGUMENT and "model expects 2 input(s), got 3" in msg, msg
    for n_in in (1, 2, 3):  # each input optional from the end
        st, msg = hip_call(spi, typed, n_in, hidden)
        assert st == N.SPI_ERR_DEVICE and "host-only replica" in msg, msg
    st, msg = hip_call(spi, typed, 4, hidden)
    assert st == N.SPI_ERR_INVALID_ARGUMENT and "model expects 3 input(s), got 4" in msg, msg
    for dt in (torch.int32, torch.float32):
        st, msg = hip_call(spi, typed, 3, hidden, in_dtypes=[torch.int64, torch.int64, dt])
        assert st == N.SPI_ERR_INVALID_ARGUMENT and "Input type mismatch" in msg, msg
    for bad in ([B, S - 1], [B, S + 1], [B + 1, S], [B * S], [B, S, 1]):
        st, msg = hip_call(spi, typed, 3, hidden, in_dims=[[B, S], [B, S], bad])
        assert st == N.SPI_ERR_INVALID_ARGUMENT and "Tensor layout mismatch" in msg, (bad, msg)
    # a third buffer one element short of its dims
    ins_dims = [[B, S]] * 3
    ins = [torch.zeros(B * S, dtype=torch.int64) for _ in range(3)]
    out = torch.zeros(hidden[0])
    params = spi.make_params(ins_dims, [torch.int64] * 3, models_gpu=[typed])
    bufs = [spi.tensor_interface(ins[0]), spi.tensor_interface(ins[1]),
            spi.make_vector_interface(ins[2].data_ptr(), B * S - 1, 8), spi.tensor_interface(out)]
    with spi.worker_context(0, 0, None):
        with pytest.raises(spi.StarPUCodeletException, match="Input buffer too small"):
            spi.InferenceCodelet.hip_inference_func(bufs, params)


def test_config_field_replaces_the_padding(spi):
    """Same struct size and ABI version; a zeroed config has bert_io 0 at the old padding's offset."""
    N = spi._native
    assert N.SPI_ABI_VERSION == 1 and N.ModelConfig.bert_io.offset == 36 and N.ModelConfig.bert_io.size == 4
    import ctypes as C
    assert C.sizeof(N.ModelConfig) == 40 and N.ModelConfig().bert_io == 0


def test_make_pack_check():
    """The stand-alone packer program under the host sanitizers, with its bert_io case."""
    csrc = os.path.join(ROOT, "starpu-inference-server_amd", "csrc")
    r = subprocess.run(["make", "-C", csrc, "pack_check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("bert_d128|fp16|bert_io=15 ")]
    assert line and line[0].endswith("out[pooler,mean] in[ids,mask,types]"), r.stdout[-2000:]
    with open(os.path.join(HERE, "golden", "replica_digests.json")) as f:
        want = json.load(f)["cases"]["bert_d128|fp16|"]
    assert f"bert_d128|fp16| {want[0]} {want[1]} {want[2]}" in r.stdout

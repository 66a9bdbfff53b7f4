"""BERT task heads (SPI_BERT_HEAD_SEQUENCE / _TOKEN / _QA), host side: the formula the GPU tests use against
HF's own head models, what the packer appends, describes and refuses, and the codelet's I/O contract
(check_io), the workspace plan and plan_check on host-only replicas (device -1).  The model is bert_d128 of
the digest table with the closed-form weights, plus `classifier.*` and `qa_outputs.*` beside the `bert.` prefix.
"""
import importlib.util
import json
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle.cpu_codelet import normalized_max_error

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_spec = importlib.util.spec_from_file_location("make_replica_digests",
                                               os.path.join(HERE, "golden", "make_replica_digests.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

D, S, L, KW = 128, 16, 5, dict(num_heads=2, seq_len=16)
HEADS = {"seq_head": 128, "token_head": 256, "qa_head": 512}
LABELS = {"seq_head": L, "token_head": L, "qa_head": 2}
POOL_BYTES = (D * D + D) * 4


class Named(torch.nn.Module):
    """A module exposing the tensors of a dict by name."""

    def __init__(self, tensors):
        super().__init__()
        self._d = tensors

    def named_parameters(self, *a, **k):
        return iter([])

    def named_buffers(self, *a, **k):
        return iter(self._d.items())


def tensors_of(spi, module):
    return {n: torch.from_numpy(a) for n, a in spi.named_tensors(module)}


def with_heads(spi, zoo, extra=None, drop=()):
    """bert_d128's filled tensors plus classifier [L,D] and qa_outputs [2,D] with the same closed-form fill;
    `extra`: name -> shape of further tensors; `drop`: substrings of names to leave out."""
    d = tensors_of(spi, gen.filled(spi, gen.MODELS["bert_d128"][0](zoo)))
    shapes = {"classifier.weight": (L, D), "classifier.bias": (L,), "qa_outputs.weight": (2, D), "qa_outputs.bias": (2,)}
    shapes.update(extra or {})
    for name, shape in shapes.items():
        d[name] = torch.from_numpy(gen.fill(name, shape))
    return Named({n: t for n, t in d.items() if not any(x in n for x in drop)})


@pytest.fixture(scope="module")
def small(spi, zoo):
    return with_heads(spi, zoo)


# ---- the formula against HF ------------------------------------------------------------------------


@pytest.mark.parametrize("head", ["sequence", "token", "qa"])
def test_formula_equals_the_hf_head_model(zoo, head):
    """logits = W . x + b in float64 on HF BertModel's own outputs (x = pooler_output for the sequence head,
    last_hidden_state for the token and QA heads) equals the HF head model's output within 1e-6 normalised."""
    B, seq = 3, 17
    m = zoo.bert(layers=2, hidden=D, heads=2, intermediate=256, vocab=1000, max_position=128, init_std=0.05,
                 head=head, num_labels=L)
    hf = m.model
    assert type(hf).__name__ == {"sequence": "BertForSequenceClassification", "token": "BertForTokenClassification",
                                 "qa": "BertForQuestionAnswering"}[head]
    rng = np.random.default_rng(7)
    ids = torch.from_numpy(rng.integers(0, 1000, (B, seq), dtype=np.int64))
    mask = torch.ones(B, seq, dtype=torch.int64)
    mask[1, 9:] = 0
    with torch.no_grad():
        want = hf(input_ids=ids, attention_mask=mask, return_dict=False)
        base = hf.bert(input_ids=ids, attention_mask=mask, return_dict=False)
        got = m(ids, mask)
    dense = hf.qa_outputs if head == "qa" else hf.classifier
    W, b = dense.weight.detach().double().numpy(), dense.bias.detach().double().numpy()
    assert W.shape == ((2, D) if head == "qa" else (L, D))
    x = base[1] if head == "sequence" else base[0]
    ref = x.double().numpy() @ W.T + b
    refs = [ref[..., 0], ref[..., 1]] if head == "qa" else [ref]
    assert len(got) == 1 + len(refs) and torch.equal(got[0], base[0])  # the wrapper: hidden, then HF's logits
    for i, r in enumerate(refs):
        err = normalized_max_error(want[i].numpy(), r)
        print(f"HF pin {head} output {i}: {err:.3e}, max|ref| {np.abs(r).max():.3f}")
        assert want[i].shape == r.shape and err < 1e-6
        assert torch.equal(got[1 + i], want[i])
        assert np.abs(r).max() > 0.3  # the re-drawn head gives logits a normalised comparison can see


# ---- packer ----------------------------------------------------------------------------------------


@pytest.mark.parametrize("prec", ["fp32", "fp16", "fp16m"])
def test_no_head_bit_is_the_recorded_replica(spi, small, prec):
    """classifier.* / qa_outputs.* in the parameter list change nothing without a head bit."""
    with open(os.path.join(HERE, "golden", "replica_digests.json")) as f:
        want = json.load(f)["cases"][f"bert_d128|{prec}|"]
    r = spi.ModelReplica(small, -1, prec, **KW)
    assert ["%016x" % r.weight_digest, r.weight_bytes, r.description, r.flops(1)] == want
    assert r.num_labels == 0
    base = spi.ModelReplica(small, -1, prec, bert_io=("pooler", "mean", "token_types"), **KW)
    assert base.description == want[2] + " out[hidden,pooler,mean] in[ids,mask,types]" and base.num_labels == 0
    assert base.weight_bytes <= want[1] + POOL_BYTES + 2 * D * 4 + 3 * 256


def test_names_and_bits(spi):
    cd = importlib.import_module("starpu-inference-server_amd.codelet")
    N = spi._native
    assert (N.BERT_HEAD_SEQUENCE, N.BERT_HEAD_TOKEN, N.BERT_HEAD_QA) == (128, 256, 512)
    for name, bit in HEADS.items():
        assert cd.bert_io_bits(name) == bit and cd.bert_io_bits(("no_hidden", name)) == 4 | bit
    assert N.SPI_ABI_VERSION == 1
    import ctypes as C
    assert C.sizeof(N.ModelConfig) == 40


@pytest.mark.parametrize("head", list(HEADS))
def test_packing_appends_the_head(spi, small, head):
    base = spi.ModelReplica(small, -1, "fp16", **KW)
    labels = LABELS[head]
    grow = (labels * D + labels) * 4 + (POOL_BYTES if head == "seq_head" else 0)
    outs = {"seq_head": f"seq_logits{L}", "token_head": f"token_logits{L}", "qa_head": "qa_start,qa_end"}[head]
    a = spi.ModelReplica(small, -1, "fp16", bert_io=head, **KW)
    b = spi.ModelReplica(small, -1, "fp16", bert_io=HEADS[head], **KW)
    assert a.bert_io == HEADS[head] and a.num_labels == b.num_labels == labels
    assert base.weight_bytes + grow <= a.weight_bytes <= base.weight_bytes + grow + 3 * 256
    assert (a.weight_digest, a.weight_bytes) == (b.weight_digest, b.weight_bytes)
    assert a.weight_digest != base.weight_digest
    assert a.description == base.description + f" out[hidden,{outs}] in[ids,mask]"
    tokens = 3 * S  # flops at seq_len
    extra = 2.0 * 3 * D * labels + 2.0 * 3 * D * D if head == "seq_head" else 2.0 * tokens * D * labels
    assert a.flops(3) == base.flops(3) + extra
    others = [spi.ModelReplica(small, -1, "fp16", bert_io=h, **KW).weight_digest for h in HEADS if h != head]
    assert a.weight_digest not in others
    # logits alone are a valid replica; the blob does not depend on the outputs selected
    alone = spi.ModelReplica(small, -1, "fp16", bert_io=("no_hidden", head), **KW)
    assert alone.description == base.description + f" out[{outs}] in[ids,mask]"
    assert alone.weight_digest == a.weight_digest
    if head == "seq_head":  # the pooler is packed once, as an output or not
        both = spi.ModelReplica(small, -1, "fp16", bert_io=("pooler", head), **KW)
        assert (both.weight_digest, both.weight_bytes) == (a.weight_digest, a.weight_bytes)
        assert both.flops(3) == a.flops(3)
        assert both.description == base.description + f" out[hidden,pooler,{outs}] in[ids,mask]"


def test_head_parameters_under_a_wrapper_prefix(spi, zoo, small):
    """model.bert.* beside model.classifier.*: looked up on the unstripped names."""
    d = {"model." + n: t for n, t in tensors_of(spi, small).items()}
    wrapped = spi.ModelReplica(Named(d), -1, "fp16", bert_io="token_head", **KW)
    plain = spi.ModelReplica(small, -1, "fp16", bert_io="token_head", **KW)
    assert wrapped.num_labels == L and wrapped.weight_bytes == plain.weight_bytes
    hf = zoo.bert(layers=2, hidden=D, heads=2, intermediate=256, vocab=64, max_position=32, head="token", num_labels=9)
    assert spi.ModelReplica(hf, -1, "fp16", bert_io="token_head", **KW).num_labels == 9


def test_rejected_heads(spi, zoo, small):
    def refuses(module, io, match, **kw):
        with pytest.raises(spi.InferenceExecutionException, match=match):
            spi.ModelReplica(module, -1, "fp16", bert_io=io, **kw)
    refuses(small, 16, "unknown bits 16", **KW)
    refuses(small, 1 | 32 | 64, "unknown bits 96", **KW)
    refuses(small, 128 | 32, "unknown bits 32", **KW)
    for two in (("seq_head", "token_head"), ("token_head", "qa_head"), ("seq_head", "qa_head"), 128 | 256 | 512):
        refuses(small, two, "at most one of SPI_BERT_HEAD_SEQUENCE, SPI_BERT_HEAD_TOKEN, SPI_BERT_HEAD_QA", **KW)
    refuses(small, "no_hidden", "SPI_BERT_NO_HIDDEN leaves no output", **KW)
    resnet = zoo.resnet([1, 1, 1, 1], False, image=64, calibrate=False)
    for head in HEADS:
        refuses(resnet, head, "not a BERT", image_size=64)
    with pytest.raises(spi.InferenceExecutionException, match="not a BERT"):
        spi.ModelReplica(None, -1, "fp32", family="affine", bert_io="qa_head")
    # missing and ambiguous parameters, by name
    refuses(with_heads(spi, zoo, drop=("classifier.weight",)), "token_head",
            r"SPI_BERT_HEAD_TOKEN needs parameter 'classifier\.weight'", **KW)
    refuses(with_heads(spi, zoo, drop=("classifier.bias",)), "seq_head",
            r"SPI_BERT_HEAD_SEQUENCE needs parameter 'classifier\.bias'", **KW)
    refuses(with_heads(spi, zoo, drop=("qa_outputs",)), "qa_head", r"SPI_BERT_HEAD_QA needs parameter 'qa_outputs\.weight'", **KW)
    twice = with_heads(spi, zoo, extra={"aux.classifier.weight": (L, D), "aux.classifier.bias": (L,)})
    refuses(twice, "token_head", r"parameter 'classifier\.weight' is ambiguous \(2 tensors", **KW)
    spi.ModelReplica(twice, -1, "fp16", bert_io="qa_head", **KW)  # the other head's name is not looked at
    # shapes
    refuses(with_heads(spi, zoo, extra={"classifier.weight": (L, D - 64)}), "token_head", r"classifier\.weight must be \[L\]\[D\]", **KW)
    refuses(with_heads(spi, zoo, extra={"classifier.weight": (L * D,)}), "seq_head", r"classifier\.weight must be \[L\]\[D\]", **KW)
    refuses(with_heads(spi, zoo, extra={"classifier.bias": (L + 1,)}), "token_head", r"classifier\.bias \[L\]", **KW)
    refuses(with_heads(spi, zoo, extra={"qa_outputs.bias": (2, 1)}), "qa_head", r"qa_outputs\.bias \[L\]", **KW)
    # label ranges: token 1 .. 64, sequence 1 .. 1024, QA exactly 2
    many = lambda n: with_heads(spi, zoo, extra={"classifier.weight": (n, D), "classifier.bias": (n,)})  # noqa: E731
    refuses(many(65), "token_head", "SPI_BERT_HEAD_TOKEN takes 1 .. 64 labels, classifier.weight has 65", **KW)
    assert spi.ModelReplica(many(64), -1, "fp16", bert_io="token_head", **KW).num_labels == 64
    assert spi.ModelReplica(many(65), -1, "fp16", bert_io="seq_head", **KW).num_labels == 65
    refuses(many(1025), "seq_head", "SPI_BERT_HEAD_SEQUENCE takes 1 .. 1024 labels", **KW)
    assert spi.ModelReplica(many(1), -1, "fp16", bert_io="token_head", **KW).num_labels == 1
    for n in (1, 3):
        refuses(with_heads(spi, zoo, extra={"qa_outputs.weight": (n, D), "qa_outputs.bias": (n,)}), "qa_head",
                rf"SPI_BERT_HEAD_QA needs qa_outputs\.weight \[2\]\[D\], got {n} rows", **KW)
    # the sequence head needs the pooler, with SPI_BERT_OUT_POOLER's message
    refuses(with_heads(spi, zoo, drop=("pooler.dense",)), "seq_head", r"needs parameter 'pooler\.dense\.weight'", **KW)
    refuses(with_heads(spi, zoo, drop=("pooler.dense.bias",)), ("no_hidden", "seq_head"),
            r"needs parameter 'pooler\.dense\.bias'", **KW)
    spi.ModelReplica(with_heads(spi, zoo, drop=("pooler.dense",)), -1, "fp16", bert_io="token_head", **KW)


# ---- check_io, workspace plan, plan_check ----------------------------------------------------------


def hip_call(spi, rep, out_elems, B):
    """spi_hip_inference_func over host buffers; returns (status, message) of the raised error."""
    ins = [torch.zeros(B * S, dtype=torch.int64) for _ in range(2)]
    outs = [torch.zeros(max(n, 1), dtype=torch.float32) for n in out_elems]
    params = spi.make_params([[B, S]] * 2, [torch.int64] * 2, num_outputs=len(outs), models_gpu=[rep],
                             output_types=[torch.float32] * len(outs))
    bufs = [spi.tensor_interface(t) for t in ins] + [spi.make_vector_interface(t.data_ptr(), n, 4)
                                                     for t, n in zip(outs, out_elems)]
    with spi.worker_context(0, 0, None):
        with pytest.raises(spi.StarPUCodeletException) as e:
            spi.InferenceCodelet.hip_inference_func(bufs, params)
    return e.value.status, str(e.value)


def expected_elems(spec, B):
    labels = 2 if "qa_head" in spec else L
    e = [] if "no_hidden" in spec else [B * S * D]
    e += [B * D] * (("pooler" in spec) + ("mean" in spec))
    return e + {"seq_head": [B * labels], "token_head": [B * S * labels], "qa_head": [B * S, B * S]}[spec[-1]]


IO_SPECS = [pre + mid + (head,) for head in HEADS for pre in ((), ("no_hidden",))
            for mid in ((), ("mean",), ("pooler", "mean"))]


@pytest.mark.parametrize("spec", IO_SPECS, ids="|".join)
def test_check_io_outputs(spi, small, spec):
    N = spi._native
    cd = importlib.import_module("starpu-inference-server_amd.codelet")
    rep = spi.ModelReplica(small, -1, "fp16", max_batch=4, bert_io=spec, **KW)
    B = 3
    good = expected_elems(spec, B)
    assert len(good) <= 5 and len(good) == len(spec) - 2 * ("no_hidden" in spec) + 1 + (spec[-1] == "qa_head")
    specs = cd.output_specs(B, seq=S, dim=D, bert_io=spec, num_labels=rep.num_labels)
    assert [int(np.prod(s)) for s, _ in specs] == good and all(dt == torch.float32 for _, dt in specs)
    st, msg = hip_call(spi, rep, good, B)  # the contract holds: only the missing device stops it
    assert st == N.SPI_ERR_DEVICE and "host-only replica" in msg, msg
    for wrong in (good + [B * D], good[:-1]):  # one output too many, one too few
        st, msg = hip_call(spi, rep, wrong, B)
        assert st == N.SPI_ERR_INVALID_ARGUMENT and "Mismatch between model outputs and StarPU buffers" in msg, msg
    for i in range(len(good)):
        wrong = list(good)
        wrong[i] += 1
        st, msg = hip_call(spi, rep, wrong, B)
        assert st == N.SPI_ERR_OUTPUT_MISMATCH and "Output buffer size mismatch in bytes" in msg, (i, msg)
    # the plan at max_batch: the class-token rows' buffer (index 8, kBtCls) also holds the sequence head's
    # pooled vector when the pooler is not an output; every GEMM of the forward still fits
    plan, _ = workspace_plan(spi, rep)
    assert plan[8] == 4 * D * 4 * (("no_hidden" in spec) + (spec[-1] == "seq_head" and "pooler" not in spec))
    assert plan_steps(spi, rep, 4, S) == plan_steps(spi, spi.ModelReplica(small, -1, "fp16", max_batch=4, **KW), 4, S)


def workspace_plan(spi, rep):
    import ctypes as C
    lib = spi.lib
    bytes_out = (C.c_size_t * 32)()
    n, floats, before = C.c_int32(0), C.c_size_t(0), C.c_size_t(0)
    st = lib.spi_model_workspace_plan(rep.handle, bytes_out, 32, C.byref(n), C.byref(floats), C.byref(before))
    assert st == spi._native.SPI_OK
    return list(bytes_out[:n.value]), floats.value


def plan_steps(spi, rep, batch, seq):
    import ctypes as C
    steps = C.c_int32(0)
    st = spi.lib.spi_model_plan_check(rep.handle, batch, seq, C.byref(steps))
    assert st == spi._native.SPI_OK, spi._native.last_error()
    return steps.value


def test_workspace_plan_without_a_head_is_unchanged(spi, small):
    """The pooled vector's place is sized with the class-token rows' buffer: no new buffer, nothing without a
    head bit (tests/golden/workspace_plans.json holds the recorded plans)."""
    plain, _ = workspace_plan(spi, spi.ModelReplica(small, -1, "fp16", max_batch=4, **KW))
    tok, _ = workspace_plan(spi, spi.ModelReplica(small, -1, "fp16", max_batch=4, bert_io="token_head", **KW))
    assert tok == plain and plain[8] == 0


def test_make_pack_check_and_plan_check():
    """The stand-alone packer and plan programs under the host sanitizers (as tests/test_bert_io.py runs the
    packer's; both build into csrc/build, which git ignores): one case per head in the packer's, and in the
    plans' the two- to five-output tasks, the class-token buffer's two parts and the walk at max_batch."""
    csrc = os.path.join(ROOT, "starpu-inference-server_amd", "csrc")
    r = subprocess.run(["make", "-C", csrc, "pack_check", "plan_check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    for head, outs in (("seq_head", "seq_logits5"), ("token_head", "token_logits5"), ("qa_head", "qa_start,qa_end")):
        line = [ln for ln in lines if ln.startswith(f"bert_d128|fp16|{head} ")]
        assert line and line[0].endswith(f"out[hidden,{outs}] in[ids,mask]"), r.stdout[-2000:]
    for name, outs, cls in (("seq_head", 2, 4096), ("no_hidden|seq_head", 1, 8192), ("no_hidden|token_head", 1, 4096),
                            ("pooler|mean|qa_head", 5, 0)):
        line = [ln for ln in lines if ln.startswith(f"bert_d128|fp16|{name}| ")]
        assert line and f"| {outs} outputs," in line[0] and f"class-token buffer {cls} bytes, 8 steps fit" in line[0], \
            r.stdout[-2000:]

"""Classification outputs of image replicas (spi_model_set_image_outputs), host side: what the setter
refuses, the codelet's I/O contract (Model::check_io) on host-only replicas (device -1), where check_io
runs and the forward cannot, and both CPU codelets against a reference computed from the module's own
logits."""
import importlib
import json
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PROBS, TOPK, NO_LOGITS, TOPK_PROBS = 1, 2, 4, 8
CLASSES, K = 10, 3
# every legal combination of the bits
COMBOS = [PROBS, TOPK, PROBS | TOPK, TOPK | TOPK_PROBS, PROBS | TOPK | TOPK_PROBS, NO_LOGITS | PROBS,
          NO_LOGITS | TOPK, NO_LOGITS | TOPK | TOPK_PROBS, NO_LOGITS | PROBS | TOPK,
          NO_LOGITS | PROBS | TOPK | TOPK_PROBS]


@pytest.fixture(scope="module")
def small(zoo):
    """name -> (module, ModelReplica keywords) of the two small image models."""
    return {"resnet": (zoo.resnet([1, 1, 1, 1], False, image=64, num_classes=CLASSES, calibrate=False),
                       dict(image_size=64)),
            "vit": (zoo.vit(image=32, patch=16, layers=2, heads=2, dim=128, mlp_dim=256, num_classes=CLASSES),
                    dict(num_heads=2, image_size=32))}


def replica(spi, small, which, prec="fp16", **kw):
    module, base = small[which]
    return spi.ModelReplica(module, -1, prec, max_batch=4, **base, **kw)


def test_image_io_names_and_ints(spi):
    assert spi.image_io_bits(("probs", "topk", "no_logits", "topk_probs")) == 15
    assert spi.image_io_bits("topk") == 2 and spi.image_io_bits(9) == 9 and spi.image_io_bits(None) == 0
    with pytest.raises(spi.InferenceExecutionException, match="unknown image_io name"):
        spi.image_io_bits(("probs", "labels"))
    N = spi._native
    assert (N.IMAGE_OUT_PROBS, N.IMAGE_OUT_TOPK, N.IMAGE_NO_LOGITS, N.IMAGE_TOPK_PROBS) == (1, 2, 4, 8)


@pytest.mark.parametrize("which", ["resnet", "vit"])
def test_refusals(spi, small, which):
    N = spi._native
    rep = replica(spi, small, which)
    plain = rep.description

    def refuses(io, k, match, status=N.SPI_ERR_INVALID_ARGUMENT):
        with pytest.raises(spi.InferenceExecutionException, match=match) as e:
            rep.set_image_outputs(io, k)
        assert e.value.status == status
        assert rep.description == plain and (rep.image_io, rep.top_k) == (0, 0)  # nothing changed

    refuses(16, 0, "unknown bits 16")
    refuses(PROBS | 32 | 64, 0, "unknown bits 96")
    refuses(NO_LOGITS, 0, "SPI_IMAGE_NO_LOGITS leaves no output")
    refuses(NO_LOGITS | TOPK_PROBS, 0, "SPI_IMAGE_NO_LOGITS leaves no output")
    refuses(TOPK_PROBS, 0, "SPI_IMAGE_TOPK_PROBS needs SPI_IMAGE_OUT_TOPK")
    refuses(PROBS | TOPK_PROBS, 0, "SPI_IMAGE_TOPK_PROBS needs SPI_IMAGE_OUT_TOPK")
    for k in (0, -1, CLASSES + 1, 65):
        refuses(TOPK, k, r"top_k -?\d+ outside 1 \.\. min\(classes, 64\) = 10")
    refuses(PROBS, 1, "top_k 1 without SPI_IMAGE_OUT_TOPK")
    refuses(0, 5, "top_k 5 without SPI_IMAGE_OUT_TOPK")
    rep.set_image_outputs(TOPK, CLASSES)  # the largest k
    assert rep.description == plain + " out[logits,top10]"
    rep.set_image_outputs(0, 0)  # back to the one-output contract
    assert rep.description == plain


def test_refuses_more_than_64_of_many_classes_and_wide_rows(spi, zoo):
    N = spi._native
    m = zoo.vit(image=32, patch=16, layers=1, heads=2, dim=128, mlp_dim=256, num_classes=16385)
    rep = spi.ModelReplica(m, -1, "fp16", max_batch=1, num_heads=2, image_size=32)
    with pytest.raises(spi.InferenceExecutionException, match="16385 classes; at most 16384") as e:
        rep.set_image_outputs("probs")
    assert e.value.status == N.SPI_ERR_UNSUPPORTED
    m = zoo.vit(image=32, patch=16, layers=1, heads=2, dim=128, mlp_dim=256, num_classes=100)
    rep = spi.ModelReplica(m, -1, "fp16", max_batch=1, num_heads=2, image_size=32)
    with pytest.raises(spi.InferenceExecutionException, match=r"top_k 65 outside 1 \.\. min\(classes, 64\) = 64"):
        rep.set_image_outputs("topk", 65)
    rep.set_image_outputs("topk", 64)


def test_other_families_are_unsupported(spi, zoo):
    N = spi._native
    bert = zoo.bert(layers=2, hidden=128, heads=2, intermediate=256, vocab=64, max_position=32)
    for make in (lambda **kw: spi.ModelReplica(bert, -1, "fp16", num_heads=2, seq_len=16, **kw),
                 lambda **kw: spi.ModelReplica(None, -1, "fp32", family="affine", **kw)):
        rep = make()
        for io, k in (("probs", 0), ("topk", 1), (("no_logits", "topk", "topk_probs"), 3), (0, 0)):
            with pytest.raises(spi.InferenceExecutionException, match="only ResNet / ViT replicas") as e:
                rep.set_image_outputs(io, k)
            assert e.value.status == N.SPI_ERR_UNSUPPORTED
        with pytest.raises(spi.InferenceExecutionException, match="only ResNet / ViT replicas"):
            make(image_io="probs")


def out_specs(io, B, k=K):
    """(elements, dtype) per output, in the contract's order."""
    e = [] if io & NO_LOGITS else [(B * CLASSES, torch.float32)]
    if io & PROBS:
        e.append((B * CLASSES, torch.float32))
    if io & TOPK:
        e += [(B * k, torch.float32), (B * k, torch.int64)]
    return e


def hip_call(spi, rep, image, specs, B=3):
    """spi_hip_inference_func over host buffers; returns (status, message) of the raised error."""
    N = spi._native
    x = torch.zeros(B, 3, image, image)
    outs = [torch.zeros(max(n, 1), dtype=dt) for n, dt in specs]
    params = spi.make_params([list(x.shape)], [torch.float32], num_outputs=len(outs), models_gpu=[rep],
                             output_types=[dt for _, dt in specs])
    bufs = [spi.tensor_interface(x)] + [spi.make_vector_interface(t.data_ptr(), n, t.element_size())
                                        for t, (n, _) in zip(outs, specs)]
    with spi.worker_context(0, 0, None):  # replica index = device id
        with pytest.raises(spi.StarPUCodeletException) as e:
            spi.InferenceCodelet.hip_inference_func(bufs, params)
    assert e.value.status in (N.SPI_ERR_INVALID_ARGUMENT, N.SPI_ERR_OUTPUT_MISMATCH, N.SPI_ERR_DEVICE)
    return e.value.status, str(e.value)


@pytest.mark.parametrize("io", COMBOS)
@pytest.mark.parametrize("which", ["resnet", "vit"])
def test_check_io_outputs(spi, small, which, io):
    N = spi._native
    rep = replica(spi, small, which, image_io=io, top_k=K if io & TOPK else 0)
    image = small[which][1]["image_size"]
    B = 3
    good = out_specs(io, B)
    assert len(good) == (not io & NO_LOGITS) + bool(io & PROBS) + 2 * bool(io & TOPK)
    assert [(int(np.prod(s)), dt) for s, dt in spi.output_specs(B, CLASSES, io, K if io & TOPK else 0)] == good
    st, msg = hip_call(spi, rep, image, good, B)  # the contract holds: only the missing device stops it
    assert st == N.SPI_ERR_DEVICE and "host-only replica" in msg, msg
    for wrong in (good + [(B * CLASSES, torch.float32)], good[:-1]):  # an extra output, a missing one
        st, msg = hip_call(spi, rep, image, wrong, B)
        assert st == N.SPI_ERR_INVALID_ARGUMENT and "Mismatch between model outputs and StarPU buffers" in msg, msg
    for i, (n, dt) in enumerate(good):
        for delta in (-1, 1, B):
            wrong = list(good)
            wrong[i] = (n + delta, dt)
            st, msg = hip_call(spi, rep, image, wrong, B)
            assert st == N.SPI_ERR_OUTPUT_MISMATCH and "Output buffer size mismatch in bytes" in msg, (i, delta, msg)
        for other in (torch.float16, torch.int32, torch.int64 if dt == torch.float32 else torch.float32):
            wrong = list(good)
            wrong[i] = (n, other)
            st, msg = hip_call(spi, rep, image, wrong, B)
            assert st == N.SPI_ERR_INVALID_ARGUMENT and "Output type mismatch" in msg, (i, other, msg)
    if io & TOPK:
        # an fp32 index buffer of the same byte count is still the wrong element type
        wrong = good[:-1] + [(2 * B * K, torch.float32)]
        st, msg = hip_call(spi, rep, image, wrong, B)
        assert st == N.SPI_ERR_INVALID_ARGUMENT and "Output type mismatch" in msg, msg
    if io & PROBS:  # a short probability buffer: the top-k row count instead of the class count
        i = 0 if io & NO_LOGITS else 1
        wrong = list(good)
        wrong[i] = (B * K, torch.float32)
        st, msg = hip_call(spi, rep, image, wrong, B)
        assert st == N.SPI_ERR_OUTPUT_MISMATCH, msg


@pytest.mark.parametrize("which", ["resnet", "vit"])
def test_plain_replica_keeps_the_one_output_contract(spi, small, which):
    N = spi._native
    rep = replica(spi, small, which)
    image = small[which][1]["image_size"]
    st, msg = hip_call(spi, rep, image, out_specs(0, 3))
    assert st == N.SPI_ERR_DEVICE and "host-only replica" in msg, msg
    st, msg = hip_call(spi, rep, image, out_specs(PROBS, 3))
    assert st == N.SPI_ERR_INVALID_ARGUMENT and "Mismatch between model outputs and StarPU buffers" in msg, msg


@pytest.mark.parametrize("prec", ["fp32", "fp16", "fp16m"])
@pytest.mark.parametrize("which", ["resnet", "vit"])
def test_description_digest_and_flops(spi, small, which, prec):
    plain = replica(spi, small, which, prec)
    if which == "vit":  # the recorded replica of the same shape: the text is the one from before
        with open(os.path.join(HERE, "golden", "replica_digests.json")) as f:
            want = json.load(f)["cases"][f"vit_d128|{prec}|"]
        small_batch = spi.ModelReplica(small[which][0], -1, prec, **small[which][1])
        assert small_batch.description == want[2] and small_batch.flops(1) == want[3]
    assert " out[" not in plain.description
    for io, k, suffix in ((PROBS, 0, "out[logits,probs]"), (TOPK, 5, "out[logits,top5]"),
                          (PROBS | TOPK | TOPK_PROBS, 5, "out[logits,probs,top5]"),
                          (NO_LOGITS | TOPK, 1, "out[top1]"), (NO_LOGITS | PROBS | TOPK, 10, "out[probs,top10]")):
        rep = replica(spi, small, which, prec, image_io=io, top_k=k)
        assert rep.description == plain.description + " " + suffix
        assert (rep.weight_digest, rep.weight_bytes) == (plain.weight_digest, plain.weight_bytes)
        assert rep.flops(1) == plain.flops(1) and rep.flops(3) == plain.flops(3)
        assert (rep.image_io, rep.top_k) == (io, k)
    zero = replica(spi, small, which, prec, image_io=0, top_k=0)
    assert zero.description == plain.description


# ---- the CPU codelets --------------------------------------------------------------------------------


class Quantised(torch.nn.Module):
    """The model's logits rounded to multiples of 0.25, so that equal logits occur."""

    def __init__(self, model):
        super().__init__()
        self.model = model

    def forward(self, x):
        return torch.round(self.model(x) * 4) / 4


@pytest.fixture(scope="module")
def quantised(small):
    m = Quantised(small["resnet"][0]).eval()
    x = np.random.default_rng(11).random((4, 3, 64, 64), dtype=np.float32)
    with torch.inference_mode():
        logits = m(torch.from_numpy(x)).numpy().copy()
    assert logits.shape == (4, CLASSES) and logits.dtype == np.float32
    assert any(len(np.unique(row)) < CLASSES for row in logits), "the fixture has no equal logits"
    return m, x, logits


def reference(logits, k):
    """float64 softmax, the stable descending order's first k indices, and the logits there."""
    x = logits.astype(np.float64)
    e = np.exp(x - x.max(1, keepdims=True))
    idx = np.argsort(-logits, kind="stable")[:, :k]
    return e / e.sum(1, keepdims=True), idx, np.take_along_axis(logits, idx, 1)


def cpu_call(spi, model_cpu, x, io, k):
    B = x.shape[0]
    specs = spi.output_specs(B, CLASSES, io, k)
    outs = [torch.full(shape, -7, dtype=dt) for shape, dt in specs]
    params = spi.make_params([list(x.shape)], [torch.float32], num_outputs=len(outs), model_cpu=model_cpu,
                             output_types=[dt for _, dt in specs])
    bufs = [spi.tensor_interface(torch.from_numpy(x))] + [spi.tensor_interface(o) for o in outs]
    with spi.worker_context(3, -1, None):
        spi.InferenceCodelet.cpu_inference_func(bufs, params)
    return [o.numpy() for o in outs]


@pytest.fixture(scope="module")
def codelets(spi, quantised, tmp_path_factory):
    """name -> a function (io, k) -> the CPU codelet's model_cpu with those outputs set."""
    lt = importlib.import_module("starpu-inference-server_amd.libtorch")
    m, x, _ = quantised
    path = str(tmp_path_factory.mktemp("image_outputs") / "quantised.pt")
    torch.jit.trace(m, torch.from_numpy(x)).save(path)
    ts = lt.TorchScriptModule(path)

    def libtorch(io, k):
        ts.set_image_outputs(io, k)
        return ts
    return {"python": lambda io, k: spi.TorchCpuForward(m, image_outputs=(io, k)) if io else spi.TorchCpuForward(m),
            "libtorch": libtorch}


@pytest.mark.parametrize("io", COMBOS)
@pytest.mark.parametrize("which", ["python", "libtorch"])
def test_cpu_codelets(spi, quantised, codelets, which, io):
    _, x, logits = quantised
    k = K if io & TOPK else 0
    got = cpu_call(spi, codelets[which](io, k), x, io, k)
    p64, idx, vals = reference(logits, K)
    o = 0
    if not io & NO_LOGITS:
        assert np.array_equal(got[o], logits)
        o += 1
    probs = None
    if io & PROBS:
        probs = got[o]
        o += 1
        err = np.max(np.abs(probs - p64).max(1) / p64.max(1))
        assert err <= 1e-5, err
        assert np.all(np.abs(probs.astype(np.float64).sum(1) - 1) <= 1e-5)
    if io & TOPK:
        topv, topi = got[o], got[o + 1]
        assert topi.dtype == np.int64 and np.array_equal(topi, idx)
        if io & TOPK_PROBS:
            err = np.max(np.abs(topv - np.take_along_axis(p64, idx, 1)).max(1) / p64.max(1))
            assert err <= 1e-5, err
            if probs is not None:  # the bits of the probability output
                assert np.array_equal(topv, np.take_along_axis(probs, idx, 1))
        else:
            assert np.array_equal(topv.view(np.uint32), vals.view(np.uint32))


@pytest.mark.parametrize("which", ["python", "libtorch"])
def test_cpu_codelet_without_bits_still_refuses_two_outputs(spi, quantised, codelets, which):
    _, x, _ = quantised
    with pytest.raises(spi.StarPUCodeletException, match="Mismatch between model outputs and StarPU buffers"):
        cpu_call(spi, codelets[which](0, 0), x, PROBS, 0)
    assert np.array_equal(cpu_call(spi, codelets[which](0, 0), x, 0, 0)[0], quantised[2])


def test_cpu_codelet_setters_refuse(spi, quantised, codelets):
    m = quantised[0]
    ts = codelets["libtorch"](0, 0)
    for io, k in ((16, 0), (NO_LOGITS, 0), (TOPK_PROBS, 0), (TOPK, 0), (TOPK, 65), (PROBS, 2)):
        with pytest.raises(spi.InferenceExecutionException):
            ts.set_image_outputs(io, k)
        with pytest.raises(spi.InferenceExecutionException, match="image outputs"):
            spi.TorchCpuForward(m, image_outputs=(io, k))
    # the class count is known at the forward only
    with pytest.raises(spi.StarPUCodeletException, match="top_k exceeds the class count"):
        cpu_call(spi, codelets["libtorch"](TOPK, CLASSES + 1), quantised[1], TOPK, CLASSES + 1)
    with pytest.raises(spi.StarPUCodeletException, match="top_k exceeds the class count"):
        cpu_call(spi, spi.TorchCpuForward(m, image_outputs=(TOPK, CLASSES + 1)), quantised[1], TOPK, CLASSES + 1)
    ts.set_image_outputs(0, 0)

"""ConvNeXt replicas on the GPU: zoo.convnext([1, 1, 2, 1], [96, 192, 384, 768], image=64, num_classes=10) -- maps
16 / 8 / 4 / 2 -- and the widths of convnext_base ([1, 1, 1, 1], 128 .. 1024); batch 2, input default_rng(1).random.
Bars.  fp32 against the oracle at the project's 1e-5.  fp16: tools/prec_emulate_convnext.py (fp16-rounded weights
and activations, fp32 accumulation; it emulates the formats, not the kernels) gives 4.52e-4 for the tiny widths
and 4.50e-4 for the base widths at this input; each bar is 1.5x that figure, the headroom test_resnext_gpu.py
documents: 6.78e-4 and 6.74e-4, inside the project's 3e-3 bound for reduced-size nets.  (The figure moves with
the summation alone: float64 accumulation gives 4.88e-4 and 3.97e-4 at the same input.)
"""
import functools
import importlib

import numpy as np
import pytest
import torch

from oracle.cpu_codelet import cpu_inference, normalized_max_error

pytestmark = pytest.mark.gpu

TINY = ((1, 1, 2, 1), (96, 192, 384, 768))
BASE = ((1, 1, 1, 1), (128, 256, 512, 1024))
TOL = {("fp32", TINY): 1e-5, ("fp32", BASE): 1e-5, ("fp16", TINY): 6.78e-4, ("fp16", BASE): 6.74e-4}


@functools.lru_cache(maxsize=None)
def case(arch, batch=2):
    zoo = importlib.import_module("starpu-inference-server_amd.zoo")
    m = zoo.convnext(list(arch[0]), list(arch[1]), image=64, num_classes=10)
    x = np.random.default_rng(1).random((batch, 3, 64, 64), dtype=np.float32)
    ref = cpu_inference(m, [x])[0]
    ref.setflags(write=False)
    return m, x, ref


def hip_forward(spi, replica, x, out_shape, graphs=False):
    xin = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    out = torch.full(out_shape, float("nan"), device="cuda", dtype=torch.float32)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    replica.set_graphs(graphs)
    spi.run_hip(replica, [xin], out, stream=stream.cuda_stream)
    for _ in range(2 if graphs else 0):  # several replays of the captured graph
        spi.run_hip(replica, [xin], out, stream=stream.cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("arch", [TINY, BASE], ids=["tiny_dims", "base_dims"])
def test_convnext_against_oracle(spi, gpu, arch, prec):
    """Parity at the precision's bar at batch 2 and at 1 of max_batch 4; the captured graph gives the eager bits;
    the description names the family."""
    m, x, ref = case(arch)
    rep = spi.ModelReplica(m, 0, prec, max_batch=4, image_size=64)
    depths = ",".join(str(d) for d in arch[0])
    assert rep.description.startswith(f"convnext[{depths}] C{arch[1][0]} img64 classes10 "), rep.description
    got = hip_forward(spi, rep, x, ref.shape)
    ref1 = cpu_inference(m, [x[:1]])[0]
    err, err1 = normalized_max_error(got, ref), normalized_max_error(hip_forward(spi, rep, x[:1], ref1.shape), ref1)
    print(f"convnext {arch[1]}@64 {prec}: err {err:.3e}, batch 1 of 4 {err1:.3e}")
    assert err < TOL[prec, arch] and err1 < TOL[prec, arch]
    np.testing.assert_array_equal(got, hip_forward(spi, rep, x, ref.shape, graphs=True))


def test_convnext_routing(spi, gpu):
    m, x, ref = case(TINY)
    rep = spi.ModelReplica(m, 0, "fp16", max_batch=2, image_size=64)
    ops = rep.profile([torch.from_numpy(x).cuda()], torch.empty(ref.shape, device="cuda"),
                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    names = [o["name"] for o in ops]
    assert [n for n in names if n.startswith("dwconv7_ln_")] == [
        "dwconv7_ln_c96_h16", "dwconv7_ln_c192_h8", "dwconv7_ln_c384_h4", "dwconv7_ln_c384_h4", "dwconv7_ln_c768_h2"], names
    assert [n for n in names if n.startswith("ln_s2d_")] == ["ln_s2d_c96", "ln_s2d_c192", "ln_s2d_c384"], names
    assert names.count("ln_rows_c96") == 1 and names.count("pool_ln_c768") == 1, names


def test_convnext_u8_task_with_image_outputs(spi, gpu):
    # an 8-bit NHWC task under an input transform, softmax + top-3 outputs, against the oracle on the normalised image
    m, _, _ = case(TINY)
    u8 = np.random.default_rng(2).integers(0, 256, (2, 64, 64, 3), dtype=np.uint8)
    scale, shift = [1 / 255.0 / s for s in (0.229, 0.224, 0.225)], [-mu / s for mu, s in zip((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))]
    ref = cpu_inference(m, [np.ascontiguousarray((u8.astype(np.float32) * np.float32(scale) + np.float32(shift)).transpose(0, 3, 1, 2))])[0]
    rep = spi.ModelReplica(m, 0, "fp32", max_batch=2, image_size=64, image_io=("probs", "topk"), top_k=3)
    rep.set_input_transform(scale, shift)
    assert rep.description.endswith(" out[logits,probs,top3]"), rep.description
    outs = [torch.full(s, float("nan") if dt == torch.float32 else -1, dtype=dt, device="cuda")
            for s, dt in spi.output_specs(2, 10, rep.image_io, rep.top_k)]
    torch.cuda.synchronize()
    spi.run_hip(rep, [torch.from_numpy(u8).cuda()], outs, stream=torch.cuda.Stream().cuda_stream)
    torch.cuda.synchronize()
    logits, probs, topv, topi = (o.cpu().numpy() for o in outs)
    err = normalized_max_error(logits, ref)
    print(f"convnext tiny dims fp32 u8 nhwc: err {err:.3e}")
    assert err < 1e-5
    e = np.exp(logits.astype(np.float64) - logits.max(1, keepdims=True))  # the launch's own input
    assert normalized_max_error(probs, e / e.sum(1, keepdims=True)) < 1e-5
    assert np.array_equal(topi, np.argsort(-logits, kind="stable")[:, :3])
    assert np.array_equal(topv, np.take_along_axis(logits, topi, 1))

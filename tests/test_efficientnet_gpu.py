"""EfficientNet replicas on the GPU: zoo.efficientnet(1.0, 1.0, image=64, num_classes=10) -- efficientnet_b0's 16 blocks
on maps 32 .. 2 -- and width 1.1, whose widths are multiples of 8 but not of 16 (partial channel slabs); batch 2, input
default_rng(1).random.
Bars.  fp32 against the oracle at the project's 1e-5.  fp16: tools/prec_emulate_efficientnet.py (BatchNorm folded in
fp32, fp16-rounded weights and activations, fp32 accumulation; it emulates the formats, not the kernels) gives
1.146e-3 for width 1.0 and 1.205e-3 for width 1.1 at this input; each bar is 1.5x that figure, the headroom
test_resnext_gpu.py documents: 1.719e-3 and 1.808e-3, inside the project's 3e-3 bound for reduced-size nets.  (The
figure moves with the summation alone: float64 accumulation gives 1.583e-3 and 9.12e-4 at the same input; input
seeds 2 and 3 give 1.69e-3 / 1.16e-3 and 8.5e-4 / 8.6e-4.)
"""
import functools
import importlib

import numpy as np
import pytest
import torch

from oracle.cpu_codelet import cpu_inference, normalized_max_error

pytestmark = pytest.mark.gpu

TOL = {("fp32", 1.0): 1e-5, ("fp32", 1.1): 1e-5, ("fp16", 1.0): 1.719e-3, ("fp16", 1.1): 1.808e-3}


@functools.lru_cache(maxsize=None)
def case(width):
    zoo = importlib.import_module("starpu-inference-server_amd.zoo")
    m = zoo.efficientnet(width, 1.0, image=64, num_classes=10)
    x = np.random.default_rng(1).random((2, 3, 64, 64), dtype=np.float32)
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
@pytest.mark.parametrize("width", [1.0, 1.1])
def test_efficientnet_against_oracle(spi, gpu, width, prec):
    """Parity at the precision's bar at batch 2 and at 1 of max_batch 4; the captured graph gives the eager bits;
    the description names the family."""
    m, x, ref = case(width)
    rep = spi.ModelReplica(m, 0, prec, max_batch=4, image_size=64)
    assert rep.description.startswith("efficientnet[1,2,2,3,3,4,1] C32 img64 classes10 "), rep.description
    got = hip_forward(spi, rep, x, ref.shape)
    ref1 = cpu_inference(m, [x[:1]])[0]
    err, err1 = normalized_max_error(got, ref), normalized_max_error(hip_forward(spi, rep, x[:1], ref1.shape), ref1)
    print(f"efficientnet width {width}@64 {prec}: err {err:.3e}, batch 1 of 4 {err1:.3e}")
    assert err < TOL[prec, width] and err1 < TOL[prec, width]
    np.testing.assert_array_equal(got, hip_forward(spi, rep, x, ref.shape, graphs=True))


def test_efficientnet_routing(spi, gpu):
    m, x, ref = case(1.0)
    rep = spi.ModelReplica(m, 0, "fp16", max_batch=2, image_size=64)
    ops = rep.profile([torch.from_numpy(x).cuda()], torch.empty(ref.shape, device="cuda"),
                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    names = [o["name"] for o in ops]
    # (k, stride, expanded channels, input side) of b0's 16 blocks at image 64
    blocks = ([(3, 1, 32, 32), (3, 2, 96, 32), (3, 1, 144, 16), (5, 2, 144, 16), (5, 1, 240, 8), (3, 2, 240, 8)] +
              [(3, 1, 480, 4)] * 2 + [(5, 1, 480, 4)] + [(5, 1, 672, 4)] * 2 + [(5, 2, 672, 4)] + [(5, 1, 1152, 2)] * 3 +
              [(3, 1, 1152, 2)])
    want = [n for k, s, c, h in blocks for n in (f"dwconv{k}s{s}_c{c}_h{h}", f"se_gate_c{c}", f"se_scale_c{c}")]
    assert [n for n in names if n.startswith(("dwconv", "se_"))] == want, names
    assert names[0] == "ingest_nchw" and names[1].startswith("conv3x3_c3_k32_s2") and names[-1].startswith("avgpool_fc"), names


def test_efficientnet_u8_task_with_image_outputs(spi, gpu):
    # an 8-bit NHWC task under an input transform, softmax + top-3 outputs, against the oracle on the normalised image
    m, _, _ = case(1.0)
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
    print(f"efficientnet width 1.0 fp32 u8 nhwc: err {err:.3e}")
    assert err < 1e-5
    e = np.exp(logits.astype(np.float64) - logits.max(1, keepdims=True))  # the launch's own input
    assert normalized_max_error(probs, e / e.sum(1, keepdims=True)) < 1e-5
    assert np.array_equal(topi, np.argsort(-logits, kind="stable")[:, :3])
    assert np.array_equal(topv, np.take_along_axis(logits, topi, 1))

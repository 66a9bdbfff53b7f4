"""Swin replicas on the GPU: zoo.swin((2, 2, 2), (2, 4, 8), 64, window=7, image=112, num_classes=10) -- maps 28 / 14 / 7:
shifted blocks in two stages, the forced-zero shift in the third, merges at 4 C = 256 and 512 -- and the widths of
swin_t's first stages ((2, 2), heads (3, 6), embed 96); batch 2, input default_rng(1).random.
Bars.  fp32 against the oracle at the project's 1e-5.  fp16: tools/prec_emulate_swin.py (fp16-rounded weights, GEMM
and attention operands, fp32 accumulation; it emulates the formats, not the kernels) gives 1.503e-3 for the first
model and 3.70e-4 for the second at this input; each bar is 1.5x that figure, the headroom test_resnext_gpu.py
documents: 2.25e-3 and 5.55e-4, inside the project's 3e-3 bound for reduced-size nets.  (float64 accumulation gives
1.483e-3 for the first.)  Measured on an MI355X: fp32 2.2e-7 .. 3.4e-7; fp16 1.56e-3 / 1.57e-3 and 4.93e-4.
"""
import functools
import importlib

import numpy as np
import pytest
import torch

from oracle.cpu_codelet import cpu_inference, normalized_max_error
from test_convnext_gpu import hip_forward  # one forward on a fresh stream; graphs=True: three replays of the capture

pytestmark = pytest.mark.gpu

SMALL = ((2, 2, 2), (2, 4, 8), 64)
WIDE = ((2, 2), (3, 6), 96)
EMU = {SMALL: 1.503e-3, WIDE: 3.70e-4}
TOL = {(p, a): 1e-5 if p == "fp32" else min(1.5 * EMU[a], 3e-3) for p in ("fp32", "fp16") for a in (SMALL, WIDE)}
IMG = 112


@functools.lru_cache(maxsize=None)
def case(arch, batch=2):
    zoo = importlib.import_module("starpu-inference-server_amd.zoo")
    m = zoo.swin(arch[0], arch[1], arch[2], window=7, image=IMG, num_classes=10)
    x = np.random.default_rng(1).random((batch, 3, IMG, IMG), dtype=np.float32)
    ref = cpu_inference(m, [x])[0]
    ref.setflags(write=False)
    return m, x, ref


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("arch", [SMALL, WIDE], ids=["embed64_3stages", "embed96_2stages"])
def test_swin_against_oracle(spi, gpu, arch, prec):
    """Parity at the precision's bar at batch 2 and at 1 of max_batch 4; the captured graph gives the eager bits;
    the description names the family."""
    m, x, ref = case(arch)
    rep = spi.ModelReplica(m, 0, prec, max_batch=4, image_size=IMG)
    depths = ",".join(str(d) for d in arch[0])
    assert rep.description.startswith(f"swin[{depths}] C{arch[2]} ws7 img{IMG} classes10 "), rep.description
    got = hip_forward(spi, rep, x, ref.shape)
    ref1 = cpu_inference(m, [x[:1]])[0]
    err, err1 = normalized_max_error(got, ref), normalized_max_error(hip_forward(spi, rep, x[:1], ref1.shape), ref1)
    print(f"swin embed {arch[2]}@{IMG} {prec}: err {err:.3e}, batch 1 of 4 {err1:.3e}")
    assert err < TOL[prec, arch] and err1 < TOL[prec, arch]
    np.testing.assert_array_equal(got, hip_forward(spi, rep, x, ref.shape, graphs=True))


def test_swin_routing(spi, gpu):
    m, x, ref = case(SMALL)
    rep = spi.ModelReplica(m, 0, "fp16", max_batch=2, image_size=IMG)
    ops = rep.profile([torch.from_numpy(x).cuda()], torch.empty(ref.shape, device="cuda"),
                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    names = [o["name"] for o in ops]
    assert [n for n in names if n.startswith("window_attn_")] == [
        "window_attn_c64_h28_s0", "window_attn_c64_h28_s3", "window_attn_c128_h14_s0", "window_attn_c128_h14_s3",
        "window_attn_c256_h7_s0", "window_attn_c256_h7_s0"], names
    assert [n for n in names if n.startswith("s2d_ln_")] == ["s2d_ln_c64", "s2d_ln_c128"], names
    assert sum(n.startswith("avgpool_fc_") for n in names) == 1, names


def test_swin_u8_task_with_image_outputs(spi, gpu):
    # an 8-bit NHWC task under an input transform, softmax + top-3 outputs, against the oracle on the normalised image
    m, _, _ = case(SMALL)
    u8 = np.random.default_rng(2).integers(0, 256, (2, IMG, IMG, 3), dtype=np.uint8)
    scale, shift = [1 / 255.0 / s for s in (0.229, 0.224, 0.225)], [-mu / s for mu, s in zip((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))]
    ref = cpu_inference(m, [np.ascontiguousarray((u8.astype(np.float32) * np.float32(scale) + np.float32(shift)).transpose(0, 3, 1, 2))])[0]
    rep = spi.ModelReplica(m, 0, "fp32", max_batch=2, image_size=IMG, image_io=("probs", "topk"), top_k=3)
    rep.set_input_transform(scale, shift)
    assert rep.description.endswith(" out[logits,probs,top3]"), rep.description
    outs = [torch.full(s, float("nan") if dt == torch.float32 else -1, dtype=dt, device="cuda")
            for s, dt in spi.output_specs(2, 10, rep.image_io, rep.top_k)]
    torch.cuda.synchronize()
    spi.run_hip(rep, [torch.from_numpy(u8).cuda()], outs, stream=torch.cuda.Stream().cuda_stream)
    torch.cuda.synchronize()
    logits, probs, topv, topi = (o.cpu().numpy() for o in outs)
    err = normalized_max_error(logits, ref)
    print(f"swin embed 64 fp32 u8 nhwc: err {err:.3e}")
    assert err < 1e-5
    e = np.exp(logits.astype(np.float64) - logits.max(1, keepdims=True))  # the launch's own input
    assert normalized_max_error(probs, e / e.sum(1, keepdims=True)) < 1e-5
    assert np.array_equal(topi, np.argsort(-logits, kind="stable")[:, :3])
    assert np.array_equal(topv, np.take_along_axis(logits, topi, 1))

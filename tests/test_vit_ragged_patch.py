"""ViT patch rows that are no whole number of the dense GEMM's 16-byte A chunks (patch 14: K = 3 * 14 * 14 = 588
fp16, 1176 bytes): the patch projection's last chunk of a row also reads the first 8 bytes behind the row,
against zero weights.  The workspace plan ends the patch buffer with 16 bytes for the last row's chunk and the
replica zeroes the buffer once, so what is read is finite whatever the allocation held before.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle.cpu_codelet import cpu_inference, normalized_max_error


def plan_bytes(spi, rep):
    out = (C.c_size_t * 32)()
    n, floats, before = C.c_int32(0), C.c_size_t(0), C.c_size_t(0)
    assert spi.lib.spi_model_workspace_plan(rep.handle, out, 32, C.byref(n), C.byref(floats), C.byref(before)) == 0
    return list(out[:n.value])


@pytest.mark.parametrize("prec,es", [("fp16", 2), ("fp32", 4)])
def test_patch_buffer_ends_with_a_chunk_when_rows_are_ragged(spi, zoo, prec, es):
    """Buffer 0 (kVtPatches): max_batch * patches * K elements, plus 16 bytes only where K * es % 16 != 0."""
    B = 3
    for patch, ragged in ((14, {2: True, 4: False}), (16, {2: False, 4: False}), (6, {2: True, 4: False}),
                          (5, {2: True, 4: True})):
        image = 4 * patch  # 16 patches
        m = zoo.vit(image=image, patch=patch, layers=1, heads=2, dim=128, mlp_dim=256, num_classes=10)
        rep = spi.ModelReplica(m, -1, prec, max_batch=B, num_heads=2, image_size=image)
        K = 3 * patch * patch
        assert ((K * es) % 16 != 0) == ragged[es]
        assert plan_bytes(spi, rep)[0] == B * 16 * K * es + (16 if ragged[es] else 0), (patch, prec)


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 2])  # below max_batch: the rows behind the task's; at it: the tail
def test_ragged_patch_rows_read_nothing_stale(spi, zoo, gpu, batch):
    """Fresh replicas of a patch-14 ViT right after NaN-filled allocations of every size class were freed:
    the logits are finite, the same bits replica after replica, and the oracle's at test_parity_gpu's fp16 bar,
    which is set for that file's images: uniform in [0, 1).  (A first version drew N(0, 1) pixels, three times
    the spread the bar was measured for, and sat at 1.05e-3 / 1.11e-3 with every value finite.)"""
    image, patch = 224, 14  # test_parity_gpu's patch-14 model (6.6e-4 there), whose cases showed the stale read
    m = zoo.vit(image=image, patch=patch, layers=2, heads=4, dim=256, mlp_dim=512)
    x = np.random.default_rng(batch).random((batch, 3, image, image), dtype=np.float32)
    ref = cpu_inference(m, [x])[0]
    xin = torch.from_numpy(x).cuda()
    first = None
    for _ in range(4):
        junk = [torch.full((n,), float("nan"), device="cuda", dtype=torch.float16) for n in (1 << 8, 1 << 12, 1 << 16, 1 << 20)]
        torch.cuda.synchronize()
        del junk
        torch.cuda.empty_cache()  # back to the driver, where the replica's workspace comes from
        rep = spi.ModelReplica(m, 0, "fp16", max_batch=2, image_size=image)
        out = torch.full(ref.shape, float("nan"), device="cuda")
        spi.run_hip(rep, [xin], out)
        got = out.cpu().numpy()
        assert np.isfinite(got).all()
        err = normalized_max_error(got, ref)
        print(f"vit patch 14 batch {batch} of 2, fresh replica: {err:.3e}")
        assert err < 1e-3
        first = got if first is None else first
        assert np.array_equal(got, first), "fresh replicas differ: something unwritten was read"

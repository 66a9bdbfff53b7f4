"""32-wide attention heads beside the 64-wide ones, on host-only replicas (device id -1) and on the CPU: what the
packer accepts and refuses, where the head count comes from, the workspace plan of a 32-wide replica, and the
CPU emulation whose worst case sets the fp16 bar of test_attention_hd32_ops_gpu.py.

Emulation figure measured here (normalised max error against the float64 reference on the same fp16 operand):
  attention, width 32, scale 1 / sqrt(32), over hd_refs.ATTN_CASES: worst 4.49e-4 at (1, 257, 4 heads, "head")."""
import ctypes as C

import numpy as np
import pytest

import hd_refs as H
import op_refs as R

PRECS = ["fp32", "fp16", "fp16m", "fp16x3"]
TOL_QKV = 1.5e-3  # test_qkv_attention_ops_gpu.TOL_QKV (a GPU module: not imported here)


def bert32(zoo, **kw):
    return zoo.bert(**{**dict(layers=2, hidden=128, heads=4, intermediate=512, vocab=1000), **kw})


@pytest.mark.parametrize("prec", PRECS)
def test_four_heads_of_32_build(spi, zoo, prec):
    rep = spi.ModelReplica(bert32(zoo), -1, prec, num_heads=4)
    assert " H4 " in rep.description and " D128 " in rep.description, rep.description


def test_head_count_comes_from_the_module(spi, zoo):
    assert " H4 " in spi.ModelReplica(bert32(zoo), -1, "fp16", num_heads=0).description
    assert " H4 " in spi.ModelReplica(bert32(zoo), -1, "fp16").description
    assert " H2 " in spi.ModelReplica(bert32(zoo, heads=2), -1, "fp16").description
    vit = zoo.vit(image=32, patch=8, layers=2, heads=4, dim=128, mlp_dim=256, num_classes=10)
    assert " H4 " in spi.ModelReplica(vit, -1, "fp16", image_size=32).description
    vit2 = zoo.vit(image=32, patch=8, layers=2, heads=2, dim=128, mlp_dim=256, num_classes=10)
    assert " H2 " in spi.ModelReplica(vit2, -1, "fp16", image_size=32).description


def test_explicit_head_count_wins(spi, zoo):
    # the weights do not depend on the head count: the four-head module packed as two 64-wide heads
    rep2 = spi.ModelReplica(bert32(zoo), -1, "fp16", num_heads=2)
    rep4 = spi.ModelReplica(bert32(zoo), -1, "fp16", num_heads=4)
    assert " H2 " in rep2.description and " H4 " in rep4.description
    assert rep2.weight_bytes == rep4.weight_bytes


def test_zoo_minilm(spi, zoo):
    m = zoo.build("minilm_l6", vocab=1000)
    cfg = m.bert.config
    assert (cfg.num_hidden_layers, cfg.hidden_size, cfg.num_attention_heads, cfg.intermediate_size) == (6, 384, 12, 1536)
    d = spi.ModelReplica(m, -1, "fp16", seq_len=128).description
    assert "L6 " in d and " D384 " in d and " H12 " in d and " FF1536 " in d, d
    assert zoo.build("minilm_l12", vocab=1000).bert.config.num_hidden_layers == 12


@pytest.mark.parametrize("heads,why", [(8, "head dim 16"), (1, "head dim 128"), (3, "not a divisor")])
def test_other_widths_are_refused(spi, zoo, heads, why):
    with pytest.raises(spi.InferenceExecutionException) as e:
        spi.ModelReplica(bert32(zoo), -1, "fp16", num_heads=heads)
    msg = str(e.value)
    assert "128" in msg and f"{heads} attention heads" in msg and "32 or 64" in msg, (why, msg)


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_plan_holds_every_launch(spi, zoo, prec):
    rep = spi.ModelReplica(bert32(zoo, max_position=512), -1, prec, max_batch=8, num_heads=4)
    for B in (1, rep.max_batch):
        for S in (1, 128, 300):
            n = C.c_int32(-1)
            st = spi.lib.spi_model_plan_check(rep.handle, B, S, C.byref(n))
            assert st == 0 and n.value >= 1, (B, S, st, spi.lib.spi_last_error().decode())


def test_attention_emulation_sets_the_fp16_bar():
    """The fp16 kernels' arithmetic on the CPU against float64 at width 32, over the parity list of the GPU test:
    every case within ATTN_EMU_WORST, the worst within a tenth of it (the constant is the measurement, rounded
    up), and three times it -- the GPU bar -- within the fused kernel's TOL_QKV."""
    errs = {}
    for B, S, heads, kind in H.ATTN_CASES:
        q16, mask = H.attn_case(B, S, heads).astype(np.float16), R.attn_mask(B, S, kind)
        ref = H.attention_ref(q16, mask, B, S, heads, H.SCALE)
        assert np.isfinite(ref).all()
        errs[(B, S, heads, kind)] = R.nerr(H.emulate_attention_f16(q16, mask, B, S, heads, H.SCALE), ref)
    worst = max(errs, key=errs.get)
    print(f"attention emulation width 32: worst {errs[worst]:.3e} at {worst}")
    assert 0.9 * H.ATTN_EMU_WORST <= errs[worst] <= H.ATTN_EMU_WORST
    assert 3 * H.ATTN_EMU_WORST <= TOL_QKV


@pytest.mark.parametrize("S,variant", [(S, v) for S, v in R.ATTN_EXACT_CASES if S in (1, 17, 129, 257, 577)])
def test_exact_cases_are_exact(S, variant):
    qkv, mask, want = H.attn_exact_case(S, variant)
    assert np.array_equal(qkv, qkv.astype(np.float16).astype(np.float32)) and (want != 0).all()
    got = H.attention_ref(qkv, mask, 2, S, 4, H.SCALE).reshape(2, S, 4, 32)[..., 0]
    assert want.shape == (2, S, 4) and (np.sign(want[..., 0]) == -np.sign(want[..., 1])).all()
    assert np.abs(got - want).max() < 1e-12
    emu = H.emulate_attention_f16(qkv, mask, 2, S, 4, H.SCALE).astype(np.float64).reshape(2, S, 4, 32)[..., 0]
    assert (np.abs(emu - want) / np.abs(want)).max() <= 2.0 ** -10
    # the neighbouring sub-head's column 0 (heads swapped in pairs) is off by twice the value: far past the bar
    assert (np.abs(got[..., [1, 0, 3, 2]] - want) / np.abs(want)).min() >= 2

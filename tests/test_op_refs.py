"""The references of tests/op_refs.py against the torch ops they restate, without a GPU -- what makes
the bars of test_qkv_attention_ops_gpu.py, test_attention_ops_gpu.py and test_elementwise_ops_gpu.py
trustworthy -- and the emulations of qkv_attn.hip's and attention.hip's arithmetic from which the fp16
attention kernels' GPU bars are taken."""
import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import op_refs as R

# The emulated kernel arithmetic (fp32 accumulation, fp16 q / k / v, fp16 P, fp16 output) against the
# float64 reference, normalised max error over every parity case.  Measured on such an emulation: 2.5e-4
# to 5.2e-4 over all the cases; the bar leaves that 15 % headroom.  The GPU bar is 3x its worst case.
EMU_TOL = 6e-4
# float64 against float64: summation order only
TOL64 = 1e-12


@pytest.fixture(scope="module")
def ops(spi):
    return importlib.import_module("starpu-inference-server_amd.ops")


# ---- fused QKV + attention ----------------------------------------------------------------------


@pytest.mark.parametrize("B,S,heads,masked", [(2, 17, 3, True), (1, 129, 2, False), (2, 64, 2, True)])
def test_qkv_ref_equals_sdpa_float64(ops, B, S, heads, masked):
    c = R.qkv_case(ops, B, S, heads, False, masked)
    got = R.qkv_attention_ref(c["A16"], c["W16"], c["bias"], c["mask"], B, S, heads, 0.125, round16=False)
    qkv = torch.from_numpy(c["A16"].astype(np.float64) @ c["W16"].astype(np.float64).T + c["bias"])
    q, k, v = qkv.view(B, S, 3, heads, 64).permute(2, 0, 3, 1, 4)
    m = None if c["mask"] is None else torch.from_numpy(c["mask"]).double()[:, None, None, :]
    ref = F.scaled_dot_product_attention(q, k, v, attn_mask=m, scale=0.125)
    ref = ref.permute(0, 2, 1, 3).reshape(B * S, heads * 64).numpy()
    assert R.nerr(got, ref) < TOL64


def test_qkv_ref_folded_equals_layernorm_linear_attention(ops):
    """The folded form on fold_linear's outputs (fp32 rows as A, so nothing but the weights is rounded):
    exactly LN(x) -> the fp16 folded weights, and LN -> linear -> attention to fp16-weight rounding."""
    B, S, heads = 2, 40, 3
    D = heads * 64
    c = R.qkv_case(ops, B, S, heads, True, True)
    x64 = c["x"].astype(np.float64)
    got = R.qkv_attention_ref(c["x"], c["W16"], c["bias"], c["mask"], B, S, heads, 0.125, stats=c["stats"], c1=c["c1"],
                              eps=R.EPS, round16=False)
    xhat = (x64 - x64.mean(1, keepdims=True)) / np.sqrt(x64.var(1, keepdims=True) + R.EPS)
    # rstd (x W'^T - mean c1) + b' = xhat W'^T + b' with W' the weights as packed.  What differs: the
    # statistics travel as fp32 (2^-24 relative on a mean of up to 6 sigma times c1) and c1 is an fp32 sum
    # of D fp16 weights: 1e-5 of max|ref| covers both with an order of magnitude to spare.
    same = R.qkv_attention_ref(xhat, c["W16"], c["bias"], c["mask"], B, S, heads, 0.125, round16=False)
    assert R.nerr(got, same) < 1e-5
    # against the unfolded layer in float64: LayerNorm -> linear (W, b before the fold) -> attention.
    # Each folded weight is rounded to fp16, 2^-11 relative; a 2^-11 relative error of q and k moves a
    # score by about 2^-11 sqrt(64) sigma^2 / 8 = 1e-3 and the output by that fraction of max|v|: 5e-3.
    rng = np.random.default_rng(B * S + heads)  # qkv_case's draw of W and b
    W = (rng.standard_normal((3 * D, D)) * 1.5 / np.sqrt(D)).astype(np.float32)
    b = (rng.standard_normal(3 * D) * 0.5).astype(np.float32)
    ln = F.layer_norm(torch.from_numpy(x64), (D,), torch.from_numpy(c["gamma"]).double(),
                      torch.from_numpy(c["beta"]).double(), R.EPS).numpy()
    ref = R.qkv_attention_ref(ln, W, b, c["mask"], B, S, heads, 0.125, round16=False)
    assert R.nerr(got, ref) < 5e-3


def test_qkv_ref_fully_masked_sequence_is_the_mean_of_v(ops):
    B, S, heads = 2, 19, 2
    c = R.qkv_case(ops, B, S, heads, False, False)
    mask = np.zeros((B, S), np.float32)
    mask[1, :] = R.FMIN
    got = R.qkv_attention_ref(c["A16"], c["W16"], c["bias"], mask, B, S, heads, 0.125)
    qkv = (c["A16"].astype(np.float64) @ c["W16"].astype(np.float64).T + c["bias"]).astype(np.float16)
    v = qkv.astype(np.float64)[S:, 2 * heads * 64:]
    assert np.abs(got[S:] - v.mean(0, keepdims=True)).max() < TOL64


@pytest.mark.parametrize("B,S,heads,fold,masked", R.QKV_CASES)
def test_qkv_emulation_within_bar(ops, B, S, heads, fold, masked):
    c = R.qkv_case(ops, B, S, heads, fold, masked)
    args = (c["A16"], c["W16"], c["bias"], c["mask"], B, S, heads, 0.125)
    kw = dict(stats=c["stats"], c1=c["c1"], eps=R.EPS)
    ref = R.qkv_attention_ref(*args, **kw)
    e = R.nerr(R.emulate_qkv_attention(*args, **kw), ref)
    print(f"emulation B{B} S{S} H{heads} fold{int(fold)} mask{int(masked)}: {e:.3e}")
    assert np.isfinite(ref).all() and e < EMU_TOL


def test_combine_stats_restated(ops):
    x = R.make_rows(np.random.default_rng(3), 9, 192).astype(np.float64)
    st = ops.chunk_stats(x)
    for a, b in zip(R.combine_stats64(st, R.EPS), ops.combine_stats(st, R.EPS)):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_allclose(R.combine_stats64(st, R.EPS)[1], 1 / np.sqrt(x.var(1) + R.EPS), rtol=1e-12)


# ---- the standalone attention kernels -----------------------------------------------------------


def _sdpa64(qkv, mask, B, S, heads, scale):
    q, k, v = torch.from_numpy(qkv.astype(np.float64)).view(B, S, 3, heads, 64).permute(2, 0, 3, 1, 4)
    m = None if mask is None else torch.from_numpy(mask).double()[:, None, None, :]
    o = F.scaled_dot_product_attention(q, k, v, attn_mask=m, scale=scale)
    return o.permute(0, 2, 1, 3).reshape(B * S, heads * 64).numpy()


@pytest.mark.parametrize("B,S,heads,kind,scale", [(2, 17, 3, None, 0.125), (2, 197, 3, "head", 0.125),
                                                  (1, 257, 2, "middle", 0.25), (2, 70, 2, "tail", 0.125)])
def test_attention_ref_equals_sdpa_float64(B, S, heads, kind, scale):
    qkv, mask = R.attn_case(B, S, heads), R.attn_mask(B, S, kind)
    got = R.attention_ref(qkv, mask, B, S, heads, scale)
    assert got.shape == (B * S, heads * 64) and got.dtype == np.float64
    assert R.nerr(got, _sdpa64(qkv, mask, B, S, heads, scale)) < TOL64


def test_attn_mask_kinds():
    assert R.attn_mask(2, 300, None) is None
    m = R.attn_mask(2, 300, "head") != 0
    assert m[1, :70].all() and not m[1, 70:].any() and m[0, :3].all() and not m[0, 3:].any()
    assert not (R.attn_mask(1, 300, "head") != 0)[0, 70:].any() and (R.attn_mask(1, 300, "head") != 0)[0, :70].all()
    m = R.attn_mask(2, 17, "head") != 0  # keys 0 .. S - 2: the last key stays
    assert m[1, :16].all() and not m[1, 16]
    m = R.attn_mask(2, 300, "middle") != 0
    assert m[1, 123:197].all() and m[1].sum() == 74 and not m[0].any()
    assert (R.attn_mask(1, 150, "middle") != 0)[0].nonzero()[0].tolist() == list(range(123, 150))
    assert not R.attn_mask(2, 100, "middle").any()
    m = R.attn_mask(2, 225, "tail") != 0
    assert m[1, 112:].all() and not m[1, :112].any() and not m[0].any()
    for B, S, _, kind in R.ATTN_CASES:  # a masked value is FMIN, and no sequence of a parity case is masked whole
        m = R.attn_mask(B, S, kind)
        assert m is None or (set(np.unique(m)) <= {0.0, R.FMIN} and (m == 0).any(axis=1).all())
    assert all(kind is None for (_, S, _, kind) in R.ATTN_CASES if S == 1)


@pytest.mark.parametrize("B,S,heads,kind", R.ATTN_CASES)
def test_attention_emulation_within_bar(B, S, heads, kind):
    """The fp16 kernels' arithmetic on the CPU against the float64 reference on the same fp16 operand: the
    figure the fp16 GPU bar of test_attention_ops_gpu.py is three times of."""
    q16, mask = R.attn_case(B, S, heads).astype(np.float16), R.attn_mask(B, S, kind)
    ref = R.attention_ref(q16, mask, B, S, heads, 0.125)
    e = R.nerr(R.emulate_attention_f16(q16, mask, B, S, heads, 0.125), ref)
    print(f"attention emulation B{B} S{S} H{heads} mask {kind}: {e:.3e}")
    assert np.isfinite(ref).all() and e <= R.ATTN_EMU_TOL


@pytest.mark.parametrize("S,variant", R.ATTN_EXACT_CASES)
def test_attention_exact_cases_are_exact(S, variant):
    """The near-exact inputs give the quotient they claim in the float64 reference, and the emulated fp16
    arithmetic lands within the GPU test's 2^-10."""
    qkv, mask, want = R.attn_exact_case(S, variant)
    assert np.array_equal(qkv, qkv.astype(np.float16).astype(np.float32)) and (want != 0).all()
    w = np.repeat(want.reshape(2 * S, 1), 2, axis=1)
    ref = R.attention_ref(qkv, mask, 2, S, 2, 0.125)[:, ::64]
    assert np.abs(ref / w - 1).max() < TOL64
    emu = R.emulate_attention_f16(qkv, mask, 2, S, 2, 0.125).astype(np.float64)[:, ::64]
    assert np.abs(emu / w - 1).max() <= 2.0 ** -10


@pytest.mark.parametrize("S", R.ATTN_EXACT_S)
def test_attention_exact_cases_discriminate(S):
    """One zero-valued padding key let into the softmax of the all-ones case moves the result from 1 to
    S / (S + 1): 1 / 578 = 1.7e-3 at the longest sequence, above the 2^-10 bar."""
    qkv, _, _ = R.attn_exact_case(S, "ones")
    leaky = np.zeros((2, S + 1, 384), np.float32)
    leaky[:, :S] = qkv.reshape(2, S, 384)
    got = R.attention_ref(leaky.reshape(-1, 384), None, 2, S + 1, 2, 0.125).reshape(2, S + 1, 128)[:, :S, ::64]
    off = np.abs(got - 1)
    assert abs(off.min() - 1 / (S + 1)) < TOL64 and off.min() > 1.5 * 2.0 ** -10


# ---- hi + lo weights (krep = 2) -----------------------------------------------------------------

# What the krep GPU tests (test_hilo_weight_ops_gpu.py, the fp16m pair of test_conv_pair_ops_gpu.py, the
# folded consumer of test_ln_fold_ops_gpu.py) can tell apart at their 1e-5 bar: a contraction over fp16(w)
# alone must sit above HI_ONLY_MIN from the hi + lo float64 reference, an fp32-accumulated emulation of the
# right arithmetic below EMU32_MAX.  Measured here over every case: hi only 1.1e-4 to 5.4e-4, emulation
# 1e-7 to 1.2e-6.
HI_ONLY_MIN, EMU32_MAX = 1e-4, 3e-6


def _dense_sides(form, M, N, K):
    A16, W, b, Rr = R.krep_dense_case(M, N, K)
    res, act = (Rr if form == "res32" else None), {"relu": "relu", "gelu": "gelu"}.get(form)
    ref = R.epilogue64(R.dense_acc64(A16, R.hilo_values(W)), b, res, act)
    hi = R.epilogue64(R.dense_acc64(A16, R.hi_values(W)), b, res, act)
    emu = R.epilogue64(R.dense_acc32_hilo(A16, W), b, res, act)
    return ref, hi, emu


def _conv_sides(B, H, cin, cout, k, stride, pad, res=False):
    x, [(w, b)] = R.conv_case(B, H, cin, [(cout, k, stride, pad)])
    x16 = x.astype(np.float16)
    ref = R.conv_acc(x16, R.hilo_values(w), stride, pad)
    r = np.random.default_rng(H + cout).standard_normal(ref.shape).astype(np.float32) if res else None
    return (R.epilogue64(ref, b, r), R.epilogue64(R.conv_acc(x16, R.hi_values(w), stride, pad), b, r),
            R.epilogue64(R.conv_acc32_hilo(x16, w, stride, pad), b, r))


def _pair_sides(case):
    """Conv 1 of a pair case, on the weights the pair test draws for it."""
    B, H, cin, c0, c1 = case
    x, wb = R.conv_case(B, H, cin, [c0, c1])
    x16, (w, b) = x.astype(np.float16), wb[1]
    return (R.epilogue64(R.conv_acc(x16, R.hilo_values(w), c1[2], c1[3]), b),
            R.epilogue64(R.conv_acc(x16, R.hi_values(w), c1[2], c1[3]), b),
            R.epilogue64(R.conv_acc32_hilo(x16, w, c1[2], c1[3]), b))


def _fold_sides(ops, M, N, K):
    A16, stats, wf, bias, c1 = R.krep_fold_case(ops, M, N, K)
    return (R.fold_consumer64(R.dense_acc64(A16, R.hilo_values(wf)), stats, c1, bias),
            R.fold_consumer64(R.dense_acc64(A16, R.hi_values(wf)), stats, c1, bias),
            R.fold_consumer32(R.dense_acc32_hilo(A16, wf), stats, c1, bias))


KREP_SIDES = (
    [(f"dense-{M}x{N}x{K}-{f}", _dense_sides, (f, M, N, K)) for (M, N, K) in R.KREP_DENSE for f in R.KREP_FORMS]
    + [("dense-gelu", _dense_sides, ("gelu",) + R.KREP_GELU)]
    + [(f"forced-{plan}", _dense_sides, ("plain",) + shape) for plan, shape in R.KREP_FORCED]
    + [("conv-" + "x".join(map(str, c)), _conv_sides, c) for c in R.KREP_CONV]
    + [("conv-res", _conv_sides, R.KREP_CONV_RES + (True,))]
    + [("pair-" + R.pair_id(c), _pair_sides, (c,)) for c in R.PAIR_HILO_CASES])


@pytest.mark.parametrize("what,sides,args", KREP_SIDES, ids=[s[0] for s in KREP_SIDES])
def test_krep_cases_discriminate(what, sides, args):
    ref, hi, emu = sides(*args)
    e_hi, e_emu = R.nerr(hi, ref), R.nerr(emu, ref)
    print(f"{what}: hi only {e_hi:.3e}, fp32 emulation {e_emu:.3e}")
    assert e_hi > HI_ONLY_MIN and e_emu < EMU32_MAX


@pytest.mark.parametrize("M,N,K", R.KREP_FOLD)
def test_krep_folded_consumer_discriminates(ops, M, N, K):
    ref, hi, emu = _fold_sides(ops, M, N, K)
    e_hi, e_emu = R.nerr(hi, ref), R.nerr(emu, ref)
    print(f"fold {M}x{N}x{K}: hi only {e_hi:.3e}, fp32 emulation {e_emu:.3e}")
    assert e_hi > HI_ONLY_MIN and e_emu < EMU32_MAX


def test_hilo_values_are_what_the_pack_holds(ops):
    """hilo_values against the packed image itself, and |lo| <= ulp(hi) / 2."""
    w = (np.random.default_rng(8).standard_normal((70, 96)) * 3).astype(np.float32)
    img = ops.pack_weight_hilo_host(w).astype(np.float64)
    blocks = img[:70].reshape(70, 2, 2, 64)  # [n][blk][hi | lo][64]
    np.testing.assert_array_equal((blocks[:, :, 0] + blocks[:, :, 1]).reshape(70, 128)[:, :96], R.hilo_values(w))
    assert (np.abs(R.hilo_values(w) - R.hi_values(w)) <= np.spacing(np.abs(w.astype(np.float16))).astype(np.float64) / 2).all()
    assert R.nerr(R.hilo_values(w), w.astype(np.float64)) < 2.0 ** -21


# ---- the conv kinds (test_conv_kinds_ops_gpu.py) --------------------------------------------------

TOL32, TOL16 = 1e-5, 2e-3  # the GPU bars: into an fp32 or split output, into an fp16 output


@pytest.fixture(scope="module")
def kind_table():
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_kind_plans.json")) as f:
        return json.load(f)


def _kind(table, setting, prec, shape, form="11"):
    key = R.kind_key(setting, prec, R.shape9(shape))
    route = table["routes"].get(key, {}).get(form, 0)
    return R.conv_kind_name(prec, R.shape9(shape), table["plans"][key], route)


def test_conv_kind_plan_table_pinned(spi, kind_table):
    """Every (setting, precision, shape) the GPU tests launch: the planner and the weight-resident route give
    exactly the recorded integers, so each GPU case id names the kind that case runs on."""
    keys = {R.kind_key(st, prec, shape): (st, prec, shape) for _, st, prec, shape in R.conv_kind_runs()}
    assert kind_table["settings"] == R.KIND_SETTINGS and set(kind_table["plans"]) == set(keys)
    bad = []
    for key, (st, prec, shape) in keys.items():
        with R.kind_knobs(spi.lib, st):
            got = R.query_conv_plan(spi.lib, prec, shape)
            routes = {f: R.query_conv_route(spi.lib, prec, shape, f[0] == "1", "relu" if f[1] == "1" else None)
                      for f in kind_table["routes"].get(key, {})}
        if got != kind_table["plans"][key] or routes != kind_table["routes"].get(key, {}):
            bad.append((key, got, routes))
    assert not bad, f"{len(bad)} cases differ from the table, first: {bad[:3]}"
    assert set(kind_table["routes"]) == {k for k, (_, prec, s) in keys.items() if prec == "fp16" and s[3:5] == (64, 64)}


def test_conv_kind_table_reaches_every_kind(kind_table):
    """What the table has to say for the GPU file to cover the seven device paths (and each form of them)."""
    S = R.CONV3_SHAPES
    def pl(st, prec, name):
        return dict(zip(R.PLAN_FIELDS, kind_table["plans"][R.kind_key(st, prec, R.shape9(S[name]))]))

    for prec in ("fp16", "fp16x3s"):
        es = 64 if prec == "fp16" else 32
        for name in S:
            if name != "S10":  # the default rule
                want = "halo64" if name in ("S4", "S9") else "halo128" if name == "S7" else "win64x4"
                assert _kind(kind_table, "rule", prec, S[name]).split("-")[0] == want, (prec, name)
            p = pl("win1", prec, name)  # halo off: the window on 4 waves, S10 at 128 x 64 in one slice
            assert (p["win"], p["halo"], p["nw"], p["bn"]) == (1, 0, 4, 64) and p["bm"] == (128 if name == "S10" else 64)
            assert name != "S10" or p["splits"] == 1
            p = pl("win2", prec, name)  # 8 waves exactly where the k-steps are a multiple of 6
            ksteps = 9 * S[name][3] // es
            assert p["win"] == 1 and p["nw"] == (8 if ksteps % 6 == 0 and name != "S10" else 4), (prec, name, p)
            p = pl("win0", prec, name)  # the plain tap walk: 2 stages, 3 from 12 k-steps per slice (split S10: 18)
            assert (p["win"], p["halo"], p["stages"]) == (0, 0, 3 if p["k_per_split"] // es >= 12 else 2), (prec, name, p)
            assert p["stages"] == 2 or (prec, name) == ("fp16x3s", "S10"), (prec, name, p)
        assert [n for n in S if pl("win2", prec, n)["nw"] == 8] == \
            (["S2", "S4", "S9"] if prec == "fp16" else [n for n in S if n != "S10"])
    for prec in ("fp32", "fp16", "fp16x3s"):
        for name in S:
            if name == "S10":
                continue
            halo = pl("halo64a", prec, name)["halo"]
            if name in ("S1", "S2", "S6"):
                assert halo == 2, (prec, name)
            elif name in ("S4", "S5", "S9"):
                assert halo == 1, (prec, name)
            elif name in ("S7", "S8"):  # no 64-row candidate fits: the window kind, for fp32 the tap walk
                assert halo == 0 and pl("halo64a", prec, name)["win"] == (prec != "fp32"), (prec, name)
            for rows in (128, 256):
                for m in "as":
                    p = pl(f"halo{rows}{m}", prec, name)
                    assert (p["halo"], p["bm"], p["nw"]) == (1, rows, 8 if rows == 256 else 4), (prec, name, rows, m)
    assert not any(p[5] for k, p in kind_table["plans"].items() if "|fp32|" in k), "fp32 never takes the window kind"
    p = pl("rule-max3", "fp16x3s", "S9")
    assert p["halo"] == 1 and p["splits"] == 3 and (S["S9"][3] // 32) % p["splits"], p  # 8 blocks in 3 slices
    kinds = {_kind(kind_table, st, prec, shape).split("-")[0] for _, st, prec, shape in R.conv_kind_runs()}
    assert {"wres", "halo64", "haloS64", "halo128", "halo256", "win64x4", "win64x8", "win128x4", "tap64x64",
            "tap128x64", "tap128x128", "gen64x64", "gen128x64", "gen128x128"} <= kinds, kinds
    geo = {s: {prec: _kind(kind_table, "default", prec, s) for prec in R.CONV_PRECS if R.conv_accepts(prec, s)}
           for s in R.CONV_GEO_SHAPES}
    assert geo[(1, 11, 7, 32, 64, 3, 1, 2, 1)] == {"fp32": "tap64x64", "fp16": "gen64x64", "fp16x3": "tap64x64",
                                                   "fp16x3s": "tap64x64"}
    assert all(k.startswith("gen") for k in geo[(1, 10, 12, 64, 64, 7, 7, 2, 3)].values())
    assert "fp16x3s" not in geo[(1, 10, 12, 64, 64, 7, 7, 2, 3)] and "fp16x3s" not in geo[(1, 9, 11, 16, 24, 3, 3, 1, 1)]
    assert all(k.startswith("gen") for k in geo[(1, 9, 11, 16, 24, 3, 3, 1, 1)].values())


def test_weight_resident_route(spi):
    """spi_debug_conv_route without a device: SPI_CONV_WRES=2 takes every weight-resident shape but the
    84-wide one (its one-row halo, 3 x 86 pixels, no longer fits 256), =0 takes none, and nothing but an fp16
    3x3 / s1 / p1 64 -> 64 conv without GELU is ever routed there."""
    for shape in R.WRES_SHAPES:
        s = R.shape9(shape)
        for res in (False, True):
            for act in (None, "relu"):
                with R.kind_knobs(spi.lib, "wres2"):
                    assert R.query_conv_route(spi.lib, "fp16", s, res, act) == int(shape != R.WRES_REFUSED), shape
                    assert R.query_conv_route(spi.lib, "fp16x3s", s, res, act) == 0
                with R.kind_knobs(spi.lib, "wres0"):
                    assert R.query_conv_route(spi.lib, "fp16", s, res, act) == 0, shape
    with R.kind_knobs(spi.lib, "wres2"):
        assert spi.lib.spi_debug_conv_route(1, 1, 8, 8, 64, 64, 3, 3, 1, 1, 0, 2) == 0  # GELU
        assert spi.lib.spi_debug_conv_route(1, 1, 8, 8, 64, 64, 3, 3, 2, 1, 0, 0) == 0  # stride 2
        assert spi.lib.spi_debug_conv_route(1, 1, 8, 8, 64, 128, 3, 3, 1, 1, 0, 0) == 0
        assert spi.lib.spi_debug_conv_route(1, 1, 8, 8, 64, 64, 3, 3, 1, 1, 0, 0) == 1
        assert spi.lib.spi_debug_conv_route(7, 1, 8, 8, 64, 64, 3, 3, 1, 1, 0, 0) == -1


def test_split_values_are_what_the_layout_holds(ops):
    x = (np.random.default_rng(9).standard_normal((2, 3, 5, 64)) * 5).astype(np.float32)
    back = ops.from_split(ops.to_split(torch.from_numpy(x))).numpy()
    np.testing.assert_array_equal(R.split_values(x), back.astype(np.float64))
    xv, wv = R.operand_values("fp16", x, x)
    np.testing.assert_array_equal(xv, x.astype(np.float16).astype(np.float64))
    np.testing.assert_array_equal(wv, xv)
    xv, wv = R.operand_values("fp16x3s", x, x)
    np.testing.assert_array_equal(xv, R.split_values(x))
    np.testing.assert_array_equal(wv, x.astype(np.float64))


def test_conv_acc_takes_rectangles():
    """conv_case / conv_acc on an H x W map and a KH x KW filter against a direct sum, and the square callers'
    draws unchanged."""
    x, [(w, _)] = R.conv_case(2, 5, 4, [(3, (1, 3), 2, 1)], W=8)
    assert x.shape == (2, 5, 8, 4) and w.shape == (3, 1, 3, 4)
    got = R.conv_acc(x, w, 2, 1)
    xp = np.zeros((2, 7, 10, 4))
    xp[:, 1:6, 1:9] = x
    want = np.zeros((2, 4, 4, 3))
    for oh in range(4):
        for ow in range(4):
            want[:, oh, ow] = np.einsum("bkc,nkc->bn", xp[:, 2 * oh, 2 * ow:2 * ow + 3], w[:, 0].astype(np.float64))
    assert got.shape == want.shape and np.abs(got - want).max() < TOL64
    xs, [(ws_, bs)] = R.conv_case(2, 5, 4, [(3, 3, 1, 1)])
    rng = np.random.default_rng(2 * 1000 + 5 * 10 + 4)
    np.testing.assert_array_equal(xs, rng.standard_normal((2, 5, 5, 4)).astype(np.float32))
    np.testing.assert_array_equal(ws_, (rng.standard_normal((3, 3, 3, 4)) * np.sqrt(2.0 / 36)).astype(np.float32))


@pytest.mark.parametrize("name", list(R.CONV3_SHAPES))
@pytest.mark.parametrize("prec", ["fp16", "fp16x3s"])
def test_conv_kind_cases_discriminate(name, prec):
    """For the GPU file's inputs: the right arithmetic (an fp32-accumulated torch conv of the same operands)
    stays 3x below the bars, and each indexing slip a window, band or tap-walk kernel can make -- no column /
    row / image mask, H and W exchanged, the images joined into one -- sits at least 10x above them."""
    shape = R.shape9(R.CONV3_SHAPES[name])
    x, w, b, r = R.conv_kind_case(shape)
    xv, wv = R.operand_values(prec, x, w)
    rv = R.operand_values(prec, r)
    ref = R.epilogue64(R.conv_acc(xv, wv, 1, 1), b, rv, "relu")
    emu = R.epilogue64(R.conv_acc(xv.astype(np.float32), wv.astype(np.float32), 1, 1, torch.float32), b, rv, "relu")
    if prec == "fp16":
        e32, e16 = R.nerr(emu, ref), R.nerr(emu.astype(np.float16), ref)
    else:  # fp32 accumulation of hi + lo operands: the fp32 sum of the split values stands in for them
        e32, e16 = R.nerr(emu, ref), None
    wrong = {"flat": R.conv3_flat_unmasked(xv, wv, shape), "hw": R.conv3_hw_exchanged(xv, wv, shape)}
    if shape[0] > 1:
        wrong["joined"] = R.conv3_images_joined(xv, wv, shape)
    # the window kind's own walk: right as it stands, wrong without the mask's column terms and with d.H
    # written for d.W in the window's first pixel (which a square map cannot see)
    bm = 128 if name == "S10" else 64
    assert R.nerr(R.conv3_window_walk(xv, wv, shape, bm), R.conv_acc(xv, wv, 1, 1)) < TOL64
    wrong["window-no-column-mask"] = R.conv3_window_walk(xv, wv, shape, bm, col_mask=False)
    wrong["window-h-for-w"] = R.conv3_window_walk(xv, wv, shape, bm, pitch=shape[1])
    errs ={k: R.nerr(R.epilogue64(v, b, rv, "relu"), ref) for k, v in wrong.items()}
    print(f"{name} {prec}: fp32 accumulation {e32:.3e}" + (f", rounded to fp16 {e16:.3e}" if e16 else "") +
          "; wrong convs " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    assert 3 * e32 < TOL32 and (e16 is None or 3 * e16 < TOL16)
    bar = TOL16 if prec == "fp16" else TOL32
    assert all(v > 10 * bar for v in errs.values()), errs


def test_conv_exact_cases_are_exact(ops):
    """Every shape the GPU file launches has an integer case whose reference stays within 2048 (asserted by
    the builder), whose operands every layout holds exactly, and which an fp32-accumulated conv reproduces
    to the bit."""
    shapes = list(dict.fromkeys(s for _, _, _, s in R.conv_kind_runs()))
    assert len(shapes) == len(R.CONV3_SHAPES) + len(R.WRES_SHAPES) + len(R.CONV_GEO_SHAPES)
    for shape in shapes:
        x, w, b, r, ref = R.conv_exact_case(shape)
        assert np.abs(ref).max() <= R.EXACT_MAX and ref.shape[1:3] == R.conv_out_hw(shape)
        for a in (x, w, b, r, ref):
            np.testing.assert_array_equal(a.astype(np.float16).astype(np.float64), a)
        np.testing.assert_array_equal(R.split_values(x), x)
        emu = R.epilogue64(R.conv_acc(x, w, shape[7], shape[8], torch.float32), b, r, "relu")
        np.testing.assert_array_equal(emu, ref)
    t = torch.from_numpy(ref.astype(np.float32))
    np.testing.assert_array_equal(ops.from_split(ops.to_split(t)).numpy(), ref)


# ---- the HBM-bound kernels ----------------------------------------------------------------------


@pytest.mark.parametrize("k,stride,pad", [(3, 2, 1), (2, 2, 0)])
@pytest.mark.parametrize("B,H,W,C", [(1, 5, 5, 8), (2, 9, 7, 64), (1, 113, 57, 32)])
def test_maxpool_ref_equals_torch(B, H, W, C, k, stride, pad):
    x = np.random.default_rng(H * W + C).standard_normal((B, H, W, C)).astype(np.float32)
    ref = F.max_pool2d(torch.from_numpy(x).permute(0, 3, 1, 2), k, stride, pad).permute(0, 2, 3, 1).numpy()
    got = R.maxpool_ref(x, k, stride, pad)
    assert got.dtype == np.float32 and got.shape == ref.shape
    np.testing.assert_array_equal(got, ref)


def test_avgpool_ref_equals_torch():
    x = np.random.default_rng(1).standard_normal((3, 49, 96)).astype(np.float32)
    ref = F.adaptive_avg_pool1d(torch.from_numpy(x).double().permute(0, 2, 1), 1)[..., 0].numpy()
    assert R.nerr(R.avgpool_ref(x), ref) < TOL64


def test_bert_embed_ref_equals_torch():
    rng = np.random.default_rng(2)
    vocab, npos, D, B, S = 50, 128, 200, 3, 7
    word, pos = (rng.standard_normal((n, D)).astype(np.float32) for n in (vocab, npos))
    type0, gamma, beta = (rng.standard_normal(D).astype(np.float32) for _ in range(3))
    ids = rng.integers(0, vocab, B * S)
    ids[:5] = [0, vocab - 1, -1, vocab, 2 ** 40]
    got = R.bert_embed_ref(ids, word, pos, type0, gamma, beta, S, 1e-12)
    t = lambda a: torch.from_numpy(a).double()  # noqa: E731
    emb = F.embedding(torch.from_numpy(np.clip(ids, 0, vocab - 1)), t(word)) + t(type0) + t(pos)[:S].repeat(B, 1)
    ref = F.layer_norm(emb, (D,), t(gamma), t(beta), 1e-12).numpy()
    # the reference adds in fp32 as the kernels do, torch here in float64: two fp32 roundings, 2^-23
    assert R.nerr(got, ref) < 1e-6
    # row 2 holds id -1: word row 0 at position 2
    np.testing.assert_array_equal(got[2], R.bert_embed_ref(np.int64([0]), word, pos[2:], type0, gamma, beta, 1, 1e-12)[0])


def test_ingest_ref_equals_permute_pad():
    rng = np.random.default_rng(4)
    x = rng.standard_normal((2, 3, 5, 7)).astype(np.float32)
    ref = F.pad(torch.from_numpy(x).permute(0, 2, 3, 1), (0, 5))
    np.testing.assert_array_equal(R.ingest_ref(x, 8, False), ref.numpy())
    np.testing.assert_array_equal(R.ingest_ref(x, 8, True), ref.half().numpy())
    u8 = rng.integers(0, 256, (2, 5, 7, 3), dtype=np.uint8)
    scale, shift = np.float32([0.017, 0.0175, 0.0174]), np.float32([-2.1, -2.0, -1.8])
    img = R.xf_image(u8, True, scale, shift)
    want = torch.from_numpy(u8).permute(0, 3, 1, 2).float() * torch.from_numpy(scale).view(1, 3, 1, 1)
    want = want + torch.from_numpy(shift).view(1, 3, 1, 1)  # two torch ops: two fp32 roundings
    np.testing.assert_array_equal(img, want.numpy())
    np.testing.assert_array_equal(R.xf_image(np.ascontiguousarray(u8.transpose(0, 3, 1, 2)), False, scale, shift), img)


def test_split_round_trips(ops):
    x = torch.from_numpy(np.random.default_rng(5).standard_normal((3, 4, 64)).astype(np.float32)) * 7
    s = ops.to_split(x)
    back = ops.from_split(s)
    # hi + lo keeps 22 significant bits, |x - (hi + lo)| <= 2^-22 |x|, until lo is an fp16 subnormal
    # (spacing 2^-24: half of it)
    assert bool(((back - x).abs() <= torch.clamp(x.abs() * 2.0 ** -22, min=2.0 ** -25)).all())
    # a value the layout holds is a fixed point: split -> values -> split gives the same bits
    assert torch.equal(ops.to_split(back).view(torch.int16), s.view(torch.int16))


def test_small_refs_equal_torch():
    rng = np.random.default_rng(6)
    mask = rng.integers(0, 2, 37)
    ref = (1.0 - torch.from_numpy(mask).float()) * torch.finfo(torch.float32).min
    np.testing.assert_array_equal(R.mask_to_bias_ref(mask), ref.numpy())
    patches, cls, pos = (rng.standard_normal(s).astype(np.float32) for s in ((2, 9, 40), (40,), (10, 40)))
    t = torch.cat([torch.from_numpy(cls).expand(2, 1, 40), torch.from_numpy(patches)], 1) + torch.from_numpy(pos)
    np.testing.assert_array_equal(R.vit_assemble_ref(patches, cls, pos), t.numpy())
    x = rng.standard_normal((21, 12)).astype(np.float32)
    np.testing.assert_array_equal(R.gather_rows_ref(x, 4, 5, False), x[[0, 5, 10, 15]])
    np.testing.assert_array_equal(R.gather_rows_ref(x, 4, 5, True), torch.from_numpy(x[[0, 5, 10, 15]]).half().numpy())


# ---- the fused stem (test_stem_ops_gpu.py) ------------------------------------------------------


def moved(mutant, ref):
    """The largest move of an output element, in units of max|ref| (what normalized_max_error would report)."""
    return R.nerr(mutant, ref)


@pytest.mark.parametrize("B,H,W,kind", [(3, 9, 7, "rand"), (1, 13, 190, "rand"), (3, 1, 223, "rand")])
def test_stem_ref_equals_torch_float64(B, H, W, kind):
    x, _, w, b = R.stem_case(B, H, W, kind)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))  # noqa: E731
    ref = F.max_pool2d(F.relu(F.conv2d(t(x), t(w), t(b), 2, 3)), 3, 2, 1).permute(0, 2, 3, 1).numpy()
    got = R.stem_ref(x.astype(np.float64), w.astype(np.float64), b)
    assert got.shape == (B,) + R.stem_out_hw(H, W)[2:] + (64,)
    assert R.nerr(got, ref) < TOL64


def test_stem_shapes_reach_the_edges_they_name():
    """The case table against test_stem_ops_gpu's docstring: every width and height the kernel's paths turn
    on, odd image starts, and which shapes run the 8-wave form."""
    widths, heights = {s[2] for s in R.STEM_SHAPES}, {s[1] for s in R.STEM_SHAPES}
    assert widths >= {1, 7, 8, 47, 127, 128, 129, 130, 131, 132, 190, 221, 222, 223, 224}
    assert heights >= {1, 2, 9, 10, 11, 13, 23, 40}
    geo = {s[:3]: R.stem_out_hw(s[1], s[2]) for s in R.STEM_SHAPES}
    assert geo[(1, 2, 129)] == (1, 65, 1, 33) and geo[(1, 23, 130)][1] == 65  # a second group of one column
    assert geo[(3, 9, 131)][1:] == (66, 3, 33) and geo[(1, 11, 132)][1] == 66  # of two; PH odd under PR = 2
    assert any(ow > 64 and ph == 1 for (_, ow, ph, _) in geo.values())          # PH = 1 under PR = 2, 8 waves
    assert any(ow > 64 and ow % 2 and pw % 2 == 0 for (_, ow, _, pw) in geo.values())
    assert any(ow > 64 and pw % 2 for (_, ow, _, pw) in geo.values())           # odd PW
    assert sum(B == 3 and (3 * H * W) % 2 == 1 for (B, H, W, _) in R.STEM_SHAPES) >= 3  # images 16 bytes off
    assert {k for (_, _, _, k) in R.STEM_SHAPES} == {"rand", "randn"}
    for W in R.STEM_REFUSED_W:
        assert R.stem_out_hw(9, W)[1] == 113
    # the 8-wave form away from 224, and every form at every shape's three rows_per_block settings
    assert sum(R.stem_form(0, ow) == (2, 8) for (_, ow, _, _) in geo.values()) >= 8
    assert {R.stem_form(r, ow) for r in (0, 1, 2) for (_, ow, _, _) in geo.values()} == {(1, 4), (2, 4), (2, 8)}


@pytest.mark.parametrize("B,H,W,kind", R.STEM_SHAPES, ids=[f"{s[0]}x{s[1]}x{s[2]}" for s in R.STEM_SHAPES])
def test_stem_cases_discriminate(B, H, W, kind):
    """What a subtly wrong stem kernel computes, on the GPU test's own inputs: each mutant moves an output
    element by more than 10x the bar of the case that is to catch it (1e-5 into the split output for the two
    lo halves, which an fp16 output cannot see; 1e-3 for the rest, caught at every precision)."""
    x, u8, w, b = R.stem_case(B, H, W, kind)
    _, _, PH, PW = R.stem_out_hw(H, W)
    xv, wv = R.stem_operands(3, x, w)
    ref = R.stem_ref(xv, wv, b)
    got = {}
    if PW > 32:  # two groups: the column a group takes from the one before
        got["left neighbour at pooled column 32"] = (moved(R.stem_ref(xv, wv, b, no_left_at=32), ref), 1e-3)
    for PR in (1, 2):
        if PH > PR:
            got[f"recomputed row above, PR = {PR}"] = (moved(R.stem_ref(xv, wv, b, no_row_above=PR), ref), 1e-3)
    got["lo weights"] = (moved(R.stem_ref(xv, R.hi_values(w), b), ref), 1e-5)
    got["lo image"] = (moved(R.stem_ref(R.hi_values(x), wv, b), ref), 1e-5)
    xu = R.split_values(R.xf_image(u8, False, R.STEM_SCALE, R.STEM_SHIFT))
    got["padding as shift[c]"] = (moved(R.stem_ref(xu, wv, b, pad_value=R.split_values(R.STEM_SHIFT)),
                                        R.stem_ref(xu, wv, b)), 1e-3)
    if W > 3:  # tap kw = 6 is image column 2 ow + 3
        w6 = wv.copy()
        w6[..., 6] = 0
        got["tap kw = 6"] = (moved(R.stem_ref(xv, w6, b), ref), 1e-3)
    if W % 2:
        xl = xv.copy()
        xl[..., W - 1] = 0
        got["last column of an odd W"] = (moved(R.stem_ref(xl, wv, b), ref), 1e-3)
    print({k: f"{v / bar:.0f}x" for k, (v, bar) in got.items()})
    for name, (v, bar) in got.items():
        assert v > 10 * bar, f"{name}: moves {v:.2e}, bar {bar:.0e}"


@pytest.mark.parametrize("B,H,W", R.STEM_LATTICE_SHAPES)
def test_stem_lattice_cases_discriminate(B, H, W):
    """The lattice cases: the stored bits change when a lo half is dropped -- at every code that has it, and
    in the lo-weight variant at fp16m, whose fp16 output a parity bar of 1e-3 cannot hold to the lo weights."""
    for variant in ("mixed", "lowt"):
        _, x, w, b = R.stem_lattice_case(B, H, W, variant)
        for code in (1, 2, 3, 4):
            want = R.stem_expected_bits(code, R.stem_lattice_ref(code, x, w, b))
            assert float(want.astype(np.float64).max()) > 0
            if code >= 2:
                no_w = R.stem_expected_bits(code, R.stem_lattice_ref(code, x, w, b, drop_lo_w=True))
                assert not np.array_equal(no_w.view(np.int16), want.view(np.int16)), (variant, code)
            if code >= 3 and variant == "mixed":
                no_x = R.stem_expected_bits(code, R.stem_lattice_ref(code, x, w, b, drop_lo_x=True))
                assert not np.array_equal(no_x.view(np.int16), want.view(np.int16)), code
    # the lo-weight variant's interior is bias + 4 sum(lo), on the lattice and not the bias
    _, x, w, b = R.stem_lattice_case(B, H, W, "lowt")
    lo_sum = (R.hilo_values(w) - R.hi_values(w)).reshape(64, -1).sum(1)
    np.testing.assert_array_equal(R.stem_conv64(R.hi_values(x), R.hilo_values(w))[0, 2, 4], 4 * lo_sum)
    if H >= 14:  # a pooled pixel whose nine stem pixels are all interior
        np.testing.assert_array_equal(R.stem_lattice_ref(2, x, w, b)[0, 2, 3], b.astype(np.float64) + 4 * lo_sum)
    assert (np.abs(4 * lo_sum) >= 2.0 ** -10).sum() > 32  # above an fp16 ulp at 1 in most channels


def test_stem_split_bits_round_trip(ops):
    ref = np.random.default_rng(9).standard_normal((2, 3, 5, 64)) * 3
    bits = R.stem_split_bits(ref)
    want = ops.to_split(torch.from_numpy(ref.astype(np.float32))).view(torch.float16).numpy()
    np.testing.assert_array_equal(bits.view(np.int16), want.reshape(bits.shape).view(np.int16))
    assert R.nerr(R.stem_from_split(bits), ref) < 2.0 ** -21
    np.testing.assert_array_equal(R.stem_hi_of_split(bits), ref.astype(np.float32).astype(np.float16))


# ---- fused avgpool + FC (test_fc_ops_gpu.py) ----------------------------------------------------


def test_fc_ref_equals_torch_float64():
    x, W, b = R.fc_case(3, 7, 96, 70)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))  # noqa: E731
    ref = F.relu(F.linear(t(x).mean(1), t(W), t(b))).numpy()
    assert R.nerr(R.fc_ref(x, W, b, "relu"), ref) < TOL64


@pytest.mark.parametrize("case", R.FC_CASES, ids=["x".join(map(str, c[:4])) for c in R.FC_CASES])
def test_fc_cases_discriminate(case):
    """The pooled epilogue's slipped indices on the GPU test's inputs, each above 10x the 1e-5 bar wherever the
    case can show it: the next image's rows (B > 1, HW < 64), / 64 (HW < 64), a row part dropped (HW >= 4)."""
    B, HW, C, N, has_bias, act = case
    x, W, b = R.fc_case(B, HW, C, N)
    for prec in ("fp32", "fp16", "fp16x3s"):
        xv, wv = R.operand_values(prec, x, W)
        bias = b if has_bias else None
        ref = R.fc_ref(xv, wv, bias, act)
        assert np.abs(ref).max() > 0.1
        if B > 1 and HW < 64:
            assert moved(R.fc_ref(xv, wv, bias, act, "next"), ref) > 10 * R.FC_BAR
        if HW < 64:
            assert moved(R.fc_ref(xv, wv, bias, act, "div64"), ref) > 10 * R.FC_BAR
        if HW >= 4:
            assert moved(R.fc_ref(xv, wv, bias, act, "part3"), ref) > 10 * R.FC_BAR


def test_fc_case_table_covers_the_issue():
    col = lambda i: {c[i] for c in R.FC_CASES}  # noqa: E731
    assert col(1) >= {1, 2, 3, 4, 5, 7, 16, 49, 63, 64} and col(0) == {1, 3, 65}
    assert col(3) == {1, 64, 65, 70, 1000} and col(2) == {32, 96, 512, 2048}
    assert col(4) == {True, False} and col(5) == {None, "relu"}
    assert all(B * HW <= 320 for (B, HW, _, _, _, _) in R.FC_CASES)


@pytest.mark.parametrize("B,HW,C,N", R.FC_EXACT)
def test_fc_exact_case_is_exact(B, HW, C, N):
    x, W, b = R.fc_exact_case(B, HW, C, N)
    ref = R.fc_ref(x, W, b, None)
    assert np.array_equal(ref, ref.astype(np.float32)) and np.abs(x.reshape(B * HW, C) @ W.T).max() * HW < 2 ** 24
    for prec in ("fp16", "fp16x3s"):  # the operands survive every precision's rounding
        xv, wv = R.operand_values(prec, x, W)
        assert np.array_equal(xv, x) and np.array_equal(wv, W)
    assert not np.array_equal(R.fc_ref(x, W, b, None, "part3") if HW >= 4 else ref + 1, ref)


def test_forced_splits_restates_finish_plan(spi):
    """op_refs.forced_splits against the planner under SPI_GEMM_PLAN (the GPU tests assert plans with it)."""
    import ctypes as C
    import os
    try:
        for plan, (M, N, K) in R.DENSE32_FORCED:
            bm, bn, st, sp = (int(v) for v in plan.split(","))
            os.environ["SPI_GEMM_PLAN"] = plan
            spi.lib.spi_debug_gemm_reload_env()
            out = (C.c_longlong * 14)()
            assert spi.lib.spi_debug_gemm_plan(0, M, N, K, K, 1, 0, C.c_uint(0), out) == 0
            splits, kt = R.forced_splits(R.dense32_ksteps(K), sp if bn == 64 else 1)
            assert [int(v) for v in out[4:8]] == [bm, bn, st, splits] and int(out[11]) == kt * 32, (plan, list(out))
    finally:
        os.environ.pop("SPI_GEMM_PLAN", None)
        spi.lib.spi_debug_gemm_reload_env()

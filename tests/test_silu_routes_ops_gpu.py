"""Op-level parity of the SiLU epilogue (Act::Silu, act 3 of spi_op_gemm and spi_op_conv2d) on every route an
EfficientNet forward takes it through, and of the fp16 dense GEMM with an fp16 output at EfficientNet's shapes
(K below one k-step, N across a tile edge), which had no op test: the general kernel's vector, per-element and
split-K epilogues on 64 x 64, 128 x 64 and 128 x 128 tiles, fp16x3 / fp16x3s, gemm256 at both tile heights with
its scalar epilogue, fp16 residual and split-K, and the window, halo, tap-walk and gather conv kinds.  The
weight-resident conv has no SiLU: it must refuse, and the general kernel's output must not depend on the knob.

House rules (test_fc_ops_gpu.py's): the reference is float64 on the values the kernel multiplies
(op_refs.operand_values; a residual as its tensor holds it); every output is followed by 8 guard rows of NaN
(and NaN in the slack of a strided C) that must survive; every launch runs twice on the module's one workspace,
never re-zeroed, to identical bits; the route is asserted through spi_debug_gemm_plan / spi_debug_conv_plan /
spi_debug_conv_route before a launch, under knobs that op_refs.gemm_knobs / kind_knobs put back on the way out.
The launches are op_refs.silu_gemm_runs(): test_op_refs.py shows on the CPU, for the same inputs, that a quarter
of every case's pre-activations are negative and that GELU for SiLU, a sigmoid without the product, SiLU before
the residual, SiLU per split-K slice and ReLU on the negative lobe each sit above 10x the bar.

Two figures per case, both held to the case's bar: the normalised max error, and op_refs.silu_lobe_err -- the
max error over the entries whose pre-activation is <= 0, over the lobe's depth 0.2785 (SiLU forms only; the
"res" form has no activation).  Bars, from the tests that hold the same routes with ReLU / GELU: 1e-5 for fp32,
fp16x3 and fp16x3s outputs and for fp16 operands into fp32; 2e-3 for fp16 outputs.

Of the ten dense shapes only 100 x 320 x 1152 splits K by the default rule (3 slices at fp16, 6 at fp32);
70 x 1152 x 192 has too few k-steps for the rule and splits under the forced plans.

Worst figures measured on an MI355X (normalised / lobe; each case prints its own, the module prints the worst
of each group at its end):
  general kernel, default rule   fp32 6.4e-7 / 4.0e-6; fp16 into fp32 2.7e-7 / 1.5e-6; fp16 out 3.8e-4 / 4.4e-4
  general kernel, forced plans   fp32 9.8e-7 / 4.6e-6 (100 x 320 x 1152 at "128,128,2,1"); fp16 into fp32
                                 3.9e-7 / 1.9e-6; fp16 out 3.7e-4 / 4.4e-4
  fp16x3 / fp16x3s               2.1e-7 / 1.8e-6
  gemm256 (vector and scalar)    into fp32 2.6e-7 / 1.5e-6; fp16 out 3.5e-4 / 4.4e-4; split-K 2.8e-7 / 2.0e-6;
                                 refused over an fp32 residual, the general kernel 2.7e-7 / 1.1e-6
  saturation                     4.1e-10 / 6.6e-8; the columns at -89 and below are -0
  convs but S9                   fp32 3.5e-7 / 2.8e-6; fp16x3s 4.6e-7 / 1.7e-6; fp16 3.6e-4 / 4.4e-4
  S9 (K = 2304), halo64, 3 slices  fp32 7.7e-7 / 7.7e-6; fp16x3s 6.2e-7 / 5.1e-6; fp16 (2 slices) 3.6e-4 / 4.4e-4
The fp16 lobe figure is the output's rounding: half an fp16 ulp in [0.25, 0.5), 2^-13 = 1.2e-4, over 0.2785.
Every group leaves 2x under its bar but S9's lobe figure at fp32 (1.3x) and in the split layout (1.97x).  That is
the accumulation, not the activation: torch's own fp32-accumulated conv of the same operands, with SiLU in fp32 on
the CPU, gives 7.5e-7 .. 1.4e-6 / 5.3e-6 .. 7.8e-6 against the float64 reference (one pass, or three channel
slices summed), as the lobe figure divides the absolute error of 2304-term fp32 sums of size 6 by 0.2785.
"""
import importlib

import numpy as np
import pytest
import torch

import op_refs as R

pytestmark = pytest.mark.gpu

GUARD = 8
NAN = float("nan")
RUNS = R.silu_gemm_runs()
WORST = {}  # group -> [bar, worst normalised, worst lobe, where]


@pytest.fixture(scope="module")
def ops(spi, gpu):
    return importlib.import_module("starpu-inference-server_amd.ops")


@pytest.fixture(scope="module")
def ws(ops):
    return ops.workspace()


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    yield
    for (group, bar), (e, lobe, what) in sorted(WORST.items()):
        print(f"\nsilu routes, worst of {group} (bar {bar:.0e}): normalised {e:.3e}, lobe {lobe:.3e} at {what}")


def hold(group, what, bar, got, ref, pre, silu=True):
    """Print a case's two figures, keep the group's worst, and hold both to the bar."""
    e = R.nerr(got, ref)
    lobe = R.silu_lobe_err(got, ref, pre) if silu else 0.0
    print(f"{what}: normalised {e:.3e} lobe {lobe:.3e} (bar {bar:.0e})")
    w = WORST.setdefault((group, bar), [0.0, 0.0, what])
    if max(e, lobe) > max(w[0], w[1]):
        w[2] = what
    w[0], w[1] = max(w[0], e), max(w[1], lobe)
    assert e < bar and lobe < bar, f"{what}: normalised {e:.3e}, lobe {lobe:.3e}, bar {bar:.0e}"


# ---- buffers ------------------------------------------------------------------------------------


def nan_buffer(rows, cols, kind):
    """[rows][cols] of NaN on the device: kind "f16", "f32", or "split" (fp32 storage, both fp16 halves NaN)."""
    if kind == "split":
        return torch.full((rows, 2 * cols), NAN, dtype=torch.float16, device="cuda").view(torch.float32)
    return torch.full((rows, cols), NAN, dtype=torch.float16 if kind == "f16" else torch.float32, device="cuda")


def all_nan(t, kind):
    t = t.contiguous()
    return bool(torch.isnan(t.view(torch.float16) if kind == "split" else t).all())


def encode(ops, kind, a):
    t = torch.from_numpy(np.ascontiguousarray(a, np.float32))
    return (t.half() if kind == "f16" else ops.to_split(t) if kind == "split" else t).cuda()


def decode(ops, kind, t):
    t = t.contiguous().cpu()
    return (ops.from_split(t) if kind == "split" else t.float()).double().numpy()


def act_kind(prec):
    return {"fp16": "f16", "fp16x3s": "split"}.get(prec, "f32")


def out_kind(prec, out_f32):
    return "split" if prec == "fp16x3s" else "f16" if prec == "fp16" and not out_f32 else "f32"


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ---- dense --------------------------------------------------------------------------------------

_dense = {}


def dense_inputs(ops, prec, shape, case=None):
    """One (precision, shape)'s device operands -- A at lda = K + 8 (split: + 32) with NaN in the slack, the packed
    weight, the bias -- the float64 accumulator, and the residual of each kind on demand (ldr = N + 16 / + 64)."""
    key = (prec, shape, case is not None)
    if key not in _dense:
        M, N, K = shape
        A, W, b, Rr = case or R.silu_dense_case(M, N, K)
        kind = act_kind(prec)
        a_buf = nan_buffer(M, K + (32 if kind == "split" else 8), kind)
        a_buf[:, :K] = encode(ops, kind, A)
        av, wv = R.operand_values(prec, A, W)
        _dense[key] = dict(A=a_buf[:, :K], b=b, b_d=torch.from_numpy(b).cuda(), Rr=Rr, res={},
                           Wp=ops.pack_weight("fp16x3" if kind == "split" else prec, W), acc=R.dense_acc64(av, wv))
    return _dense[key]


def residual(ops, c, kind):
    if kind not in c["res"]:
        M, N = c["Rr"].shape
        buf = nan_buffer(M, N + (64 if kind == "split" else 16), kind)
        buf[:, :N] = encode(ops, kind, c["Rr"])
        c["res"][kind] = (buf[:, :N], R.silu_res_values(kind, c["Rr"]))
    return c["res"][kind]


def launch_gemm(ops, ws, r, c, what):
    """Two launches of a run into NaN buffers on the one workspace; returns the decoded output of the first."""
    M, N, K = r["shape"]
    act = R.SILU_FORMS[r["form"]][0]
    okind = out_kind(r["prec"], r["out_f32"])
    res = residual(ops, c, r["res"])[0] if r["res"] else None
    outs = []
    for _ in range(2):
        if r["c_kind"] == "unaligned":
            buf = nan_buffer(1, 1 + (M + GUARD) * N, okind).view(-1)[1:].view(M + GUARD, N)
            assert buf.data_ptr() % 16 == (2 if okind == "f16" else 4)
        else:
            buf = nan_buffer(M + GUARD, N + (32 if okind == "split" else 8), okind)
        out = buf[:M, :N]
        ops.gemm(r["prec"], c["A"], c["Wp"], N, bias=c["b_d"], residual=res, out=out, act=act, ws=ws)
        torch.cuda.synchronize()
        assert all_nan(buf[M:], okind), f"{what}: rows past M were written"
        assert buf.shape[1] == N or all_nan(buf[:M, N:], okind), f"{what}: C's slack columns were written"
        outs.append(out.clone())
    assert same_bits(outs[0], outs[1]), f"{what}: two launches on one workspace differ"
    return decode(ops, okind, outs[0])


def check_plan(r, v):
    """What each group expects of spi_debug_gemm_plan's answer, before the launch."""
    what = R.silu_run_id(r)
    assert R.gemm_route(v) in R.SILU_GEMM_ROUTES, (what, v)
    M, N, K = r["shape"]
    es = 64 if r["prec"] == "fp16" else 32
    if r["group"] == "rule":
        assert v[0] == 0 and (v[4], v[5]) == (64, 64) and (v[7] > 1) == (r["shape"] == (100, 320, 1152)), (what, v)
    elif r["group"] in ("forced", "x3") and r["env"]:
        bm, bn, stages, splits = (int(x) for x in r["env"]["SPI_GEMM_PLAN"].split(","))
        want, kt = R.forced_splits(-(-K // 64) * 64 // es, splits if bn == 64 else 1)
        assert v[0] == 0 and (v[4], v[5], v[6], v[7], v[11]) == (bm, bn, stages, want, kt * es), (what, v)
        if r["env"]["SPI_GEMM_PLAN"] == "64,64,2,5" and K == 1152:
            assert want == 5 and (-(-K // 64) * 64 // es) % 5, (what, v)  # 18 or 36 steps: a short last slice
    elif r["group"] == "g256":
        bm = 256 if r["env"]["SPI_GEMM_256_MIN"] == "1" else 128
        assert v[0] == (0 if r["refused"] else bm) and v[1] == 1, (what, v)
        assert v[0] or (v[4], v[5], v[7]) == (64, 64, 1), (what, v)
    elif r["group"] == "g256split":
        assert v[0] in (128, 256) and v[1] == 2, (what, v)


def run_gemm(ops, ws, r):
    what = R.silu_run_id(r)
    act, has_res = R.SILU_FORMS[r["form"]]
    c = dense_inputs(ops, r["prec"], r["shape"])
    with R.gemm_knobs(ops.lib, r["env"]):
        v = R.query_gemm_plan(ops.lib, r["prec"], *r["shape"], R.silu_run_lda(r), R.silu_run_flags(r))
        assert c["A"].stride(0) == R.silu_run_lda(r) and c["A"].data_ptr() % 16 == 0 and c["Wp"].data_ptr() % 16 == 0
        check_plan(r, v)
        got = launch_gemm(ops, ws, r, c, what)
    rv = residual(ops, c, r["res"])[1] if has_res else None
    pre = R.preact64(c["acc"], c["b"], rv)
    assert np.isfinite(got).all(), f"{what}: non-finite outputs"
    group = f"{r['group']} {r['prec']}" + (" general" if r["refused"] else " scalar" if r["c_kind"] == "unaligned" else "")
    hold(group, f"{what} -> {R.gemm_route(v)} x{v[1] if v[0] else v[7]}", R.silu_bar(r["prec"], r["out_f32"]), got,
         R.epilogue64(c["acc"], c["b"], rv, act), pre, act == "silu")


def runs_of(group, **match):
    out = [r for r in RUNS if r["group"] == group and all(r[k] == v for k, v in match.items())]
    assert out, (group, match)
    return out


@pytest.mark.parametrize("shape", R.SILU_DENSE, ids=["x".join(map(str, s)) for s in R.SILU_DENSE])
@pytest.mark.parametrize("prec,out_f32", R.SILU_OUTS, ids=["fp32", "fp16", "fp16-f32out"])
def test_default_rule(ops, ws, prec, out_f32, shape):
    """The general kernel by the default rule: 64 x 64 tiles, the vector epilogue on whole tile columns and the
    per-element one on the last ragged column, the split-K finisher on 100 x 320 x 1152; all three forms."""
    for r in runs_of("rule", prec=prec, out_f32=out_f32, shape=shape):
        run_gemm(ops, ws, r)


@pytest.mark.parametrize("plan", R.SILU_FORCED)
def test_forced_plans(ops, ws, plan):
    """128 x 128, 128 x 64 (both ring depths) and 64 x 64 tiles, a 2-way split and a 5-way split of 18 (fp16) or
    36 (fp32) steps with a short last slice; two shapes with a ragged last tile column, two of whole tiles."""
    for r in runs_of("forced", env={"SPI_GEMM_PLAN": plan}):
        run_gemm(ops, ws, r)


@pytest.mark.parametrize("plan", R.SILU_X3_PLANS, ids=["rule", "64,64,3,2"])
@pytest.mark.parametrize("prec", ["fp16x3", "fp16x3s"])
def test_fp16x3(ops, ws, prec, plan):
    """spi_op_gemm accepts act 3 at fp16x3 and in the split layout: SiLU over bias and residual."""
    for r in runs_of("x3", prec=prec, env={"SPI_GEMM_PLAN": plan} if plan else {}):
        run_gemm(ops, ws, r)


@pytest.mark.parametrize("tiles", R.SILU_G256_MIN, ids=["bm256", "bm128", "bm128b2"])
def test_gemm256(ops, ws, tiles):
    """gemm256's SiLU instances: a guarded tile only (M = 50), a full tile and a guarded one (M = 300 at 256 rows;
    ragged at 128), fp16 and fp32 outputs, no residual and an fp16 one, the scalar epilogue behind a C one
    element off 16 bytes; over an fp32 residual gemm256 has no activation instance and must refuse -- the general
    kernel is then right."""
    for r in runs_of("g256", env={"SPI_GEMM_256_MIN": tiles}):
        run_gemm(ops, ws, r)


@pytest.mark.parametrize("extra", R.SILU_G256_SPLIT_ENV, ids=["max2", "uncapped"])
@pytest.mark.parametrize("tiles", R.SILU_G256_MIN, ids=["bm256", "bm128", "bm128b2"])
def test_gemm256_split_k(ops, ws, tiles, extra):
    """SiLU behind gemm256's slice sum (two slices of 16 k-tiles), not on each slice."""
    for r in runs_of("g256split", env={"SPI_GEMM_256_MIN": tiles, **extra}):
        run_gemm(ops, ws, r)


@pytest.mark.parametrize("kernel,prec,out_f32", [("gemm", "fp32", True), ("gemm", "fp16", False), ("gemm256", "fp16", False),
                                                 ("gemm256", "fp16", True)])
def test_saturation(ops, ws, kernel, prec, out_f32):
    """A = 0, so column n's pre-activation is its bias, one of +100 .. -1e4: exp(-v) overflows below -88 and the
    quotient is -0 (device_math.hpp).  Every output finite, the columns at -89 and below under 1e-30, the rest
    within the bar of float64 on both figures."""
    M, N, K = R.SILU_SAT_SHAPES[kernel]
    rng = np.random.default_rng(N)
    b = np.array([R.SILU_SAT_BIAS[n % len(R.SILU_SAT_BIAS)] for n in range(N)], np.float32)
    case = (np.zeros((M, K), np.float32), (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32), b, np.zeros((M, N), np.float32))
    env = {"SPI_GEMM_256_MIN": "1"} if kernel == "gemm256" else {}
    r = {"group": "saturation", "env": env, "prec": prec, "shape": (M, N, K), "form": "silu", "out_f32": out_f32,
         "res": None, "c_kind": "strided", "refused": False}
    c = dense_inputs(ops, prec, r["shape"], case)
    what = R.silu_run_id(r)
    with R.gemm_knobs(ops.lib, env):
        v = R.query_gemm_plan(ops.lib, prec, M, N, K, R.silu_run_lda(r), R.silu_run_flags(r))
        assert R.gemm_route(v) == (("gemm256", 256, 256, False) if kernel == "gemm256" else ("gemm", 64, 64, False)), v
        got = launch_gemm(ops, ws, r, c, what)
    assert np.isfinite(got).all(), f"{what}: non-finite outputs"
    pre = np.broadcast_to(b.astype(np.float64), (M, N))
    tiny = pre[0] <= -89
    assert tiny.sum() >= 3 * (N // 9) and np.abs(got[:, tiny]).max() < 1e-30, what
    hold(f"saturation {prec}", what, R.silu_bar(prec, out_f32), got[:, ~tiny], R.silu64(pre[:, ~tiny]), pre[:, ~tiny])


# ---- convs --------------------------------------------------------------------------------------

_conv = {}


def conv_inputs(ops, prec, shape):
    key = (prec, shape)
    if key not in _conv:
        x, w, b, _ = R.conv_kind_case(shape)
        xv, wv = R.operand_values(prec, x, w)
        _conv[key] = dict(x=encode(ops, act_kind(prec), x), wp=ops.pack_weight(prec, w.reshape(shape[4], -1)), b=b,
                          b_d=torch.from_numpy(b).cuda(), pre=R.preact64(R.conv_acc(xv, wv, shape[7], shape[8]), b))
    return _conv[key]


def run_conv(ops, ws, setting, prec, shape, want_kind, act="silu", route=None):
    """Two launches of a conv with bias and `act` under a knob setting, the plan's kind (and, where given, the
    weight-resident route) asserted first; returns (the raw output of the first, decoded, float64 pre-activation)."""
    B, H, W, cin, cout, kh, kw, stride, pad = shape
    c = conv_inputs(ops, prec, shape)
    oh, ow = R.conv_out_hw(shape)
    M, kind = B * oh * ow, act_kind(prec)
    outs = []
    with R.kind_knobs(ops.lib, setting):
        plan = R.query_conv_plan(ops.lib, prec, shape)
        name = R.conv_kind_name(prec, shape, plan)
        what = f"conv {setting} {prec} {'x'.join(map(str, shape))} {act} -> {name}"
        assert want_kind(name, dict(zip(R.PLAN_FIELDS, plan))), what
        if route is not None:
            assert R.query_conv_route(ops.lib, prec, shape, False, act) == route, what
        for _ in range(2):
            buf = nan_buffer(M + GUARD, cout, kind)
            ops.conv2d(prec, c["x"], c["wp"], cout, kh, kw, stride, pad, bias=c["b_d"], act=act, ws=ws, out=buf[:M])
            torch.cuda.synchronize()
            assert all_nan(buf[M:], kind), f"{what}: rows past M were written"
            outs.append(buf[:M].clone())
    assert same_bits(outs[0], outs[1]), f"{what}: two launches on one workspace differ"
    got = decode(ops, kind, outs[0]).reshape(B, oh, ow, cout)
    assert np.isfinite(got).all(), f"{what}: non-finite outputs"
    return outs[0], got, c["pre"], what


def hold_conv(group, prec, got, pre, what):
    hold(f"{group} {prec}", what, R.silu_bar(prec, False), got, R.silu64(pre), pre)


@pytest.mark.parametrize("setting,prec", [(s, p) for s, (precs, _) in R.SILU_CONV_KINDS.items() for p in precs])
def test_conv3x3_kinds(ops, ws, setting, prec):
    """The kw-window walk on 4 and on 8 waves, the 64- / 128- / 256-row halo bands and the default rule's halo
    under a capped split-K, each on the smallest CONV3_SHAPES entry whose plan takes the kind."""
    name, shape, plan = R.silu_conv_pick(ops.lib, setting, prec)
    pred = R.SILU_CONV_KINDS[setting][1]
    _, got, pre, what = run_conv(ops, ws, setting, prec, shape, lambda n, p: pred(p) and n.startswith(("win", "halo")))
    hold_conv("conv 3x3", prec, got, pre, f"{name} {what}")


@pytest.mark.parametrize("prec", ["fp16", "fp32"])
def test_conv_tap_walk(ops, ws, prec):
    _, got, pre, what = run_conv(ops, ws, "default", prec, R.SILU_CONV_TAP, lambda n, p: n.startswith("tap"))
    hold_conv("conv tap", prec, got, pre, what)


@pytest.mark.parametrize("prec", ["fp16", "fp32"])
def test_conv_gather_stem_form(ops, ws, prec):
    """EfficientNet's stem: 3x3 / stride 2 over the padded image channels."""
    _, got, pre, what = run_conv(ops, ws, "default", prec, R.SILU_CONV_GATHER[prec], lambda n, p: n.startswith("gen"))
    hold_conv("conv gather", prec, got, pre, what)


def test_weight_resident_conv_refuses_silu(ops, ws):
    """conv_wres.hip has ReLU only.  Under SPI_CONV_WRES=2 spi_debug_conv_route says 1 with ReLU and 0 with SiLU
    (and GELU); the SiLU output is the general kernel's, bit for bit what SPI_CONV_WRES=0 gives, and meets the bar."""
    shape = R.shape9(R.SILU_CONV_WRES)
    assert R.SILU_CONV_WRES in R.WRES_SHAPES
    general = lambda n, p: not n.startswith("wres")  # noqa: E731
    run_conv(ops, ws, "wres2", "fp16", shape, general, act="relu", route=1)
    with R.kind_knobs(ops.lib, "wres2"):
        assert R.query_conv_route(ops.lib, "fp16", shape, False, "gelu") == 0
    raw2, got, pre, what = run_conv(ops, ws, "wres2", "fp16", shape, general, route=0)
    raw0, _, _, _ = run_conv(ops, ws, "wres0", "fp16", shape, general, route=0)
    assert same_bits(raw2, raw0), "the SiLU conv depends on SPI_CONV_WRES"
    hold_conv("conv wres refusal", "fp16", got, pre, what)

"""Op-level parity of every device path spi_op_conv2d can take -- the gather (kConvGen), the tap walk
(kConvTap), the three kw-window forms (kConvTapW: 64 x 64 on 4 waves, 128 x 64, 64 x 64 on 8 waves in two K
groups), the halo bands (kConvHalo at 64 / 128 / 256 rows, kConvHaloS) and the weight-resident 64 -> 64 conv
(conv_wres.hip) -- on non-square maps, non-square filters, strides and paddings no model uses.

The reference is a torch float64 conv on the values the kernel multiplies (op_refs.operand_values: fp16-rounded
x and w for fp16, the split layout's hi + lo against the fp32 weight for fp16x3s, the fp32 values for fp32 and
fp16x3), so only the accumulation separates the two and the bars are the project's operand-exact ones: 1e-5
normalised max error into an fp32 or split output, 2e-3 into fp16.  test_op_refs.py shows on the CPU, for the
same inputs, that an fp32-accumulated conv sits 3x below those bars and that a conv without the column / row /
image masks, with H and W exchanged or with the images joined sits far above them; the integer cases
(op_refs.conv_exact_case) must come out to the bit, on every kind.

Every case
  * reads spi_debug_conv_plan (and, for fp16 64 -> 64, spi_debug_conv_route) under its knobs before it
    launches and holds it to tests/golden/conv_kind_plans.json, from which its id takes the kind it names;
  * writes into a view of a larger buffer, 8 rows of NaN in front and 8 behind, which must survive;
  * reads x and the residual from views into NaN-filled buffers (at least W + 3 pixels either side): a kernel
    that consumes a pixel before the first image or after the last one shows NaN, even against a zero weight;
  * runs twice on the module's one workspace when its plan splits K, to the same bits (tickets back at zero,
    slabs summed in slice order).
"""
import json
import os

import numpy as np
import pytest
import torch

import op_refs as R

pytestmark = pytest.mark.gpu

TOL32, TOL16 = 1e-5, 2e-3
GUARD = 8
NAN = float("nan")
# form -> (residual, activation, bias)
FORMS = {"res-relu": (True, "relu", True), "relu": (False, "relu", True), "res": (True, None, True),
         "plain": (False, None, False)}

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_kind_plans.json")) as _f:
    TABLE = json.load(_f)
S3 = {R.shape9(v): k for k, v in R.CONV3_SHAPES.items()}
RUNS = R.conv_kind_runs()


def tol(prec):
    return TOL16 if prec == "fp16" else TOL32


def recorded(setting, prec, shape, form="res-relu"):
    """(plan, route or None) of the table; the route is the form's."""
    key = R.kind_key(setting, prec, shape)
    res, act, _ = FORMS[form]
    route = TABLE["routes"].get(key)
    return TABLE["plans"][key], None if route is None else route[f"{int(res)}{int(act is not None)}"]


def case_id(setting, prec, shape, form="res-relu"):
    plan, route = recorded(setting, prec, shape, form)
    name = S3.get(shape) or "x".join(map(str, shape[:3] if shape[3:] == (64, 64, 3, 3, 1, 1) else shape))
    return f"{name}-{prec}-{setting}-{R.conv_kind_name(prec, shape, plan, route or 0)}"


def params(group, forms):
    seen, out = set(), []
    for g, setting, prec, shape in RUNS:
        if g == group and (setting, prec, shape) not in seen:
            seen.add((setting, prec, shape))
            out += [pytest.param(setting, prec, shape, f, id=case_id(setting, prec, shape, f) + "-" + f) for f in forms]
    return out


@pytest.fixture(scope="module")
def ops(spi, gpu):
    import importlib
    return importlib.import_module("starpu-inference-server_amd.ops")


@pytest.fixture(scope="module")
def ws(ops):
    return ops.workspace()


WORST = {}


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    yield
    for prec, (e, what) in sorted(WORST.items()):
        print(f"\nconv kinds, worst normalised max error {prec}: {e:.3e} (bar {tol(prec):.0e}) at {what}")


# ---- buffers ------------------------------------------------------------------------------------


def nan_like(rows, cols, prec):
    """Host buffer [rows][cols] in the precision's storage type, every element NaN (the split layout is fp16
    pairs in fp32 storage: both halves NaN)."""
    t = torch.empty(rows, cols, dtype=torch.float16 if prec == "fp16" else torch.float32)
    (t.view(torch.float16) if prec == "fp16x3s" else t).fill_(NAN)
    return t


def all_nan(t, prec):
    return bool(torch.isnan(t.view(torch.float16) if prec == "fp16x3s" else t).all())


def encode(ops, prec, a):
    t = torch.from_numpy(np.ascontiguousarray(a, np.float32))
    return t.half() if prec == "fp16" else ops.to_split(t) if prec == "fp16x3s" else t


def decode(ops, prec, t):
    t = t.cpu()
    return (ops.from_split(t) if prec == "fp16x3s" else t.float()).double().numpy()


def framed(ops, prec, a, frame):
    """fp32 [B][H][W][C] -> a device view of that shape in the precision's layout, inside a buffer with
    `frame` NaN pixels in front and behind (C elements each: a multiple of 16 bytes for every Cin >= 8)."""
    t = encode(ops, prec, a)
    n, c = t.numel() // t.shape[-1], t.shape[-1]
    buf = nan_like(n + 2 * frame, c, prec)
    buf[frame:frame + n] = t.reshape(n, c)
    dev = buf.cuda()
    view = dev[frame:frame + n].view(t.shape)
    assert view.data_ptr() % 16 == 0 and view.is_contiguous()
    return dev, view


_inputs = {}


def inputs(ops, prec, shape, exact=False):
    """One shape's operands on the device at one precision and what the reference needs, shared by every
    setting and form: the float64 accumulator (or, exact, the integer reference) is computed once."""
    key = (prec, shape, exact)
    if key not in _inputs:
        B, H, W, cin, cout, kh, kw, stride, pad = shape
        c = {}
        if exact:
            x, w, b, r, c["ref"] = R.conv_exact_case(shape)
        else:
            x, w, b, r = R.conv_kind_case(shape)
            xv, wv = R.operand_values(prec, x, w)
            c["acc"] = R.conv_acc(xv, wv, stride, pad)
            c["rv"] = R.operand_values(prec, r)
        frame = max(W + 3, R.conv_out_hw(shape)[1] + 3, GUARD)
        c["x_buf"], c["x"] = framed(ops, prec, x, frame)
        c["r_buf"], c["r"] = framed(ops, prec, r, frame)
        c["wp"] = ops.pack_weight(prec, w.reshape(cout, -1))
        c["b"], c["b_d"] = b, torch.from_numpy(b).cuda()
        _inputs[key] = c
    return _inputs[key]


def run_case(ops, ws, setting, prec, shape, form, exact=False):
    """Launch one case under its setting on the kind the table records; returns the decoded output
    [B][OH][OW][Cout] (float64) and its reference."""
    B, H, W, cin, cout, kh, kw, stride, pad = shape
    res, act, bias = FORMS[form]
    c = inputs(ops, prec, shape, exact)
    oh, ow = R.conv_out_hw(shape)
    M = B * oh * ow
    want_plan, want_route = recorded(setting, prec, shape, form)
    what = f"{case_id(setting, prec, shape, form)} {form}"
    outs = []
    with R.kind_knobs(ops.lib, setting):
        plan = R.query_conv_plan(ops.lib, prec, shape)
        assert plan == want_plan, f"{what}: plan {plan}, recorded {want_plan}"
        route = 0
        if want_route is not None:
            route = R.query_conv_route(ops.lib, prec, shape, res, act)
            assert route == want_route, f"{what}: weight-resident route {route}, recorded {want_route}"
        splits = 1 if route else plan[3]
        for _ in range(2 if splits > 1 else 1):
            buf = nan_like(M + 2 * GUARD, cout, prec).cuda()
            out = buf[GUARD:GUARD + M]
            assert out.data_ptr() % 16 == 0
            ops.conv2d(prec, c["x"], c["wp"], cout, kh, kw, stride, pad, bias=c["b_d"] if bias else None,
                       residual=c["r"] if res else None, act=act, ws=ws, out=out)
            torch.cuda.synchronize()
            assert all_nan(buf[:GUARD], prec), f"{what}: rows in front of the output were written"
            assert all_nan(buf[GUARD + M:], prec), f"{what}: rows past M were written"
            outs.append(out.clone())
    if len(outs) == 2:
        assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), \
            f"{what}: two launches on one workspace differ"
    got = decode(ops, prec, outs[0]).reshape(B, oh, ow, cout)
    bad = np.count_nonzero(~np.isfinite(got))
    assert bad == 0, f"{what}: {bad} non-finite outputs (a frame pixel consumed, or a tile never stored)"
    if exact:
        return got, c["ref"]
    return got, R.epilogue64(c["acc"], c["b"] if bias else None, c["rv"] if res else None, act)


def check(ops, ws, setting, prec, shape, form):
    got, ref = run_case(ops, ws, setting, prec, shape, form)
    e = R.nerr(got, ref)
    what = f"{case_id(setting, prec, shape, form)} {form}"
    print(f"{what}: {e:.3e}")
    if e > WORST.get(prec, (0, ""))[0]:
        WORST[prec] = (e, what)
    assert e < tol(prec), f"{what}: {e:.3e}"
    return got


# ---- the tests ----------------------------------------------------------------------------------


@pytest.mark.parametrize("setting,prec,shape,form", params("wres", list(FORMS)))
def test_weight_resident(ops, ws, setting, prec, shape, form):
    """conv_wres.hip under SPI_CONV_WRES=2 (spi_debug_conv_route says so) and the general kernel's kind for
    the same shape under =0; the 84-wide map, whose one-row halo no longer fits, keeps the general kernel
    under both."""
    _, route = recorded(setting, prec, shape, form)
    assert route == int(setting == "wres2" and shape[:3] != R.WRES_REFUSED)
    check(ops, ws, setting, prec, shape, form)


@pytest.mark.parametrize("setting,prec,shape,form", params("halo", ["res-relu"]))
def test_halo_kinds(ops, ws, setting, prec, shape, form):
    """The six forced halo candidates and the default rule, fp32 included; S9 once more with a slice count
    that does not divide the channel blocks (SPI_GEMM_MAXSPLIT=3).  Where a forced candidate does not fit the
    map the conv falls through to the kind its id names."""
    check(ops, ws, setting, prec, shape, form)


@pytest.mark.parametrize("setting,prec,shape,form", params("window", ["res-relu", "plain"]))
def test_window_kinds(ops, ws, setting, prec, shape, form):
    """SPI_GEMM_WIN 0 to 3 with the halo kinds and the weight-resident kernel off: the plain tap walk, the
    window on 4 waves, at 128 x 64 (S10) and on 8 waves in two K groups."""
    check(ops, ws, setting, prec, shape, form)


@pytest.mark.parametrize("setting,prec,shape,form", params("geo", ["res-relu", "relu"]))
def test_tap_and_gather_geometry(ops, ws, setting, prec, shape, form):
    """KH != KW, 25 and 49 taps, k-steps straddling filter rows, stride 3, pad 0 and pad > k // 2, under the
    default plan and one forced SPI_GEMM_PLAN.  The 1x1 / pad 1 conv's outer ring has its whole window in the
    padding: exactly act(bias), rounded to the output type."""
    got = check(ops, ws, setting, prec, shape, form)
    if shape == R.CONV_RING and form == "relu":
        want = decode(ops, prec, encode(ops, prec, np.maximum(inputs(ops, prec, shape)["b"], 0)))
        for ring in (got[:, 0], got[:, -1], got[:, :, 0], got[:, :, -1]):
            assert np.array_equal(ring, np.broadcast_to(want, ring.shape)), "a padding-only window is not act(bias)"


def _exact_params():
    seen, out = set(), []
    for _, setting, prec, shape in RUNS:
        if (setting, prec, shape) not in seen:
            seen.add((setting, prec, shape))
            out.append(pytest.param(setting, prec, shape, id=case_id(setting, prec, shape)))
    return out


@pytest.mark.parametrize("setting,prec,shape", _exact_params())
def test_exact_integer_cases(ops, ws, setting, prec, shape):
    """Small-integer operands: every product and partial sum is exact in any order, so every kind, tile,
    slice count and precision must return the integer reference to the bit -- and hence agree with every
    other kind of the shape."""
    got, ref = run_case(ops, ws, setting, prec, shape, "res-relu", exact=True)
    bad = np.argwhere(got != ref)
    assert bad.size == 0, f"{case_id(setting, prec, shape)}: {len(bad)} outputs differ, first at {bad[0].tolist()}: " \
                          f"{got[tuple(bad[0])]} != {ref[tuple(bad[0])]}"


@pytest.mark.parametrize("what,prec,shape", [
    ("49 taps in the split layout", "fp16x3s", (1, 10, 12, 64, 64, 7, 7, 2, 3)),
    ("Cin 16 in the split layout", "fp16x3s", (1, 9, 11, 16, 32, 3, 3, 1, 1)),
    ("an empty output", "fp16", (1, 2, 9, 64, 64, 5, 5, 1, 1)),
    ("an empty output", "fp32", (1, 9, 2, 64, 64, 3, 5, 1, 1)),
], ids=["split-49-taps", "split-cin16", "empty-h", "empty-w"])
def test_rejections(ops, ws, what, prec, shape):
    """Refused with a message before any launch: the output buffer keeps its NaN."""
    B, H, W, cin, cout, kh, kw, stride, pad = shape
    assert not R.conv_accepts(prec, shape)
    x = torch.zeros(B, H, W, cin, device="cuda", dtype=ops.act_dtype(prec))
    wp = ops.pack_weight(prec, np.zeros((cout, kh * kw * cin), np.float32))
    out = torch.full((64, cout), NAN, device="cuda", dtype=x.dtype)
    with pytest.raises(ops.OpError) as err:
        ops.conv2d(prec, x, wp, cout, kh, kw, stride, pad, ws=ws, out=out)
    assert str(err.value), what
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()), what

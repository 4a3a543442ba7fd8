"""-m gpu: the pose backbones (csrc/backbone.hip running conv*.hip and pool_fc.hip) stage by stage against float64, teacher-forced: every
reference stage (tests/support/backbone_ref.py, BatchNorm unfolded) is fed the ENGINE's own input to that stage (Backbone.debug_tensor), so
that a difference is the stage's own and not inherited:
  stem from x; layer1 from stem (max pool inside); layer{s} from layer{s-1}; layer{s}_down from layer{s-1} (pre-activation nets: from the
  layer{s-1}_act tap, which the kernel read); layer{s}_act from layer{s}; features and the head output from layer4.
Every element of every tap is compared; the border ring of every tap is exactly zero after the forward; a second forward (under the event
profiler) is bit-identical in every tap, the features and the head.  The float64 reference runs on the device as K x K shifted NHWC
matmuls (checked against F.conv2d in float64 below).

Cases: crops 64 x 96 (even down to the 2 x 3 map: full Winograd tiles), 50 x 70 (odd at every level: half-empty tile rows and columns, the
read slack, stride 2 on odd maps) and 18 x 22 (the smallest we run: 9 x 11, 5 x 6, 3 x 3, 2 x 2, 1 x 1 -- the executor refuses no crop, and
the 3 x 3 convolutions see mostly padding); batches 1 (split-K everywhere), 3, "wino" = the smallest at which layer 1 is Winograd-eligible,
and "big" = the smallest at which layer 1 has more Winograd units than CUs (the persistent walk) AND layer2.0.conv1 leaves split-K for the
bf16x9 direct kernel; all computed from the device's CU count with the engine's own plan / eligibility functions.  vanilla_resnet34 (9
inputs) and resnet34 (32 inputs) get every crop and batch; vanilla_resnet34 (27), resnet18 and resnet34_width=2 the odd crop at 3 and "wino".
Further: block 0 of every stage isolated (the blocks after it made exact identities), a backbone created with MP_CONV_DIRECT_BF16=0 (the
stride-2 layers on the fp32 kernel at the same batch, side by side), the workspace bookkeeping across geometries, forward_f16, and the
argument checks of mp_backbone_debug_tensor.

Routes: predicted per layer with eng.conv2d_plan / eng.conv_wino_eligible exactly as run_conv_layer decides, confirmed per forward by the
event profiler's launch counts per kernel name (the persistent and the one-workgroup-per-unit Winograd launches share a profiler row:
which of the two ran follows from units > CUs, the launch's own rule), and printed in the "[stage]" lines.
test_every_route_was_taken_by_a_compared_stage asserts the five routes over the cases.

Tolerances.  Metric: max |got - ref| / max(1, max |ref|) per tap.  Bound = 2 x the worst value of the MI355X run over all cases (the
factor covers split-K partitions that depend on the CU count; the inputs are seeded).  "f32" = the same stage of the float32 oracle
(oracle/backbones.py, as cut into stages by BackboneRef) against float64 on the same input, on the CPU, worst case of the batches <= 3;
a measured error above 4 x f32 counts as a finding.
  tap            measured   f32        bound     worst case (routes of the stage's layers)
  stem           1.68e-6    1.51e-6    3.4e-6    van27-odd-wino, 7 x 7 x 27 single pass: 1323 positive terms in one fp32 accumulation
  stem (f16 in)  9.55e-7    -          2.0e-6    van9-odd-b3 through forward_f16
  layer1         4.59e-7    9.86e-7    9.2e-7    w2-odd-wino (6 x Winograd)
  layer2         4.82e-7    9.78e-7    9.7e-7    van9-even-big (2 x bf16x9 direct, 7 x Winograd)
  layer3         8.76e-7    1.31e-6    1.8e-6    van9-odd-big (split-K, bf16x9 direct, 11 x Winograd)
  layer4         5.75e-7    6.56e-7    1.2e-6    van27-odd-wino (7 x split-K)
  layer*_down    5.77e-7    5.06e-7    1.2e-6    van9-odd-big layer3_down (bf16x9 direct)
  layer*_act     9.58e-8    1.28e-7    2.0e-7    wide32-tiny-big layer3_act
  features       1.36e-6    3.60e-7    2.8e-6    van9-tiny-big: 2717 rows of a 1 x 1 map through the 512 x 512 fc; the f32 figure is the worst
                                                 of 1 + 3 rows (batches <= 3), where the engine measures 4.9e-7 .. 7.4e-7: 3.8 x f32, under
                                                 the 4 x of a finding, and the maximum over 900 x as many rows
  head output    5.56e-7    3.08e-7    1.2e-6    van9-even-wino
  un-forced      (reported) x -> features in one go: 1.47e-6 at worst (van9-tiny-big), the size of one stage's error: the damped
                 residual branches of the seeded weights do not let the stages' errors add up
No stage is above 4 x its f32 figure: no finding.  With MP_CONV_DIRECT_BF16=0 the stride-2 layers' taps differ from the bf16x9 build's
by less than 1e-7 of the scale either way (e.g. layer3_down 5.77e-7 bf16x9 against 5.56e-7 fp32)."""
from __future__ import annotations

import ctypes as C
from collections import Counter
from typing import Dict, Tuple

import pytest
import torch
import torch.nn.functional as F

from tests.support import synthetic as syn
from tests.support.backbone_ref import BackboneRef, border_is_zero, conv_matmul, nhwc_to_nchw, padded_tap
from tests.support.wino import n_units

pytestmark = pytest.mark.gpu

TOL = {"stem": 3.4e-6, "stem_f16": 2.0e-6, "layer1": 9.2e-7, "layer2": 9.7e-7, "layer3": 1.8e-6, "layer4": 1.2e-6, "down": 1.2e-6,
       "act": 2.0e-7, "features": 2.8e-6, "out": 1.2e-6}

SPLITK_WS_FLOATS = 12 << 20   # the split-K scratch the executor hands every layer (backbone.hip); the plan depends on it
ROUTES = ("f32_splitk", "f32_single", "bf16x9_direct", "wino", "wino_persistent")

NETS = {"van9": ("vanilla_resnet34", 9, "logits", 1), "wide32": ("resnet34", 32, "pose", 9), "van27": ("vanilla_resnet34", 27, "pose", 9),
        "r18": ("resnet18", 9, "logits", 1), "w2": ("resnet34_width=2", 9, "logits", 1)}
CROPS = {"even": (64, 96), "odd": (50, 70), "tiny": (18, 22)}
N_BLOCKS = {"vanilla_resnet34": (3, 4, 6, 3), "resnet34": (3, 4, 6, 3), "resnet18": (2, 2, 2, 2)}

# (net, variant, crop, batch key): variant "" = as released, "iso" = block 0 of every stage alone, "fp32s2" = MP_CONV_DIRECT_BF16=0
CASES = [(n, "", c, b) for n in ("van9", "wide32") for c in CROPS for b in ("b1", "b3", "wino", "big")]
CASES += [(n, "", "odd", b) for n in ("van27", "r18", "w2") for b in ("b3", "wino")]
CASES += [(n, "iso", "odd", b) for n in ("van9", "wide32") for b in ("b3", "big")]
CASES += [(n, "fp32s2", "odd", "big") for n in ("van9", "wide32")]


def _id(case):
    n, v, c, b = case
    return "-".join(x for x in (n, v, c, b) if x)


@pytest.fixture(scope="module")
def eng():
    from megapose6d_amd import engine

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert engine.device_info()[2].startswith("gfx950")
    return engine


# --------------------------------------------------------------------------- nets, geometry, routes
def _kind(net):
    k = NETS[net][0]
    return ("resnet34", int(k.split("=")[1])) if k.startswith("resnet34_width=") else (k, 1)


def _state_dict(net, variant):
    kind, c_in, head, n_out = NETS[net]
    sd = syn.make_state_dict(kind, c_in, head, n_out, seed=11)
    if variant == "iso":   # every block after block 0 an exact identity: layer{s} = block 0 alone (stride-2 conv, downsample, residual epilogue)
        base, _ = _kind(net)
        for s, nb in enumerate(N_BLOCKS[base], start=1):
            for i in range(1, nb):
                P = f"backbone.layer{s}.{i}."
                if base == "vanilla_resnet34":   # relu(0 * conv + 0 + x) = x: the stream is post-ReLU
                    sd[P + "bn2.weight"] = torch.zeros_like(sd[P + "bn2.weight"])
                    sd[P + "bn2.bias"] = torch.zeros_like(sd[P + "bn2.bias"])
                else:
                    sd[P + "conv2.weight"] = torch.zeros_like(sd[P + "conv2.weight"])
    return sd


_NETS: Dict[Tuple[str, str], tuple] = {}


def _net(eng, net, variant):
    """(Backbone, state dict, float64 reference on the device), created once per module"""
    if (net, variant) not in _NETS:
        kind, c_in, head, n_out = NETS[net]
        sd = _state_dict(net, variant)
        with pytest.MonkeyPatch.context() as mp:   # read per backbone, at creation
            if variant == "fp32s2":
                mp.setenv("MP_CONV_DIRECT_BF16", "0")
            else:
                mp.delenv("MP_CONV_DIRECT_BF16", raising=False)
            bb = eng.Backbone(kind, c_in, head, n_out, sd)
        _NETS[(net, variant)] = (bb, sd, BackboneRef(sd, kind, torch.float64, "cuda", conv=conv_matmul))
    return _NETS[(net, variant)]


def _geometry(net, h, w):
    """(stem kernel size, stem map, the four stage maps, stage widths): geometry() of backbone.hip"""
    base, width = _kind(net)
    k = 7 if base == "vanilla_resnet34" else 5
    half = lambda v: (v + 2 - 3) // 2 + 1
    h1, w1 = (h + 2 * (k // 2) - k) // 2 + 1, (w + 2 * (k // 2) - k) // 2 + 1
    maps = [(half(h1), half(w1))]
    for _ in range(3):
        maps.append((half(maps[-1][0]), half(maps[-1][1])))
    return k, (h1, w1), maps, [64 * width, 128 * width, 256 * width, 512 * width]


def _route(eng, n_cu, lds, N, H, W, Cp, in_border, Cout, K, stride, pad, direct_bf16, stem=False, x_f16=False):
    """the kernel run_conv_layer (conv_layer.hip) picks for this layer + the profiler rows it leaves"""
    f32 = "conv_nhwc_f32_mfma<128,64,64,32>" if Cout <= 64 else "conv_nhwc_f32_mfma<128,128,64,64>"
    if x_f16:
        return "f32_single", Counter({f32 + "/x_f16": 1})
    wino_form = not stem and K == 3 and stride == 1 and pad == 1 and Cp % 16 == 0 and Cout % 64 == 0
    if wino_form and lds >= 132 * 1024 and eng.conv_wino_eligible(N, H, W, Cp, in_border, Cout, 1, n_cu):
        return ("wino_persistent" if n_units(N, H, W, Cout) > n_cu else "wino"), Counter({"conv3x3_wino_bf16x9<64t,64c>": 1})
    mode = eng.conv2d_plan(N, H, W, Cp, in_border, Cout, K, stride, pad, n_cu, ws_floats=SPLITK_WS_FLOATS)["mode"]
    direct_form = (not stem and direct_bf16 and not wino_form and K in (1, 3) and Cp % 16 == 0 and (K * Cp) % 32 == 0 and Cout % 64 == 0)
    if direct_form and mode != 1:
        return "bf16x9_direct", Counter({"conv_nhwc_bf16x9<128,128,64,64>": 1})
    if mode == 0:
        return "f32_single", Counter({f32: 1})
    rows = Counter({f32 + "/splitk": 1, "conv_splitk_reduce": 1})
    if mode == 2:   # whole rounds single pass + a split-K tail
        rows[f32] += 1
        return "f32_single+tail", rows
    return "f32_splitk", rows


def _routes(eng, net, variant, N, h, w, x_f16=False):
    """-> ({tap: [routes of the layers that write into it]}, expected profiler launches of the convolution kernels)"""
    n_cu, lds, _ = eng.device_info()
    base, _ = _kind(net)
    c_in = NETS[net][1]
    k, (h1, w1), maps, widths = _geometry(net, h, w)
    direct = variant != "fp32s2"
    per_tap, rows = {}, Counter()

    def add(tap, *a, **kw):
        r, c = _route(eng, n_cu, lds, N, *a, direct, **kw)
        per_tap.setdefault(tap, []).append(r)
        rows.update(c)

    add("stem", h, w, (c_in + 3) // 4 * 4, 3 if base == "vanilla_resnet34" else 2, widths[0], k, 2, k // 2, stem=True, x_f16=x_f16)
    cin = widths[0]
    for s, nb in enumerate(N_BLOCKS[base]):
        (H, W), planes = maps[s], widths[s]
        for i in range(nb):
            stride = 2 if (i == 0 and s > 0) else 1
            Hi, Wi = maps[s - 1] if stride == 2 else (H, W)
            add(f"layer{s + 1}", Hi, Wi, cin, 1, planes, 3, stride, 1)
            if i == 0 and (stride != 1 or cin != planes):
                r, c = _route(eng, n_cu, lds, N, Hi, Wi, cin, 1, planes, 1, stride, 0, direct)
                per_tap.setdefault(f"layer{s + 1}", []).append(r)
                per_tap.setdefault(f"layer{s + 1}_down", []).append(r)
                rows.update(c)
            add(f"layer{s + 1}", H, W, planes, 1, planes, 3, 1, 1)
            cin = planes
    return per_tap, rows


_BATCHES: Dict[Tuple[str, str], Dict[str, int]] = {}


def _batches(eng, net, crop):
    """b1, b3, "wino" (the smallest batch whose layer 1 is Winograd-eligible), "big" (the smallest whose layer 1 walks persistently, more
    units than CUs, and whose layer2.0.conv1 leaves split-K), from the CU count of this device"""
    if (net, crop) not in _BATCHES:
        n_cu = eng.device_info()[0]
        _, _, maps, widths = _geometry(net, *CROPS[crop])
        (H, W), C0 = maps[0], widths[0]
        wino = big = None
        for N in range(1, 1 << 16):
            elig = eng.conv_wino_eligible(N, H, W, C0, 1, C0, 1, n_cu)
            if wino is None and elig:
                wino = N
            if elig and n_units(N, H, W, C0) > n_cu and eng.conv2d_plan(N, H, W, C0, 1, widths[1], 3, 2, 1, n_cu,
                                                                      ws_floats=SPLITK_WS_FLOATS)["mode"] != 1:
                big = N
                break
        assert wino and big and 3 < wino < big, (wino, big)
        _BATCHES[(net, crop)] = {"b1": 1, "b3": 3, "wino": wino, "big": big}
    return _BATCHES[(net, crop)]


# --------------------------------------------------------------------------- one case
def _tap_names(wide):
    names = ["stem"] + [f"layer{s}" for s in range(1, 5)] + [f"layer{s}_down" for s in range(2, 5)]
    return names + ([f"layer{s}_act" for s in range(1, 4)] if wide else [])


def _kind_of(tap):
    return "down" if tap.endswith("_down") else "act" if tap.endswith("_act") else tap


def _input(eng, bb, b, h, w, seed, dtype=torch.float32):
    """seeded uniform [0, 1) input -> (padded NHWC buffer for the engine, the same values as [b, c, h, w] float64 on the device)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    xn = torch.rand(b, h, w, bb.c_in, generator=g, device="cuda").to(dtype)
    xb = eng.padded_nhwc(b, h, w, bb.c_in_p, bb.in_border, "cuda", dtype=dtype)
    eng.padded_view(xb, b, h, w, bb.c_in_p, bb.in_border)[..., : bb.c_in] = xn
    return xb, nhwc_to_nchw(xn, torch.float64)


def _forward(bb, xb, b, h, w, slot=0):
    out = torch.empty(b, bb.n_out, device="cuda")
    feat = torch.empty(b, 512 * bb.width, device="cuda")
    bb.forward(xb, b, h, w, out, None, feat, slot=slot)
    torch.cuda.synchronize()
    return out, feat


def _err(got: torch.Tensor, ref: torch.Tensor):
    """max |got - ref| / max(1, max |ref|) over EVERY element -> (error, scale, all finite)"""
    assert got.shape == ref.shape, (got.shape, ref.shape)
    scale = max(1.0, ref.abs().max().item())
    return (got.double() - ref).abs().max().item() / scale, scale, bool(torch.isfinite(got).all())


def _staged(ref: BackboneRef, wide, x, tap, head_key):
    """every teacher-forced comparison: `tap` = {name: NCHW view of the engine's tap} in ref's dtype / device, x the input ->
    {name: reference value}, "features" and "out" (the head) included"""
    pairs = {"stem": ref.stem(x), "layer1": ref.stage(1, tap["stem"])}
    for s in range(2, 5):
        pairs[f"layer{s}"] = ref.stage(s, tap[f"layer{s - 1}"])
        pairs[f"layer{s}_down"] = ref.downsample(s, tap[f"layer{s - 1}_act" if wide else f"layer{s - 1}"])
    if wide:
        for s in range(1, 4):
            pairs[f"layer{s}_act"] = ref.next_act(s, tap[f"layer{s}"])
    t = ref.tail(tap["layer4"])
    pairs["features"], pairs["out"] = t["features"], t[head_key]
    return pairs


_RESULTS: Dict[tuple, dict] = {}


def _run(eng, case):
    """forward twice (the second under the profiler), compare every stage; everything a test asserts comes back in a dict (nothing is
    asserted here, so that the "[stage]" lines are complete whatever fails)"""
    if case in _RESULTS:
        return _RESULTS[case]
    net, variant, crop, bkey = case
    kind, c_in, head, n_out = NETS[net]
    bb, sd, ref = _net(eng, net, variant)
    wide = kind != "vanilla_resnet34"
    h, w = CROPS[crop]
    b = _batches(eng, net, crop)[bkey]
    xb, x64 = _input(eng, bb, b, h, w, seed=b)
    names = _tap_names(wide)
    res = {"batch": b, "err": {}, "scale": {}, "f32": {}, "problems": []}

    out, feat = _forward(bb, xb, b, h, w)
    first = {}
    for t in names:
        full, brd = padded_tap(bb, t, b, h, w)
        if not border_is_zero(full, brd):
            res["problems"].append(f"{t}: non-zero border")
        first[t] = full.clone()
    eng.profile_begin()
    try:
        out2, feat2 = _forward(bb, xb, b, h, w)
    finally:
        prof = eng.profile_end()
    for t in names:
        if not torch.equal(padded_tap(bb, t, b, h, w)[0], first[t]):
            res["problems"].append(f"{t}: the second forward differs")
    if not (torch.equal(out, out2) and torch.equal(feat, feat2)):
        res["problems"].append("features / head: the second forward differs")

    res["routes"], want_rows = _routes(eng, net, variant, b, h, w)
    got_rows = Counter({k: int(v["launches"]) for k, v in prof.items() if k.startswith("conv")})
    if got_rows != want_rows:
        res["problems"].append(f"profiler rows {dict(got_rows)} != predicted {dict(want_rows)}")

    head_key = "pose" if head == "pose" else "renderings_logits"
    with torch.no_grad():
        tap = {t: nhwc_to_nchw(first[t][:, 1:-1, 1:-1], torch.float64) for t in names}
        got = dict(tap, features=feat.cpu().double(), out=out.cpu().double())
        pairs = _staged(ref, wide, x64, tap, head_key)
        for t, r in pairs.items():
            e, sc, finite = _err(got[t], r)
            res["err"][t], res["scale"][t] = e, sc
            if not finite:
                res["problems"].append(f"{t}: non-finite values")
        res["unforced"] = _err(got["features"], ref.forward(x64)["features"])[0]
        if b <= 3:   # the float32 oracle's own error at every stage, on the CPU, from the same inputs
            ref32 = BackboneRef(sd, kind, torch.float32, "cpu")
            tap32 = {t: v.float().cpu() for t, v in tap.items()}
            for t, r32 in _staged(ref32, wide, x64.float().cpu(), tap32, head_key).items():
                res["f32"][t] = _err(r32, pairs[t].cpu())[0]
    for t in list(pairs):
        f32 = f" f32 {res['f32'][t]:.2e}" if t in res["f32"] else ""
        print(f"[stage] {_id(case)} b={b} {t}: err {res['err'][t]:.2e} (scale {res['scale'][t]:.3g}){f32} "
              f"routes {dict(Counter(res['routes'].get(t, [])))}")
    print(f"[stage] {_id(case)} b={b} un-forced x -> features: err {res['unforced']:.2e}")
    _RESULTS[case] = res
    return res


def _assert_case(res, what):
    assert not res["problems"], (what, res["problems"])
    over = {t: (e, TOL[_kind_of(t)]) for t, e in res["err"].items() if not e <= TOL[_kind_of(t)]}
    assert not over, (what, "tap: (error, bound)", over)


# --------------------------------------------------------------------------- tests
@pytest.mark.parametrize("K,stride,pad", [(7, 2, 3), (5, 2, 2), (3, 1, 1), (3, 2, 1), (1, 2, 0)])
def test_device_float64_reference_equals_conv2d(eng, K, stride, pad):
    """the shifted-matmul convolution on the device against the CPU's F.conv2d in float64, one small odd shape per kernel size and stride"""
    g = torch.Generator().manual_seed(K * 10 + stride)
    x = torch.randn(3, 20, 13, 18, generator=g, dtype=torch.float64)
    w = torch.randn(40, 20, K, K, generator=g, dtype=torch.float64)
    want = F.conv2d(x, w, stride=stride, padding=pad)
    got = conv_matmul(x.cuda(), w.cuda(), stride=stride, padding=pad).cpu()
    assert got.shape == want.shape
    assert (got - want).abs().max().item() < 1e-12 * want.abs().max().item()


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_stage_by_stage_against_float64(eng, case):
    _assert_case(_run(eng, case), _id(case))


def test_every_route_was_taken_by_a_compared_stage(eng):
    """fp32 split-K, fp32 single pass, bf16x9 direct, Winograd one workgroup per unit and Winograd persistent: each ran in a layer of a
    stage that was compared (and whose profiler rows matched the prediction)"""
    seen = Counter()
    for case in CASES:
        res = _run(eng, case)
        assert not any(p.startswith("profiler rows") for p in res["problems"]), (_id(case), res["problems"])
        for t, rs in res["routes"].items():
            assert t in res["err"]
            seen.update(rs)
    print(f"[stage] routes over all cases: {dict(seen)}")
    for r in ROUTES:
        assert seen[r] > 0, (r, dict(seen))


@pytest.mark.parametrize("net", ["van9", "wide32"])
def test_stride2_layers_on_both_routes_side_by_side(eng, net):
    """MP_CONV_DIRECT_BF16=0 at creation: the stride-2 3x3 and the 1x1 downsample layers run the fp32 kernel where the released backbone
    runs the bf16x9 direct one, at the same batch; both are held to the same bounds"""
    a, b = _run(eng, (net, "", "odd", "big")), _run(eng, (net, "fp32s2", "odd", "big"))
    for s in (2, 3, 4):
        for t in (f"layer{s}_down", f"layer{s}"):
            print(f"[stage] {net} odd big {t}: bf16x9 build err {a['err'][t]:.2e} routes {dict(Counter(a['routes'][t]))} | "
                  f"fp32 build err {b['err'][t]:.2e} routes {dict(Counter(b['routes'][t]))}")
        assert "bf16x9_direct" not in b["routes"][f"layer{s}"]
    assert a["routes"]["layer2_down"] == ["bf16x9_direct"] and b["routes"]["layer2_down"][0].startswith("f32_")
    assert "bf16x9_direct" in a["routes"]["layer2"]
    _assert_case(a, net)
    _assert_case(b, net + " fp32s2")


def test_workspace_bookkeeping_across_geometries(eng):
    """one slot: a forward at a large geometry, at a smaller one, at the large one again -- the workspace is carved up anew each time and
    its borders zeroed for the new geometry: the third run equals the first bit for bit, the borders are zero each time"""
    bb, _, _ = _net(eng, "wide32", "")
    names = _tap_names(True)
    big, small = (5, 64, 96), (3, 50, 70)
    snaps = []
    for b, h, w in (big, small, big):
        xb, _ = _input(eng, bb, b, h, w, seed=100 + b)
        out, feat = _forward(bb, xb, b, h, w, slot=3)
        snap = {"out": out.clone(), "feat": feat.clone()}
        for t in names:
            full, brd = padded_tap(bb, t, b, h, w, slot=3)
            assert border_is_zero(full, brd), (t, b, h, w)
            snap[t] = full.clone()
        snaps.append(snap)
        with pytest.raises(eng.EngineError, match="last forward"):   # the taps of another geometry are gone
            bb.debug_tensor("layer1", b + 1, h, w, slot=3)
    for k in snaps[0]:
        assert torch.equal(snaps[0][k], snaps[2][k]), k
    assert snaps[1]["layer1"].shape != snaps[0]["layer1"].shape


def test_f16_input_stem_against_float64(eng):
    """forward_f16: the stem tap against the float64 stem of the widened binary16 input"""
    bb, _, ref = _net(eng, "van9", "")
    b, (h, w) = 3, CROPS["odd"]
    xb, x64 = _input(eng, bb, b, h, w, seed=5, dtype=torch.float16)
    eng.profile_begin()
    try:
        _forward(bb, xb, b, h, w, slot=4)
    finally:
        prof = eng.profile_end()
    assert int(prof["conv_nhwc_f32_mfma<128,64,64,32>/x_f16"]["launches"]) == 1
    full, brd = padded_tap(bb, "stem", b, h, w, slot=4)
    assert border_is_zero(full, brd)
    with torch.no_grad():
        e, sc, finite = _err(nhwc_to_nchw(bb.debug_tensor("stem", b, h, w, slot=4), torch.float64), ref.stem(x64))
    print(f"[stage] van9-odd-b3 f16 input, stem: err {e:.2e} (scale {sc:.3g})")
    assert finite and e <= TOL["stem_f16"], (e, TOL["stem_f16"])


def test_debug_tensor_argument_checks(eng):
    """unknown names, names of the other kind of net, null pointers, another geometry, and "stem" after a record-path forward: clean errors"""
    from megapose6d_amd import _lib

    van, _, _ = _net(eng, "van9", "")
    wide, _, _ = _net(eng, "wide32", "")
    b, (h, w) = 1, CROPS["tiny"]
    for bb in (van, wide):
        out, _ = _forward(bb, _input(eng, bb, b, h, w, seed=1)[0], b, h, w, slot=5)
        assert bb.debug_tensor("layer4", b, h, w, slot=5).shape == (1, 1, 1, 512)
        for bad in ("", "foo", "layer", "layer0", "layer5", "layer1_down", "layer2_up", "stem_act", "Layer1"):
            with pytest.raises(eng.EngineError, match="does not apply|not a published tensor"):
                bb.debug_tensor(bad, b, h, w, slot=5)
    with pytest.raises(eng.EngineError, match="does not apply"):
        van.debug_tensor("layer1_act", b, h, w, slot=5)
    with pytest.raises(eng.EngineError, match="does not apply"):
        wide.debug_tensor("layer4_act", b, h, w, slot=5)
    assert wide.debug_tensor("layer3_act", b, h, w, slot=5).shape == (1, 2, 2, 256)
    with pytest.raises(eng.EngineError, match="no forward has run"):
        van.debug_tensor("layer1", b, h, w, slot=6)
    lib, ws = _lib.load(), van.workspace(b, h, w, out.device, 5)   # (the workspace of that forward, not a new one)
    ptr, shp, brd = C.c_void_p(), (C.c_int64 * 4)(), C.c_int32(0)
    good = [van.handle, b"layer1", ws.data_ptr(), b, h, w, C.byref(ptr), shp, C.byref(brd)]
    assert lib.mp_backbone_debug_tensor(*good) == 0 and ptr.value and list(shp) == [1, 5, 6, 64] and brd.value == 1
    for i in (0, 1, 2, 6, 7, 8):
        args = list(good)
        args[i] = None
        assert lib.mp_backbone_debug_tensor(*args) != 0, i
        with pytest.raises(eng.EngineError, match="null pointer"):
            eng.check(lib.mp_backbone_debug_tensor(*args))
    # the record path pools inside the stem kernel and never writes the stem map (all-zero records: a valid input)
    R = van.xrec_elements(3)
    assert R > 0
    rec = eng.padded_nhwc(1, 240, 320, R, van.in_border, "cuda", dtype=torch.bfloat16)
    _forward(van, rec, 1, 240, 320, slot=7)
    with pytest.raises(eng.EngineError, match="'stem' was not written"):
        van.debug_tensor("stem", 1, 240, 320, slot=7)
    assert van.debug_tensor("layer1", 1, 240, 320, slot=7).shape == (1, 60, 80, 64)

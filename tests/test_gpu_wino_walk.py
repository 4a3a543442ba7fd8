"""-m gpu: conv3x3_wino_bf16x9 (csrc/conv_wino_bf16.hip) in its PERSISTENT launch form -- one workgroup per CU walks the units blockIdx.x,
blockIdx.x + gridDim.x, ... and prepares the next unit's indices, tile table, patch requests and accumulator reset under the current
unit's epilogue -- at the shapes where a wrong unit, tile, channel block or byte offset would show:
  * the edges of the walk (one CU with two units, exact multiples of the CU count, a tail of one, one K step, 32 K steps x 8 channel
    blocks, partial last tile groups, tile groups across image boundaries, tiles_y = 1 / tiles_x = 1, borders of 2), every epilogue;
  * every 3x3 / stride-1 layer the backbones route to it at the real batch (576 rows of 240 x 320 crops);
  * the 32-bit addressing limit, from both sides;
  * non-finite inputs (NaN stays NaN on non-ReLU outputs, spreads no further than its 2 x 2 output tiles).
Every comparison takes the WHOLE output against the float64 reference computed on the device (tests/support/wino.py, itself checked
against F.conv2d in float64 below) at CONV_TOL of the output scale (2 x that for the second output of the dual epilogue); the output
border is poisoned (7.0) and must stay untouched, and the input's read slack -- exactly the documented (W + 2 b + 1) * C + 64 floats --
is poisoned with NaN.  Shapes are computed from the CU count of the device (`engine.device_info`)."""
import hashlib
import json
import math
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

from tests.support.wino import (CONV_TOL, RELU_EPILOGUES, RES_EPILOGUES, WT, conv3x3_ref_f64_device, fold_weights, guard_max_n, n_units,
                                padded_len, wino_input)

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def eng():
    from megapose6d_amd import engine

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    n_cu, lds, arch = engine.device_info()
    assert arch.startswith("gfx950")
    return engine


@pytest.fixture(scope="module")
def n_cu(eng):
    return eng.device_info()[0]


# --------------------------------------------------------------------------- launch + whole-output check
def _launch(eng, shape, epi, kernel="bf16x9", seed=0, x_hook=None, buffers=None):
    """one convolution with epilogue `epi` on `kernel` (bf16x9 | fp32 | direct); inputs from seeded generators (the large ones on the
    device).  Returns everything the reference and the checks need."""
    N, Cin, H, W, Cout, ib, ob = shape
    gh = torch.Generator().manual_seed(1000 + seed)
    gd = torch.Generator(device="cuda").manual_seed(2000 + seed)
    w = torch.randn(Cout, Cin, 3, 3, generator=gh) * (2.0 / (Cin * 9)) ** 0.5
    scale = torch.rand(Cout, generator=gh) + 0.5
    bias = torch.randn(Cout, generator=gh) * 0.1
    sc2, sh2 = torch.rand(Cout, generator=gh) + 0.5, torch.randn(Cout, generator=gh) * 0.1
    use_scale = epi != "plain"
    if buffers is not None:
        xb, yb = buffers
    else:
        xb = wino_input(eng, N, H, W, Cin, ib)
        yb = eng.padded_nhwc(N, H, W, Cout, ob, "cuda")
    if kernel == "direct":   # (the direct kernel's contract is the zeroed slack of padded_nhwc, not the Winograd kernels' NaN-readable one)
        xb[padded_len(N, H, W, Cin, ib):] = 0.0
    xv = eng.padded_view(xb, N, H, W, Cin, ib)
    xv.copy_(torch.randn(N, H, W, Cin, generator=gd, device="cuda"))
    if x_hook is not None:
        x_hook(xv)
    yb.fill_(7.0)   # poison: the interior must be fully overwritten, the border and the slack left alone
    ya = None
    if epi == "dual":
        ya = eng.padded_nhwc(N, H, W, Cout, ob, "cuda")
        ya.fill_(7.0)
    rb = None
    if epi in RES_EPILOGUES:
        rb = eng.padded_nhwc(N, H, W, Cout, ob, "cuda")
        eng.padded_view(rb, N, H, W, Cout, ob).copy_(torch.randn(N, H, W, Cout, generator=gd, device="cuda"))
    sc_np = scale.numpy() if use_scale else None
    if kernel == "bf16x9":
        wp = torch.from_numpy(eng.conv_wino_bf16_pack_weights(w.numpy(), Cin, sc_np)).cuda()
    elif kernel == "fp32":
        wp = torch.from_numpy(eng.conv_wino_pack_weights(w.numpy(), Cin, sc_np)).cuda()
    else:
        wp = torch.from_numpy(eng.conv_pack_weights(w.numpy(), Cin, sc_np)).cuda()
    args = dict(residual=rb, relu=epi in RELU_EPILOGUES, y_act=ya, act_scale=sc2.cuda() if ya is not None else None,
                act_shift=sh2.cuda() if ya is not None else None)
    b = bias.cuda() if use_scale else None
    if kernel == "direct":
        eng.conv2d_nhwc(xb, N, H, W, Cin, ib, wp, b, Cout, 3, 1, 1, yb, ob, **args)
    else:
        eng.conv3x3_wino_nhwc(xb, N, H, W, Cin, ib, wp, b, Cout, yb, ob, **args)
    torch.cuda.synchronize()
    return dict(shape=shape, epi=epi, xb=xb, xv=xv, w=w, scale=scale if use_scale else None, bias=bias if use_scale else None,
                act=(sc2, sh2) if ya is not None else None, yb=yb, ya=ya, rb=rb)


def _reference(eng, r):
    N, Cin, H, W, Cout, ib, ob = r["shape"]
    epi = r["epi"]
    res = eng.padded_view(r["rb"], N, H, W, Cout, ob) if r["rb"] is not None else None
    return conv3x3_ref_f64_device(_full(r["xb"], N, H, W, Cin, ib), ib, r["w"], r["scale"], r["bias"], res, epi in RELU_EPILOGUES,
                                  r["act"])


def _full(buf, n, h, w, c, border):
    return buf[: padded_len(n, h, w, c, border)].view(n, h + 2 * border, w + 2 * border, c)


def _assert_border_and_slack(buf, shape, name):
    N, Cin, H, W, Cout, ib, ob = shape
    full = _full(buf, N, H, W, Cout, ob)
    for edge in (full[:, :ob], full[:, -ob:], full[:, :, :ob], full[:, :, -ob:]):
        assert torch.all(edge == 7.0), f"{name}: the output border was written"
    assert torch.all(buf[padded_len(N, H, W, Cout, ob):] == 7.0), f"{name}: a store went past the output tensor"


def _check_whole(eng, r, what=""):
    """the whole output (and the second one) against the device float64 reference; border and slack untouched"""
    N, Cin, H, W, Cout, ib, ob = r["shape"]
    yv = eng.padded_view(r["yb"], N, H, W, Cout, ob)
    av = eng.padded_view(r["ya"], N, H, W, Cout, ob) if r["ya"] is not None else None
    err = err_a = scale = 0.0
    for n0, n1, ref, ref_a in _reference(eng, r):
        got = yv[n0:n1].double()
        assert torch.isfinite(got).all(), f"{what}: non-finite output in images {n0}..{n1 - 1}"
        err = max(err, (got - ref).abs().max().item())
        scale = max(scale, ref.abs().max().item())
        if av is not None:
            got_a = av[n0:n1].double()
            assert torch.isfinite(got_a).all(), f"{what}: non-finite second output in images {n0}..{n1 - 1}"
            err_a = max(err_a, (got_a - ref_a).abs().max().item())
        del got, ref, ref_a
    tol = CONV_TOL * max(1.0, scale)
    assert err < tol, (what, r["epi"], err, tol)
    assert err_a < 2 * tol, (what, r["epi"], "second output", err_a, 2 * tol)
    _assert_border_and_slack(r["yb"], r["shape"], what)
    if r["ya"] is not None:
        _assert_border_and_slack(r["ya"], r["shape"], what + " (second output)")


# --------------------------------------------------------------------------- 1. the float64 reference itself
@pytest.mark.parametrize("shape", [(3, 32, 10, 12, 64, 1, 1), (2, 48, 9, 7, 128, 2, 1)], ids=["even", "odd_hw_border2"])
@pytest.mark.parametrize("epi", ["plain", "bias_relu", "res_relu", "dual", "res"])
def test_device_f64_reference_matches_cpu_conv2d(eng, shape, epi):
    """conv3x3_ref_f64_device (nine shifted NHWC matmuls in float64, chunked over images) = CPU F.conv2d in float64 of the same fp32
    operands, every epilogue, to 1e-12 of the output scale.  The chunk size is forced down to one image so that the chunk walk is checked."""
    N, Cin, H, W, Cout, ib, ob = shape
    g = torch.Generator().manual_seed(5)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * 0.1
    scale = torch.rand(Cout, generator=g) + 0.5 if epi != "plain" else None
    bias = torch.randn(Cout, generator=g) * 0.1 if epi != "plain" else None
    res = torch.randn(N, Cout, H, W, generator=g) if epi in RES_EPILOGUES else None
    act = (torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.1) if epi == "dual" else None
    xb = wino_input(eng, N, H, W, Cin, ib)
    eng.padded_view(xb, N, H, W, Cin, ib)[:] = x.permute(0, 2, 3, 1).cuda()
    res_v = res.permute(0, 2, 3, 1).contiguous().cuda() if res is not None else None
    chunks = list(conv3x3_ref_f64_device(_full(xb, N, H, W, Cin, ib), ib, w, scale, bias, res_v, epi in RELU_EPILOGUES, act,
                                         chunk_bytes=1))
    assert [(c[0], c[1]) for c in chunks] == [(n, n + 1) for n in range(N)]
    got = torch.cat([c[2] for c in chunks]).permute(0, 3, 1, 2).cpu()
    ref = F.conv2d(x.double(), fold_weights(w, scale).double(), padding=1)
    if bias is not None:
        ref = ref + bias.double().view(1, -1, 1, 1)
    if res is not None:
        ref = ref + res.double()
    if epi in RELU_EPILOGUES:
        ref = F.relu(ref)
    s = ref.abs().max().item()
    assert (got - ref).abs().max().item() < 1e-12 * s
    if act is not None:
        ref_a = F.relu(ref * act[0].double().view(1, -1, 1, 1) + act[1].double().view(1, -1, 1, 1))
        got_a = torch.cat([c[3] for c in chunks]).permute(0, 3, 1, 2).cpu()
        assert (got_a - ref_a).abs().max().item() < 1e-12 * s


# --------------------------------------------------------------------------- 2. the edges of the persistent walk
def _n_for_groups(tiles_per_image, groups):
    """the smallest batch whose tiles fill exactly `groups` tile groups of 64 (tiles_per_image <= 64)"""
    n = -(-(WT * (groups - 1) + 1) // tiles_per_image)
    assert math.ceil(n * tiles_per_image / WT) == groups
    return n


def _tpi(H, W):
    return ((H + 1) // 2) * ((W + 1) // 2)


# name -> (Cin, H, W, Cout, in_border, out_border, tile groups as a function of the CU count)
WALK_ROWS = {
    "one_cu_walks_two": (64, 8, 8, 64, 1, 1, lambda c: c + 1),              # n_cu + 1 units, the last group holds 16 tiles
    "exactly_two_per_cu": (32, 16, 16, 128, 1, 1, lambda c: c),             # 2 n_cu units, no ragged tail, no partial group
    "tail_of_one": (48, 14, 18, 64, 1, 1, lambda c: 3 * c - 1),            # 3 n_cu - 1 units; 63 tiles per image
    "one_k_step": (16, 12, 12, 64, 1, 1, lambda c: 2 * c + c // 2 + 3),   # Cin = 16: the next unit's requests overlap the only K step
    "k32_cb8_ragged": (512, 8, 10, 512, 1, 1, lambda c: c // 8 + 5),       # 32 K steps, 8 channel blocks per tile group, ragged
    "cout256_partial_group": (64, 15, 20, 256, 1, 1, lambda c: c // 4 + 3),  # a partial last tile group in each of 4 channel blocks
    "groups_straddle_images": (64, 6, 10, 64, 1, 1, lambda c: c + c // 2 + 7),  # 3 x 5 tiles per image
    "h1_w_odd": (32, 1, 37, 64, 1, 1, lambda c: c + 5),                    # tiles_y = 1 (wino_fastdiv d == 1), half-empty tiles
    "h2_w_odd": (32, 2, 15, 128, 1, 1, lambda c: c // 2 + 3),
    "w1_h_odd": (32, 33, 1, 64, 1, 1, lambda c: c + 9),                    # tiles_x = 1
    "w2_h_odd": (64, 9, 2, 64, 1, 1, lambda c: c + 2),
    "borders_2": (64, 13, 17, 64, 2, 2, lambda c: c + c // 4 + 1),         # pitch arithmetic of both padded layouts
}


def _walk_shape(name, n_cu):
    Cin, H, W, Cout, ib, ob, groups = WALK_ROWS[name]
    N = _n_for_groups(_tpi(H, W), groups(n_cu))
    return N, Cin, H, W, Cout, ib, ob


def test_walk_rows_pin_what_they_claim(n_cu):
    """the table's shapes really have the properties the edge cases are named after, on this device's CU count"""
    shapes = {k: _walk_shape(k, n_cu) for k in WALK_ROWS}
    for k, (N, Cin, H, W, Cout, ib, ob) in shapes.items():
        assert n_units(N, H, W, Cout) > n_cu, k
    units = {k: n_units(s[0], s[2], s[3], s[4]) for k, s in shapes.items()}
    tiles = {k: s[0] * _tpi(s[2], s[3]) for k, s in shapes.items()}
    assert units["one_cu_walks_two"] == n_cu + 1 and tiles["one_cu_walks_two"] % WT != 0
    assert units["exactly_two_per_cu"] == 2 * n_cu and tiles["exactly_two_per_cu"] % WT == 0
    assert units["tail_of_one"] == 3 * n_cu - 1
    assert shapes["one_k_step"][1] == 16 and units["one_k_step"] >= 2 * n_cu
    assert shapes["k32_cb8_ragged"][1] == 512 and units["k32_cb8_ragged"] % n_cu != 0
    assert tiles["cout256_partial_group"] % WT != 0 and shapes["cout256_partial_group"][4] == 256
    assert _tpi(6, 10) == 15 and WT % 15 != 0
    for k in ("h1_w_odd", "h2_w_odd"):
        assert (shapes[k][2] + 1) // 2 == 1 and shapes[k][3] % 2 == 1
    for k in ("w1_h_odd", "w2_h_odd"):
        assert (shapes[k][3] + 1) // 2 == 1 and shapes[k][2] % 2 == 1


@pytest.mark.parametrize("row", list(WALK_ROWS))
@pytest.mark.parametrize("epi", ["plain", "bias_relu", "res_relu", "dual"])
def test_wino_walk_row_matches_f64(eng, n_cu, row, epi):
    """bf16x9 at an edge of the persistent walk (WALK_ROWS) against the device float64 reference, whole output"""
    shape = _walk_shape(row, n_cu)
    assert n_units(shape[0], shape[2], shape[3], shape[4]) > n_cu
    r = _launch(eng, shape, epi, seed=list(WALK_ROWS).index(row))
    _check_whole(eng, r, row)


def test_wino_walk_row_is_deterministic(eng, n_cu):
    """the same launch twice gives bit-identical outputs (a unit's result may not depend on which CU walks it, or when)"""
    shape = _walk_shape("groups_straddle_images", n_cu)
    outs = []
    for _ in range(2):
        r = _launch(eng, shape, "dual", seed=3)
        outs.append((r["yb"].clone(), r["ya"].clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def _walk_digests(eng, n_cu):
    """sha1 of every output buffer (border and slack included) of every WALK_ROWS row and epilogue"""
    out = {}
    for row in WALK_ROWS:
        for epi in ("plain", "bias_relu", "res_relu", "dual"):
            r = _launch(eng, _walk_shape(row, n_cu), epi, seed=list(WALK_ROWS).index(row))
            h = hashlib.sha1(r["yb"].cpu().numpy().tobytes())
            if r["ya"] is not None:
                h.update(r["ya"].cpu().numpy().tobytes())
            out[f"{row}/{epi}"] = h.hexdigest()
    return out


def test_wino_walk_forms_are_bit_identical(eng, n_cu):
    """The persistent form and the one-workgroup-per-unit form (MP_WINO_PERSIST=0) run the same unit code: every WALK_ROWS output of the
    two forms is BIT-identical.  The other form runs in a child process (the switch is read once per process)."""
    other = "1" if os.environ.get("MP_WINO_PERSIST", "1") == "0" else "0"
    code = ("import json, sys; sys.path.insert(0, %r); from megapose6d_amd import engine; import tests.test_gpu_wino_walk as t; "
            "print('DIGESTS ' + json.dumps(t._walk_digests(engine, engine.device_info()[0])))" % str(ROOT))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=600,
                       env=dict(os.environ, MP_WINO_PERSIST=other))
    assert r.returncode == 0, r.stderr[-3000:]
    theirs = json.loads(next(line for line in r.stdout.splitlines() if line.startswith("DIGESTS "))[8:])
    ours = _walk_digests(eng, n_cu)
    assert ours.keys() == theirs.keys()
    differ = [k for k in ours if ours[k] != theirs[k]]
    assert not differ, differ


# --------------------------------------------------------------------------- 3. the production layers at the full batch
BATCH, CROP = 576, (240, 320)
BACKBONES = [("vanilla_resnet34", 9, "logits", 1),   # coarse model + refiner of configs 1, 2, 4
             ("resnet34", 32, "pose", 9),           # the WideResNet-34 RGBD refiner of config 3 (make_scene(backbone="resnet34", rgbd=True))
             ("resnet18", 9, "logits", 1),
             ("resnet34_width=2", 9, "logits", 1)]


def _wino_layers(kind, c_in, head, n_out, h, w):
    """(Cin, Cout, H, W, epilogue) of every 3x3 / stride-1 conv of the backbone, from its state dict and the reference block structure
    (oracle/backbones.py): conv1 of a block is relu(bn(conv)) unless it has stride 2; conv2 adds the residual -- relu after it in the
    vanilla ResNet, none in the pre-activation WideResNet, which writes the next block's relu(bn1(.)) as the second output except after
    its last block"""
    from oracle import backbones as ob
    from tests.support import synthetic as syn

    sd = syn.make_state_dict(kind, c_in, head, n_out, seed=0)
    k = sd["backbone.conv1.weight"].shape[-1]
    hs, ws = (h + 2 * (k // 2) - k) // 2 + 1, (w + 2 * (k // 2) - k) // 2 + 1   # stem, stride 2
    res = [((hs + 2 - 3) // 2 + 1, (ws + 2 - 3) // 2 + 1)]                      # max pool
    for _ in range(3):
        res.append(((res[-1][0] + 2 - 3) // 2 + 1, (res[-1][1] + 2 - 3) // 2 + 1))
    blocks = ob._layers(sd)
    out = []
    for j, (s, i) in enumerate(blocks):
        P = f"backbone.layer{s}.{i}."
        H, W = res[s - 1]
        c1, c2 = sd[P + "conv1.weight"].shape, sd[P + "conv2.weight"].shape
        if not (i == 0 and s > 1):
            out.append((c1[1], c1[0], H, W, "bias_relu"))
        if kind == "vanilla_resnet34":
            out.append((c2[1], c2[0], H, W, "res_relu"))
        else:
            out.append((c2[1], c2[0], H, W, "res" if j == len(blocks) - 1 else "dual"))
    return sorted(set(out), key=lambda t: (t[2] * t[3], t[0], t[4]), reverse=True)


_DONE = set()   # (Cin, Cout, H, W, epilogue) already checked in this session (the backbones share most shapes)


@pytest.mark.parametrize("kind,c_in,head,n_out", BACKBONES, ids=[b[0] for b in BACKBONES])
def test_wino_production_layers_at_full_batch(eng, n_cu, kind, c_in, head, n_out):
    """Every 3x3 / stride-1 layer of the backbone at 576 rows of 240 x 320 crops: eligible for the Winograd kernel (or, if the 32-bit
    guard says no, recorded as going to the direct kernel), in the persistent form, and -- with the epilogue the backbone uses there, plus
    `plain` on the largest layer -- equal to the float64 reference over the whole output.  Shapes already checked by an earlier backbone of
    this session are not run again."""
    layers = _wino_layers(kind, c_in, head, n_out, *CROP)
    if kind == "vanilla_resnet34":
        layers.append(layers[0][:4] + ("plain",))
    routes = {}
    for Cin, Cout, H, W, epi in layers:
        ok = eng.conv_wino_eligible(BATCH, H, W, Cin, 1, Cout, 1, n_cu)
        routes[(Cin, Cout, H, W)] = "winograd" if ok else "direct"
        if not ok:   # only the addressing guard may refuse a production layer at this batch
            assert guard_max_n(H, W, Cin, Cout, 1, 1)[0] < BATCH, (kind, Cin, Cout, H, W)
            continue
        assert n_units(BATCH, H, W, Cout) > n_cu   # the launcher takes the persistent form (unless MP_WINO_PERSIST=0)
        if (Cin, Cout, H, W, epi) in _DONE:
            continue
        r = _launch(eng, (BATCH, Cin, H, W, Cout, 1, 1), epi, seed=Cin + H)
        _check_whole(eng, r, f"{kind} {Cin}->{Cout} {H}x{W}")
        _DONE.add((Cin, Cout, H, W, epi))
        del r
        torch.cuda.empty_cache()
    print(f"[{kind}] {BATCH} rows: " + ", ".join(f"{k[0]}->{k[1]}@{k[2]}x{k[3]}: {v}" for k, v in routes.items()))
    if not kind.startswith("resnet34_width="):
        assert all(v == "winograd" for v in routes.values()), routes


# --------------------------------------------------------------------------- 4. the 32-bit addressing limit
LIMIT_CASES = {"out_elems": (64, 60, 80, 128), "in_bytes": (256, 60, 80, 64)}   # Cin, H, W, Cout; borders of 1


@pytest.mark.parametrize("limit", list(LIMIT_CASES))
def test_wino_32bit_addressing_limit(eng, n_cu, limit):
    """The largest batch the guard accepts (computed from its formulas) is eligible, runs on bf16x9 and matches the float64 reference
    over the whole output -- the last tile group and the NaN-poisoned slack next to the 2 GB / 2^29-element boundary included; one image
    more is not eligible, and the launcher refuses it with its error and writes nothing."""
    Cin, H, W, Cout = LIMIT_CASES[limit]
    N, binding = guard_max_n(H, W, Cin, Cout, 1, 1)
    assert binding == limit
    assert eng.conv_wino_eligible(N, H, W, Cin, 1, Cout, 1, n_cu)
    assert not eng.conv_wino_eligible(N + 1, H, W, Cin, 1, Cout, 1, n_cu)
    # one allocation of N + 1 images each: the N-image launch sees prefixes of them (its slack = the next image, NaN-poisoned)
    xb = wino_input(eng, N + 1, H, W, Cin, 1)
    yb = eng.padded_nhwc(N + 1, H, W, Cout, 1, "cuda")
    yb.fill_(7.0)
    up = torch.from_numpy(eng.conv_wino_bf16_pack_weights((torch.randn(Cout, Cin, 3, 3) * 0.05).numpy(), Cin, None)).cuda()
    with pytest.raises(eng.EngineError, match="too large for 32-bit offsets"):
        eng.conv3x3_wino_nhwc(xb, N + 1, H, W, Cin, 1, up, None, Cout, yb, 1)
    torch.cuda.synchronize()
    assert torch.all(yb == 7.0), "the refused launch wrote its output"
    del up
    n_x = padded_len(N, H, W, Cin, 1)
    xb[n_x:] = float("nan")
    x_n = xb[: n_x + (W + 3) * Cin + 64]
    y_n = yb[: padded_len(N, H, W, Cout, 1) + (W + 2) * Cout + 64]
    r = _launch(eng, (N, Cin, H, W, Cout, 1, 1), "plain", seed=7, buffers=(x_n, y_n))
    assert torch.isnan(xb[n_x:]).all()
    _check_whole(eng, r, f"{limit}: N = {N}")
    assert torch.all(yb[padded_len(N, H, W, Cout, 1):] == 7.0)
    del r, x_n, y_n, xb, yb
    torch.cuda.empty_cache()


# --------------------------------------------------------------------------- 5. non-finite inputs
BAD = [(0, 5, 7, 3, float("nan")), (-1, 10, 12, 17, float("inf"))]   # (image, row, column, channel, value): interior pixels


def _bad_tile_mask(N, H, W, Cout):
    """output positions of the 2 x 2 tiles whose 4 x 4 input patch (input rows 2 ty - 1 .. 2 ty + 2) holds a bad pixel"""
    m = torch.zeros(N, H, W, Cout, dtype=torch.bool, device="cuda")
    for n, r, c, _, _ in BAD:
        ty0, ty1 = -(-(r - 2) // 2), (r + 1) // 2
        tx0, tx1 = -(-(c - 2) // 2), (c + 1) // 2
        m[n, 2 * ty0 : 2 * ty1 + 2, 2 * tx0 : 2 * tx1 + 2] = True
    return m


@pytest.mark.parametrize("kernel", ["bf16x9", "fp32", "direct"])
@pytest.mark.parametrize("epi", ["plain", "bias_relu", "res_relu", "dual"])
def test_non_finite_inputs_stay_in_their_tiles(eng, n_cu, kernel, epi):
    """One NaN and one +Inf in interior input pixels of two images.  Every output outside the 2 x 2 tiles whose input patch holds one is
    finite and within CONV_TOL (Winograd may spread a bad pixel to its tile-mates, no further).  Non-ReLU outputs (`plain`, the y of
    `dual`): NaN wherever the float64 reference is NaN, and -inf nowhere the reference is not -inf.  ReLU outputs follow the project-wide
    fmaxf(v, 0) convention -- NaN becomes 0 -- and are never -inf."""
    N, Cin, H, W, Cout = n_cu, 64, 15, 20, 128
    assert n_units(N, H, W, Cout) > n_cu

    def poison(xv):
        for n, r, c, ch, v in BAD:
            xv[n, r, c, ch] = v

    r = _launch(eng, (N, Cin, H, W, Cout, 1, 1), epi, kernel=kernel, seed=11, x_hook=poison)
    chunks = list(_reference(eng, r))
    ref = torch.cat([c[2] for c in chunks])
    ref_a = torch.cat([c[3] for c in chunks]) if r["ya"] is not None else None
    mask = _bad_tile_mask(N, H, W, Cout)
    y = eng.padded_view(r["yb"], N, H, W, Cout, 1).double()
    assert torch.isfinite(ref[~mask]).all() and not torch.isfinite(ref[mask]).all()
    good = y[~mask]
    assert torch.isfinite(good).all(), (kernel, epi, "a bad pixel spread past its tiles")
    tol = CONV_TOL * max(1.0, ref[~mask].abs().max().item())
    assert (good - ref[~mask]).abs().max().item() < tol
    outs = [("y", y, ref, epi not in RELU_EPILOGUES)]
    if r["ya"] is not None:
        ya = eng.padded_view(r["ya"], N, H, W, Cout, 1).double()
        assert (ya[~mask] - ref_a[~mask]).abs().max().item() < 2 * tol
        outs.append(("y_act", ya, ref_a, False))
    for name, got, rf, linear in outs:
        if linear:
            assert torch.isnan(got[torch.isnan(rf)]).all(), (kernel, epi, name, "NaN lost")
            assert not (torch.isneginf(got) & ~torch.isneginf(rf)).any(), (kernel, epi, name, "-inf where the reference has none")
        else:
            assert not torch.isneginf(got).any(), (kernel, epi, name)
    _assert_border_and_slack(r["yb"], r["shape"], kernel)

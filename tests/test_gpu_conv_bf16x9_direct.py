"""-m gpu: the direct convolution on exact bf16 pieces (csrc/conv_bf16x9.hip, mp_conv2d_bf16x9_nhwc) and the backbone's use of it.

Statements checked here:
  * every fused epilogue, at every layer shape the backbone sends to the kernel (layer{2,3,4}.0.conv1 3x3 / stride 2 and .downsample
    1x1 / stride 2) plus odd widths, partial M tiles, a half-filled 128-channel block and a border wider than the pad: equal to the float64
    convolution of the fp32 operands within CONV_TOL of the output scale, output border untouched;
  * the ends of the fp32 range (EDGE_SCALES): CONV_TOL of the scale plus at most 1e-37 absolute (a subnormal third piece);
  * two launches are bit-identical;
  * a 576-row backbone forward runs exactly those six layers on the kernel and none on the fp32 kernel of the 128-channel tile, a 2-row
    forward keeps the split-K path, and the features agree with the MP_CONV_DIRECT_BF16=0 forward within 2e-5.
Reference layers: models/torchvision_resnet.py:74-120 (BasicBlock, downsample), models/wide_resnet.py:29-56.
"""
import os

import pytest
import torch
import torch.nn.functional as F

from tests.support.wino import CONV_TOL
from tests.support.wino import conv_ref_f64 as _conv_ref_f64
from tests.support.wino import from_padded as _from_padded
from tests.support.wino import to_padded as _to_padded

pytestmark = pytest.mark.gpu

PIECE_KERNEL = "conv_nhwc_bf16x9<128,128,64,64>"
FP32_WIDE_TILE = "conv_nhwc_f32_mfma<128,128,64,64>"


@pytest.fixture(scope="module")
def eng():
    from megapose6d_amd import engine

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    n_cu, lds, arch = engine.device_info()
    assert arch.startswith("gfx950")
    return engine


DIRECT_CASES = [
    # N, Cin, H, W, Cout, K, stride, pad, in_border
    (2, 64, 60, 80, 128, 3, 2, 1, 1),     # layer2.0.conv1 (240 x 320 renders)
    (2, 64, 60, 80, 128, 1, 2, 0, 1),     # layer2.0.downsample
    (2, 128, 30, 40, 256, 3, 2, 1, 1),    # layer3.0.conv1
    (2, 128, 30, 40, 256, 1, 2, 0, 1),    # layer3.0.downsample
    (2, 256, 15, 20, 512, 3, 2, 1, 1),    # layer4.0.conv1: M = 160, a partial M tile
    (2, 256, 15, 20, 512, 1, 2, 0, 1),    # layer4.0.downsample
    (3, 64, 15, 21, 128, 3, 2, 1, 1),     # odd width
    (1, 64, 16, 16, 192, 3, 2, 1, 1),     # Cout % 128 == 64: the second channel block half empty
    (1, 32, 9, 11, 64, 1, 2, 0, 2),       # border wider than the pad, M = 30
    (2, 32, 10, 12, 128, 3, 1, 1, 1),     # stride 1, C = 32: the shortest 3x3 run (KW * C % 32 == 0)
]


def _run_direct(eng, case, epi, seed):
    N, Cin, H, W, Cout, K, s, p, ib = case
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, K, K, generator=g) * (2.0 / (Cin * K * K)) ** 0.5
    scale = torch.rand(Cout, generator=g) + 0.5
    bias = torch.randn(Cout, generator=g) * 0.1
    Ho, Wo = (H + 2 * p - K) // s + 1, (W + 2 * p - K) // s + 1
    res = torch.randn(N, Cout, Ho, Wo, generator=g)
    xb = _to_padded(eng, x, Cin, ib)
    use_scale = epi != "plain"
    wp = torch.from_numpy(eng.conv_bf16x9_pack_weights(w.numpy(), Cin, scale.numpy() if use_scale else None)).cuda()
    ob = 1
    yb = eng.padded_nhwc(N, Ho, Wo, Cout, ob, "cuda")
    yb += 7.0  # poison: interior must be fully overwritten, the border untouched
    ya = eng.padded_nhwc(N, Ho, Wo, Cout, ob, "cuda") if epi == "dual" else None
    sc2, sh2 = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.1
    rb = _to_padded(eng, res, Cout, ob) if epi in ("res_relu", "dual") else None
    eng.conv2d_bf16x9_nhwc(xb, N, H, W, Cin, ib, wp, bias.cuda() if use_scale else None, Cout, K, s, p, yb, ob,
                           residual=rb, relu=epi in ("bias_relu", "res_relu"), y_act=ya,
                           act_scale=sc2.cuda() if ya is not None else None, act_shift=sh2.cuda() if ya is not None else None)
    torch.cuda.synchronize()
    ref = _conv_ref_f64(x, w, scale if use_scale else None, bias if use_scale else None, s, p)
    if epi in ("res_relu", "dual"):
        ref = ref + res
    if epi in ("bias_relu", "res_relu"):
        ref = F.relu(ref)
    ref_a = F.relu(ref * sc2.view(1, -1, 1, 1) + sh2.view(1, -1, 1, 1)) if epi == "dual" else None
    return yb, ya, ref, ref_a, (N, Ho, Wo, Cout, ob)


@pytest.mark.parametrize("case", DIRECT_CASES)
@pytest.mark.parametrize("epi", ["plain", "bias_relu", "res_relu", "dual"])
def test_direct_bf16x9_matches_float64(eng, case, epi):
    yb, ya, ref, ref_a, (N, Ho, Wo, Cout, ob) = _run_direct(eng, case, epi, sum(case))
    got = _from_padded(eng, yb, N, Ho, Wo, Cout, ob)
    assert torch.isfinite(got).all()
    tol = CONV_TOL * max(1.0, ref.abs().max().item())
    assert (got - ref).abs().max().item() < tol
    full = yb[: N * (Ho + 2) * (Wo + 2) * Cout].view(N, Ho + 2, Wo + 2, Cout)
    assert torch.all(full[:, 0] == 7.0) and torch.all(full[:, :, 0] == 7.0) and torch.all(full[:, -1] == 7.0) and torch.all(full[:, :, -1] == 7.0)
    if epi == "dual":
        got_a = _from_padded(eng, ya, N, Ho, Wo, Cout, ob)
        assert (got_a - ref_a).abs().max().item() < tol * 2


EDGE_SCALES = [
    # (name, operand scale, weight scale): what the exact-piece split meets at the ends of the fp32 range
    ("tiny_1e-30", 1e-30, 1.0),
    ("huge_1e30", 1e30, 1e-2),
    ("third_piece_subnormal", 2.0 ** -115, 1.0),   # x3 ~ 2^-131: a SUBNORMAL bf16, which the MFMA reads as zero
    ("tiny_weights_1e-30", 1.0, 1e-30),            # the same on the weight side (split on the host)
]


@pytest.mark.parametrize("name,sx,sw", EDGE_SCALES)
@pytest.mark.parametrize("K", [3, 1])
def test_direct_bf16x9_at_the_ends_of_the_fp32_range(eng, name, sx, sw, K):
    """equal to the float64 sum of the fp32 operands to CONV_TOL of the output scale, plus at most 1e-37 absolute (a dropped subnormal piece)"""
    N, Cin, H, W, Cout, s = 2, 256, 16, 20, 128, 2
    p = K // 2
    g = torch.Generator().manual_seed(7)
    x = (torch.randn(N, Cin, H, W, generator=g).double() * sx).float()
    w = (torch.randn(Cout, Cin, K, K, generator=g).double() * (2.0 / (Cin * K * K)) ** 0.5 * sw).float()
    assert torch.isfinite(x).all() and torch.isfinite(w).all() and x.abs().max() > 0 and (x < 0).any() and (w < 0).any()
    Ho, Wo = (H + 2 * p - K) // s + 1, (W + 2 * p - K) // s + 1
    xb = _to_padded(eng, x, Cin, 1)
    yb = eng.padded_nhwc(N, Ho, Wo, Cout, 1, "cuda")
    wp = torch.from_numpy(eng.conv_bf16x9_pack_weights(w.numpy(), Cin, None)).cuda()
    eng.conv2d_bf16x9_nhwc(xb, N, H, W, Cin, 1, wp, None, Cout, K, s, p, yb, 1)
    torch.cuda.synchronize()
    got = _from_padded(eng, yb, N, Ho, Wo, Cout, 1).double()
    ref = F.conv2d(x.double(), w.double(), stride=s, padding=p)
    scale = ref.abs().max().item()
    err = (got - ref).abs().max().item()
    assert scale > 0 and torch.isfinite(got).all()
    assert err < CONV_TOL * scale + 1e-37, (name, K, err, scale)


def test_direct_bf16x9_is_deterministic(eng):
    case = (4, 128, 30, 40, 256, 3, 2, 1, 1)
    N, Cin, H, W, Cout, K, s, p, ib = case
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, K, K, generator=g) * 0.03
    xb = _to_padded(eng, x, Cin, ib)
    wp = torch.from_numpy(eng.conv_bf16x9_pack_weights(w.numpy(), Cin, None)).cuda()
    Ho, Wo = (H + 2 * p - K) // s + 1, (W + 2 * p - K) // s + 1
    outs = []
    for _ in range(2):
        yb = eng.padded_nhwc(N, Ho, Wo, Cout, 1, "cuda")
        eng.conv2d_bf16x9_nhwc(xb, N, H, W, Cin, ib, wp, None, Cout, K, s, p, yb, 1)
        outs.append(yb)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])


def _backbone(eng, kind, c_in, direct):
    from tests.support import synthetic as syn

    sd = syn.make_state_dict(kind, c_in, "logits", 1, seed=5)
    old = os.environ.get("MP_CONV_DIRECT_BF16")
    os.environ["MP_CONV_DIRECT_BF16"] = "1" if direct else "0"
    try:
        return eng.Backbone(kind, c_in, "logits", 1, sd)
    finally:
        if old is None:
            del os.environ["MP_CONV_DIRECT_BF16"]
        else:
            os.environ["MP_CONV_DIRECT_BF16"] = old


def _forward(eng, bb, x, n_feat):
    b = x.shape[0]
    xb = _to_padded(eng, x, bb.c_in_p, bb.in_border)
    out, feat = torch.empty(b, 1, device="cuda"), torch.empty(b, n_feat, device="cuda")
    eng.profile_begin()
    bb.forward(xb, b, x.shape[2], x.shape[3], out, None, feat)
    prof = eng.profile_end()
    del xb
    return feat.cpu(), prof


@pytest.mark.parametrize("kind,c_in,n_down", [("vanilla_resnet34", 9, 3), ("vanilla_resnet34", 27, 3), ("resnet34", 9, 3)])
def test_backbone_runs_the_stride2_layers_on_pieces(eng, kind, c_in, n_down):
    """576 rows: layer{2,3,4}.0.conv1 + .downsample on the piece kernel (six launches), nothing on the fp32 kernel of the 128-channel tile
    (the stem of an fp32 input stays on the 64-channel one); 2 rows: split-K as before; features vs MP_CONV_DIRECT_BF16=0 within 2e-5"""
    g = torch.Generator(device="cuda").manual_seed(0)
    x8 = torch.rand(8, c_in, 240, 320, generator=g, device="cuda")
    x = x8.repeat(72, 1, 1, 1)   # 576 rows
    bb = _backbone(eng, kind, c_in, True)
    bb_ref = _backbone(eng, kind, c_in, False)
    n_feat = 512
    feat, prof = _forward(eng, bb, x, n_feat)
    feat_ref, prof_ref = _forward(eng, bb_ref, x, n_feat)
    assert PIECE_KERNEL in prof and prof[PIECE_KERNEL]["launches"] == 2 * n_down, prof.keys()
    assert not any(k.startswith(FP32_WIDE_TILE) for k in prof), prof.keys()
    assert PIECE_KERNEL not in prof_ref and any(k.startswith(FP32_WIDE_TILE) for k in prof_ref)
    assert torch.isfinite(feat).all()
    scale = max(1.0, feat_ref.abs().max().item())
    assert (feat - feat_ref).abs().max().item() < 2e-5 * scale
    assert torch.equal(feat[:8], feat[8:16])
    # 2 rows: the layers whose plan splits every tile along K (mode 1) stay on the fp32 split-K path, the others run single pass on pieces
    small, prof_s = _forward(eng, bb, x8[:2].contiguous(), n_feat)
    n_cu = eng.device_info()[0]
    w = 512 if kind == "vanilla_resnet34" else 512 * bb.width
    shapes = [(w // 8, 60, 80, w // 4), (w // 4, 30, 40, w // 2), (w // 2, 15, 20, w)]
    modes = [eng.conv2d_plan(2, h, ww, cin, 1, cout, k, 2, k // 2, n_cu, ws_floats=12 << 20)["mode"]
             for cin, h, ww, cout in shapes for k in (3, 1)]
    assert 1 in modes and any(k.endswith("/splitk") for k in prof_s)
    assert prof_s.get(PIECE_KERNEL, {"launches": 0})["launches"] == sum(m != 1 for m in modes)
    assert (small - feat[:2]).abs().max().item() < 2e-5 * scale

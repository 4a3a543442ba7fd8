"""Shared pieces of the convolution kernel tests (tests/test_gpu_kernels.py, tests/test_gpu_wino_walk.py): the padded-NHWC layouts, the
float64 references -- on the CPU through F.conv2d, and on the device as nine shifted NHWC matmuls for tensors too large for the CPU -- and
the fused epilogues the kernels offer."""
import math

import torch
import torch.nn.functional as F

# What the hardware achieves (profiles/r04_wino_bf16_native_check.txt, r04_stem_native_check_v1.txt: <= 7e-6 of the output scale for every
# convolution kernel against the direct fp32 sum) with a margin of 3: a kernel that loses a piece product or a bit of an operand (2^-16
# relative and up) fails this; the round-4 bound of 2e-4 would have let a 20x regression pass.  The reference sum is formed in float64
# from the fp32 operands (the folded weight w * scale rounded to fp32 first, as the packers do), so the bound measures OUR error only.
CONV_TOL = 2e-5

# the fused epilogues: plain = conv only; bias_relu = relu(conv * scale + bias); res_relu = relu(... + residual); dual = y = ... + residual
# (no ReLU) and the second output relu(y * act_scale + act_shift) (WideResNet blocks); res = ... + residual, no ReLU, no second output
# (the last WideResNet block)
EPILOGUES = ("plain", "bias_relu", "res_relu", "dual")
RELU_EPILOGUES = ("bias_relu", "res_relu")
RES_EPILOGUES = ("res_relu", "dual", "res")

WT = 64      # tiles (2 x 2 output pixels) per unit of the Winograd kernels
WCOUT = 64   # output channels per unit


def to_padded(eng, x_nchw, cp, border):
    n, c, h, w = x_nchw.shape
    buf = eng.padded_nhwc(n, h, w, cp, border, "cuda")
    v = eng.padded_view(buf, n, h, w, cp, border)
    v[..., :c] = x_nchw.permute(0, 2, 3, 1).cuda()
    return buf


def from_padded(eng, buf, n, h, w, c, border):
    return eng.padded_view(buf, n, h, w, c, border).permute(0, 3, 1, 2).contiguous().cpu()


def padded_len(n, h, w, c, border):
    return n * (h + 2 * border) * (w + 2 * border) * c


def wino_slack(w, c, border):
    """floats of read slack a Winograd launch may touch behind an odd-sized input (include/mp_engine.h): one padded row and one pixel, + 64"""
    return (w + 2 * border + 1) * c + 64


def wino_input(eng, n, h, w, c, border):
    """zeroed padded-NHWC input for a Winograd launch whose read slack -- exactly wino_slack() floats, no more -- is poisoned with NaN:
    nothing read there may reach an output"""
    n_x = padded_len(n, h, w, c, border)
    xb = torch.full((n_x + wino_slack(w, c, border),), float("nan"), device="cuda")
    xb[:n_x] = 0.0
    return xb


def fold_weights(w, scale):
    """the folded weight w * scale, rounded to fp32 as the packers round it"""
    return (w.double() * scale.double().view(-1, 1, 1, 1)).float() if scale is not None else w.float()


def conv_ref_f64(x, w, scale, bias, stride, pad):
    wf = fold_weights(w, scale)
    y = F.conv2d(x.double(), wf.double(), None, stride=stride, padding=pad)
    if bias is not None:
        y = y + bias.double().view(1, -1, 1, 1)
    return y.float()


def conv3x3_ref_f64_device(xpad, border, w, scale=None, bias=None, residual=None, relu=False, act=None, chunk_bytes=1 << 30):
    """float64 reference of a 3x3 / stride-1 / pad-1 convolution + fused epilogue on the device, for inputs too large for the CPU:
    nine shifted NHWC matmuls (one per kernel tap) over chunks of images.  `xpad`: the [N, H + 2b, W + 2b, C] view of a padded-NHWC
    buffer (its zero border is the convolution's padding), `w` [Cout, C, 3, 3] and `scale` folded and rounded to fp32 as the packers do,
    `residual` an [N, H, W, Cout] view, `act` = (act_scale, act_shift) of the second output.  Yields (n0, n1, y, y_act | None) with
    y [n1 - n0, H, W, Cout] float64."""
    N, Hp, Wp, C = xpad.shape
    H, W = Hp - 2 * border, Wp - 2 * border
    wt = fold_weights(w, scale).double().to(xpad.device).permute(2, 3, 1, 0).contiguous()   # [3, 3, C, Cout]
    b64 = bias.double().to(xpad.device) if bias is not None else None
    a64 = (act[0].double().to(xpad.device), act[1].double().to(xpad.device)) if act is not None else None
    step = max(1, chunk_bytes // ((H + 2) * (W + 2) * max(C, wt.shape[-1]) * 8))
    for n0 in range(0, N, step):
        n1 = min(N, n0 + step)
        xc = xpad[n0:n1, border - 1 : border + H + 1, border - 1 : border + W + 1, :].double()
        y = torch.zeros(n1 - n0, H, W, wt.shape[-1], dtype=torch.float64, device=xpad.device)
        for kh in range(3):
            for kw in range(3):
                y += xc[:, kh : kh + H, kw : kw + W, :] @ wt[kh, kw]
        del xc
        if b64 is not None:
            y += b64
        if residual is not None:
            y += residual[n0:n1].double()
        if relu:
            y = torch.relu(y)
        ya = torch.relu(y * a64[0] + a64[1]) if a64 is not None else None
        yield n0, n1, y, ya


def n_units(N, H, W, Cout):
    """units (64 tiles x 64 output channels) of a Winograd launch: what the persistent form's resident workgroups walk"""
    return math.ceil(N * ((H + 1) // 2) * ((W + 1) // 2) / WT) * (Cout // WCOUT)


def guard_max_n(H, W, C, Cout, in_border, out_border):
    """the largest batch the 32-bit addressing guard of the Winograd kernels accepts, from the guard's own formulas
    (mp_conv_wino_eligible, mp_conv3x3_wino_bf16_nhwc): n_tiles < 2^30, in_bytes = ((N * Hp + 2) * Wp * C * 4) < 2^31,
    out_elems = N * Hop * Wop * Cout < 2^29.  Returns (N, name of the binding limit)."""
    Hp, Wp = H + 2 * in_border, W + 2 * in_border
    Hop, Wop = H + 2 * out_border, W + 2 * out_border
    limits = {
        "n_tiles": ((1 << 30) - 1) // (((H + 1) // 2) * ((W + 1) // 2)),
        "in_bytes": (((1 << 31) - 1) // (Wp * C * 4) - 2) // Hp,
        "out_elems": ((1 << 29) - 1) // (Hop * Wop * Cout),
    }
    name = min(limits, key=limits.get)
    return limits[name], name

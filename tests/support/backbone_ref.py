"""Plain references of the pose backbones ONE STAGE AT A TIME (tests/test_gpu_backbone_stages.py, tests/test_backbone_stage_ref_cpu.py).

`BackboneRef` works on a reference-layout state dict (oracle/backbones.py restates the same graphs end to end) and applies every
BatchNorm UNFOLDED, so that the rounding of the engine's load-time fold (w * g / sqrt(var + eps) in float32) is part of what a
comparison measures.  Each function maps the input of one stage to its output, so a test can feed it the ENGINE's own input to that stage
(Backbone.debug_tensor) and see the stage's own error.  All tensors are NCHW, in the dtype and on the device of the instance.

The convolution is pluggable: F.conv2d (CPU), or `conv_matmul` -- K x K shifted, strided NHWC matmuls, the generalisation of
tests/support/wino.conv3x3_ref_f64_device -- for float64 on the device, where the large-batch cases are too slow for the CPU."""
from __future__ import annotations

from typing import Callable, Dict, List

import torch
import torch.nn.functional as F

EPS = 1e-5   # eval BatchNorm of the reference nets


def conv_matmul(x: torch.Tensor, w: torch.Tensor, stride: int = 1, padding: int = 0) -> torch.Tensor:
    """conv2d(x [N, C, H, W], w [Cout, C, KH, KW]) without bias as KH x KW matmuls of shifted, strided NHWC views (any device / dtype)"""
    N, C, H, W = x.shape
    Cout, Cw, KH, KW = w.shape
    assert C == Cw, (x.shape, w.shape)
    Ho, Wo = (H + 2 * padding - KH) // stride + 1, (W + 2 * padding - KW) // stride + 1
    xp = F.pad(x.permute(0, 2, 3, 1), (0, 0, padding, padding, padding, padding))   # [N, H + 2p, W + 2p, C]
    wt = w.permute(2, 3, 1, 0).contiguous()                                             # [KH, KW, C, Cout]
    y = torch.zeros(N, Ho, Wo, Cout, dtype=x.dtype, device=x.device)
    for kh in range(KH):
        for kw in range(KW):
            y += xp[:, kh : kh + (Ho - 1) * stride + 1 : stride, kw : kw + (Wo - 1) * stride + 1 : stride, :] @ wt[kh, kw]
    return y.permute(0, 3, 1, 2)


def nhwc_to_nchw(t: torch.Tensor, dtype=None) -> torch.Tensor:
    """[n, h, w, c] (a debug tap's interior) -> [n, c, h, w], same device"""
    t = t.permute(0, 3, 1, 2)
    return t if dtype is None else t.to(dtype)


def padded_tap(bb, what: str, batch: int, h: int, w: int, slot: int = 0):
    """the WHOLE padded buffer of a backbone tap as a [n, h + 2b, w + 2b, c] view of the workspace + its border b: Backbone.debug_tensor
    returns the interior only; this one lets a test check the border ring around it"""
    flat, (n, hh, ww, c), b = bb.debug_buffer(what, batch, h, w, slot)
    return flat.view(n, hh + 2 * b, ww + 2 * b, c), b


def border_is_zero(full: torch.Tensor, b: int) -> bool:
    """True if the ring of width b around the interior of a padded [n, H, W, c] view holds nothing but zeros"""
    ring = full.clone()
    ring[:, b : ring.shape[1] - b, b : ring.shape[2] - b] = 0
    return not bool((ring != 0).any())


class BackboneRef:
    """vanilla_resnet34 | resnet34 | resnet18 | resnet34_width=N (shapes come from the state dict) in `dtype` on `device`"""

    def __init__(self, sd: Dict[str, torch.Tensor], kind: str, dtype=torch.float64, device="cpu",
                 conv: Callable[..., torch.Tensor] = F.conv2d, prefix: str = "backbone."):
        self.sd = {k: v.to(device=device, dtype=dtype) for k, v in sd.items() if torch.is_tensor(v) and v.dtype.is_floating_point}
        self.wide = kind != "vanilla_resnet34"
        self.conv, self.p, self.dtype, self.device = conv, prefix, dtype, torch.device(device)
        self.blocks: Dict[int, List[int]] = {}
        for s in range(1, 5):
            i = 0
            while f"{prefix}layer{s}.{i}.conv1.weight" in self.sd:
                self.blocks.setdefault(s, []).append(i)
                i += 1

    # ------------------------------------------------------------------ pieces
    def _bn(self, key: str, x: torch.Tensor) -> torch.Tensor:
        sd = self.sd
        m, v, g, b = sd[key + ".running_mean"], sd[key + ".running_var"], sd[key + ".weight"], sd[key + ".bias"]
        if x.device.type == "cpu":   # the call oracle/backbones.py makes: the float32 composition equals it bit for bit
            return F.batch_norm(x, m, v, g, b, False, 0.0, EPS)
        sh = (1, -1, 1, 1)           # the same function spelled out (float64 on the device)
        return (x - m.view(sh)) / torch.sqrt(v.view(sh) + EPS) * g.view(sh) + b.view(sh)

    def _conv(self, x: torch.Tensor, key: str, stride: int, padding: int) -> torch.Tensor:
        return self.conv(x, self.sd[key], stride=stride, padding=padding)

    def _stride(self, s: int, i: int) -> int:
        return 2 if (i == 0 and s > 1) else 1

    def _has_down(self, s: int) -> bool:
        return f"{self.p}layer{s}.0.downsample.{'weight' if self.wide else '0.weight'}" in self.sd

    # ------------------------------------------------------------------ stages
    def stem(self, x: torch.Tensor) -> torch.Tensor:
        """relu(bn1(conv1(x))): 7x7 / 2 / pad 3 (vanilla) or 5x5 / 2 / pad 2 (pre-activation nets); the max pool belongs to stage 1"""
        k = self.sd[self.p + "conv1.weight"].shape[-1]
        return F.relu(self._bn(self.p + "bn1", self._conv(x, self.p + "conv1.weight", 2, k // 2)))

    def next_act(self, s: int, x: torch.Tensor) -> torch.Tensor:
        """pre-activation nets: relu(bn1(x)) with the bn1 of stage s + 1's first block, x = the output of stage s"""
        assert self.wide and 1 <= s <= 3
        return F.relu(self._bn(f"{self.p}layer{s + 1}.0.bn1", x))

    def downsample(self, s: int, x_in: torch.Tensor) -> torch.Tensor:
        """the 1x1 / stride-2 shortcut of stage s's first block.  vanilla: bn(conv(x_in)), x_in = the output of stage s - 1;
        pre-activation nets: conv(x_in), x_in = relu(bn1(.)) of that output (next_act(s - 1, .), what the block's convolutions read)"""
        P = f"{self.p}layer{s}.0."
        if self.wide:
            return self._conv(x_in, P + "downsample.weight", self._stride(s, 0), 0)
        return self._bn(P + "downsample.1", self._conv(x_in, P + "downsample.0.weight", self._stride(s, 0), 0))

    def block(self, s: int, i: int, x: torch.Tensor) -> torch.Tensor:
        P, stride = f"{self.p}layer{s}.{i}.", self._stride(s, i)
        down = i == 0 and self._has_down(s)
        if not self.wide:
            out = F.relu(self._bn(P + "bn1", self._conv(x, P + "conv1.weight", stride, 1)))
            out = self._bn(P + "bn2", self._conv(out, P + "conv2.weight", 1, 1))
            return F.relu(out + (self.downsample(s, x) if down else x))
        a = F.relu(self._bn(P + "bn1", x))
        res = self.downsample(s, a) if down else x
        out = F.relu(self._bn(P + "bn2", self._conv(a, P + "conv1.weight", stride, 1)))
        return self._conv(out, P + "conv2.weight", 1, 1) + res

    def stage(self, s: int, x_in: torch.Tensor) -> torch.Tensor:
        """every block of layer{s}; s = 1 takes the stem map and pools it first (3x3 / 2 / pad 1).  The pre-activation nets apply their
        own bn1 + ReLU to x_in inside."""
        x = F.max_pool2d(x_in, 3, 2, 1) if s == 1 else x_in
        for i in self.blocks[s]:
            x = self.block(s, i, x)
        return x

    def tail(self, x: torch.Tensor) -> Dict[str, torch.Tensor]:
        """average pool (+ fc on the vanilla net) -> "features", then whichever head the state dict has -> "pose" | "renderings_logits".
        Small: always on the CPU."""
        sd = {k: v.cpu() for k, v in self.sd.items() if not k.startswith(self.p + "layer")}
        x = x.cpu()
        if self.wide:
            feat = x.flatten(2).mean(dim=-1)
        else:
            feat = F.linear(F.adaptive_avg_pool2d(x, 1).flatten(1), sd[self.p + "fc.weight"], sd[self.p + "fc.bias"])
        out = {"features": feat}
        if "pose_fc.weight" in sd:
            out["pose"] = F.linear(feat, sd["pose_fc.weight"], sd["pose_fc.bias"])
        if "views_logits_head.weight" in sd:
            out["renderings_logits"] = F.linear(feat, sd["views_logits_head.weight"], sd["views_logits_head.bias"])
        return out

    def forward(self, x: torch.Tensor) -> Dict[str, torch.Tensor]:
        """the stages composed (the un-forced path)"""
        x = self.stem(x)
        for s in range(1, 5):
            x = self.stage(s, x)
        return self.tail(x)

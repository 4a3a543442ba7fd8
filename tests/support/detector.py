"""Shared pieces of the detector stage tests (tests/test_gpu_zz_detector_stages.py): reading the engine's debug taps (padded NHWC maps,
row matrices whose rows are padded past their logical width), the layout conversions the oracle (oracle/mask_rcnn.py) needs, a float64
MultiScaleRoIAlign reference that takes its decisions in float32 as the kernel does, and a rank-for-rank matcher of selection results that tolerates only counted, near-tied exceptions."""
from __future__ import annotations

from typing import Callable, Optional, Sequence

import numpy as np
import torch


def nhwc_to_nchw(t: torch.Tensor, dtype=torch.float64) -> torch.Tensor:
    """[n, h, w, c] (a debug tap's interior) -> contiguous [n, c, h, w] on the CPU"""
    return t.detach().cpu().permute(0, 3, 1, 2).contiguous().to(dtype)


def raw_debug(net, what: str):
    """the WHOLE buffer behind a debug tap, borders and row padding included -> (flat CPU tensor, shape4, border, row_stride).
    DetectorNet.debug_tensor returns the logical view only; this one lets a test check what lies outside it (zero borders, zero pad
    columns of the padded row matrices)."""
    flat, shp, border, rs = net.debug_buffer(what)
    return flat.cpu(), shp, border, rs


def debug_rows(net, what: str) -> torch.Tensor:
    """a row-matrix tap ("class_logits", "mask_logits") as [rows, row_stride]: every row in full, the pad columns past the logical
    width included"""
    flat, shp, border, rs = raw_debug(net, what)
    assert border == 0 and rs >= shp[1], (what, shp, rs)
    return flat.view(shp[0], rs)


def mask_logits_28(rows: torch.Tensor, n_det: int) -> torch.Tensor:
    """mask_logits rows [n_det * 14 * 14 * 4, Cs] -> [n_det, Cs, 28, 28].  Row ((det * 14 + y) * 14 + x) * 4 + a * 2 + b holds mask pixel
    (2 y + a, 2 x + b): the 2x2 stride-2 transposed convolution runs as a 1x1 convolution onto 4 sub-pixel channel groups."""
    cs = rows.shape[1]
    t = rows.reshape(n_det, 14, 14, 2, 2, cs).permute(0, 5, 1, 3, 2, 4)   # det, c, y, a, x, b
    return t.reshape(n_det, cs, 28, 28)


def debug_map(net, what: str) -> torch.Tensor:
    """a padded-NHWC tap as its [n, h, w, c] interior, after asserting that the border ring around it is zero"""
    flat, shp, b, _ = raw_debug(net, what)
    n, h, w, c = shp
    assert b > 0, (what, b)
    full = flat.view(n, h + 2 * b, w + 2 * b, c)
    inner = full[:, b : b + h, b : b + w].clone()
    full[:, b : b + h, b : b + w] = 0
    assert (full == 0).all(), f"{what}: non-zero border"
    return inner


def roi_levels(boxes: torch.Tensor, k_min: int = 2, k_max: int = 5) -> torch.Tensor:
    """LevelMapper of MultiScaleRoIAlign (ops/poolers.py) in float32: k = floor(4 + log2(sqrt(area) / 224) + 1e-6) clamped to
    [k_min, k_max]; boxes [K, 4] float32"""
    boxes = boxes.float()
    area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    return torch.floor(4 + torch.log2(torch.sqrt(area) / 224) + torch.tensor(1e-6)).clamp(k_min, k_max).long()


def multiscale_roi_align_f64(maps: Sequence[torch.Tensor], boxes: Sequence[torch.Tensor], image_sizes, P: int, chunk_bytes: int = 1 << 28):
    """float64 reference of MultiScaleRoIAlign(["0".."3"], P, sampling_ratio = 2) (oracle.mask_rcnn.multiscale_roi_align).
    maps: P2..P5 as [n, h, w, c] (NHWC interiors of the engine's taps, any float dtype); boxes: one [k, 4] float32 tensor per image.
    -> (out [K, P, P, c] float64, levels [K] in 2..5), K = the boxes of all images in order.

    What DECIDES something runs in float32, operation for operation as oracle.thirdparty.roi_align and det_roi_align_kernel do: the
    level, the scaled box, max(size, 1), the bin size, the sample coordinates, the skip test (< -1 or > size), the clamps at 0 and at
    the last row / column, the integer corner.  The fractional part c - floor(c) is exact in float32; from it on everything is float64:
    1 - l, the four corner weights, the interpolation and the mean of the 2 x 2 samples."""
    f32 = torch.float32
    rois = torch.cat([b.to(f32).reshape(-1, 4) for b in boxes])
    bidx = torch.cat([torch.full((len(b),), i, dtype=torch.long) for i, b in enumerate(boxes)])
    K, C = len(rois), int(maps[0].shape[-1])
    oh, ow = max(s[0] for s in image_sizes), max(s[1] for s in image_sizes)
    scales = []
    for f in maps:   # poolers.py infer_scale, from the sizes of the (unpadded) images
        s1 = 2.0 ** float(torch.tensor(float(f.shape[1]) / float(oh)).log2().round())
        s2 = 2.0 ** float(torch.tensor(float(f.shape[2]) / float(ow)).log2().round())
        assert s1 == s2, (s1, s2)
        scales.append(s1)
    k_min, k_max = int(-np.log2(scales[0])), int(-np.log2(scales[-1]))
    levels = roi_levels(rois, k_min, k_max)
    out = torch.zeros(K, P, P, C, dtype=torch.float64)
    g = 2
    per_roi = (P * g) ** 2 * C * 8 * 3   # gathered corner values, their weighted copy and the accumulator
    step = max(1, chunk_bytes // per_roi)

    def prep(c, size):
        invalid = (c < -1.0) | (c > size)
        c = torch.where(c <= 0, torch.zeros_like(c), c)
        lo = c.floor().long()
        at_edge = lo >= size - 1
        lo = torch.where(at_edge, torch.full_like(lo, size - 1), lo)
        hi = torch.where(at_edge, lo, lo + 1)
        c = torch.where(at_edge, lo.to(f32), c)
        l = (c - lo.to(f32)).double()   # exact in float32
        return invalid, lo, hi, l, 1.0 - l

    for li, (f, sc) in enumerate(zip(maps, scales)):
        n, H, W, _ = f.shape
        flat = f.reshape(n * H * W, C).double()
        sel_all = torch.where(levels == li + k_min)[0]
        for s0 in range(0, len(sel_all), step):
            sel = sel_all[s0 : s0 + step]
            b = rois[sel]
            x1, y1, x2, y2 = b[:, 0] * sc, b[:, 1] * sc, b[:, 2] * sc, b[:, 3] * sc
            rw, rh = torch.clamp(x2 - x1, min=1.0), torch.clamp(y2 - y1, min=1.0)
            bin_h, bin_w = rh / P, rw / P
            i_ = torch.arange(g, dtype=f32)
            p_ = torch.arange(P, dtype=f32)
            ys = y1[:, None, None] + p_[None, :, None] * bin_h[:, None, None] + ((i_[None, None, :] + 0.5) * bin_h[:, None, None] / g)
            xs = x1[:, None, None] + p_[None, :, None] * bin_w[:, None, None] + ((i_[None, None, :] + 0.5) * bin_w[:, None, None] / g)
            assert ys.dtype == f32 and xs.dtype == f32
            inv_y, ylo, yhi, ly, hy = prep(ys, H)   # [k, P, g]
            inv_x, xlo, xhi, lx, hx = prep(xs, W)
            live = (~(inv_y[:, :, :, None, None] | inv_x[:, None, None, :, :])).double()   # [k, P, g, P, g]
            base = (bidx[sel] * (H * W))[:, None, None, None, None]
            acc = torch.zeros(len(sel), P, g, P, g, C, dtype=torch.float64)
            for yi, wy in ((ylo, hy), (yhi, ly)):
                for xi, wx in ((xlo, hx), (xhi, lx)):
                    idx = base + yi[:, :, :, None, None] * W + xi[:, None, None, :, :]
                    wgt = wy[:, :, :, None, None] * wx[:, None, None, :, :] * live
                    acc += flat[idx.reshape(-1)].view(*idx.shape, C) * wgt[..., None]
            out[sel] = acc.sum(dim=(2, 4)) / float(g * g)
    return out, levels


def iou_f32(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """pairwise IoU [len(a), len(b)] in float32 with torchvision's nms_kernel operation order (the order det_nms_kernel uses)"""
    a, b = a.astype(np.float32), b.astype(np.float32)
    w = np.maximum(np.float32(0), np.minimum(a[:, None, 2], b[None, :, 2]) - np.maximum(a[:, None, 0], b[None, :, 0]))
    h = np.maximum(np.float32(0), np.minimum(a[:, None, 3], b[None, :, 3]) - np.maximum(a[:, None, 1], b[None, :, 1]))
    inter = w * h
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / (area_a[:, None] + area_b[None, :] - inter)


def match_ranked(same: Callable[[int, int], bool], n_got: int, ref_keys: Sequence[float], eps: float,
                 got_keys: Optional[Sequence[float]] = None):
    """Rank-for-rank comparison of a selection result (got) with the oracle's (ref).  `same(i, j)`: got entry i is ref entry j.
    Position i must hold ref entry i, with two exceptions, each counted:
      * a neighbour swap: got[i], got[i + 1] = ref[i + 1], ref[i] where the ref keys of the pair differ by less than eps;
      * the cut: the last position holds another entry whose key (got_keys) is within eps of the ref entry's key.
    eps = 0 admits no exception.  -> (n_exceptions, None) or (n_exceptions, message of the first mismatch)"""
    n_ref = len(ref_keys)
    if n_got != n_ref:
        return 0, f"{n_got} entries, the oracle has {n_ref}"
    exc, i = 0, 0
    while i < n_ref:
        if same(i, i):
            i += 1
        elif i + 1 < n_ref and same(i, i + 1) and same(i + 1, i) and abs(float(ref_keys[i]) - float(ref_keys[i + 1])) < eps:
            exc += 1
            i += 2
        elif i == n_ref - 1 and got_keys is not None and abs(float(got_keys[i]) - float(ref_keys[i])) < eps:
            exc += 1
            i += 1
        else:
            return exc, f"rank {i} of {n_ref}: not the oracle's entry (ref key {float(ref_keys[i])!r})"
    return exc, None

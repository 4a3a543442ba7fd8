"""float64 references and case tables for the kernels in front of and behind the backbone: the roi_align crop (csrc/crop_device.h,
crop.hip), depth normalisation and the observation repack (crop.hip), the max pool, the pre-activation and the pool + fc + heads tail
(pool_fc.hip).  Used by tests/test_input_tail_ref_cpu.py (the references and tables against the oracle, on the CPU) and
tests/test_gpu_input_tail_kernels.py (the kernels against the references).

roi_align: the sample COORDINATES are formed in float32 in exactly the expression order of torchvision's roi_align_kernel.cpp and of
crop_pixel -- (start + p * bin) + ((i + 0.5) * bin) / 4 with bin = max(x2 - x1, 1) / out -- because the library is compiled without
contraction, so these are the kernel's coordinates bit for bit; taps and validity follow from them.  Everything behind the taps (the
weights 1 - l, the products, the 16-sample sum, the division) is float64, so a comparison measures the kernel's own rounding.
"""
from __future__ import annotations

import functools
from typing import Dict, NamedTuple, Optional, Sequence

import numpy as np
import torch

F32 = np.float32
N_GRID = 4                 # sampling_ratio
VALID_RULE = 0.99          # cropping.py:140: depth crop zeroed where roi_align(depth > 0) < 0.99
VALID_BAND = 1e-5          # a valid fraction this close to VALID_RULE may fall either way (fp32 summation order): left out of comparisons
CROP_TOL = 1e-5            # x max(1, max|image|): the project's roi_align tolerance (tests/test_gpu_kernels.py), here against float64


class Taps(NamedTuple):
    lo: np.ndarray      # [n_out, 4] int64
    hi: np.ndarray
    l: np.ndarray       # [n_out, 4] float64 weight of `hi`; `lo` weighs 1 - l
    valid: np.ndarray   # [n_out, 4] bool


def sample_coords(start, size_roi, n_out: int) -> np.ndarray:
    """[n_out, 4] float32 sample coordinates of one axis of one roi"""
    bin_ = np.maximum(F32(size_roi), F32(1.0)) / F32(n_out)
    p = np.arange(n_out, dtype=F32)[:, None]
    i = np.arange(N_GRID, dtype=F32)[None, :]
    c = (F32(start) + p * bin_) + ((i + F32(0.5)) * bin_) / F32(N_GRID)
    assert c.dtype == F32
    return c


def make_taps(c: np.ndarray, size: int) -> Taps:
    """pre_calc_for_bilinear_interpolate on one axis: c < -1 or c > size is invalid, c <= 0 becomes 0, lo >= size - 1 clamps"""
    valid = ~((c < F32(-1.0)) | (c > F32(size)))
    c = np.where(c <= 0, F32(0.0), c)
    lo = c.astype(np.int64)                       # truncation of a non-negative float
    edge = lo >= size - 1
    lo = np.where(edge, size - 1, lo)
    hi = np.where(edge, lo, lo + 1)
    c64 = np.where(edge, lo.astype(np.float64), c.astype(np.float64))
    return Taps(lo, hi, c64 - lo, valid)


def axis_taps(x1, x2, n_out: int, size: int) -> Taps:
    return make_taps(sample_coords(x1, F32(x2) - F32(x1), n_out), size)


def patch_path(ty: Taps, tx: Taps) -> np.ndarray:
    """[out_h, out_w] bool: crop_pixel's switch restated from the taps -- the separable 4x4-patch path is taken where the four samples of
    the bin span fewer than 4 source rows AND fewer than 4 source columns, the general 16-sample path elsewhere"""
    return ((ty.hi[:, 3] - ty.lo[:, 0]) < 4)[:, None] & ((tx.hi[:, 3] - tx.lo[:, 0]) < 4)[None, :]


def crop_paths(H: int, W: int, boxes, out_h: int, out_w: int) -> np.ndarray:
    """[b, out_h, out_w] bool patch_path of every box (no image needed)"""
    boxes = np.asarray(boxes, dtype=F32).reshape(-1, 4)
    return np.stack([patch_path(axis_taps(b[1], b[3], out_h, H), axis_taps(b[0], b[2], out_w, W)) for b in boxes])


class CropRef(NamedTuple):
    crop: np.ndarray                    # [b, C, out_h, out_w] float64, plain roi_align
    valid_frac: Optional[np.ndarray]    # [b, out_h, out_w] float64 roi_align(depth > 0)   (C = 4 only)
    ruled: np.ndarray                   # crop with the depth channel zeroed where valid_frac < 0.99 (= crop for C = 3)
    patch_path: np.ndarray              # [b, out_h, out_w] bool
    excluded: np.ndarray                # [b, out_h, out_w] bool: depth pixels whose valid_frac lies within VALID_BAND of the rule


def _bilinear_sum(img: np.ndarray, ty: Taps, tx: Taps) -> np.ndarray:
    """sum over the 4 x 4 samples of the bilinear interpolation of img [C, H, W] float64 -> [C, out_h, out_w]; invalid samples add 0"""
    acc = np.zeros((img.shape[0], ty.lo.shape[0], tx.lo.shape[0]), dtype=np.float64)
    for a in range(N_GRID):
        for b in range(N_GRID):
            yl, yh, ly = ty.lo[:, a], ty.hi[:, a], ty.l[:, a][:, None]
            xl, xh, lx = tx.lo[:, b], tx.hi[:, b], tx.l[:, b][None, :]
            hy, hx = 1.0 - ly, 1.0 - lx
            val = (hy * hx) * img[:, yl][:, :, xl] + (hy * lx) * img[:, yl][:, :, xh] + (ly * hx) * img[:, yh][:, :, xl] \
                + (ly * lx) * img[:, yh][:, :, xh]
            ok = ty.valid[:, a][:, None] & tx.valid[:, b][None, :]
            acc += np.where(ok[None], val, 0.0)
    return acc


def roi_align_f64(images, im_ids, boxes, out_h: int, out_w: int) -> CropRef:
    """torchvision.ops.roi_align(sampling_ratio=4, aligned=False) of images [n_im, C, H, W] (fp32 values) for boxes [b, 4] = x1, y1, x2, y2
    on frame im_ids [b], plus the RGBD validity rule of lib3d/cropping.py:131-142 for C = 4.  Ids outside [0, n_im) and non-finite boxes
    are undefined in the reference and refused here."""
    images = np.asarray(images, dtype=F32)
    boxes = np.asarray(boxes, dtype=F32).reshape(-1, 4)
    im_ids = np.asarray(im_ids, dtype=np.int64).reshape(-1)
    n_im, C, H, W = images.shape
    assert np.isfinite(boxes).all() and ((im_ids >= 0) & (im_ids < n_im)).all() and len(im_ids) == len(boxes)
    img64 = images.astype(np.float64)
    b = len(boxes)
    crop = np.zeros((b, C, out_h, out_w))
    frac = np.zeros((b, out_h, out_w)) if C == 4 else None
    path = np.zeros((b, out_h, out_w), dtype=bool)
    for k in range(b):
        x1, y1, x2, y2 = boxes[k]
        ty, tx = axis_taps(y1, y2, out_h, H), axis_taps(x1, x2, out_w, W)
        crop[k] = _bilinear_sum(img64[im_ids[k]], ty, tx) / (N_GRID * N_GRID)
        if C == 4:
            frac[k] = _bilinear_sum((img64[im_ids[k], 3:4] > 0).astype(np.float64), ty, tx)[0] / (N_GRID * N_GRID)
        path[k] = patch_path(ty, tx)
    ruled = crop.copy()
    excluded = np.zeros((b, out_h, out_w), dtype=bool)
    if C == 4:
        ruled[:, 3] = np.where(frac < VALID_RULE, 0.0, crop[:, 3])
        excluded = np.abs(frac - VALID_RULE) <= VALID_BAND
    return CropRef(crop, frac, ruled, path, excluded)


# ---------------------------------------------------------------------------------------------------------------------------------- #
# crop cases.  One case = one launch: image size, output size, <= 3 boxes and the frame each reads.  Bins are (x2 - x1) / out_w by
# (y2 - y1) / out_h source pixels per output pixel; a pixel is on the patch path iff its taps span < 4 source pixels on both axes.
H0, W0 = 37, 53
CROP_CASES: Dict[str, dict] = {
    # bins around 1, fractional: all on the patch path.  36 x 52 = 1872 pixels = 7.3 blocks of 256
    "unit_full": dict(out=(36, 52), boxes=[[0.3, 0.4, 52.1, 36.2]], ids=[1]),
    "unit_bins": dict(out=(17, 23), boxes=[[5.2, 3.1, 30.7, 22.4], [10.5, 8.25, 31.2, 23.9], [20.1, 2.2, 48.3, 30.3]], ids=[0, 1, 1]),
    # bins >= 4 on both axes: every in-image pixel takes the general 16-sample path
    "general_4": dict(out=(9, 13), boxes=[[0, 0, 53, 37], [0.5, 0.25, 52.5, 36.25], [0.3, 0.2, 52.9, 36.8]], ids=[0, 1, 0]),
    "general_5": dict(out=(7, 10), boxes=[[0, 0, 53, 37], [2.5, 1.5, 50.5, 35.5], [4.2, 3.3, 49.9, 33.1]], ids=[1, 1, 0]),
    "general_6": dict(out=(6, 8), boxes=[[0, 0, 53, 37], [3.1, 2.2, 51.3, 36.4], [10, 5, 50, 35]], ids=[0, 1, 1]),
    "general_7": dict(out=(5, 7), boxes=[[0, 0, 53, 37], [1.7, 0.9, 52.2, 36.6], [8.4, 2.1, 51.9, 35.2]], ids=[1, 0, 1]),
    "general_4b": dict(out=(8, 12), boxes=[[0.7, 0.1, 52.3, 36.9], [2, 2, 51, 36], [0, 0, 53, 37]], ids=[0, 0, 1]),
    "general_4c": dict(out=(9, 12), boxes=[[0, 0, 53, 37], [1.5, 0.5, 52.5, 36.9], [0.2, 0.1, 50.1, 36.3]], ids=[1, 0, 1]),
    "general_4d": dict(out=(8, 11), boxes=[[0.4, 0.6, 52.8, 36.7], [3.3, 1.1, 50.6, 34.9], [0, 0, 53, 37]], ids=[0, 1, 0]),
    "general_4e": dict(out=(7, 12), boxes=[[0, 0, 53, 37], [1.1, 2.3, 51.7, 36.2], [2.6, 0.8, 52.9, 35.5]], ids=[1, 1, 0]),
    # ... with every side overhanging by more than 1 px: invalid samples inside the general path
    "general_overhang": dict(out=(9, 13), boxes=[[-6, -5, 59, 42], [-3.5, -2.5, 56.5, 39.5], [-12, -9, 66, 47]], ids=[0, 1, 1]),
    # bin about 1.1 on one axis and 3.1 on the other, both ways round
    "anisotropic": dict(out=(20, 10), boxes=[[5, 4, 36, 26], [10.2, 3.3, 41.4, 25.2]], ids=[1, 0]),
    "anisotropic_t": dict(out=(7, 28), boxes=[[4.5, 6, 35.3, 27.7]], ids=[0]),
    # bins 2.5 - 3.1: both paths inside one crop
    "mixed": dict(out=(12, 17), boxes=[[0, 0, 53, 37], [2, 1, 47, 33], [3.3, 2.2, 52.6, 36.1]], ids=[0, 1, 0]),
    # each side overhung by more than 1 px (samples < -1 / > size: invalid), the last box on all four sides at once
    "overhang_far": dict(out=(13, 19), boxes=[[-5.5, -4.2, 14.3, 9.1], [40.2, 26.3, 59.7, 40.9], [-3.0, -2.6, 56.4, 40.2]], ids=[1, 0, 1]),
    # each side overhung by less than 1 px: samples in (-1, 0] clamp to 0 and stay valid; (size - 1, size] clamps, beyond size is invalid
    "overhang_near": dict(out=(13, 19), boxes=[[-0.7, -0.6, 18.6, 12.7], [34.3, 24.4, 53.8, 37.7], [-0.9, -0.95, 53.9, 37.9]], ids=[0, 1, 1]),
    # boxes ending exactly at x2 = W, y2 = H
    "exact_end": dict(out=(13, 19), boxes=[[34, 24, 53, 37], [0, 0, 53, 37], [27.5, 18.25, 53, 37]], ids=[1, 0, 0]),
    # entirely outside below-right and above-left (exactly 0), next to one that only touches the corner
    "outside": dict(out=(6, 9), boxes=[[60, 45, 80, 60], [-30, -25, -5, -4], [50, 35, 70, 50]], ids=[0, 1, 1], zero_rows=[0, 1]),
    # x2 < x1 / y2 < y1, a zero-size box, a box smaller than a pixel: the roi is clamped to 1 px
    "degenerate": dict(out=(4, 5), boxes=[[20.5, 10.5, 15.0, 5.0], [25.3, 17.8, 25.3, 17.8], [30, 20, 30.4, 20.3]], ids=[1, 0, 1]),
    # one output pixel: the whole image, a small box, a bin of 4
    "one_pixel": dict(out=(1, 1), boxes=[[0, 0, 53, 37], [10, 10, 12.5, 12.2], [5.5, 5.5, 9.6, 9.7]], ids=[0, 1, 0]),
    # a 1 x W and an H x 1 image: every tap of the short axis clamps to 0
    "row_image": dict(hw=(1, W0), out=(3, 21), boxes=[[2.2, 0, 40.1, 1], [-2, -0.5, 30, 1.5], [0, 0, 53, 1]], ids=[1, 0, 1]),
    "row_image_general": dict(hw=(1, W0), out=(2, 9), boxes=[[0, 0, 53, 1], [3.5, -0.2, 50.5, 0.9]], ids=[0, 1]),
    "col_image": dict(hw=(H0, 1), out=(19, 3), boxes=[[0, 1.3, 1, 30.2], [-0.5, -3, 1.5, 33], [0, 0, 1, 37]], ids=[0, 1, 1]),
    "col_image_general": dict(hw=(H0, 1), out=(7, 2), boxes=[[0, 0, 1, 37], [-0.3, 2.5, 0.8, 35.5]], ids=[1, 0]),
}
N_IM = 2

# the rasteriser's fused crop (mp_raster_render_crop) at h, w = 64, 80 over 480 x 640 observations: bins of 5.5 - 8 source pixels, the
# second box overhanging every side
FUSED_BOXES = [[60.0, 40.0, 580.0, 440.0], [-30.0, -20.0, 610.0, 470.0], [100.5, 60.25, 540.0, 420.0]]
FUSED_IDS = [1, 0, 1]


def crop_case_shape(name: str):
    c = CROP_CASES[name]
    return c.get("hw", (H0, W0)), c["out"]


@functools.lru_cache(maxsize=None)
def crop_case_images(name: str, C: int) -> torch.Tensor:
    """[2, C, H, W] fp32 frames of a case: colours in [0, 1); depth in [0, 2) with about 5 % of its pixels 0 (invalid)"""
    (H, W), _ = crop_case_shape(name)
    g = torch.Generator().manual_seed(1000 * C + sorted(CROP_CASES).index(name))
    im = torch.rand(N_IM, C, H, W, generator=g)
    if C == 4:
        im[:, 3] = im[:, 3] * 2
        im[:, 3][torch.rand(N_IM, H, W, generator=g) < 0.05] = 0.0
    return im


@functools.lru_cache(maxsize=None)
def crop_case_ref(name: str, C: int) -> CropRef:
    """the float64 reference of a case, computed once and shared (treat as read-only)"""
    c = CROP_CASES[name]
    return roi_align_f64(crop_case_images(name, C).numpy(), c["ids"], c["boxes"], *c["out"])


# ---------------------------------------------------------------------------------------------------------------------------------- #
def normalize_depth_f64(x, tCR, mode: int) -> np.ndarray:
    """models/pose_rigid.py:466-496 on x [b, ...] (fp32 values) with z = tCR[:, 2], in float64: 0 none, 1 tCR_scale d / z,
    2 tCR_scale_clamp_center clamp(d / z, 0, 2) - 1, 3 tCR_center_clamp clamp(d - z, -2, 2)"""
    x = np.asarray(x, dtype=F32).astype(np.float64)
    z = np.asarray(tCR, dtype=F32).astype(np.float64)[:, 2].reshape((-1,) + (1,) * (x.ndim - 1))
    if mode == 0:
        return x
    if mode == 1:
        return x / z
    if mode == 2:
        return np.clip(x / z, 0.0, 2.0) - 1.0
    if mode == 3:
        return np.clip(x - z, -2.0, 2.0)
    raise ValueError(f"unknown depth normalisation mode {mode}")


DEPTH_TCR = [[0.1, -0.2, 0.8], [0.0, 0.3, -1.3], [-0.4, 0.1, 2.4]]     # a different z per row, one negative
DEPTH_HW = (13, 21)                                                  # 273 pixels: one block of 256 and a partial one
# C, listed channels
DEPTH_LAYOUTS = [(5, [3]), (32, [3]), (32, [3, 10, 31])]
DEPTH_BORDERS = [0, 2, 3]


def depth_values(n_ch: int) -> torch.Tensor:
    """[3, 13, 21, n_ch] fp32 depths: a quarter exactly 0 (background), the rest N(0, 3^2) -- negative depths, d / z beyond [0, 2] and
    d - z beyond +-2 on every row of DEPTH_TCR.  Finite, and no z is 0: non-finite depths and z = 0 are out of scope."""
    g = torch.Generator().manual_seed(40 + n_ch)
    d = torch.randn(3, *DEPTH_HW, n_ch, generator=g) * 3
    d[torch.rand(3, *DEPTH_HW, n_ch, generator=g) < 0.25] = 0.0
    return d


def bn_relu_f64(m: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor):
    """(pre, relu(pre)) with pre = m * scale[c] + shift[c] in float64, m [N, C, H, W]"""
    pre = m.double() * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    return pre, torch.relu(pre)


POOL_SHAPES = [(1, 1), (2, 2), (5, 8), (9, 7)]
POOL_CHANNELS = [4, 12, 128]
POOL_IN_BORDERS = [1, 2, 3]
POOL_OUT_BORDERS = [0, 1, 2]


@functools.lru_cache(maxsize=None)
def pool_inputs(H: int, W: int, C: int, N: int = 2):
    """x [N, C, H, W] in [0, 1), its 3x3 / stride-2 / pad-1 max pool m (torch), and a scale / shift pair per channel.  Odd channels: shifts
    around -0.8, so relu cuts about half of m * s + h.  Even channels: h = -fl32(m0 * s) with m0 the pooled value of pixel (0, 0) of image
    0, so there m * s + h is the rounding residual of the product (|.| <= 2^-24 m0 s): a fused multiply-add returns it, a separate
    multiply and add returns 0."""
    g = torch.Generator().manual_seed(H * 100 + W * 10 + C)
    x = torch.rand(N, C, H, W, generator=g)
    m = torch.nn.functional.max_pool2d(x, 3, 2, 1)
    sc = torch.rand(C, generator=g) + 0.5
    sh = torch.randn(C, generator=g) * 0.4 - 0.8
    even = torch.arange(0, C, 2)
    sh[even] = -(m[0, even, 0, 0] * sc[even])
    return x, m, sc, sh


def pool_fc_heads_f64(x: torch.Tensor, fc_w, fc_b, head_w: torch.Tensor, head_b: torch.Tensor):
    """models/pose_rigid.py:326-333 in float64: features = mean over H x W of x [N, C, H, W], through the fc layer if there is one;
    out = heads(features); sigmoid(out).  -> (feat [N, n_feat], out [N, n_out], sigmoid)"""
    pooled = x.double().mean(dim=(2, 3))
    feat = pooled @ fc_w.double().t() + fc_b.double() if fc_w is not None else pooled
    out = feat @ head_w.double().t() + head_b.double()
    return feat, out, torch.sigmoid(out)


# N, H, W, C, border, fc?, n_feat, n_out
POOL_FC_CASES = [
    (3, 8, 10, 512, 1, True, 512, 9),
    (2, 8, 10, 512, 1, False, 512, 1),
    (1, 4, 5, 1024, 1, False, 1024, 9),     # WideResNet, width 2
    (3, 1, 1, 64, 0, True, 40, 5),          # H * W = 1, n_feat below a wave
    (2, 3, 2, 20, 2, True, 300, 4),         # n_feat above the 256 threads of the workgroup, C below a wave
    (2, 8, 10, 128, 1, True, 128, 26),      # views-logits head: more outputs than waves
]


def pool_fc_inputs(case: Sequence):
    """|x| in [0.5, 1.5] with random sign, weight magnitudes in [0.02, 0.08] with random sign: one dropped or misplaced term moves an
    output by >= 0.5 * 0.02 / (H * W) (pooling), 0.01 (fc, heads): far above the tolerance.  Rows of the batch differ."""
    N, H, W, C, border, fc, n_feat, n_out = case
    g = torch.Generator().manual_seed(N * 1000 + C + n_out)

    def signed(lo, hi, *shape):
        mag = lo + (hi - lo) * torch.rand(*shape, generator=g)
        return mag * (torch.randint(0, 2, shape, generator=g) * 2 - 1).float()

    x = signed(0.5, 1.5, N, C, H, W)
    fc_w = signed(0.02, 0.08, n_feat, C) if fc else None
    fc_b = signed(0.02, 0.08, n_feat) if fc else None
    return x, fc_w, fc_b, signed(0.02, 0.08, n_out, n_feat), signed(0.02, 0.08, n_out)

"""-m gpu: the kernels in front of and behind the backbone -- the roi_align crop (stand-alone and fused into the rasteriser's launch), the
observation repack, depth normalisation, the max pool, the pre-activation and the pool + fc + heads tail -- each against the float64
references of tests/support/input_tail_ref.py, at the shapes, borders and box families of its case tables.  The tables and references
themselves are checked on the CPU by tests/test_input_tail_ref_cpu.py (agreement with the fp32 oracle, the census of the crop's two
arithmetic paths, the validity-rule exclusions), so a failure here is the kernel's.

Every output buffer is poisoned (a NaN with its own payload) and compared bit for bit wherever the kernel must not write.  Nothing here
is larger than a 480 x 640 frame or a batch of 3, ids are in range and boxes finite.

Bounds (none tuned to the kernels):
  crop           |got - ref64| < 1e-5 * max(1, max|image|)   the project's roi_align tolerance, here against float64
  normalise      |got - ref64| <= 2 * 2^-23 * max(1, |ref64|)   one or two correctly rounded fp32 operations per mode
  max pool       bit-equal to F.max_pool2d
  pre-activation |got - ref64| <= 2^-23 * |ref64|             one fmaf rounding + the float64 -> fp32 double rounding; 0 where ref64 <= 0
  tail           feat, out within 1e-4 * max(1, max|ref64|), sigmoid within 1e-5   (test_maxpool_and_tail's, here against float64)

Worst error measured on the MI355X, as a share of the bound (printed by every test, summed up when the module ends):
  crop, stand-alone   0.014 (C = 3), 0.018 (C = 4) over the table: 9414 output pixels per C, 31.8 % of them on the general path, no
                      validity-rule pixel excluded; on most cases the kernel lands on the fp32 oracle's own error
  crop, fused         0.014; 99.9 % of the 3 x 64 x 80 pixels on the general path, 2 of 15360 depth pixels excluded
  normalise           0.25 in modes 1 - 3 (half an ulp at |ref| just above 1)
  pre-activation      0.50 (half an ulp: the fmaf is correctly rounded)
  tail                feat 0.0042, out 0.0013, sigmoid 0.0081
No kernel defect showed.  Against a scratch build with one arithmetic slip per kernel (general path of the NHWC4 crop scaled by 1.0001,
row validity dropped on the patch path, mode 3's upper clamp one ulp high, 1e-30 in the packed RGB's 4th channel, a separate multiply
and add in the pool's second output, the heads' last feature dropped above 256) each slip failed the tests aimed at it and no other.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from tests.support import input_tail_ref as itr

pytestmark = pytest.mark.gpu

WORST = {}
POISON_BITS = 0x7FC0BEEF   # a quiet NaN with a payload of its own


def _note(name: str, share: float) -> None:
    WORST[name] = max(WORST.get(name, 0.0), float(share))
    print(f"  {name}: {share:.4f} of the bound")


@pytest.fixture(scope="module")
def eng():
    from megapose6d_amd import engine

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert engine.device_info()[2].startswith("gfx950")
    yield engine
    print("\nworst error per kernel, as a share of its bound:")
    for k, v in sorted(WORST.items()):
        print(f"  {k:24s} {v:.4f}")


def _poisoned(*shape) -> torch.Tensor:
    return torch.full(shape, POISON_BITS, dtype=torch.int32, device="cuda").view(torch.float32)


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32)


def _is_poison(t: torch.Tensor) -> bool:
    return bool((_bits(t) == POISON_BITS).all())


# ---------------------------------------------------------------------------------------------------------------------------------- #
# crop
def _check_crop(name, got, ref: itr.CropRef, images, zero_rows=()):
    """got [b, C, oh, ow] float64 against the ruled reference on every pixel that is not excluded"""
    tol = itr.CROP_TOL * max(1.0, float(np.abs(images).max()))
    err = np.abs(got - ref.ruled)
    C = got.shape[1]
    if C == 4:
        err[:, 3][ref.excluded] = 0.0
    print(f"  {name}: worst {err.max():.2e} of {tol:.1e}; general path {1 - ref.patch_path.mean():.1%}, excluded {int(ref.excluded.sum())}")
    _note(f"crop C={C}" if not name.startswith("fused") else "crop fused", err.max() / tol)
    assert np.isfinite(got).all() and ref.excluded.mean() <= 1e-3
    assert err.max() < tol, (name, np.unravel_index(err.argmax(), err.shape))
    for k in zero_rows:
        assert not got[k].any(), (name, k)


@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("name", sorted(itr.CROP_CASES))
def test_crop_roi_align_vs_float64(eng, name, C):
    """mp_crop_roi_align on every case of the table into channels 2 .. 2 + C of a poisoned 8-channel NHWC tensor (`mixed`: at an offset of
    40 floats into its buffer)"""
    c = itr.CROP_CASES[name]
    (oh, ow), b = c["out"], len(c["boxes"])
    images, ref = itr.crop_case_images(name, C), itr.crop_case_ref(name, C)
    Cp, c0, off = 8, 2, 40 if name == "mixed" else 0
    buf = _poisoned(off + b * oh * ow * Cp)
    eng.crop_roi_align(images.cuda(), torch.tensor(c["ids"], dtype=torch.int32).cuda(), torch.tensor(c["boxes"], dtype=torch.float32).cuda(),
                       oh, ow, buf, oh * ow * Cp, ow * Cp, Cp, c0, out_offset_floats=off)
    torch.cuda.synchronize()
    out = buf[off:].view(b, oh, ow, Cp)
    assert _is_poison(buf[:off]) and _is_poison(out[..., :c0]) and _is_poison(out[..., c0 + C:])
    got = out[..., c0:c0 + C].permute(0, 3, 1, 2).double().cpu().numpy()
    _check_crop(name, got, ref, images.numpy(), c.get("zero_rows", ()))


def test_crop_roi_align_refuses_and_empty_batch(eng):
    """b = 0 launches nothing; b = 65536 (one grid row per box, at most 65535) and C = 2 are refused with nothing launched"""
    from megapose6d_amd import _lib

    images = torch.rand(2, 3, 9, 11).cuda()
    ids, boxes = torch.zeros(1, dtype=torch.int32).cuda(), torch.tensor([[1.0, 1.0, 8.0, 7.0]]).cuda()
    out = _poisoned(1, 4, 5, 8)
    rc = _lib.load().mp_crop_roi_align(images.data_ptr(), 2, 3, 9, 11, ids.data_ptr(), boxes.data_ptr(), 0, 4, 5, out.data_ptr(), 4 * 5 * 8, 5 * 8, 8,
                                       0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0 and _is_poison(out)
    many = 65536
    with pytest.raises(eng.EngineError, match="bad size"):
        eng.crop_roi_align(images, torch.zeros(many, dtype=torch.int32).cuda(), boxes.repeat(many, 1), 4, 5, out, 0, 5 * 8, 8, 0)
    with pytest.raises(eng.EngineError, match="C must be 3 or 4"):
        eng.crop_roi_align(images[:, :2].contiguous(), ids, boxes, 4, 5, out, 4 * 5 * 8, 5 * 8, 8, 0)
    torch.cuda.synchronize()
    assert _is_poison(out)
    eng.crop_roi_align(images, ids, boxes, 4, 5, out, 4 * 5 * 8, 5 * 8, 8, 0)      # and the same call with b = 1 does write
    torch.cuda.synchronize()
    assert not torch.isnan(out[..., :3]).any() and _is_poison(out[..., 3:])


_FUSED = {}


def _fused_inputs(C):
    """two 480 x 640 frames (depth: a block and 0.1 % of the pixels invalid) + the float64 crop of FUSED_BOXES at 64 x 80, once per C"""
    if C not in _FUSED:
        g = torch.Generator().manual_seed(77 + C)
        images = torch.rand(2, C, 480, 640, generator=g)
        if C == 4:
            images[:, 3] = images[:, 3] * 2
            images[:, 3][torch.rand(2, 480, 640, generator=g) < 0.001] = 0.0
            images[:, 3, 100:220, 150:400] = 0.0
        _FUSED[C] = (images, itr.roi_align_f64(images.numpy(), itr.FUSED_IDS, itr.FUSED_BOXES, 64, 80))
    return _FUSED[C]


@pytest.mark.parametrize("V", [1, 4])
@pytest.mark.parametrize("C", [3, 4])
def test_fused_crop_on_the_general_path(eng, engine_meshes, C, V):
    """mp_raster_render_crop at h, w = 64, 80 over 480 x 640 observations: boxes covering most of the frame give bins of 5.5 - 8 source
    pixels, so nearly every pixel runs crop_pixel's general 16-sample path -- from a planar observation and from a PackedObservation (the
    NHWC4 instantiation).  Bit-equal to the stand-alone crop + a plain raster launch, and within the crop bound of the float64 reference."""
    from tests.support import synthetic as syn

    images, ref = _fused_inputs(C)
    general = 1.0 - ref.patch_path.mean()
    assert general > 0.9, general
    db = eng.MeshDB(engine_meshes)
    rng = np.random.RandomState(7)
    n_items, h, w, Cp = 3, 64, 80, 32
    im_ids = torch.tensor(itr.FUSED_IDS, dtype=torch.int32).cuda()
    boxes = torch.tensor(itr.FUSED_BOXES, dtype=torch.float32).cuda()
    T = torch.from_numpy(np.stack([syn.random_pose(rng, z_range=(0.3, 0.6)) for _ in range(n_items * V)])).cuda()
    K = torch.from_numpy(np.repeat(syn.K_EXAMPLE[None].astype(np.float32), n_items * V, 0)).cuda()
    K[:, :2] *= w / 640.0
    ids = torch.tensor([0, 1, 2], dtype=torch.int32).repeat_interleave(V).cuda()
    dev_images = images.cuda()

    def launch(crop):
        x = _poisoned(n_items, h, w, Cp)
        if crop is None:
            eng.crop_roi_align(dev_images, im_ids, boxes, h, w, x, h * w * Cp, w * Cp, Cp, 0)
        eng.raster_render(db, ids, T, K, h, w, 1, eng.make_lights(), x, h * w * Cp, w * Cp, Cp, C, C + 3, -1, views_per_item=V, stride_view=6,
                          crop=crop)
        torch.cuda.synchronize()
        return x

    want = launch(None)
    assert _is_poison(want[..., C + 6 * V:]) and not torch.isnan(want[..., :C + 6 * V]).any()
    for source in (dev_images, eng.PackedObservation(dev_images)):
        got = launch((source, im_ids, boxes, 0))
        assert torch.equal(_bits(got), _bits(want)), type(source).__name__
    _check_crop(f"fused C={C} V={V}", want[..., :C].permute(0, 3, 1, 2).double().cpu().numpy(), ref, images.numpy())


@pytest.mark.parametrize("C", [3, 4])
def test_pack_observation_nhwc4(eng, C):
    """[2, C, 37, 53] -> [2, 37, 53, 4]: 1961 pixels per frame (7.66 blocks); the 4th channel of an RGB observation is exactly 0"""
    g = torch.Generator().manual_seed(C)
    images = torch.randn(2, C, 37, 53, generator=g)
    packed = eng.PackedObservation(images.cuda())
    torch.cuda.synchronize()
    assert (packed.n_im, packed.C, packed.H, packed.W) == (2, C, 37, 53) and packed.data.shape == (2, 37, 53, 4)
    got = packed.data.cpu()
    assert torch.equal(got[..., :C], images.permute(0, 2, 3, 1))
    if C == 3:
        assert torch.equal(_bits(got[..., 3]), torch.zeros(2, 37, 53, dtype=torch.int32))


# ---------------------------------------------------------------------------------------------------------------------------------- #
# depth normalisation
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_normalize_depth_f32_vs_reference_formulas(eng, mode):
    """mp_normalize_depth (fp32) against models/pose_rigid.py:466-496 in float64: b = 3 with its own z per row (one negative), borders 0, 2
    and 3, 5 and 32 channels, channel lists [3] and [3, 10, 31], 273 pixels per row.  Depths hold 0 (background), negative values, d / z
    beyond [0, 2] and d - z beyond +-2.  Non-finite depths and z = 0 are out of scope: the reference formulas give NaN / inf there and
    no caller produces them."""
    tCR = torch.tensor(itr.DEPTH_TCR)
    z = tCR[:, 2].double().numpy().reshape(3, 1, 1, 1)
    h, w = itr.DEPTH_HW
    for C, chans in itr.DEPTH_LAYOUTS:
        d = itr.depth_values(len(chans))
        ref = itr.normalize_depth_f64(d.numpy(), tCR.numpy(), mode)
        for border in itr.DEPTH_BORDERS:
            x = _poisoned(3, h + 2 * border, w + 2 * border, C)
            inner = x[:, border:border + h, border:border + w]
            inner[..., chans] = d.cuda()
            before = x.clone()
            eng.normalize_depth(x, 3, h, w, border, C, chans, tCR.cuda(), mode)
            torch.cuda.synchronize()
            if mode == 0:
                assert torch.equal(_bits(x), _bits(before))
                continue
            listed = torch.zeros_like(x, dtype=torch.bool)
            listed[:, border:border + h, border:border + w][..., chans] = True
            assert _is_poison(x[~listed]), (C, chans, border)          # unlisted channels and the border keep their bits
            got = inner[..., chans].double().cpu().numpy()
            bound = 2.0 * 2.0 ** -23 * np.maximum(1.0, np.abs(ref))
            err = np.abs(got - ref)
            _note(f"normalize_depth mode {mode}", (err / bound).max())
            assert (err <= bound).all(), (C, chans, border, np.unravel_index((err / bound).argmax(), err.shape))
            d64 = d.double().numpy()
            if mode == 2:
                q = d64 / z
                assert (got[np.broadcast_to(d64 == 0, got.shape)] == -1.0).all()                      # background
                assert (got[q > 2.0 + 1e-6] == 1.0).all() and (got[q < -1e-6] == -1.0).all()          # clamped: exactly the bound
                assert (q > 2.0 + 1e-6).any() and (q < -1e-6).any()
            if mode == 3:
                s = d64 - z
                assert (got[s > 2.0 + 1e-6] == 2.0).all() and (got[s < -2.0 - 1e-6] == -2.0).all()
                assert (s > 2.0 + 1e-6).any() and (s < -2.0 - 1e-6).any()


def test_normalize_depth_refuses_an_unknown_mode(eng):
    x = _poisoned(1, 4, 4, 5)
    with pytest.raises(eng.EngineError, match="unknown mode"):
        eng.normalize_depth(x, 1, 4, 4, 0, 5, [3], torch.tensor([[0.0, 0.0, 1.0]]).cuda(), 7)
    torch.cuda.synchronize()
    assert _is_poison(x)


# ---------------------------------------------------------------------------------------------------------------------------------- #
# max pool / pre-activation
def _padded(eng, x_nchw, border):
    """zero-bordered padded-NHWC buffer of x [N, C, H, W]"""
    n, c, h, w = x_nchw.shape
    buf = eng.padded_nhwc(n, h, w, c, border, "cuda")
    eng.padded_view(buf, n, h, w, c, border).copy_(x_nchw.permute(0, 2, 3, 1).cuda())
    return buf


def _interior(buf, n, h, w, c, border):
    """(interior [n, c, h, w] on the host, True if everything around it still holds the poison)"""
    full = buf.view(n, h + 2 * border, w + 2 * border, c)
    mask = torch.ones_like(full, dtype=torch.bool)
    mask[:, border:border + h, border:border + w] = False
    return full[:, border:border + h, border:border + w].permute(0, 3, 1, 2).contiguous().cpu(), _is_poison(full[mask])


@pytest.mark.parametrize("C", itr.POOL_CHANNELS)
@pytest.mark.parametrize("hw", itr.POOL_SHAPES)
def test_maxpool_and_bn_relu_shapes_borders_outputs(eng, hw, C):
    """mp_maxpool3x3s2 over in_border 1 / 2 / 3 x out_border 0 / 1 / 2 x (y only, y_act only, both), and mp_bn_relu_nhwc over the pooled
    map: the second output of the pool kernel bit for bit (at border 0 as well).  The even channels carry cancelling scale / shift pairs
    (tests/support/input_tail_ref.pool_inputs), which only a fused multiply-add gets right."""
    H, W = hw
    N = 2
    x, m, sc, sh = itr.pool_inputs(H, W, C)
    Ho, Wo = m.shape[2:]
    pre, act_ref = itr.bn_relu_f64(m, sc, sh)
    bound = 2.0 ** -23 * act_ref.abs()
    d_sc, d_sh = sc.cuda(), sh.cuda()
    for ib in itr.POOL_IN_BORDERS:
        xb = _padded(eng, x, ib)
        for ob in itr.POOL_OUT_BORDERS:
            n_out = N * (Ho + 2 * ob) * (Wo + 2 * ob) * C
            acts = []
            for want_y, want_act in ((True, False), (False, True), (True, True)):
                y = _poisoned(n_out) if want_y else None
                ya = _poisoned(n_out) if want_act else None
                eng.maxpool3x3s2(xb, N, H, W, C, ib, y, ob, ya, d_sc if want_act else None, d_sh if want_act else None)
                torch.cuda.synchronize()
                if want_y:
                    got, clean = _interior(y, N, Ho, Wo, C, ob)
                    assert clean and torch.equal(got, m), (ib, ob, want_y, want_act)
                if want_act:
                    got, clean = _interior(ya, N, Ho, Wo, C, ob)
                    err = (got.double() - act_ref).abs()
                    assert clean and (err <= bound).all(), (ib, ob, want_y, want_act, err.max().item())
                    assert (got[pre <= 0] == 0).all()
                    if (act_ref > 0).any():
                        _note("maxpool y_act", (err[act_ref > 0] / bound[act_ref > 0]).max().item())
                    acts.append(ya)
            assert torch.equal(_bits(acts[0]), _bits(acts[1]))
            # the stand-alone pre-activation over the pooled map (same border in and out)
            yb = _poisoned(n_out)
            yb.view(N, Ho + 2 * ob, Wo + 2 * ob, C)[:, ob:ob + Ho, ob:ob + Wo] = m.permute(0, 2, 3, 1).cuda()
            ya2 = _poisoned(n_out)
            eng.bn_relu_nhwc(yb, N, Ho, Wo, C, ob, ya2, d_sc, d_sh)
            torch.cuda.synchronize()
            assert torch.equal(_bits(ya2), _bits(acts[0])), (ib, ob)


# ---------------------------------------------------------------------------------------------------------------------------------- #
# global average pool + fc + heads + sigmoid
@pytest.mark.parametrize("case", itr.POOL_FC_CASES, ids=lambda c: "x".join(str(int(v)) for v in c))
def test_pool_fc_heads_vs_float64(eng, case):
    """mp_pool_fc_heads stand-alone: with and without the fc layer (WideResNet: features = pooled, also at width 2), 1 to 26 outputs,
    n_feat below a wave and above the workgroup, H * W = 1, borders 0 / 1 / 2; d_out is the same bits whether or not the optional
    outputs are asked for"""
    N, H, W, C, border, fc, n_feat, n_out = case
    x, fc_w, fc_b, hw, hb = itr.pool_fc_inputs(case)
    f_ref, o_ref, s_ref = itr.pool_fc_heads_f64(x, fc_w, fc_b, hw, hb)
    xb = _padded(eng, x, border)
    dev = [t.cuda() if t is not None else None for t in (fc_w, fc_b, hw, hb)]
    feat, out, sig = _poisoned(N, n_feat), _poisoned(N, n_out), _poisoned(N, n_out)
    eng.pool_fc_heads(xb, N, H, W, C, border, dev[0], dev[1], n_feat, dev[2], dev[3], n_out, feat, out, sig)
    out2 = _poisoned(N, n_out)
    eng.pool_fc_heads(xb, N, H, W, C, border, dev[0], dev[1], n_feat, dev[2], dev[3], n_out, None, out2, None)
    torch.cuda.synchronize()
    e_f = (feat.double().cpu() - f_ref).abs().max().item() / (1e-4 * max(1.0, f_ref.abs().max().item()))
    e_o = (out.double().cpu() - o_ref).abs().max().item() / (1e-4 * max(1.0, o_ref.abs().max().item()))
    e_s = (sig.double().cpu() - s_ref).abs().max().item() / 1e-5
    _note("pool_fc_heads feat", e_f)
    _note("pool_fc_heads out", e_o)
    _note("pool_fc_heads sigmoid", e_s)
    assert e_f < 1 and e_o < 1 and e_s < 1, (e_f, e_o, e_s)
    assert torch.equal(_bits(out), _bits(out2))
    assert N == 1 or not torch.equal(out[0], out[1])


def test_pool_fc_heads_refuses_missing_fc_with_other_width(eng):
    x = torch.rand(1, 8, 2, 2)
    out = _poisoned(1, 3)
    with pytest.raises(eng.EngineError, match="n_feat != C"):
        eng.pool_fc_heads(_padded(eng, x, 1), 1, 2, 2, 8, 1, None, None, 12, torch.rand(3, 12).cuda(), torch.rand(3).cuda(), 3, None, out, None)
    torch.cuda.synchronize()
    assert _is_poison(out)

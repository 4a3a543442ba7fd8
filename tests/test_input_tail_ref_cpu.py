"""CPU: the float64 references and case tables of tests/support/input_tail_ref.py, before any kernel is compared with them.

- roi_align_f64 against the fp32 oracle (oracle.thirdparty.roi_align, sequential fp32 sums in torchvision's order) on every crop case;
- the census of the crop table: how many output pixels take each arithmetic path of crop_pixel (asserted, since a table without
  general-path pixels checks half of the kernel);
- the validity rule: how many depth pixels sit so close to the 0.99 threshold that the summation order decides them (left out of
  comparisons; must be next to none), and that both outcomes are well represented among the rest;
- the table's own promises (ids in range, finite boxes, the boxes that must give 0, batch sizes);
- the small references against torch's own operators.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.support import input_tail_ref as itr

CASES = sorted(itr.CROP_CASES)


def _oracle(name, C):
    from oracle import thirdparty as tp

    c = itr.CROP_CASES[name]
    imgs = itr.crop_case_images(name, C)
    rois = torch.cat([torch.tensor(c["ids"]).float()[:, None], torch.tensor(c["boxes"], dtype=torch.float32).reshape(-1, 4)], 1)
    ref = tp.roi_align(imgs, rois, c["out"], sampling_ratio=4)
    if C == 3:
        return ref, None
    vc = tp.roi_align((imgs[:, 3:4] > 0).float(), rois, c["out"], sampling_ratio=4)
    ruled = ref.clone()
    ruled[:, 3:4] = ref[:, 3:4] * (vc >= 0.99).float()      # cropping.py:131-142
    return ref, ruled


@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("name", CASES)
def test_roi_align_f64_agrees_with_the_fp32_oracle(name, C):
    r = itr.crop_case_ref(name, C)
    imgs = itr.crop_case_images(name, C)
    plain, ruled = _oracle(name, C)
    tol = itr.CROP_TOL * max(1.0, imgs.abs().max().item())
    err = np.abs(r.crop - plain.double().numpy()).max()
    print(f"{name} C={C}: |ref64 - oracle| {err:.2e} of {tol:.1e}")
    assert err < tol
    if C == 4:
        keep = ~r.excluded
        assert r.excluded.mean() <= 1e-3, (name, int(r.excluded.sum()))
        assert np.abs(r.ruled[:, 3] - ruled[:, 3].double().numpy())[keep].max() < tol
        assert np.array_equal(r.ruled[:, :3], r.crop[:, :3])
    else:
        assert r.valid_frac is None and np.array_equal(r.ruled, r.crop) and not r.excluded.any()


def test_crop_table_keeps_its_promises():
    sizes = set()
    for name, c in itr.CROP_CASES.items():
        boxes = np.asarray(c["boxes"], dtype=np.float32)
        assert boxes.shape == (len(c["ids"]), 4) and 1 <= len(boxes) <= 3, name
        assert np.isfinite(boxes).all() and all(0 <= i < itr.N_IM for i in c["ids"]), name
        sizes.add(c["out"][0] * c["out"][1])
        for C in (3, 4):
            r = itr.crop_case_ref(name, C)
            for k in c.get("zero_rows", []):
                assert not r.crop[k].any() and not r.ruled[k].any(), (name, k)     # exactly 0: every sample is invalid
    assert any(1 in c["ids"] for c in itr.CROP_CASES.values()) and any(0 in c["ids"] for c in itr.CROP_CASES.values())
    assert 1 in sizes and max(sizes) == 36 * 52 and any(s % 256 and s > 256 for s in sizes)
    assert {itr.crop_case_shape(n)[0] for n in itr.CROP_CASES} == {(37, 53), (1, 53), (37, 1)}
    # the families of the table, restated from the taps
    (H, W) = (itr.H0, itr.W0)
    assert itr.crop_case_ref("unit_full", 3).patch_path.all() and itr.crop_case_ref("unit_bins", 3).patch_path.all()
    for n in ("general_4", "general_5", "general_6", "general_7", "general_4b", "general_4c", "general_4d", "general_4e"):
        p = itr.crop_case_ref(n, 3).patch_path      # (a last row / column that ends at the image edge clamps its taps into a patch)
        assert not p[:, :-1, :-1].any() and p.mean() < 0.1, n
    m = itr.crop_case_ref("mixed", 3).patch_path.mean()
    assert 0.1 < m < 0.9, m
    # near overhang: samples in (-1, 0] exist and are valid; far overhang: invalid samples exist on every side
    near = itr.sample_coords(-0.7, np.float32(18.6) - np.float32(-0.7), 19)
    assert ((near > -1) & (near <= 0)).any() and itr.make_taps(near, W).valid.all()
    for b in itr.CROP_CASES["overhang_far"]["boxes"]:
        for x1, x2, n, size in ((b[0], b[2], 19, W), (b[1], b[3], 13, H)):
            t = itr.axis_taps(x1, x2, n, size)
            assert (~t.valid).any() and t.valid.any()
    lo_x, hi_x = (itr.sample_coords(b[0], np.float32(b[2]) - np.float32(b[0]), 19) for b in itr.CROP_CASES["overhang_far"]["boxes"][:2])
    assert (lo_x < -1).any() and (hi_x > W).any()
    # degenerate boxes: the roi is 1 px, so the bin is 1 / out
    c = itr.sample_coords(20.5, np.float32(15.0) - np.float32(20.5), 5)
    assert np.isclose(c[1, 0] - c[0, 0], 0.2)


def test_crop_table_census_of_the_two_paths():
    """at least 25 % of all output pixels (and at least 1000) on the general 16-sample path, at least 25 % on the 4x4-patch path"""
    paths = np.concatenate([itr.crop_case_ref(n, 3).patch_path.ravel() for n in CASES])
    n, n_patch = paths.size, int(paths.sum())
    n_general = n - n_patch
    print(f"crop census: {n} output pixels, general path {n_general} ({n_general / n:.1%}), patch path {n_patch} ({n_patch / n:.1%})")
    assert n_general >= 1000 and n_general >= 0.25 * n, (n_general, n)
    assert n_patch >= 0.25 * n, (n_patch, n)
    for name in CASES:      # the path does not depend on C
        assert np.array_equal(itr.crop_case_ref(name, 3).patch_path, itr.crop_case_ref(name, 4).patch_path)
        c = itr.CROP_CASES[name]
        (H, W), out = itr.crop_case_shape(name)
        assert np.array_equal(itr.crop_paths(H, W, c["boxes"], *out), itr.crop_case_ref(name, 3).patch_path)


def test_validity_rule_outcomes_and_exclusions():
    """per case at most 0.1 % of the depth pixels within 1e-5 of the 0.99 threshold; over the table, kept and zeroed depth pixels each
    >= 10 % of all depth pixels"""
    n = kept = zeroed = excluded = 0
    for name in CASES:
        r = itr.crop_case_ref(name, 4)
        assert r.excluded.mean() <= 1e-3, (name, int(r.excluded.sum()))
        keep = ~r.excluded
        n += r.excluded.size
        excluded += int(r.excluded.sum())
        kept += int((r.valid_frac >= itr.VALID_RULE)[keep].sum())
        zeroed += int((r.valid_frac < itr.VALID_RULE)[keep].sum())
    print(f"validity rule: {n} depth pixels, kept {kept} ({kept / n:.1%}), zeroed {zeroed} ({zeroed / n:.1%}), excluded {excluded}")
    assert kept >= 0.1 * n and zeroed >= 0.1 * n, (kept, zeroed, n)


def test_fused_crop_boxes_are_on_the_general_path():
    """the boxes tests/test_gpu_input_tail_kernels.py hands the rasteriser's fused crop: more than 90 % general-path pixels"""
    p = itr.crop_paths(480, 640, itr.FUSED_BOXES, 64, 80)
    print(f"fused crop boxes: general path {1 - p.mean():.1%}")
    assert 1 - p.mean() > 0.9


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_normalize_depth_f64_is_the_reference_formula(mode):
    g = torch.Generator().manual_seed(mode)
    d = torch.randn(3, 2, 1, 5, 7, generator=g) * 3
    tCR = torch.tensor([[0.1, 0.2, 0.8], [0.0, 0.0, -1.3], [0.3, 0.1, 2.4]])
    z = tCR[:, 2].double()[(...,) + (None,) * 4]
    want = {0: d.double(), 1: d.double() / z, 2: torch.clamp(d.double() / z, 0, 2) - 1, 3: torch.clamp(d.double() - z, -2, 2)}[mode]
    assert np.array_equal(itr.normalize_depth_f64(d.numpy(), tCR.numpy(), mode), want.numpy())
    with pytest.raises(ValueError):
        itr.normalize_depth_f64(d.numpy(), tCR.numpy(), 7)


def test_depth_inputs_reach_every_branch_of_every_mode():
    """per row of DEPTH_TCR (one z negative): background, negative depths, d / z below 0 and above 2, d - z below -2 and above 2, and
    values strictly inside the clamps; all finite, no z = 0"""
    tCR = np.asarray(itr.DEPTH_TCR, dtype=np.float32)
    assert (tCR[:, 2] != 0).all() and (tCR[:, 2] < 0).any() and len(set(tCR[:, 2])) == 3
    assert (itr.DEPTH_HW[0] * itr.DEPTH_HW[1]) % 256 != 0 and itr.DEPTH_HW[0] * itr.DEPTH_HW[1] > 256
    for C, chans in itr.DEPTH_LAYOUTS:
        assert all(0 <= c < C for c in chans)
        d = itr.depth_values(len(chans)).numpy()
        assert np.isfinite(d).all()
        q, s = itr.normalize_depth_f64(d, tCR, 1), d.astype(np.float64) - tCR[:, 2].astype(np.float64).reshape(3, 1, 1, 1)
        for r in range(3):
            assert (d[r] == 0).mean() > 0.1 and (d[r] < 0).any()
            assert (q[r] < -1e-3).any() and (q[r] > 2.001).any() and ((q[r] > 1e-3) & (q[r] < 1.999)).any(), r
            assert (s[r] < -2.001).any() and (s[r] > 2.001).any() and (np.abs(s[r]) < 1.999).any(), r


def test_pool_inputs_hold_cancelling_pairs():
    """inputs in [0, 1]; on the even channels of pixel (0, 0) m * s + h is a rounding residual: non-zero, below 2^-23, of both signs over
    the table; elsewhere the pre-activation has both signs"""
    pos = neg = cut = passed = 0
    for (H, W) in itr.POOL_SHAPES:
        for C in itr.POOL_CHANNELS:
            x, m, sc, sh = itr.pool_inputs(H, W, C)
            assert 0 <= x.min() and x.max() <= 1 and m.shape == (2, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1)
            pre, act = itr.bn_relu_f64(m, sc, sh)
            res = pre[0, 0::2, 0, 0]
            assert (res.abs() < 2.0 ** -23).all()
            pos, neg = pos + int((res > 0).sum()), neg + int((res < 0).sum())
            odd = pre[:, 1::2]
            cut, passed = cut + int((odd < 0).sum()), passed + int((odd > 0).sum())
            # a separate multiply and add rounds the product first: exactly 0 on the cancelling pairs
            unfused = (m * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))[0, 0::2, 0, 0]
            assert (unfused == 0).all()
    assert pos >= 20 and neg >= 20, (pos, neg)
    assert cut > 0.2 * (cut + passed) and passed > 0.2 * (cut + passed), (cut, passed)


def test_pool_fc_and_bn_relu_references_against_torch():
    for case in itr.POOL_FC_CASES:
        N, H, W, C, border, fc, n_feat, n_out = case
        assert N <= 3 and (fc or n_feat == C)
        x, fc_w, fc_b, hw, hb = itr.pool_fc_inputs(case)
        assert x.shape == (N, C, H, W) and hw.shape == (n_out, n_feat) and (fc_w is None) == (not fc)
        assert 0.5 <= x.abs().min() and x.abs().max() <= 1.5 and (x < 0).any() and (x > 0).any()
        assert 0.02 <= hw.abs().min() and hw.abs().max() <= 0.08
        assert N == 1 or not torch.equal(x[0], x[1])
        feat, out, sig = itr.pool_fc_heads_f64(x, fc_w, fc_b, hw, hb)
        f32 = x.mean(dim=(2, 3))
        if fc:
            f32 = F.linear(f32, fc_w, fc_b)
        o32 = F.linear(f32, hw, hb)
        assert (feat.float() - f32).abs().max() < 1e-5 and (out.float() - o32).abs().max() < 1e-5
        assert (sig.float() - torch.sigmoid(o32)).abs().max() < 1e-5
    m, s, h = torch.rand(2, 8, 3, 3), torch.randn(8), torch.randn(8)
    pre, act = itr.bn_relu_f64(m, s, h)
    assert (act.float() - F.relu(m * s.view(1, -1, 1, 1) + h.view(1, -1, 1, 1))).abs().max() < 1e-6 and (act >= 0).all()
    assert torch.equal(act, pre.clamp(min=0))

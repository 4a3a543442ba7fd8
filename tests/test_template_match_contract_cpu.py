"""CPU: the contract of the training-free detector (megapose6d_amd/csrc/template_match_core.h).  The host emulation
(tests/template_match_emul.cpp: the lines the kernels compile, walked tile by tile) against an independent numpy restatement written on
whole images (tests/support/template_match.py), every byte of ori, mag2, resp and the three location maps, exactly; the cases that can be
derived by hand; the order of templates; the limits; the feature selection; the detector end to end on renders of the oracle's
rasteriser; and the emulation once more as a stand-alone program under the sanitizers."""
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests.support import template_match as tmm


def _same(got, ref, what):
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    bad = np.argwhere(got != ref)
    assert len(bad) == 0, f"{what}: differs at {len(bad)} entries, first {bad[0].tolist()}"


def _quant_tiles(w):
    return (None, (1, 1), (5, 3), (w + 1, 2))


def _chain(images, T, templates, features, n_objects, blur=True, tiles=(None, None, None)):
    ori, mag2 = tmm.emul_quantize(images, blur, tile=tiles[0])
    resp = tmm.emul_response(ori, T, tile=tiles[1])
    h, w = images.shape[1:3]
    return (ori, mag2, resp) + tmm.emul_match(resp, h, w, T, templates, features, n_objects, tile=tiles[2])


# ---- 1. emulation = restatement ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blur", (True, False))
@pytest.mark.parametrize("h,w", tmm.SHAPES)
def test_emulation_equals_the_restatement(h, w, blur):
    images = tmm.image_case(2, h, w, 1)
    want_ori, want_mag2 = tmm.restate_quantize(images, blur)
    if h >= 8 and w >= 8:
        assert (want_ori > 0).any(), "the case must keep some orientations"
    for tile in _quant_tiles(w):
        ori, mag2 = tmm.emul_quantize(images, blur, tile=tile)
        _same(ori, want_ori, f"ori {h}x{w} blur={blur} tile={tile}")
        _same(mag2, want_mag2, f"mag2 {h}x{w} blur={blur} tile={tile}")
    templates, features = tmm.table_case(h, w, 65, 1)
    for T in tmm.SPREADS:
        want_resp = tmm.restate_response(want_ori, T)
        want = tmm.restate_match(want_ori, T, templates, features, tmm.N_OBJECTS)
        for rt, mt in ((None, None), ((1, 1), (1, 1)), ((5, 3), (5, 3)), ((w + 9, 2), (w + 1, 1))):
            resp = tmm.emul_response(want_ori, T, tile=rt)
            _same(resp, want_resp, f"resp {h}x{w} T={T} tile={rt}")
            got = tmm.emul_match(resp, h, w, T, templates, features, tmm.N_OBJECTS, tile=mt)
            for name, a, b in zip(("best_score", "best_f", "best_template"), got, want):
                _same(a, b, f"{name} {h}x{w} T={T} tile={mt}")
        if h >= 8 and w >= 8:
            assert (want[2] >= 0).any() and (want[0] > 0).any(), "some template must be valid and score"


def test_every_bin_boundary_against_the_restatement():
    """all gradients with |g| <= 40, the largest ones (|g| <= 1020), and the exact boundaries 0, 45, 90 and 135 degrees"""
    g = np.arange(-40, 41)
    gx, gy = (a.ravel() for a in np.meshgrid(g, g))
    rng = np.random.RandomState(0)
    gx = np.concatenate([gx, rng.randint(-1020, 1021, 20000), [1020, -1020, 1020, 1019, 0, 7, -7, 7, -7, 0]])
    gy = np.concatenate([gy, rng.randint(-1020, 1021, 20000), [1020, 1020, -1020, 1020, 5, 0, 0, 7, 7, -5]])
    want = tmm.restate_bin(gx, gy)
    got = np.asarray([tmm.emul_bin(int(a), int(b)) for a, b in zip(gx, gy)])
    keep = (gx != 0) | (gy != 0)
    assert np.array_equal(got[keep], want[keep])
    # by hand: 0 degrees -> 0; 45 -> 2 (the bin [45, 67.5) owns its lower end); 90 -> 4; 135 -> 6; the opposite direction is the same angle
    for (x, y), b in (((7, 0), 0), ((-7, 0), 0), ((7, 7), 2), ((-7, -7), 2), ((0, 5), 4), ((0, -5), 4), ((-7, 7), 6), ((7, -7), 6), ((10, 4), 0), ((10, 5), 1),
                      ((5, 12), 2), ((5, 13), 3), ((-5, 13), 4), ((-5, 12), 5), ((-10, 5), 6), ((-10, 4), 7)):
        assert tmm.emul_bin(x, y) == b, (x, y, b)
    # and against the angle itself, away from the boundaries
    theta = np.degrees(np.arctan2(gy[keep].astype(np.float64), gx[keep].astype(np.float64))) % 180.0
    off = np.abs(theta / 22.5 - np.round(theta / 22.5)) > 1e-6
    assert np.array_equal(got[keep][off], np.floor(theta[off] / 22.5).astype(int))


# ---- 2. by hand --------------------------------------------------------------------------------------------------------------------------
def _grey(a):
    return np.repeat(np.asarray(a, np.uint8)[None, ..., None], 3, -1)


def test_a_vertical_step_edge_gives_bin_0_on_the_edge_columns():
    img = np.zeros((9, 12), np.uint8)
    img[:, 6:] = 200
    ori, mag2 = tmm.emul_quantize(_grey(img), blur=False, weak=30)
    want = np.zeros((9, 12), np.uint8)
    want[1:-1, 5:7] = 1          # columns 5 and 6 carry the gradient; in the first and last row only 2 x 2 = 4 candidates vote
    assert np.array_equal(ori[0], want)
    assert (mag2[0][:, 5:7] == (4 * 200) ** 2).all() and (np.delete(mag2[0], (5, 6), 1) == 0).all()
    blurred, _ = tmm.emul_quantize(_grey(img), blur=True, weak=30)
    assert set(np.unique(blurred).tolist()) == {0, 1} and (blurred[0][1:-1, 5:7] == 1).all() and not blurred[0][:, :3].any() and not blurred[0][:, 9:].any()


def test_a_diagonal_edge_lands_in_the_bin_that_owns_its_lower_end():
    ys, xs = np.mgrid[0:12, 0:12]
    down = np.where(xs + ys >= 11, 200, 0)          # gradient (+, +): 45 degrees -> bin 2 = [45, 67.5)
    up = np.where(xs - ys >= 0, 200, 0)             # gradient (+, -) = (-, +): 135 degrees -> bin 6 = [135, 157.5)
    for img, bit in ((down, 1 << 2), (up, 1 << 6)):
        ori, _ = tmm.emul_quantize(_grey(img), blur=False, weak=30)
        assert set(np.unique(ori).tolist()) == {0, bit}
        assert (ori[0][2:-2, 2:-2][(np.abs(np.gradient(img.astype(float))[0]) > 0)[2:-2, 2:-2]] == bit).all()


def test_a_flat_image_sets_no_bit_at_any_threshold():
    for weak in (0, 1, 30):
        ori, mag2 = tmm.emul_quantize(np.full((1, 7, 9, 3), 77, np.uint8), blur=False, weak=weak)
        assert not ori.any() and not mag2.any()


def _sobel(P):
    p = np.pad(np.asarray(P, np.int64), 1, mode="edge")
    gx = (p[:-2, 2:] + 2 * p[1:-1, 2:] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[1:-1, :-2] + p[2:, :-2])
    gy = (p[2:, :-2] + 2 * p[2:, 1:-1] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[:-2, 1:-1] + p[:-2, 2:])
    return gx, gy


def test_the_majority_needs_five():
    """two 3 x 3 images at weak_threshold 30 (900 squared).  Their squared magnitudes are
         five:  [[0, 1600, 1600], [50, 1700, 1250], [250, 1700, 650]]      four:  [[50, 1700, 1250], [250, 1700, 650], [400, 1600, 400]]
    so five resp. four pixels are candidates, each with |gy| <= |gx| / 4 and gx > 0: bin 0.  Only the centre sees all of them."""
    five, four = [[0, 0, 10], [0, 0, 10], [0, 5, 10]], [[0, 0, 10], [0, 5, 10], [0, 5, 10]]
    for img, count in ((five, 5), (four, 4)):
        gx, gy = _sobel(img)
        cand = gx * gx + gy * gy >= 900
        assert cand.sum() == count and (gx[cand] > 0).all() and (4 * np.abs(gy[cand]) <= gx[cand]).all()
        ori, _ = tmm.emul_quantize(_grey(img), blur=False, weak=30)
        centre_sees = cand.sum()
        want = np.zeros((3, 3), np.uint8)
        if count == 5:
            p = np.pad(cand.astype(int), 1)
            votes = sum(p[dy:dy + 3, dx:dx + 3] for dy in range(3) for dx in range(3))
            want[votes >= 5] = 1
            assert want[1, 1] == 1 and centre_sees == 5
        assert np.array_equal(ori[0], want), (count, ori[0])


def test_a_template_cut_from_an_image_scores_4f_at_home():
    images = tmm.image_case(1, 48, 64, 5)
    ori, _ = tmm.emul_quantize(images)
    x0, y0, width, height = 19, 13, 30, 24
    feats = tmm.cut_template(ori[0], x0, y0, width, height)
    f = len(feats)
    assert f == 63, "the region must hold at least 63 orientation pixels"
    table = np.asarray([[0, 0, f, width, height]], np.int32)
    score, fb, best = tmm.emul_match(tmm.emul_response(ori, 1), 48, 64, 1, table, feats, 1)
    assert score[0, 0, y0, x0] == 4 * f == 252 and fb[0, 0, y0, x0] == f and best[0, 0, y0, x0] == 0
    assert (score[0, 0] == 252).sum() == 1, "nowhere else at T = 1"
    score, fb, best = tmm.emul_match(tmm.emul_response(ori, 8), 48, 64, 8, table, feats, 1)
    assert score[0, 0, y0 // 8, x0 // 8] == 252, "the location within [0, 8) above and left of it"
    assert best[0, 0, y0 // 8, x0 // 8] == 0 and (best[0, 0, (48 - height) // 8 + 1:] == -1).all() and (best[0, 0, :, (64 - width) // 8 + 1:] == -1).all()


# ---- 3. the order ------------------------------------------------------------------------------------------------------------------------
def test_equal_ratios_go_to_the_lower_index_and_close_ratios_are_ordered_exactly():
    # 251 / 252 against 247 / 248 (0.99603 against 0.99597), and the closest pair there is: 1 / (4 * 63 * 4 * 62) apart
    assert tmm.emul_better((251, 63, 9), (247, 62, 0)) and not tmm.emul_better((247, 62, 0), (251, 63, 9))
    assert tmm.emul_better((249, 63, 9), (245, 62, 0)) and not tmm.emul_better((245, 62, 0), (249, 63, 9))
    assert tmm.emul_better((4, 1, 0), (8, 2, 1)) and not tmm.emul_better((8, 2, 1), (4, 1, 0)), "equal ratios: the lower index"
    assert tmm.emul_better((0, 5, 3), (0, 0, -1)) and not tmm.emul_better((0, 0, -1), (0, 5, 3)), "a valid template with score 0 beats none"
    rng = np.random.RandomState(1)
    for _ in range(20000):
        fa, fb = rng.randint(1, 64, 2)
        a, b = (int(rng.randint(0, 4 * fa + 1)), int(fa), int(rng.randint(0, 100))), (int(rng.randint(0, 4 * fb + 1)), int(fb), int(rng.randint(100, 200)))
        ra, rb = Fraction(a[0], 4 * a[1]), Fraction(b[0], 4 * b[1])
        assert tmm.emul_better(a, b) == (ra >= rb) and tmm.emul_better(b, a) == (rb > ra), (a, b)
    # through the match: at (3, 3) bit 0 is set; a template of two features on it (8 / 8) and one of one feature (4 / 4)
    ori = np.zeros((1, 8, 8), np.uint8)
    ori[0, 3, 3] = 1
    resp = tmm.emul_response(ori, 1)
    feats = np.asarray([[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 1, 0], [0, 0, 1, 0]], np.uint8)
    for table, want in (([[0, 0, 2, 1, 1], [0, 2, 1, 1, 1]], 0), ([[0, 2, 1, 1, 1], [0, 0, 2, 1, 1]], 0), ([[0, 3, 2, 1, 1], [0, 2, 1, 1, 1]], 1)):
        score, fb, best = tmm.emul_match(resp, 8, 8, 1, np.asarray(table, np.int32), feats, 1)
        assert best[0, 0, 3, 3] == want and score[0, 0, 3, 3] * table[want][2] == 4 * table[want][2] * fb[0, 0, 3, 3]
        _same(best, tmm.restate_match(ori, 1, table, feats, 1)[2], "the order through the restatement")


# ---- 4. the limits -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(tmm.limit_cases())))
def test_limits_against_the_restatement(case):
    name, images, T, templates, features, n_objects = tmm.limit_cases()[case]
    h, w = images.shape[1:3]
    ori, mag2, resp, score, fb, best = _chain(images, T, templates, features, n_objects)
    want_ori, want_mag2 = tmm.restate_quantize(images)
    _same(ori, want_ori, name)
    _same(mag2, want_mag2, name)
    _same(resp, tmm.restate_response(want_ori, T), name)
    for a, b in zip((score, fb, best), tmm.restate_match(want_ori, T, templates, features, n_objects)):
        _same(a, b, name)
    if len(images) == 3:
        assert not ori[2].any() and not resp[2].any() and not score[2].any(), "the black image"
    if "exactly" in name:
        assert (best[0, 0] >= 0).sum() == 1 and best[0, 0, 0, 0] == 0, "a template of the image's size has one valid location"
        assert (best[0, 1] == -1).all() and not score[0, 1].any() and not fb[0, 1].any(), "one pixel larger: none"
    if len(templates) >= 65:
        assert set(np.unique(templates[:, 2])) >= {1, 63} and (best[:, tmm.N_OBJECTS - 1] == -1).all(), "f = 1 and 63; an object without templates"


def test_rejected_tables_and_arguments():
    images = tmm.image_case(1, 13, 17, 4)
    ori, _ = tmm.emul_quantize(images)
    resp = tmm.emul_response(ori, 2)
    feats = np.zeros((70, 4), np.uint8)
    feats[:, :2] = 3

    def rc(table, features=feats, n_objects=2, T=2, r=resp):
        return tmm.emul_match(r, 13, 17, T, np.asarray(table, np.int32), features, n_objects, rc_only=True)

    assert rc([[0, 0, 1, 4, 4]]) == 0 and rc([[1, 7, 63, 4, 4]]) == 0
    assert rc([[0, 0, 0, 4, 4]]) != 0 and rc([[0, 0, 64, 4, 4]]) != 0, "f = 0 and f = 64"
    assert rc([[0, 0, 1, 3, 4]]) != 0 and rc([[0, 0, 1, 4, 3]]) != 0, "a feature at (3, 3) outside a box of width or height 3"
    assert rc([[0, 0, 1, 4, 4], [0, 69, 2, 4, 4]]) != 0 and rc([[0, -1, 1, 4, 4]]) != 0, "features outside the table"
    assert rc([[2, 0, 1, 4, 4]]) != 0 and rc([[-1, 0, 1, 4, 4]]) != 0, "an object outside 0 .. n_objects - 1"
    assert rc([[0, 0, 1, 257, 4]]) != 0 and rc([[0, 0, 1, 4, 0]]) != 0, "a box side outside 1 .. 256"
    bad = feats.copy()
    bad[5, 2] = 8
    assert rc([[0, 5, 1, 4, 4]], features=bad) != 0, "an orientation index above 7"
    assert rc([[0, 0, 1, 4, 4]], n_objects=0) != 0
    assert tmm.emul_response(ori, 0, rc_only=True) != 0 and tmm.emul_response(ori, 9, rc_only=True) != 0
    assert tmm.emul_quantize(images, weak=-1, rc_only=True) != 0 and tmm.emul_quantize(images, weak=1444, rc_only=True) != 0
    # n = 0 is a no-op at every stage
    none = images[:0]
    assert tmm.emul_quantize(none, rc_only=True) == 0 and tmm.emul_response(ori[:0], 2, rc_only=True) == 0
    assert tmm.emul_match(resp[:0], 13, 17, 2, [[0, 0, 0, 4, 4]], feats, 2, rc_only=True) == 0


# ---- 5. select_features ------------------------------------------------------------------------------------------------------------------
def _dilate(mask):
    h, w = mask.shape
    p = np.pad(mask, 1)
    return np.any([p[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)], axis=0)


def test_select_features():
    from megapose6d_amd.template_detector import select_features

    images = tmm.image_case(1, 48, 64, 5)
    ori, mag2 = tmm.emul_quantize(images)
    mask = np.zeros((48, 64), bool)
    mask[6:40, 10:58] = True
    feats, (x0, y0, width, height), distance = select_features(ori[0], mag2[0], mask, 40, strong_threshold=55)
    again = select_features(ori[0].copy(), mag2[0].copy(), mask.copy(), 40, strong_threshold=55)
    assert np.array_equal(feats, again[0]) and again[1:] == ((x0, y0, width, height), distance), "deterministic"
    assert feats.dtype == np.uint8 and feats.shape == (40, 4) and not feats[:, 3].any()
    xs, ys = feats[:, 0].astype(int) + x0, feats[:, 1].astype(int) + y0
    # every feature is a candidate: a bit set, strong, inside the mask dilated by one pixel; its index is that bit
    assert (ori[0][ys, xs] == 1 << feats[:, 2].astype(int)).all() and (mag2[0][ys, xs] >= 55 * 55).all()
    assert ((xs >= 9) & (xs <= 58) & (ys >= 5) & (ys <= 40)).all()
    # the minimum mutual distance that held
    d2 = (xs[:, None] - xs[None]) ** 2 + (ys[:, None] - ys[None]) ** 2
    assert distance > 1 and d2[~np.eye(40, dtype=bool)].min() >= distance ** 2
    # the first pick is the strongest candidate, the earliest in (y, x) among equals
    cand = _dilate(mask) & (ori[0] != 0) & (mag2[0] >= 55 * 55)
    cy, cx = np.nonzero(cand & (mag2[0] == mag2[0][cand].max()))
    assert (ys[0], xs[0]) == (cy[0], cx[0])
    # the crop box is the features' bounding box
    assert (x0, y0) == (xs.min(), ys.min()) and (width, height) == (xs.max() - x0 + 1, ys.max() - y0 + 1)
    assert feats[:, 0].min() == 0 and feats[:, 1].min() == 0 and feats[:, 0].max() == width - 1 and feats[:, 1].max() == height - 1
    # fewer candidates than asked: all are returned, at distance 1
    small = np.zeros((48, 64), bool)
    small[20:26, 20:30] = True
    n_cand = int((_dilate(small) & (ori[0] != 0) & (mag2[0] >= 55 * 55)).sum())
    few, box, d = select_features(ori[0], mag2[0], small, 63, strong_threshold=55)
    assert 0 < n_cand < 63 and len(few) == n_cand and d == 1
    none, box, d = select_features(np.zeros((5, 5), np.uint8), np.zeros((5, 5), np.int32), np.ones((5, 5), bool))
    assert none.shape == (0, 4) and box == (0, 0, 0, 0)
    with pytest.raises(ValueError):
        select_features(ori[0], mag2[0], mask, 64)


# ---- 6. end to end on the CPU ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_detector(tmp_path_factory):
    """templates of two synthetic objects from renders of the oracle's rasteriser (72 rotations x 2 distances at 120 x 160), quantised by
    the emulation; the model's torch part then runs on CPU tensors"""
    from megapose6d_amd.pose_estimator import load_SO3_grid
    from megapose6d_amd.template_detector import TemplateMatchingModel, TemplateSet
    from oracle import mesh_loader, raster
    from tests.support import synthetic as syn

    ds = syn.make_object_dataset(tmp_path_factory.mktemp("tm_meshes"), n_objects=2, seed=0)
    meshes = [mesh_loader.load_object(o) for o in ds.list_objects]
    h, w = tmm.DET_HW
    R = load_SO3_grid(tmm.DET_GRID).numpy()
    flags = raster.FLAG_DEPTH | raster.FLAG_MSAA4

    def render(o, T):
        rgb, _, dep = raster.render(meshes[o], T, np.repeat(tmm.DET_K[None], len(T), 0), h, w, flags)
        return np.round(np.clip(rgb, 0, 1) * 255).astype(np.uint8), dep > 0

    renders, masks, obj, view, dist = [], [], [], [], []
    for o in range(2):
        for d in tmm.DET_DISTANCES:
            T = np.repeat(np.eye(4, dtype=np.float32)[None], len(R), 0)
            T[:, :3, :3], T[:, 2, 3] = R, d
            r, m = render(o, T)
            renders.append(r), masks.append(m)
            obj += [o] * len(R)
            view += list(range(len(R)))
            dist += [d] * len(R)
    ts = TemplateSet.from_renders([o.label for o in ds.list_objects], np.concatenate(renders), np.concatenate(masks), obj, view, dist,
                                  quantize=lambda r: tmm.emul_quantize(r, True, 30), device="cpu")
    return TemplateMatchingModel(ts), render, R


def _detect_on_cpu(model, image):
    ts = model.templates
    h, w = image.shape[:2]
    ori, _ = tmm.emul_quantize(image[None], ts.blur, ts.weak_threshold)
    score, fb, best = tmm.emul_match(tmm.emul_response(ori, model.T), h, w, model.T, ts.templates, ts.features, ts.n_objects)
    sim = score.astype(np.float64) / np.maximum(4 * fb.astype(np.float64), 1)
    out = model.detections_from_match(torch.from_numpy(score), torch.from_numpy(fb), torch.from_numpy(best), (h, w))[0]
    return out, sim.max()


def test_planted_objects_are_found_and_the_background_gives_nothing(oracle_detector):
    """CONDITIONS at the default threshold: every planted object has a detection of its label with box IoU >= 0.5 against the box of its
    pasted silhouette; the background alone gives no detection.  Recorded on the emulation: similarity of the matching
    detections 0.798 .. 0.833, highest background similarity 0.603; LINE-MOD's customary 0.8 is above one planted object, so the default
    threshold is the midpoint, 0.70."""
    from megapose6d_amd.template_detector import DEFAULT_THRESHOLD

    model, render, R = oracle_detector
    ts = model.templates
    assert model.threshold == DEFAULT_THRESHOLD and len(ts) + ts.n_dropped == 2 * 72 * 2 and len(ts) >= 250
    assert (ts.templates[:, 2] >= 8).all() and (ts.templates[:, 2] <= 63).all() and (ts.templates[:, 2] == 63).any()
    planted, clutter = [], []
    for seed, plant in tmm.DET_SCENES:
        poses = tmm.det_query_poses(R, seed, plant)
        renders, masks = {}, {}
        for o, T in poses.items():
            r, m = render(o, T[None])
            renders[o], masks[o] = r[0], m[0]
        image, boxes = tmm.det_compose(seed, plant, renders, masks)
        assert all(dx % 8 and dy % 8 for _, (dx, dy) in plant.values()), "the paste is not aligned with the location grid"
        out, _ = _detect_on_cpu(model, image)
        assert out["masks"].shape == (len(out["boxes"]), 1, *tmm.DET_HW) and out["labels"].dtype == torch.int64
        for o, box in boxes.items():
            hits = [(tmm.box_iou(box, b.tolist()), float(s)) for b, l, s in zip(out["boxes"], out["labels"], out["scores"]) if int(l) == o + 1]
            print(f"scene {seed} object {o}: box {box}, detections of its label (iou, similarity) {[(round(i, 3), round(s, 4)) for i, s in hits]}")
            good = [s for i, s in hits if i >= 0.5]
            assert good, f"scene {seed}: object {o} has no detection with IoU >= 0.5 (its label's detections: {hits})"
            planted.append(max(good))
        nothing, top = _detect_on_cpu(model, np.array(tmm.det_background(seed)))
        print(f"scene {seed} background: highest similarity {top:.4f}, {len(nothing['boxes'])} detections")
        assert len(nothing["boxes"]) == 0 and nothing["masks"].shape == (0, 1, *tmm.DET_HW), f"scene {seed}: the background alone gives detections"
        clutter.append(top)
    print(f"planted similarities {sorted(round(s, 4) for s in planted)}, highest background similarity {max(clutter):.4f}")
    assert max(clutter) < DEFAULT_THRESHOLD <= min(planted)


def test_suppression_and_masks_of_the_torch_part(oracle_detector):
    """two overlapping maxima of one label: the weaker goes; across labels only when asked; the mask is the silhouette at the box"""
    from megapose6d_amd.template_detector import TemplateMatchingModel

    model, _, _ = oracle_detector
    ts = model.templates
    area = (ts.boxes[:, 2] - ts.boxes[:, 0] + 1) * (ts.boxes[:, 3] - ts.boxes[:, 1] + 1)
    t0 = int(np.argmax(np.where(ts.templates[:, 0] == 0, area, 0)))          # the largest silhouettes: shifted by two cells they still overlap
    t1 = int(np.argmax(np.where(ts.templates[:, 0] == 1, area, 0)))
    shifted = ts.boxes[t0] + [16, 0, 16, 0]
    assert tmm.box_iou(ts.boxes[t0].tolist(), shifted.tolist()) > 0.3
    model = TemplateMatchingModel(ts, nms_iou=0.3)
    gh, gw = 15, 20
    score, fb = torch.zeros((1, 2, gh, gw), dtype=torch.uint8), torch.zeros((1, 2, gh, gw), dtype=torch.uint8)
    best = torch.full((1, 2, gh, gw), -1, dtype=torch.int32)
    for o, t, (y, x), s in ((0, t0, (4, 5), 240), (0, t0, (4, 7), 230), (1, t1, (4, 6), 235), (0, t0, (9, 14), 100)):
        score[0, o, y, x], fb[0, o, y, x], best[0, o, y, x] = s, 63, t
    out = model.detections_from_match(score, fb, best, tmm.DET_HW)[0]
    assert out["labels"].tolist() == [1, 2] and np.allclose(out["scores"].numpy(), [240 / 252, 235 / 252]), "per label; 100 / 252 is under the threshold"
    x1, y1, x2, y2 = (int(v) for v in out["boxes"][0].tolist())
    assert (x1, y1, x2, y2) == tuple((ts.boxes[t0] + [40, 32, 40, 32]).tolist())
    m = out["masks"][0, 0].numpy() > 0
    ys, xs = np.nonzero(m)
    assert (xs.min(), ys.min(), xs.max(), ys.max()) == (max(x1, 0), max(y1, 0), x2, y2) and np.array_equal(m[max(y1, 0):y2 + 1, max(x1, 0):x2 + 1], ts.masks[t0][max(-y1, 0):, max(-x1, 0):])
    across = TemplateMatchingModel(ts, nms_iou=0.3, nms_across_labels=True).detections_from_match(score, fb, best, tmm.DET_HW)[0]
    assert across["labels"].tolist() == [1]
    assert model.config.label_to_category_id == {"obj_000000": 1, "obj_000001": 2}


# ---- 7. under the sanitizers -------------------------------------------------------------------------------------------------------------
def test_emulation_under_the_sanitizers(tmp_path):
    """the emulation as a stand-alone program (tests/template_match_asan_main.cpp) under the address and undefined-behaviour sanitizers:
    tiles with halos and strided maps are where off-by-ones live.  Host code only; the program compares every case with what the plain
    build returned."""
    cases = []
    for (h, w), T, blur, tiles in (((1, 1), 8, True, (None, None, None)), ((1, 7), 2, True, ((1, 1), (1, 1), (1, 1))), ((7, 1), 5, False, ((5, 3), (5, 3), (5, 3))),
                                   ((3, 3), 1, True, ((4, 2), (12, 2), (4, 1))), ((8, 8), 8, True, (None, None, None)), ((13, 17), 5, True, ((5, 3), (5, 3), (5, 3))),
                                   ((13, 17), 2, False, (None, None, None)), ((48, 64), 8, True, (None, None, None)), ((48, 64), 5, True, ((65, 2), (73, 2), (65, 1)))):
        images = tmm.image_case(2, h, w, 1)
        templates, features = tmm.table_case(h, w, 65, 1)
        cases.append((images, T, blur, tiles, templates, features, tmm.N_OBJECTS))
    for name, images, T, templates, features, n_objects in tmm.limit_cases():
        cases.append((images, T, True, (None, None, None), templates, features, n_objects))
    lim = tmm.limits()
    with open(tmp_path / "cases.bin", "wb") as f:
        for images, T, blur, tiles, templates, features, n_objects in cases:
            n, h, w = images.shape[:3]
            qt, rt, mt = tiles[0] or (lim["quant_tile_w"], lim["quant_tile_h"]), tiles[1] or tmm.resp_tile(T), tiles[2] or (lim["loc_w"], lim["loc_h"])
            got = _chain(images, T, templates, features, n_objects, blur=blur, tiles=tiles)
            f.write(np.asarray([n, h, w, int(blur), tmm.WEAK, T, *qt, *rt, *mt, len(templates), len(features), n_objects], np.int32).tobytes())
            f.write(images.tobytes() + np.ascontiguousarray(templates, np.int32).tobytes() + np.ascontiguousarray(features, np.uint8).tobytes())
            f.write(b"".join(a.tobytes() for a in got))
    exe = tmp_path / "template_match_asan"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", str(tmm.CSRC), "-I",
                    str(tmm.TESTS), "-o", str(exe), str(tmm.TESTS / "template_match_asan_main.cpp")], check=True)
    run = subprocess.run([str(exe), str(tmp_path / "cases.bin")], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and run.stdout.strip() == f"{len(cases)} cases, 0 bad", (run.stdout, run.stderr[-2000:])

"""GPU: the ground-truth-info kernels (csrc/gt_info.hip) through the C ABI against the host emulation built from the same arithmetic
headers (tests/gt_info_emul.cpp): counts, boxes, visib_fract and both masks bit for bit, for every forced split, on the vector and the
scalar path.  Then `evaluation.gt_info` end to end on the synthetic objects, the emulation fed the ORACLE rasteriser's depths of the same
nine tile intrinsics, and the tile seams: nine engine tiles stitched against one oracle render of the whole canvas.  Bad arguments are
refused before any launch.  Reads nothing outside the tree."""
import numpy as np
import pandas as pd
import pytest
import torch

from support import gt_info as gi
from support import pose_error as pes

pytestmark = pytest.mark.gpu


def _dev(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _gpu(c, split=0, delta=0.015):
    from megapose6d_amd import engine as eng

    out = eng.gt_info(_dev(c["gt"]), _dev(c["test"]), _dev(c["K"]), canvas=c["canvas"], delta=delta, gt_ids=_dev(c.get("gt_ids")),
                      im_ids=_dev(c.get("im_ids")), with_masks=True, split=split)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _emul(c, delta=0.015):
    return gi.gt_info(c["gt"], c["test"], c["K"], c["canvas"], delta=delta, gt_ids=c.get("gt_ids"), im_ids=c.get("im_ids"))


def _same(got, ref, what=""):
    for k in ("counts", "boxes", "mask", "mask_visib"):
        assert np.array_equal(got[k], ref[k]), (k, what)
    assert np.array_equal(got["visib_fract"].view(np.uint32), ref["visib_fract"].view(np.uint32)), what


def _check(c, splits=(0,), **kw):
    ref = _emul(c, **kw)
    for split in splits:
        _same(_gpu(c, split=split, **kw), ref, split)
    return ref


# (b, h, w, canvas, shared ids, forced splits)
SHAPES = [(1, 1, 1, 1, False, ()), (3, 5, 7, 3, False, ()), (2, 4, 260, 3, False, ()), (4, 33, 64, 1, False, (1, 2, 7)), (2, 64, 1024, 3, False, ()),
          (1, 1024, 8, 1, False, ()), (5, 48, 64, 3, True, (1, 2, 7)), (2, 480, 640, 3, False, ())]


@pytest.mark.parametrize("b,h,w,canvas,share,splits", SHAPES)
def test_gt_info_kernel_matches_the_emulation_bit_for_bit(b, h, w, canvas, share, splits):
    c = gi.case(2000 + b + h + w, b, h, w, canvas, n_gt=2 if share else None, n_im=2 if share else None, share=share)
    ref = _check(c, splits=(0,) + splits)
    if h * w >= 48 * 64:
        assert ref["counts"][:, 3].min() >= 1000 and np.all(ref["counts"][:, 3] < ref["counts"][:, 1])
        assert canvas == 1 or (np.all(ref["counts"][:, 0] > ref["counts"][:, 1]) and np.all(ref["boxes"][:, 0] < 0))
    print(f"gt_info ({b},{h}x{w},{canvas}): px_count_visib {ref['counts'][:, 3].min()} .. {ref['counts'][:, 3].max()}")


def test_gt_info_empty_centre_seam_and_invalid_rows():
    ref = _check(gi.case(41, 2, 48, 64, 3, variant="empty_centre"), splits=(0, 3))
    assert np.all(ref["counts"][:, 0] > 0) and np.all(ref["counts"][:, 1:] == 0) and np.all(ref["boxes"][:, 4:] == -1)
    ref = _check(gi.case(42, 2, 48, 64, 3, variant="seam"), splits=(0, 3))
    assert np.all(ref["boxes"][:, 0] <= -3)
    c = gi.case(43, 4, 37, 53, 3)
    c["K"][1, 0, 0] = np.nan
    c["K"][2, 2, 1] = np.inf
    c["test"][0, 5:9, :] = [[np.nan], [-1.0], [np.inf], [0.0]]
    ref = _check(c, splits=(0, 2))
    assert np.all(ref["counts"][1:3] == -1) and np.all(np.isnan(ref["visib_fract"][1:3])) and not ref["mask"][1:3].any() and ref["counts"][0, 3] > 0
    c = gi.case(44, 2, 40, 64, 1)                             # the vector path's invalid row
    c["K"][0, 1, 1] = -np.inf
    _check(c)
    # exact hit on delta: r = 1 on the optical axis of a 1 x 1 map
    K1 = gi.vs.intrinsics(50.0, 0.5, 0.5)[None]
    one = lambda z: np.full((1, 1, 1), z, np.float32)          # noqa: E731
    for test, want in ((np.float32(0.75), [1, 1, 1, 1]), (np.float32(0.75) - np.float32(2.0 ** -24), [1, 1, 1, 0])):
        ref = _check(dict(gt=one(1.0)[None], test=one(test), K=K1, canvas=1), delta=0.25)
        assert list(ref["counts"][0]) == want


def _raw(lib, gt, test, K, b, h, w, canvas, mask=None, mask_visib=None, split=0):
    """the C ABI on resident tensors -> counts, boxes, fract"""
    counts, boxes = torch.empty(b, 4, dtype=torch.int32, device="cuda"), torch.empty(b, 8, dtype=torch.int32, device="cuda")
    fract = torch.empty(b, device="cuda")
    ws = torch.empty(int(lib.mp_gt_info_workspace_bytes(b)), dtype=torch.uint8, device="cuda")
    rc = lib.mp_gt_info(gt.data_ptr(), None, test.data_ptr(), None, b, b, K.data_ptr(), b, h, w, canvas, 0.015, split, counts.data_ptr(), boxes.data_ptr(),
                        fract.data_ptr(), None if mask is None else mask.data_ptr(), None if mask_visib is None else mask_visib.data_ptr(),
                        ws.data_ptr(), ws.numel(), None)
    assert rc == 0
    torch.cuda.synchronize()
    return dict(counts=counts.cpu().numpy(), boxes=boxes.cpu().numpy(), visib_fract=fract.cpu().numpy())


def test_gt_info_on_unaligned_bases_and_with_one_mask_at_a_time():
    """w % 4 == 0 but the maps start 4 bytes off a 16-byte boundary, or a mask one byte off a 4-byte one: the scalar path, the same
    results; each mask pointer may be NULL on its own"""
    from megapose6d_amd import _lib

    lib = _lib.load()
    b, h, w = 3, 40, 64
    c = gi.case(5, b, h, w, 3)
    ref = _emul(c)
    K = _dev(c["K"])
    pad = lambda a: torch.cat([torch.zeros(1), torch.from_numpy(a).flatten()]).cuda()[1:].view(a.shape)   # noqa: E731
    bytes_ = lambda off: torch.full((b * h * w + 4,), 7, dtype=torch.uint8, device="cuda")[off:off + b * h * w].view(b, h, w)   # noqa: E731
    for gt, test, off in ((pad(c["gt"]), pad(c["test"]), 0), (_dev(c["gt"]), _dev(c["test"]), 1), (_dev(c["gt"]), pad(c["test"]), 0)):
        assert (gt.data_ptr() % 16 == 4 or test.data_ptr() % 16 == 4 or off) and gt.is_contiguous() and test.is_contiguous()
        m, mv = bytes_(off), bytes_(off)
        assert m.data_ptr() % 4 == off
        got = _raw(lib, gt, test, K, b, h, w, 3, m, mv)
        _same(dict(got, mask=m.cpu().numpy(), mask_visib=mv.cpu().numpy()), ref, off)
    gt, test = _dev(c["gt"]), _dev(c["test"])
    for which in (0, 1, None):
        m, mv = (bytes_(0) if which != 1 else None), (bytes_(0) if which != 0 else None)
        got = _raw(lib, gt, test, K, b, h, w, 3, None if which is None else m, None if which is None else mv)
        for k in ("counts", "boxes"):
            assert np.array_equal(got[k], ref[k])
        if which == 0:
            assert np.array_equal(m.cpu().numpy(), ref["mask"])
        if which == 1:
            assert np.array_equal(mv.cpu().numpy(), ref["mask_visib"])


def test_gt_info_bad_arguments_are_refused_before_any_launch():
    from megapose6d_amd import _lib
    from megapose6d_amd import engine as eng

    z = lambda *s: torch.zeros(*s, device="cuda")             # noqa: E731
    K = torch.eye(3, device="cuda").repeat(2, 1, 1)
    with pytest.raises(eng.EngineError):
        eng.gt_info(z(2, 4, 4, 4), z(2, 4, 4), K, canvas=2)
    with pytest.raises(eng.EngineError):
        eng.gt_info(z(2, 9, 4, 1025), z(2, 4, 1025), K)
    with pytest.raises(eng.EngineError):
        eng.gt_info(z(2, 1, 4, 4), z(2, 4, 4), K)                            # canvas 3 needs nine tiles
    with pytest.raises(eng.EngineError):
        eng.gt_info(z(1, 9, 4, 4), z(2, 4, 4), K)                            # one canvas, two rows, no ids
    with pytest.raises(eng.EngineError):
        eng.gt_info(z(2, 9, 4, 4), z(2, 4, 5), K)
    with pytest.raises(eng.EngineError):
        eng.gt_info(z(2, 9, 4, 4), z(2, 4, 4), K[:1].reshape(3, 3))
    with pytest.raises(eng.EngineError):
        eng.gt_info(z(2, 9, 4, 4), z(2, 4, 4), K, split=-1)
    out = eng.gt_info(z(2, 4, 4), z(2, 4, 4), K, canvas=1)                    # [n,h,w] is canvas 1
    assert out["counts"].tolist() == [[0] * 4] * 2 and out["boxes"].tolist() == [[-1] * 8] * 2
    # the C ABI itself
    lib = _lib.load()
    maps, frames, ws = z(2, 9, 4, 4), z(2, 4, 4), torch.zeros(4096, dtype=torch.uint8, device="cuda")
    counts, boxes = torch.zeros(2, 4, dtype=torch.int32, device="cuda"), torch.zeros(2, 8, dtype=torch.int32, device="cuda")
    fract = z(2)
    need = int(lib.mp_gt_info_workspace_bytes(2))

    def call(gt=maps.data_ptr(), b=2, h=4, w=4, canvas=3, kp=K.data_ptr(), cp=counts.data_ptr(), wp=ws.data_ptr(), ws_bytes=4096, split=0, n_gt=2):
        return lib.mp_gt_info(gt, None, frames.data_ptr(), None, n_gt, 2, kp, b, h, w, canvas, 0.015, split, cp, boxes.data_ptr(), fract.data_ptr(), None, None,
                              wp, ws_bytes, None)

    assert call() == 0 and call(ws_bytes=need) == 0
    assert call(b=0) == 0 and call(b=0, gt=None, kp=None, cp=None, wp=None, ws_bytes=0) == 0       # b == 0: a successful no-op
    for bad in (dict(canvas=2), dict(canvas=0), dict(h=0), dict(w=0), dict(h=1025), dict(w=1025), dict(kp=None), dict(cp=None), dict(wp=None), dict(gt=None),
                dict(ws_bytes=need - 1), dict(b=-1), dict(b=3), dict(split=-1), dict(n_gt=0)):
        assert call(**bad) != 0, bad
    assert lib.mp_gt_info_workspace_bytes(-1) == 0 and need >= 2 * 12 * 4
    torch.cuda.synchronize()


# --------------------------------------------------------------------------------------------------------------------------------
# end to end
# --------------------------------------------------------------------------------------------------------------------------------
def _tile_K(K, canvas, H, W):
    """[3,3] float32 -> [canvas^2,3,3]: cx - (tx - c) W, cy - (ty - c) H, one fp32 subtraction each"""
    c = (canvas - 1) // 2
    out = np.repeat(np.asarray(K, np.float32)[None], canvas * canvas, axis=0)
    for t in range(canvas * canvas):
        out[t, 0, 2] = np.float32(K[0, 2]) - np.float32((t % canvas - c) * W)
        out[t, 1, 2] = np.float32(K[1, 2]) - np.float32((t // canvas - c) * H)
    return out


def e2e_scene(oracle_meshes, H=240, W=320):
    """the oracle's side of the end-to-end test, no device needed: poses, the ORACLE rasteriser's renders of the nine tile intrinsics,
    observed frames.  Rows: 0 inside frame 0 under an occluder, 1 half out of the left edge of frame 1, 2 / 3 one pose inside frames 2 / 3
    (2 = the render itself, 3 = the same with a nearer plane over the object's left half), 4 a NaN pose."""
    from oracle import raster as orr
    from tests.support import synthetic as syn

    rng = np.random.RandomState(4)
    K0 = (np.diag([0.5, 0.5, 1.0]) @ syn.K_EXAMPLE).astype(np.float32)
    K_im = np.stack([K0, K0 + np.array([[4.0, 0, 3.0], [0, -3.0, 2.0], [0, 0, 0]], np.float32), K0, K0]).astype(np.float32)
    obj, im = [0, 1, 2, 2, 0], [0, 1, 2, 3, 0]
    x_edge = -float(K_im[1, 0, 2]) / float(K_im[1, 0, 0]) * 0.5      # the camera-frame x that projects onto image column 0 at z = 0.5
    T = np.stack([pes.pose(pes.random_rotation(rng), t) for t in ([-0.03, 0.0, 0.5], [x_edge, 0.01, 0.5], [0.0, 0.0, 0.45], [0.0, 0.0, 0.45], [0, 0, 0.5])])
    T = T.astype(np.float32)
    T[3] = T[2]
    T[4, 1, 2] = np.nan
    tiles = np.zeros((5, 9, H, W), np.float32)
    for i in range(4):
        Kt = _tile_K(K_im[im[i]], 3, H, W)
        tiles[i] = orr.render(oracle_meshes[obj[i]], np.repeat(T[i][None], 9, axis=0), Kt, H, W, orr.FLAG_DEPTH)[2]   # one sample per pixel
    frames = np.zeros((4, H, W), np.float32)
    for i in (0, 1):
        frames[i] = np.where(tiles[i, 4] > 0, tiles[i, 4] + (rng.randn(H, W) * 0.002).astype(np.float32), np.float32(1.5))
    ys, _ = np.nonzero(tiles[0, 4] > 0)
    frames[0, ys.min():(ys.min() + ys.max()) // 2, :] -= 0.1         # a nearer occluder over the upper half of object 0
    frames[1, H // 2:H // 2 + 20, :] = 0.0                            # a band without observed depth
    frames[2] = tiles[2, 4]                                          # the render itself (zeros around it: unobserved)
    frames[3] = tiles[2, 4]
    x_mid = int(np.nonzero(tiles[2, 4].any(0))[0].mean())
    frames[3, :, :x_mid] = 0.2                                       # a plane 0.25 m nearer over the object's left half
    return dict(T=T, K_im=K_im, obj=obj, im=im, tiles=tiles, frames=frames, x_mid=x_mid, ok=np.array([True] * 4 + [False]))


def test_gt_info_end_to_end_against_the_emulation_on_oracle_renders(object_dataset, engine_meshes, oracle_meshes):
    from megapose6d_amd import evaluation as ev
    from megapose6d_amd.renderer import Panda3dBatchRenderer
    from megapose6d_amd.tcoll import PandasTensorCollection

    H, W = 240, 320
    labels = [o.label for o in object_dataset.list_objects]
    assert len(labels) == 3 and len(oracle_meshes) == 3 and len(engine_meshes) == 3
    s = e2e_scene(oracle_meshes, H, W)
    obj, im, ok, tiles, frames, K_im = s["obj"], s["im"], s["ok"], s["tiles"], s["frames"], s["K_im"]
    assert all((tiles[i, 4] > 0).sum() > 800 for i in range(4))
    gt = PandasTensorCollection(pd.DataFrame(dict(label=[labels[o] for o in obj], batch_im_id=im)), poses=torch.from_numpy(s["T"]).cuda())
    renderer = Panda3dBatchRenderer(object_dataset, n_workers=1)
    depth, K = torch.from_numpy(frames).cuda(), torch.from_numpy(K_im).cuda()
    df, mask, mask_visib = ev.gt_info(gt, renderer, depth, K, return_masks=True)
    assert df.index.equals(gt.infos.index) and mask.is_cuda and mask.dtype == torch.uint8 and tuple(mask.shape) == (5, H, W)
    # the emulation on the oracle's renders of the same nine tile intrinsics: exactly
    ref = gi.gt_info(tiles, frames, K_im[im], 3, im_ids=im)
    got_counts = df[list(gi.COUNT_NAMES)].to_numpy()
    assert np.array_equal(got_counts[ok], ref["counts"][ok]) and np.all(got_counts[4] == -1) and np.isnan(df["visib_fract"].iloc[4])
    assert np.array_equal(df["visib_fract"].to_numpy()[ok].astype(np.float32).view(np.uint32), ref["visib_fract"][ok].view(np.uint32))
    for i in range(4):
        a = [int(v) for v in ref["boxes"][i]]
        assert df["bbox_amodal"].iloc[i] == a[:4] and df["bbox_modal"].iloc[i] == a[4:], i
        assert df["bbox_obj"].iloc[i] == [a[0], a[1], a[2] - a[0], a[3] - a[1]] and df["bbox_visib"].iloc[i] == [a[4], a[5], a[6] - a[4], a[7] - a[5]]
    assert df["bbox_obj"].iloc[4] == [-1] * 4 and df["bbox_modal"].iloc[4] == [-1] * 4
    assert np.array_equal(mask.cpu().numpy()[ok], ref["mask"][ok]) and np.array_equal(mask_visib.cpu().numpy()[ok], ref["mask_visib"][ok])
    assert not mask[4].any() and not mask_visib[4].any()
    check_e2e_properties(s, ref)
    # fully inside the frame: canvas 1 and canvas 3 give identical tables
    inside = [0, 2, 3]
    df1 = ev.gt_info(gt[inside], renderer, depth, K, canvas=1)
    assert df1.to_dict("list") == df.iloc[inside].to_dict("list")
    # ground-truth detections for the pose estimator
    det = ev.detections_from_gt_info(gt, df, visib_gt_min=0.1)
    assert list(det.infos["label"]) == [labels[o] for o in obj[:4]] and det.bboxes.tolist() == [[float(v) for v in ref["boxes"][i, 4:]] for i in range(4)]


def check_e2e_properties(s, ref):
    """what the scene was built to show, on the emulation's results (which the engine's were just held to exactly)"""
    c, fr, bx = ref["counts"], ref["visib_fract"], ref["boxes"]
    div = lambda a, b: np.float32(a) / np.float32(b)          # noqa: E731
    assert all(c[i, 0] == c[i, 1] for i in (0, 2, 3))           # fully inside the frame: nothing on the outer tiles
    assert c[1, 0] > c[1, 1] > 0 and bx[1, 0] < 0 and 0.3 < c[1, 1] / c[1, 0] < 0.7   # half out of the left edge
    # an observed frame equal to the render itself (or within millimetres of it): everything inside the image is visible
    assert c[2, 3] == c[2, 1] and fr[2] == div(c[2, 1], c[2, 0])
    assert c[1, 3] == c[1, 1] and fr[1] == div(c[1, 1], c[1, 0]) and fr[1] < 1 and c[1, 2] < c[1, 1]
    # the same frame with a nearer plane over the left half: a strictly smaller fraction, bbox_visib inside bbox_obj
    assert 0 < fr[3] < fr[2]
    assert bx[3, 4] >= s["x_mid"] > bx[3, 0] and bx[3, 5] >= bx[3, 1] and bx[3, 6] <= bx[3, 2] and bx[3, 7] <= bx[3, 3]
    assert 0 < fr[0] < 1 and c[0, 3] < c[0, 1]                  # the occluder over object 0


def test_gt_info_tile_seams_against_one_oracle_render_of_the_whole_canvas(object_dataset, oracle_meshes):
    """nine engine tiles, stitched, against ONE oracle render of the 144 x 192 canvas under the shifted principal point.  The two routes
    subtract different integers from cx, cy before the same arithmetic, so their roundings may fall either way on a silhouette: a pixel
    may differ in coverage only if, in the single render, it has a 4-neighbour of the opposite coverage."""
    from megapose6d_amd import evaluation as ev
    from megapose6d_amd.renderer import Panda3dBatchRenderer
    from oracle import raster as orr
    from tests.support import synthetic as syn

    H, W = 48, 64
    rng = np.random.RandomState(6)
    labels = [o.label for o in object_dataset.list_objects]
    K = (np.diag([0.1, 0.1, 1.0]) @ syn.K_EXAMPLE).astype(np.float32)
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    # over the left seam; so near that it runs over the top and bottom seams; over the bottom-right corner; wholly in the left tile
    ts = ([-cx / fx * 0.3, 0.0, 0.3], [0.0, 0.0, 0.12], [(W - cx) / fx * 0.3, (H - cy) / fy * 0.3, 0.3], [-(cx + 0.5 * W) / fx * 0.3, 0.0, 0.3])
    obj = [0, 1, 2, 0]
    T = np.stack([pes.pose(pes.random_rotation(rng), t) for t in ts]).astype(np.float32)
    renderer = Panda3dBatchRenderer(object_dataset, n_workers=1)
    Kt = ev.tile_intrinsics(torch.from_numpy(K)[None].repeat(4, 1, 1).cuda(), 3, (H, W))
    tiles = renderer.render_depth([labels[o] for o in obj for _ in range(9)], torch.from_numpy(T).cuda().repeat_interleave(9, dim=0), Kt.flatten(0, 1), (H, W))
    tiles = tiles.view(4, 3, 3, H, W).cpu().numpy()
    K_canvas = K.copy()
    K_canvas[0, 2] += np.float32(W)
    K_canvas[1, 2] += np.float32(H)
    n_diff = n_cov = 0
    for i in range(4):
        stitched = np.block([[tiles[i, ty, tx] for tx in range(3)] for ty in range(3)]) > 0
        whole = orr.render(oracle_meshes[obj[i]], T[i][None], K_canvas[None], 3 * H, 3 * W, orr.FLAG_DEPTH)[2][0] > 0
        edge = np.zeros_like(whole)
        edge[1:, :] |= whole[1:, :] != whole[:-1, :]
        edge[:-1, :] |= whole[:-1, :] != whole[1:, :]
        edge[:, 1:] |= whole[:, 1:] != whole[:, :-1]
        edge[:, :-1] |= whole[:, :-1] != whole[:, 1:]
        diff = stitched != whole
        n_diff, n_cov = n_diff + int(diff.sum()), n_cov + int(whole.sum())
        assert whole.sum() > 150 and not np.any(diff & ~edge), (i, int((diff & ~edge).sum()))
        outside = whole.copy()
        outside[H:2 * H, W:2 * W] = False
        assert outside.any()                                   # every pose reaches an outer tile
        assert i != 3 or not whole[H:2 * H, W:2 * W].any()
    print(f"tile seams: {n_diff} differing pixels of {n_cov} covered, all on a silhouette")

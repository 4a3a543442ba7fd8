"""GPU: the TEASER++ refiner kernels (csrc/teaser.hip) through the three engine entry points against the host emulation built from the
same rules header (tests/teaser_emul.cpp): sample indices, degrees, core numbers, the selected set and the per-row info exactly, and
[R t] and the poses bit for bit, since every float64 sum has a fixed order.  Frames of 32 x 24 to 160 x 120, 3 to 5 rows over 2 images,
mask counts around the wave and the workgroup and one past the sampling kernel's register-resident points, both mask types, both TIM
graphs, selection "none", strided sampling (tests/support/teaser.py FRAME_CASES).  Then the refiner on rendered scenes with an
occluding plane over a third of every object, against the float64 restatement and the ground truth, under run_inference_pipeline and
as load_model builds it."""
import tempfile

import numpy as np
import pandas as pd
import pytest
import torch

from support import teaser as ts

pytestmark = pytest.mark.gpu


def _t(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same(got: torch.Tensor, want: np.ndarray, what):
    g = got.cpu().numpy()
    assert g.shape == want.shape and g.dtype == want.dtype, (what, g.shape, want.shape, g.dtype, want.dtype)
    if g.dtype.kind == "f":
        assert np.array_equal(_bits(g), _bits(want)), (what, float(np.abs(g - want).max()))
    else:
        assert np.array_equal(g, want), (what, int((g != want).sum()))


def test_sampling_matches_the_emulation():
    from megapose6d_amd import engine as eng

    counts = (1, 2, 63, 64, 65, 1023, 1025, ts.FPS_RESIDENT + 1, 20000)
    stride = max(counts)
    rng = np.random.RandomState(0)
    clouds = (rng.uniform(-0.2, 0.2, size=(len(counts), stride, 3)) + [0, 0, 0.6]).astype(np.float32)
    g = np.arange(6, dtype=np.float32)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    clouds[4, :65] = np.concatenate([lattice[:30], lattice[:30], lattice[:5]])       # exact ties: duplicated lattice points
    for n_points in (64, 65, 100, 1000):
        for fps in (True, False):
            idx, m = eng.farthest_point_sample(_t(clouds), _t(counts, torch.int32), n_points, use_fps=fps)
            want_idx, want_m = ts.emul_fps(clouds, counts, n_points, use_fps=fps)
            _same(m, want_m, ("M", n_points, fps))
            _same(idx, want_idx, ("idx", n_points, fps))
    idx, m = eng.farthest_point_sample(_t(lattice[None]), _t([216], torch.int32), 64)
    _same(idx, ts.emul_fps(lattice[None], [216], 64)[0], "lattice")
    for bad in (dict(points=torch.zeros(2, 5, 2).cuda()), dict(counts=torch.zeros(3, dtype=torch.int32).cuda()), dict(n_points=0)):
        kw = dict(points=torch.zeros(2, 5, 3).cuda(), counts=torch.zeros(2, dtype=torch.int32).cuda(), n_points=4)
        kw.update(bad)
        with pytest.raises(eng.EngineError):
            eng.farthest_point_sample(**kw)


@pytest.mark.parametrize("selection", ("kcore", "none"))
@pytest.mark.parametrize("graph", ("chain", "complete"))
def test_solve_matches_the_emulation(graph, selection):
    """the correspondence fixtures of the CPU contract test as rows of one launch, their own counts, a row of two between them"""
    from megapose6d_amd import engine as eng

    stride = 200
    S, D = np.zeros((len(ts.SOLVE_CASES) + 1, stride, 3), np.float32), np.zeros((len(ts.SOLVE_CASES) + 1, stride, 3), np.float32)
    counts = []
    for r, case in enumerate(ts.SOLVE_CASES + ((2, 0.0, 7),)):
        src, dst, _, _, _ = ts.correspondences(*case)
        S[r, : len(src)], D[r, : len(src)] = src, dst
        counts.append(len(src))
    want = ts.emul_solve(S, D, counts, min_num_inliers=25, inlier_selection=selection, rotation_tim_graph=graph)
    Rt, retval, tel = eng.teaser_solve(_t(S), _t(D), _t(counts, torch.int32), ts.NOISE_BOUND, 25, selection, graph, telemetry=True)
    _same(retval, want["retval"], "retval")
    for key in ("info", "degree", "core", "selected"):
        _same(tel[key], want[key], key)
    _same(Rt, want["Rt"], "Rt")
    assert want["retval"].tolist()[-1] == -1 and 0 in want["retval"].tolist() and want["info"][:, 3].max() >= (20 if selection == "none" else 0)


@pytest.mark.parametrize("variant", range(len(ts.FRAME_VARIANTS)))
@pytest.mark.parametrize("name", tuple(ts.FRAME_CASES))
def test_refine_matches_the_emulation(name, variant):
    from megapose6d_amd import engine as eng

    frames, kw = ts.FRAME_CASES[name]
    kw = dict(kw, **ts.FRAME_VARIANTS[variant])
    meas, im_ids, rend, K, TCO = ts.frame_case(*frames)
    want = ts.emul_frames(name, variant)
    out, retval, info, tel = eng.teaser_refine(_t(meas), _t(im_ids, torch.int32), _t(rend), _t(K), _t(TCO), noise_bound=ts.NOISE_BOUND, telemetry=True, **kw)
    _same(info, want["info"], "info")
    _same(retval, want["retval"], "retval")
    for key in ("sample_idx", "degree", "core", "selected", "Rt"):
        _same(tel[key], want[key], key)
    _same(out, want["TCO"], "TCO")
    plain = eng.teaser_refine(_t(meas), _t(im_ids, torch.int32), _t(rend), _t(K), _t(TCO), noise_bound=ts.NOISE_BOUND, **kw)
    assert torch.equal(plain[0], out) and torch.equal(plain[1], retval) and torch.equal(plain[2], info)


def test_bad_arguments_are_refused_before_any_launch():
    from megapose6d_amd import engine as eng

    meas, im_ids, rend, K, TCO = (_t(a, torch.int32 if a.dtype == np.int32 else torch.float32) for a in ts.frame_case(*ts.FRAME_CASES["tiny"][0]))
    for kw in (dict(n_points=0), dict(n_points=1025), dict(noise_bound=0.0), dict(noise_bound=float("nan")), dict(mask_type="other"),
               dict(inlier_selection="clique"), dict(rotation_tim_graph="star"), dict(min_num_inliers=-1), dict(n_min_points=-1)):
        with pytest.raises(eng.EngineError):
            eng.teaser_refine(meas, im_ids, rend, K, TCO, **kw)
    with pytest.raises(eng.EngineError):
        eng.teaser_refine(meas, im_ids, rend[:, :, :-1], K, TCO)
    s = torch.zeros(2, 1025, 3).cuda()
    with pytest.raises(eng.EngineError):
        eng.teaser_solve(s, s, torch.zeros(2, dtype=torch.int32).cuda())
    s = torch.zeros(2, 8, 3).cuda()
    with pytest.raises(eng.EngineError):
        eng.teaser_solve(s, s, torch.zeros(2, dtype=torch.int32).cuda(), noise_bound=-1.0)
    # the C entries themselves: a workspace that is too small and a null output return an error code
    lib = eng._lib.load()
    assert lib.mp_teaser_workspace_bytes(4, 24, 32) > lib.mp_teaser_workspace_bytes(4, 0, 0) > 0 and lib.mp_teaser_workspace_bytes(-1, 24, 32) == 0
    ws = torch.empty(1024, dtype=torch.uint8).cuda()
    c, Rt, rv = torch.zeros(2, dtype=torch.int32).cuda(), torch.zeros(2, 12, dtype=torch.float64).cuda(), torch.zeros(2, dtype=torch.int32).cuda()
    assert lib.mp_teaser_solve(s.data_ptr(), s.data_ptr(), c.data_ptr(), 2, 8, 0.01, 0, 0, 0, Rt.data_ptr(), rv.data_ptr(), None, None, None, None,
                               ws.data_ptr(), ws.numel(), eng._stream()) != 0
    big = torch.empty(lib.mp_teaser_workspace_bytes(2, 0, 0), dtype=torch.uint8).cuda()
    assert lib.mp_teaser_solve(s.data_ptr(), s.data_ptr(), c.data_ptr(), 2, 8, 0.01, 0, 0, 0, None, rv.data_ptr(), None, None, None, None,
                               big.data_ptr(), big.numel(), eng._stream()) != 0
    assert lib.mp_fps(s.data_ptr(), c.data_ptr(), 2, 8, 0, 1, rv.data_ptr(), rv.data_ptr(), big.data_ptr(), big.numel(), eng._stream()) != 0


# rendered scenes ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def occluded():
    """two lathe objects, two 160 x 120 frames, each holding both objects side by side; the measured depth of every object is replaced by a
    plane 6 cm in front of it over the left third of its columns.  Inputs: the true poses pushed 2.5 cm along the viewing ray (the depth
    an RGB-only estimate leaves open; the refiner pairs the two depths pixel by pixel, so it assumes the pose aligned in the image), 1 mm
    sideways and turned by a degree."""
    from megapose6d_amd.mesh_db import MeshDataBase
    from megapose6d_amd.renderer import Panda3dBatchRenderer
    from tests.support import synthetic as syn

    ds = syn.make_object_dataset(tempfile.mkdtemp(prefix="mp_teaser_"), n_objects=2, seed=31)
    renderer = Panda3dBatchRenderer(ds, n_workers=1)
    mesh_db = MeshDataBase.from_object_ds(ds).batched().cuda()
    labels = [o.label for o in ds.list_objects] * 2
    im_ids = [0, 0, 1, 1]
    K = syn.K_EXAMPLE.astype(np.float32).copy()
    K[:2] *= 0.25
    rng = np.random.RandomState(5)
    gt = np.stack([syn.random_pose(rng, (0.4, 0.5), 0.0) for _ in labels]).astype(np.float32)
    gt[:, 0, 3] = [-0.07, 0.07, -0.07, 0.07]
    gt[:, 1, 3] = 0.0
    Kt = _t(K)[None].repeat(4, 1, 1)
    d = renderer.render_depth(labels, _t(gt), Kt, (120, 160))
    frames = []
    for b in range(2):
        frame = torch.zeros(120, 160).cuda()
        for n in (2 * b, 2 * b + 1):
            cols = torch.nonzero((d[n] > 0).any(0)).flatten()
            cut = int(cols.min()) + (int(cols.max()) - int(cols.min()) + 1) // 3
            obj = d[n].clone()
            plane = float(d[n][d[n] > 0].min()) - 0.06
            obj[:, :cut] = torch.where(obj[:, :cut] > 0, torch.full_like(obj[:, :cut], plane), obj[:, :cut])
            frame = torch.where(obj > 0, obj, frame)
        frames.append(frame)
    init = gt.copy()
    for n in range(4):
        init[n, :3, :3] = (ts.rotation(rng.normal(size=3), np.deg2rad(1.0)) @ gt[n, :3, :3]).astype(np.float32)
        init[n, :3, 3] = gt[n, :3, 3] * np.float32(1.0 + 0.025 / np.linalg.norm(gt[n, :3, 3])) + np.float32([0.001, -0.001, 0.0])
    return dict(ds=ds, renderer=renderer, mesh_db=mesh_db, labels=labels, im_ids=im_ids, K=_t(K)[None].repeat(2, 1, 1), gt=gt, init=init,
                depth=torch.stack(frames))


def _add(mesh_db, labels, T_a, T_b):
    """mean distance of the object's points under the two poses"""
    out = []
    for n, label in enumerate(labels):
        p = mesh_db.points[list(mesh_db.labels).index(label)].cpu().numpy().astype(np.float64)
        out.append(float(np.linalg.norm(p @ (T_a[n, :3, :3] - T_b[n, :3, :3]).T.astype(np.float64) + (T_a[n, :3, 3] - T_b[n, :3, 3]), axis=1).mean()))
    return np.asarray(out)


def test_refiner_on_occluded_scenes(occluded):
    from megapose6d_amd import TeaserppRefiner
    from megapose6d_amd import engine as eng
    from megapose6d_amd.tcoll import PandasTensorCollection

    o = occluded
    preds = PandasTensorCollection(pd.DataFrame(dict(label=o["labels"], batch_im_id=o["im_ids"], instance_id=[0, 1, 0, 1])), poses=_t(o["init"]))
    refiner = TeaserppRefiner(o["mesh_db"], o["renderer"])
    out, extra = refiner.refine_poses(preds, depth=o["depth"], K=o["K"])
    assert torch.equal(out.poses_input, preds.poses) and set(extra) >= {"retval", "num_inliers", "n_selected", "n_points", "gnc_iterations"}
    assert extra["retval"].tolist() == [0, 0, 0, 0]
    before, after = _add(o["mesh_db"], o["labels"], o["init"], o["gt"]), _add(o["mesh_db"], o["labels"], out.poses.cpu().numpy(), o["gt"])
    print("ADD before", before, "after", after, {k: v.tolist() for k, v in extra.items()})
    assert (after < before / 2).all()
    # the same inputs through the engine call, against the emulation (bit for bit) and the float64 restatement (RT_TOL)
    im_ids = _t(o["im_ids"], torch.int32)
    K_rows = o["K"][im_ids.long()]
    rend = o["renderer"].render_depth(o["labels"], _t(o["init"]), K_rows, (120, 160)).contiguous()
    poses, retval, info, tel = eng.teaser_refine(o["depth"], im_ids, rend, K_rows, _t(o["init"]), telemetry=True)
    assert torch.equal(poses, out.poses) and torch.equal(retval, extra["retval"]) and torch.equal(info[:, 4], extra["num_inliers"])
    host = [a.cpu().numpy() for a in (o["depth"], rend, K_rows)]
    want = ts.emul_refine(host[0], o["im_ids"], host[1], host[2], o["init"])
    _same(poses, want["TCO"], "TCO")
    _same(tel["Rt"], want["Rt"], "Rt")
    _same(info, want["info"], "info")
    for n in range(4):
        ref = ts.ref_refine_row(host[0][o["im_ids"][n]], host[1][n], host[2][n])
        assert np.array_equal(tel["sample_idx"][n, : len(ref["sample_idx"])].cpu().numpy(), ref["sample_idx"])
        assert info[n].tolist() == [ref["N"], len(ref["sample_idx"]), ref["n_selected"], ref["gnc_iterations"], ref["num_inliers"]]
        diff = float(np.abs(tel["Rt"][n].cpu().numpy() - ref["Rt"]).max())
        print(f"row {n}: N {ref['N']}, selected {ref['n_selected']}, inliers {ref['num_inliers']}, |Rt - restatement| {diff:.2e}")
        assert diff <= ts.RT_TOL
        # the occluded third was sampled, and is no inlier of the transform (it sits 6 cm and more in front of the object, the bound is 1 cm)
        assert 0.5 * len(ref["sample_idx"]) <= ref["num_inliers"] <= 0.85 * len(ref["sample_idx"])


def test_pipeline_and_load_model_run_the_refiner():
    from megapose6d_amd import TeaserppRefiner
    from megapose6d_amd import load_model as lm
    from tests.support.scene import make_scene

    est, obs, det, gt = make_scene(n_objects=1, seed=0, SO3_grid_size=72, rgbd=True)
    est.depth_refiner = lm.make_depth_refiner("teaserpp", est.mesh_db, est.refiner_model.renderer)
    assert isinstance(est.depth_refiner, TeaserppRefiner)
    final, extra = est.run_inference_pipeline(obs, detections=det, n_refiner_iterations=1, n_pose_hypotheses=1, run_depth_refiner=True)
    assert "depth_refiner" in extra and len(final) == 1 and torch.isfinite(final.poses).all()
    assert "depth refiner=" in extra["timing_str"] and "poses_input" in extra["depth_refiner"]["preds"].tensors
    assert est.depth_refiner.debug["n_mask_points"].item() > 0

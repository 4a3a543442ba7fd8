"""-m gpu: edge cases of the hot path through the reference-shaped API (ragged chunks, several frames, repeated labels,
meshes of different sizes, degenerate inputs) -- the cases the reference's own code paths distinguish."""
import tempfile

import numpy as np
import pandas as pd
import pytest
import torch

from conftest import assert_logits_close  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def multi_scene():
    """2 frames with different intrinsics, 3 detections: two instances of obj_000000 in frame 0, obj_000001 in frame 1."""
    from tests.support import synthetic as syn
    from tests.support.scene import build_estimator, render_observation
    from megapose6d_amd.tcoll import PandasTensorCollection
    from megapose6d_amd.types import ObservationTensor

    tmp = tempfile.mkdtemp(prefix="mp_edge_")
    ds = syn.make_object_dataset(tmp, n_objects=2, seed=21, n_theta=48, n_z=60)  # 2882-vertex meshes ...
    v, f, c = syn.make_lathe_mesh(99, n_theta=80, n_z=70)                          # ... and a 5602-vertex one (padding path)
    syn.write_ply(ds[1].mesh_path, v, f, c)
    est = build_estimator(ds, SO3_grid_size=72)
    rng = np.random.RandomState(4)
    K0 = syn.K_EXAMPLE.astype(np.float32)
    K1 = K0.copy()
    K1[0, 0] *= 0.9; K1[1, 1] *= 0.9; K1[0, 2] += 11.0
    r = est.coarse_model.renderer
    posesA = np.stack([syn.random_pose(rng, (0.5, 0.7), 0.25) for _ in range(2)])
    posesA[1, 0, 3] += 0.12
    im0, bb0 = render_observation(r, ["obj_000000", "obj_000000"], posesA, K0, seed=1)
    poseB = np.stack([syn.random_pose(rng, (0.5, 0.7), 0.1)])
    im1, bb1 = render_observation(r, ["obj_000001"], poseB, K1, seed=2)
    obs = ObservationTensor(torch.cat([im0, im1]), torch.from_numpy(np.stack([K0, K1])).cuda())
    infos = pd.DataFrame(dict(label=["obj_000000", "obj_000000", "obj_000001"], batch_im_id=[0, 0, 1]))
    det = PandasTensorCollection(infos, bboxes=torch.from_numpy(np.concatenate([bb0, bb1])).cuda())
    return tmp, ds, est, obs, det


def _oracle(tmp, ds, grid=72):
    from megapose6d_amd import mesh_io
    from tests.support import synthetic as syn
    from megapose6d_amd.mesh_db import MeshDataBase
    from megapose6d_amd.pose_estimator import load_SO3_grid
    from oracle import pipeline as op
    from oracle import raster as orr

    meshes = {o.label: mesh_io.load_rigid_object(o) for o in ds.list_objects}
    db = MeshDataBase.from_object_ds(ds).batched()
    rend = orr.OracleBatchRenderer(meshes)
    preds = {}
    for role, seed in (("coarse", 11), ("refiner", 12)):
        cfg = syn.make_cfg(role)
        head, n_out = ("pose", 9) if role == "refiner" else ("logits", 1)
        preds[role] = op.OraclePosePredictor(cfg, syn.make_state_dict("vanilla_resnet34", syn.n_inputs_for(cfg), head, n_out, seed=seed),
                                             db.labels.tolist(), db.points, rend)
    return op.OraclePoseEstimator(preds["coarse"], preds["refiner"], load_SO3_grid(grid), bsz=24)


def test_multi_frame_multi_instance_vs_oracle(multi_scene):
    tmp, ds, est, obs, det = multi_scene
    final, extra = est.run_inference_pipeline(obs, detections=det, n_refiner_iterations=2, n_pose_hypotheses=2)
    # add_instance_id (inference/utils.py:151-171): instances numbered within (batch_im_id, label)
    assert final.infos.sort_values(["batch_im_id", "instance_id"])["instance_id"].tolist() == [0, 1, 0]
    infos = det.infos.copy()
    infos["instance_id"] = [0, 1, 0]
    res = _oracle(tmp, ds).run(obs.images.cpu(), obs.K.cpu(), infos, det.bboxes.cpu(), n_refiner_iterations=2, n_pose_hypotheses=2)
    lg = extra["coarse"]["data"]["logits"].flatten().cpu()
    scale = max(1.0, res["coarse_logits"].abs().max().item())
    assert_logits_close(lg.numpy(), res["coarse_logits"].numpy(), scale)
    key = lambda df: list(zip(df["batch_im_id"], df["label"], df["instance_id"], df["hypothesis_id"]))
    got_f = extra["coarse_filter"]["preds"]
    assert sorted(key(got_f.infos)) == sorted(key(res["filtered_infos"]))
    order = [key(got_f.infos).index(k) for k in key(res["filtered_infos"])]
    for n in range(2):
        p = extra["refiner_all_hypotheses"]["preds"][f"iteration={n + 1}"].poses.cpu()[order]
        assert (p - res["refiner_poses"][n]).abs().max().item() < 1e-4
    kf = lambda df: list(zip(df["batch_im_id"], df["label"], df["instance_id"]))
    of = [kf(final.infos).index(k) for k in kf(res["final_infos"])]
    assert (final.poses.cpu()[of] - res["final_TCO"]).abs().max().item() < 1e-4


def test_ragged_chunks_match_single_launch(multi_scene):
    """216 coarse rows in chunks of 50 (last chunk ragged) and refiner rows in chunks of 4 == one big launch"""
    tmp, ds, est, obs, det = multi_scene
    f1, e1 = est.run_inference_pipeline(obs, detections=det, n_refiner_iterations=2, n_pose_hypotheses=3)
    old = est.max_rows_per_launch
    try:
        est.max_rows_per_launch = 50
        f2, e2 = est.run_inference_pipeline(obs, detections=det, n_refiner_iterations=2, n_pose_hypotheses=3)
        assert e2["coarse"]["data"]["n_batches"] == 5
        est.max_rows_per_launch = 4
        est.n_streams = 2
        est.min_rows_per_stream = 2
        f3, _ = est.run_inference_pipeline(obs, detections=det, n_refiner_iterations=2, n_pose_hypotheses=3)
    finally:
        est.max_rows_per_launch, est.n_streams, est.min_rows_per_stream = old, 1, 64
    assert (e1["coarse"]["data"]["logits"] - e2["coarse"]["data"]["logits"]).abs().max().item() < 1e-4
    assert (f1.poses - f2.poses).abs().max().item() < 2e-5 and (f1.poses - f3.poses).abs().max().item() < 2e-5  # tiny launches take the split-K conv path: another summation order


def test_coarse_estimates_entry_point_and_single_row(multi_scene):
    """run_inference_pipeline(coarse_estimates=...) skips coarse + top-K (pose_estimator.py:587-590); 1 row, 1 iteration = config 1"""
    from megapose6d_amd.tcoll import PandasTensorCollection

    tmp, ds, est, obs, det = multi_scene
    _, e = est.run_inference_pipeline(obs, detections=det, n_refiner_iterations=1, n_pose_hypotheses=1)
    ce = e["coarse_filter"]["preds"]
    one = PandasTensorCollection(ce.infos.iloc[[2]].copy(), poses=ce.poses[[2]].clone())
    final, extra = est.run_inference_pipeline(obs, coarse_estimates=one, n_refiner_iterations=1)
    assert extra["coarse"]["data"] is None and len(final) == 1
    ref = e["refiner_all_hypotheses"]["preds"]["iteration=1"].poses[2]
    assert (final.poses[0] - ref).abs().max().item() < 1e-5


def test_degenerate_inputs(multi_scene):
    from megapose6d_amd.tcoll import PandasTensorCollection

    tmp, ds, est, obs, det = multi_scene
    # unknown label -> KeyError (label -> mesh lookup, rigid_mesh_database.py:147 / panda3d_batch_renderer.py:243)
    bad = PandasTensorCollection(det.infos.assign(label=["obj_000000", "nope", "obj_000001"]), bboxes=det.bboxes)
    with pytest.raises(KeyError):
        est.run_inference_pipeline(obs, detections=bad, n_refiner_iterations=1)
    # missing required columns -> AssertionError (inference/types.py:77-86)
    with pytest.raises(AssertionError):
        est.forward_coarse_model(obs, PandasTensorCollection(pd.DataFrame(dict(label=["obj_000000"])), bboxes=det.bboxes[:1]))
    # neither detections nor a detector
    with pytest.raises(AssertionError):
        est.run_inference_pipeline(obs)
    # a non-finite hypothesis renders zeros and yields a finite logit; the other rows are unaffected
    T = est.forward_coarse_model(obs, det)[0].poses[:4].clone()
    ref = est.coarse_model.forward_coarse(obs.images, obs.K[[0]].repeat(4, 1, 1), ["obj_000000"] * 4, T,
                                          im_ids=torch.zeros(4, dtype=torch.int32, device="cuda"))["logits"].clone()
    T[1, 0, 3] = float("nan")
    out = est.coarse_model.forward_coarse(obs.images, obs.K[[0]].repeat(4, 1, 1), ["obj_000000"] * 4, T,
                                          im_ids=torch.zeros(4, dtype=torch.int32, device="cuda"), return_debug_data=True)
    assert torch.equal(out["logits"][[0, 2, 3]], ref[[0, 2, 3]])
    assert out["renders"][1].abs().max() == 0
    # object far outside the frame: still finite outputs
    T2 = T[[0]].clone()
    T2[0, 0, 3] = 5.0
    o2 = est.coarse_model.forward_coarse(obs.images, obs.K[[0]], ["obj_000000"], T2, im_ids=torch.zeros(1, dtype=torch.int32, device="cuda"))
    assert torch.isfinite(o2["logits"]).all()


def test_mesh_with_too_few_vertices_is_rejected(tmp_path):
    """lib3d/mesh_ops.py:79: the deterministic 2000-point sampling asserts n_points <= n_vertices"""
    from tests.support import synthetic as syn
    from megapose6d_amd.mesh_db import MeshDataBase

    v, f, c = syn.make_lathe_mesh(1, n_theta=16, n_z=20)
    syn.write_ply(tmp_path / "small.ply", v, f, c)
    db = MeshDataBase.from_object_ds(syn.RigidObjectDataset([syn.RigidObject("small", tmp_path / "small.ply", mesh_units="mm")])).batched()
    with pytest.raises(AssertionError):
        db.sampled_points(2000)


def test_pose_predictor_stand_alone_helpers_match_the_fused_step():
    """PosePredictor.compute_crops_multiview / normalize_depth / normalize_images / *_dims (models/pose_rigid.py:132-158, 249-303,
    410-496) as stand-alone calls agree with what the fused step computes"""
    from tests.support.scene import make_scene

    est, obs, det, gt = make_scene(n_objects=2, seed=9, rgbd=True, SO3_grid_size=72)
    ref = est.refiner_model
    assert ref.input_rgb_dims == [0, 1, 2] and ref.input_depth_dims == [3] and ref.render_rgb_dims == [0, 1, 2] and ref.render_depth_dims == [6]
    assert est.coarse_model.input_depth_dims == [] and est.coarse_model.render_depth_dims == []
    coarse, _ = est.forward_coarse_model(obs, det)
    T = coarse.poses[[3, 80]].contiguous()
    labels = coarse.infos["label"].iloc[[3, 80]].tolist()
    K = obs.K[[0, 0]].contiguous()
    im_ids = torch.zeros(2, dtype=torch.int32, device="cuda")
    st = ref._step(ref._prep_images(obs.images), im_ids, K, labels, T, want_sigmoid=False)
    TCV_O, KV = st["TCV_O"], st["KV_crop"]
    got = ref.compute_crops_multiview(obs.images, K, TCV_O, TCV_O[..., :3, 3].contiguous(), labels)
    # views 1..3 as in the fused step; view 0 of the pipeline is overridden by the 2000-point K_crop (pose_rigid.py:550-552)
    assert got.shape == (2, 4, 3, 3) and ((got[:, 1:] - KV[:, 1:]).abs() / KV[:, 1:].abs().clamp(min=1.0)).max().item() < 1e-5
    assert ((got[:, 0] - KV[:, 0]).abs() / KV[:, 0].abs().clamp(min=1.0)).max().item() < 0.2 and not torch.equal(got[:, 0], KV[:, 0])
    with pytest.raises(NotImplementedError):
        ref.compute_crops_multiview(obs.images, K, TCV_O, TCV_O[..., :3, 3] + 0.01, labels)
    # depth normalisation (default tCR_scale_clamp_center): clamp(d / z, 0, 2) - 1
    d = torch.rand(2, 3, 1, 24, 32, device="cuda") * 2.0
    tCR = torch.tensor([[0.0, 0.0, 0.5], [0.1, 0.0, 0.8]], device="cuda")
    want = torch.clamp(d / tCR[:, 2].view(2, 1, 1, 1, 1), 0, 2) - 1
    assert ref.depth_normalization_type == "tCR_scale_clamp_center"
    assert (ref.normalize_depth(d, tCR) - want).abs().max().item() < 1e-6
    images = torch.rand(2, 4, 24, 32, device="cuda")
    renders = torch.rand(2, 28, 24, 32, device="cuda")
    im2, re2 = ref.normalize_images(images, renders, tCR)
    assert torch.equal(im2[:, :3], images[:, :3]) and (im2[:, 3] - (torch.clamp(images[:, 3] / tCR[:, 2].view(2, 1, 1), 0, 2) - 1)).abs().max() < 1e-6
    depth_dims = [6, 13, 20, 27]
    other = [c for c in range(28) if c not in depth_dims]
    assert torch.equal(re2[:, other], renders[:, other])
    assert (re2[:, depth_dims] - (torch.clamp(renders[:, depth_dims] / tCR[:, 2].view(2, 1, 1, 1), 0, 2) - 1)).abs().max() < 1e-6
    assert torch.equal(images, images.clone()) and not torch.equal(re2, renders)   # inputs untouched (copies returned)


# -- the stage scaffold of PoseEstimator: timer, debug data, kept outputs, ragged chunks on two streams -----------------------------------
def _coarse_top2(est, obs, det):
    """the fixture's detections with instance ids -> (detections, their 216 coarse rows, the 6 top-2 rows)"""
    from megapose6d_amd.pose_estimator import add_instance_id
    from megapose6d_amd.tcoll import PandasTensorCollection

    det = add_instance_id(PandasTensorCollection(det.infos.copy(), bboxes=det.bboxes))
    coarse, _ = est.forward_coarse_model(obs, det)
    return det, coarse, est.filter_pose_estimates(coarse, top_K=2, filter_field="coarse_logit")


def _assert_collections_equal(a, b):
    assert list(a.tensors) == list(b.tensors)
    for k in a.tensors:
        assert torch.equal(a.tensors[k], b.tensors[k]), k


def test_timed_stages_equal_untimed_stages(multi_scene):
    """cuda_timer=True fences the stage and reports device times; it changes no result and no key of any extra_data"""
    tmp, ds, est, obs, det = multi_scene
    det = _coarse_top2(est, obs, det)[0]
    runs = []
    for timed in (False, True):
        coarse, ce = est.forward_coarse_model(obs, det, cuda_timer=timed)
        top = est.filter_pose_estimates(coarse, top_K=2, filter_field="coarse_logit")
        preds, re = est.forward_refiner(obs, top, n_iterations=2, cuda_timer=timed)
        scored, se = est.forward_scoring_model(obs, preds["iteration=2"].clone(), cuda_timer=timed)
        runs.append((coarse, ce, preds, re, scored, se))
    (c0, ce0, p0, re0, s0, se0), (c1, ce1, p1, re1, s1, se1) = runs
    for e0, e1 in ((ce0, ce1), (se0, se1)):
        assert torch.equal(e0["logits"], e1["logits"]) and torch.equal(e0["scores"], e1["scores"])
    assert torch.equal(ce0["TCO"], ce1["TCO"])
    _assert_collections_equal(c0, c1)
    _assert_collections_equal(s0, s1)
    assert sorted(p0) == sorted(p1) == ["iteration=1", "iteration=2"]
    for k in p0:
        assert list(p0[k].tensors) == ["poses", "poses_input", "K_crop", "K", "boxes_rend", "boxes_crop"]
        _assert_collections_equal(p0[k], p1[k])
        assert torch.equal(re0["pose_outputs"][k], re1["pose_outputs"][k])
    assert s0.infos["pose_logit"].tolist() == s1.infos["pose_logit"].tolist()
    assert c0.infos["coarse_logit"].tolist() == c1.infos["coarse_logit"].tolist()
    for e0, e1 in ((ce0, ce1), (re0, re1), (se0, se1)):
        assert e0["model_time"] == 0.0
        assert e1["model_time"] > 0 and e1["render_time"] > 0
    stage_keys = {"render_time", "model_time", "time", "logits", "scores", "debug", "n_batches", "timing_str"}
    for e in (ce0, ce1):
        assert set(e) == stage_keys | {"TCO"}
    for e in (se0, se1):
        assert set(e) == stage_keys
    for e in (re0, re1):
        assert set(e) == {"n_iterations", "outputs", "model_time", "render_time", "time", "pose_outputs"}
        assert e["n_iterations"] == 2 and e["outputs"] == []


def test_stage_debug_data_is_the_models_debug_data(multi_scene):
    """return_debug_data=True of the coarse and scoring stages: the crops / renders of coarse_model.forward_coarse, stage-shaped"""
    tmp, ds, est, obs, det = multi_scene
    det, coarse, top = _coarse_top2(est, obs, det)
    B, M = len(det), 72
    h, w = est.coarse_model.render_size
    n_in = est.coarse_model.backbone.n_inputs

    def direct(infos, poses):
        im = infos["batch_im_id"].values.astype(np.int64)
        return est.coarse_model.forward_coarse(obs.images, obs.K[torch.as_tensor(im, device="cuda")].float(), infos["label"].tolist(),
                                               poses.contiguous(), im_ids=torch.as_tensor(im.astype(np.int32), device="cuda"),
                                               return_debug_data=True)

    dbg = est.forward_coarse_model(obs, det, return_debug_data=True)[1]["debug"]
    assert set(dbg) == {"images_crop", "renders"}
    assert dbg["images_crop"].shape == (B, M, 3, h, w) and dbg["renders"].shape == (B, M, n_in - 3, h, w)
    d = 2   # the detection of frame 1 (other intrinsics, the larger mesh)
    ref = direct(coarse.infos.iloc[d * M:(d + 1) * M], coarse.poses[d * M:(d + 1) * M])
    assert torch.equal(dbg["images_crop"][d], ref["images_crop"]) and torch.equal(dbg["renders"][d], ref["renders"])

    R = len(top)
    dbg = est.forward_scoring_model(obs, top.clone(), return_debug_data=True)[1]["debug"]
    assert set(dbg) == {"images_crop", "renders"}
    assert dbg["images_crop"].shape == (R, 3, h, w) and dbg["renders"].shape == (R, n_in - 3, h, w)
    sel = np.flatnonzero(top.infos["bbox_id"].values == d)
    assert sel.size == 2
    ref = direct(top.infos.iloc[sel], top.poses[sel.tolist()])
    assert torch.equal(dbg["images_crop"][sel.tolist()], ref["images_crop"]) and torch.equal(dbg["renders"][sel.tolist()], ref["renders"])


def test_refiner_keep_all_outputs(multi_scene):
    """keep_all_outputs=True: one dict of materialised PosePredictorOutputs per chunk, the same poses as without"""
    tmp, ds, est, obs, det = multi_scene
    top = _coarse_top2(est, obs, det)[2]
    R = len(top)
    assert R == 6
    old = est.max_rows_per_launch
    try:
        est.max_rows_per_launch = 4
        preds, extra = est.forward_refiner(obs, top, n_iterations=2, keep_all_outputs=True)
        plain, plain_extra = est.forward_refiner(obs, top, n_iterations=2, keep_all_outputs=False)
    finally:
        est.max_rows_per_launch = old
    assert len(extra["outputs"]) == 2 and plain_extra["outputs"] == []
    for outputs_, rows in zip(extra["outputs"], (4, 2)):
        assert sorted(outputs_) == ["iteration=1", "iteration=2"]
        for o in outputs_.values():
            assert o.renders is not None and o.images_crop is not None
            assert o.renders.shape[0] == rows and o.images_crop.shape[0] == rows and o.TCO_output.shape == (rows, 4, 4)
    for k in ("iteration=1", "iteration=2"):
        assert preds[k].infos["refiner_batch_idx"].tolist() == (np.arange(R) // 4).tolist()
        assert preds[k].infos["refiner_instance_idx"].tolist() == (np.arange(R) % 4).tolist()
        assert torch.equal(preds[k].poses, plain[k].poses)


def test_scoring_under_ragged_chunks_and_two_streams(multi_scene):
    """9 scoring rows in chunks of 4 interleaved on two streams == one launch (the bound test_ragged_chunks_match_single_launch uses)"""
    tmp, ds, est, obs, det = multi_scene
    _, e1 = est.run_inference_pipeline(obs, detections=det, n_refiner_iterations=2, n_pose_hypotheses=3)
    old = est.max_rows_per_launch, est.n_streams, est.min_rows_per_stream
    try:
        est.max_rows_per_launch, est.n_streams, est.min_rows_per_stream = 4, 2, 2
        _, e2 = est.run_inference_pipeline(obs, detections=det, n_refiner_iterations=2, n_pose_hypotheses=3)
    finally:
        est.max_rows_per_launch, est.n_streams, est.min_rows_per_stream = old
    l1, l2 = e1["scoring"]["data"]["logits"], e2["scoring"]["data"]["logits"]
    R = l1.shape[0]
    assert R == 9 and l2.shape == l1.shape == (R, 1)
    assert e1["scoring"]["data"]["n_batches"] == 1 and e2["scoring"]["data"]["n_batches"] == -(-R // 4)
    err = (l1 - l2).abs().max().item()
    print(f"scoring logits, chunks of 4 on two streams vs one launch: max abs diff {err:.3e}")
    assert err < 1e-4

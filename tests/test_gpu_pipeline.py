"""-m gpu: end-to-end parity of the HIP pipeline (through the reference-shaped API) against
 (a) golden outputs of the REFERENCE's own orchestration (tests/golden/pipeline.npz) and (b) the CPU oracle.
Tolerances: poses 1e-4 abs on R and t (BASELINE.json north_star); logits 1e-4 relative to the logit scale."""
import tempfile
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
import torch

from conftest import assert_logits_close  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"


@pytest.fixture(scope="module")
def scene72():
    from tests.support.scene import build_estimator
    from tests.support import synthetic as syn

    tmp = tempfile.mkdtemp(prefix="mp_t_")
    ds = syn.make_object_dataset(tmp, n_objects=1, seed=0)
    est = build_estimator(ds, SO3_grid_size=72)
    return ds, est


def _golden_inputs():
    from megapose6d_amd.load_model import make_detections
    from megapose6d_amd.types import ObservationTensor

    g = {k: v for k, v in np.load(GOLD / "pipeline.npz").items()}
    obs = ObservationTensor.from_numpy(g["img_u8"], None, g["K"]).cuda()
    det = make_detections(["obj_000000"], g["bboxes"]).cuda()
    return g, obs, det


def test_pipeline_matches_reference_golden(scene72):
    ds, est = scene72
    g, obs, det = _golden_inputs()
    final, extra = est.run_inference_pipeline(obs, detections=det, n_refiner_iterations=3, n_pose_hypotheses=2)
    cd = extra["coarse"]
    assert np.abs(cd["preds"].poses.cpu().numpy() - g["coarse_TCO"]).max() < 1e-5
    lg = cd["data"]["logits"].cpu().numpy().flatten()
    scale = max(1.0, float(np.abs(g["coarse_logits"]).max()))
    assert_logits_close(lg, g["coarse_logits"], scale)
    hyp = extra["coarse_filter"]["preds"].infos["hypothesis_id"].tolist()
    assert sorted(hyp) == sorted(g["filtered_hyp_ids"].tolist())
    order = [hyp.index(h) for h in g["filtered_hyp_ids"].tolist()]
    for n in range(1, 4):
        p = extra["refiner_all_hypotheses"]["preds"][f"iteration={n}"]
        assert np.abs(p.poses.cpu().numpy()[order] - g[f"refiner_poses_{n}"]).max() < 1e-4, n
        kc, kg = p.K_crop.cpu().numpy()[order], g[f"refiner_K_crop_{n}"]
        assert (np.abs(kc - kg) / np.maximum(np.abs(kg), 1)).max() < 2e-6   # fp32 round-off of values up to ~1e3
        assert np.abs(p.boxes_crop.cpu().numpy()[order] - g[f"refiner_boxes_crop_{n}"]).max() < 1e-3   # pixels
    sl = extra["scoring"]["data"]["logits"].cpu().numpy().flatten()[order]
    assert_logits_close(sl, g["scoring_logits"], scale)
    assert np.abs(final.poses.cpu().numpy() - g["final_TCO"]).max() < 1e-4
    # API surface
    assert list(final.infos.columns) == g["final_columns"].tolist()
    assert sorted(extra.keys()) == g["extra_keys"].tolist()
    assert set(cd["data"].keys()) >= {"render_time", "model_time", "time", "logits", "scores", "TCO", "debug", "n_batches", "timing_str"}
    assert cd["data"]["logits"].shape == (1, 72) and cd["data"]["TCO"].shape == (1, 72, 4, 4)
    assert set(extra["refiner_all_hypotheses"]["preds"]["iteration=1"].tensors) == {"poses", "poses_input", "K_crop", "K", "boxes_rend", "boxes_crop"}


def test_cnn_input_tensor_vs_oracle(scene72):
    """the assembled CNN input (crop + 4 views x (rgb, normals)) of one refiner step: crop <= 1e-5, renders identical except
    for the rare pixel whose coverage flips because a camera matrix differs in the last ulp (counted and bounded)."""
    from megapose6d_amd import mesh_io
    from tests.support import synthetic as syn
    from megapose6d_amd.mesh_db import MeshDataBase
    from oracle import pipeline as op
    from oracle import raster as orr

    ds, est = scene72
    g, obs, det = _golden_inputs()
    T0 = torch.from_numpy(g["gt_TCO"][:1]).clone()
    T0[:, :3, 3] += torch.tensor([0.01, -0.01, 0.02])
    T0 = T0.repeat(3, 1, 1)
    T0[1, 0, 3] += 0.02
    T0[2, :3, :3] = T0[2, :3, :3] @ torch.tensor([[0.96, -0.28, 0], [0.28, 0.96, 0], [0, 0, 1.0]])
    ref = est.refiner_model
    labels = ["obj_000000"] * 3
    out = ref(images=obs.images, K=obs.K.repeat(3, 1, 1), labels=labels, TCO=T0.cuda(), n_iterations=1,
              im_ids=torch.zeros(3, dtype=torch.int32, device="cuda"))["iteration=1"]
    x_gpu = torch.cat([out.images_crop, out.renders], 1).cpu()
    meshes = {o.label: mesh_io.load_rigid_object(o) for o in ds.list_objects}
    db = MeshDataBase.from_object_ds(ds).batched()
    cfg = syn.make_cfg("refiner")
    pred = op.OraclePosePredictor(cfg, syn.make_state_dict("vanilla_resnet34", 27, "pose", 9, seed=12), db.labels.tolist(), db.points,
                                  orr.OracleBatchRenderer(meshes))
    o = pred.forward(obs.images.cpu(), torch.zeros(3, dtype=torch.long), obs.K.cpu().repeat(3, 1, 1), labels, T0, 1)[0]
    assert (x_gpu[:, :3] - o["x"][:, :3]).abs().max() < 1e-5
    d = (x_gpu[:, 3:] - o["x"][:, 3:]).abs()
    assert (d > 0).float().mean().item() < 2e-4, "render pixels differing from the oracle"
    assert d.max().item() <= 1.0
    assert (out.TCV_O_input.cpu() - o["TCV_O"]).abs().max() < 2e-6
    assert (out.network_outputs["pose"].cpu() - o["net"]["pose"]).abs().max() < 1e-5
    assert (out.TCO_output.cpu() - o["TCO_output"]).abs().max() < 1e-5


def test_renderer_api_contract(scene72):
    """Panda3dBatchRenderer.render signature/behaviour (panda3d_batch_renderer.py:217-282)"""
    from megapose6d_amd.types import Panda3dLightData, make_scene_lights

    ds, est = scene72
    r = est.coarse_model.renderer
    g, obs, det = _golden_inputs()
    T = torch.from_numpy(g["gt_TCO"][:1]).repeat(2, 1, 1).cuda()
    T[1, 0, 0] = float("nan")
    K = obs.K.repeat(2, 1, 1)
    amb = [[Panda3dLightData("ambient", (1.0, 1.0, 1.0, 1.0))]] * 2
    o = r.render(["obj_000000"] * 2, T, K, amb, (240, 320), render_depth=True, render_normals=True)
    assert o.rgbs.shape == (2, 3, 240, 320) and o.normals.shape == (2, 3, 240, 320) and o.depths.shape == (2, 1, 240, 320)
    assert o.rgbs.is_cuda and o.rgbs.dtype == torch.float32 and 0 <= o.rgbs.min() and o.rgbs.max() <= 1
    assert o.rgbs[1].abs().max() == 0 and o.depths[1].abs().max() == 0  # non-finite pose -> zeros, no exception
    q = o.rgbs[0] * 255
    assert (q - q.round()).abs().max() < 1e-4  # uint8 quantised
    o2 = r.render(["obj_000000"] * 2, T, K, amb, (240, 320))
    assert o2.normals is None and o2.depths is None
    with pytest.raises(NotImplementedError):
        r.render(["obj_000000"] * 2, T, K, amb, (240, 320), render_mask=True)
    with pytest.raises(KeyError):
        r.render(["unknown"] * 2, T, K, amb, (240, 320))
    o3 = r.render(["obj_000000"] * 2, T, K, [make_scene_lights(), amb[0]], (240, 320))  # mixed light sets
    assert torch.equal(o3.rgbs[1], o.rgbs[1]) and not torch.equal(o3.rgbs[0], o.rgbs[0])


def test_full_grid_multi_object_invariants():
    """576-rotation grid, 3 objects, K=5: structure, determinism and sharded-row bookkeeping at BASELINE sizes."""
    from tests.support.scene import make_scene

    est, obs, det, gt = make_scene(n_objects=3, seed=3, SO3_grid_size=576)
    f1, e1 = est.run_inference_pipeline(obs, detections=det, n_refiner_iterations=2, n_pose_hypotheses=5)
    f2, e2 = est.run_inference_pipeline(obs, detections=det, n_refiner_iterations=2, n_pose_hypotheses=5)
    assert torch.equal(f1.poses, f2.poses)  # deterministic
    assert len(f1) == 3 and sorted(f1.infos["label"]) == sorted(det.infos["label"])
    c = e1["coarse"]["preds"]
    assert len(c) == 3 * 576 and c.infos["hypothesis_id"].tolist() == list(range(576)) * 3
    assert c.infos["bbox_id"].tolist() == [i for i in range(3) for _ in range(576)]
    cf = e1["coarse_filter"]["preds"].infos
    assert len(cf) == 15 and cf.groupby("label").size().tolist() == [5, 5, 5]
    top = c.infos.groupby("label")["coarse_logit"].nlargest(5)
    assert np.allclose(sorted(cf["coarse_logit"]), sorted(top.values))
    R = f1.poses[:, :3, :3]
    assert (R @ R.transpose(1, 2) - torch.eye(3, device="cuda")).abs().max() < 1e-4
    best = e1["scoring"]["preds"].infos.groupby("label")["pose_logit"].max()
    assert np.allclose(sorted(f1.infos["pose_logit"]), sorted(best.values))
    # strict_batching (reference batch sizes) gives the same result as the large-launch schedule
    est.strict_batching = True
    f3, _ = est.run_inference_pipeline(obs, detections=det, n_refiner_iterations=2, n_pose_hypotheses=5, bsz_images=128, bsz_objects=8)
    assert (f3.poses - f1.poses).abs().max() < 5e-5


def test_rgbd_and_wide_resnet_pipeline_vs_oracle():
    """config 3 structure: RGBD refiner (32 ch, depth normalisation + validity rule) on WideResNet34, vs the CPU oracle."""
    from megapose6d_amd import mesh_io
    from tests.support import synthetic as syn
    from megapose6d_amd.mesh_db import MeshDataBase
    from megapose6d_amd.pose_estimator import load_SO3_grid
    from tests.support.scene import make_scene
    from oracle import pipeline as op
    from oracle import raster as orr

    tmp = tempfile.mkdtemp(prefix="mp_rgbd_")
    est, obs, det, gt = make_scene(n_objects=2, seed=5, backbone="resnet34", rgbd=True, SO3_grid_size=72, tmp_dir=tmp)
    final, extra = est.run_inference_pipeline(obs, detections=det, n_refiner_iterations=2, n_pose_hypotheses=1)
    ds = syn.make_object_dataset(tmp, n_objects=2, seed=5)
    meshes = {o.label: mesh_io.load_rigid_object(o) for o in ds.list_objects}
    db = MeshDataBase.from_object_ds(ds).batched()
    rend = orr.OracleBatchRenderer(meshes)
    preds = {}
    for role, seed in (("coarse", 11), ("refiner", 12)):
        cfg = syn.make_cfg(role, "resnet34", rgbd=(role == "refiner"))
        head, n_out = ("pose", 9) if role == "refiner" else ("logits", 1)
        preds[role] = op.OraclePosePredictor(cfg, syn.make_state_dict("resnet34", syn.n_inputs_for(cfg), head, n_out, seed=seed),
                                             db.labels.tolist(), db.points, rend)
    oest = op.OraclePoseEstimator(preds["coarse"], preds["refiner"], load_SO3_grid(72), bsz=24)
    res = oest.run(obs.images.cpu(), obs.K.cpu(), det.infos.copy(), det.bboxes.cpu(), n_refiner_iterations=2, n_pose_hypotheses=1)
    lg = extra["coarse"]["data"]["logits"].flatten().cpu()
    scale = max(1.0, res["coarse_logits"].abs().max().item())
    assert_logits_close(lg.numpy(), res["coarse_logits"].numpy(), scale)
    assert extra["coarse_filter"]["preds"].infos["hypothesis_id"].tolist() == res["filtered_infos"]["hypothesis_id"].tolist()
    for n in range(2):
        p = extra["refiner_all_hypotheses"]["preds"][f"iteration={n + 1}"].poses.cpu()
        assert (p - res["refiner_poses"][n]).abs().max().item() < 1e-4
    assert (final.poses.cpu() - res["final_TCO"]).abs().max().item() < 1e-4


def test_smoke_entry():
    import __graft_entry__ as ge

    ge.smoke()


def _dist_worker(rank, world, port, q, backend="gloo"):
    import os

    local = rank if backend == "nccl" else 0
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(local),
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist

    from tests.support.scene import make_scene

    torch.cuda.set_device(local)
    # gloo: both ranks share the single test GPU (RCCL needs one device per rank); nccl: one GPU per rank, RCCL all-gathers
    dist.init_process_group(backend, rank=rank, world_size=world)
    from megapose6d_amd import distributed as mpd

    est, obs, det, _ = make_scene(n_objects=2, seed=7, SO3_grid_size=72, distributed=True)
    mpd.stats.reset()
    final, extra = est.run_inference_pipeline(obs, detections=det, n_refiner_iterations=2, n_pose_hypotheses=3)
    q.put((rank, final.poses.cpu().numpy(), extra["coarse"]["data"]["logits"].cpu().numpy(), final.infos["hypothesis_id"].tolist(),
           mpd.stats.calls))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("backend", ["gloo", "nccl"])
def test_row_sharded_pipeline_two_ranks_matches_single_rank(backend):
    """the N>1 path (rows rank::world + one all-gather per stage) must reproduce the single-rank result exactly;
    `nccl` (= RCCL, all_gather_into_tensor on device buffers) needs two visible GPUs and is skipped on a 1-GPU box"""
    import os

    if backend == "nccl" and torch.cuda.device_count() < 2:
        pytest.skip("RCCL needs one GPU per rank; this box has %d" % torch.cuda.device_count())

    import torch.multiprocessing as mp

    from tests.support.scene import make_scene

    est, obs, det, _ = make_scene(n_objects=2, seed=7, SO3_grid_size=72)
    f1, e1 = est.run_inference_pipeline(obs, detections=det, n_refiner_iterations=2, n_pose_hypotheses=3)
    ref_pose, ref_logits = f1.poses.cpu().numpy(), e1["coarse"]["data"]["logits"].cpu().numpy()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29700 + os.getpid() % 1000
    procs = [ctx.Process(target=_dist_worker, args=(r, 2, port, q, backend)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=600) for _ in range(2)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=120)
    for rank, pose, logits, hyp, n_gathers in res:
        assert n_gathers == 3, n_gathers  # coarse, refiner (all iterations packed), scoring -- one all-gather each
        assert np.abs(logits - ref_logits).max() < 5e-5 * max(1.0, np.abs(ref_logits).max())
        assert hyp == f1.infos["hypothesis_id"].tolist()
        assert np.abs(pose - ref_pose).max() < 5e-5
    assert np.array_equal(res[0][1], res[1][1])  # every rank returns the identical full result


def test_bench_self_launches_two_ranks_over_rccl():
    """`python bench.py --gpus 2` outside torchrun must spawn its own ranks (torch.distributed.run, backend nccl) and print ONE line
    with n_gpus = 2 and the RCCL world size; skipped on a 1-GPU box"""
    import json
    import subprocess
    import sys

    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    root = Path(__file__).resolve().parent.parent
    p = subprocess.run([sys.executable, str(root / "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "1", "--no-extras", "--no-cpu-baseline"],
                       capture_output=True, text=True, timeout=1500)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["rccl"]["backend"] == "nccl" and j["rccl"]["world_size"] == 2 and j["rccl"]["all_gathers_per_step"] >= 3
    assert j["config"]["objects"] == 2


def test_bench_multi_rank_code_path_with_two_ranks_on_one_gpu():
    import os
    """The world > 1 path of bench.py (row sharding, the three all-gathers per step, max-over-ranks timing, the per-rank diagnostic rows,
    the host-share estimate) exactly as the driver launches it -- `python -m torch.distributed.run --nproc-per-node 2 ... bench.py
    --gpus 2` -- on the one GPU a test box has: MP_BENCH_SHARED_GPU=1 puts both ranks on GPU 0 and swaps RCCL for gloo (a test rig, not a
    measurement).  `--full` adds the cross-rank pose check, the per-rank rows and the strong-scaling companion asserted below.  The RCCL
    variant of the same call is test_bench_self_launches_two_ranks_over_rccl (needs two GPUs)."""
    import json
    import subprocess
    import sys

    root = Path(__file__).resolve().parent.parent
    env = dict(os.environ, MP_BENCH_SHARED_GPU="1")
    port = 29800 + os.getpid() % 1000
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           str(root / "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "1", "--full", "--no-cpu-baseline"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=2400, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["scaling"] == "weak" and j["config"]["objects"] == 2
    assert j["rccl"]["backend"] == "gloo" and j["rccl"]["world_size"] == 2 and j["rccl"]["all_gathers_per_step"] == 3
    assert j["rccl"]["final_poses_identical_across_ranks"] is True
    # the strong-scaled companion (BASELINE configs[3]: 64 detections, K = 5) measured in the same launch by both ranks
    sc = j["strong_scaling_config4"]
    assert "error" not in sc, sc
    assert sc["scaling"] == "strong" and sc["n_gpus"] == 2 and sc["all_gathers_per_step"] == 3 and sc["refiner_rows_per_rank"] == 160
    assert sc["pose_hypotheses_per_s"] > 0
    assert [r["rank"] for r in j["per_rank"]] == [0, 1] and all(r["timed_region_ms_per_step"] > 0 for r in j["per_rank"])
    assert 0.0 < j["host"]["replicated_topk_ms_per_step"] < 200.0


def test_bench_plain_run_prints_the_headline_line_only(tmp_path):
    """a plain `python bench.py --gpus 1 --steps N --warmup W` times the steps, writes --dump-outputs and prints the headline line; what
    runs after the timed steps beyond that (stage split, clock probe, extras, CPU baseline + parity) waits for --full"""
    import json
    import subprocess
    import sys

    root = Path(__file__).resolve().parent.parent
    p = subprocess.run([sys.executable, str(root / "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "1", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    j = json.loads(lines[0])
    assert j["unit"] == "pose-hypotheses/s" and j["higher_is_better"] is True and j["metric"] and j["dtype"].startswith("f32")
    assert j["steps"] == 1 and j["warmup"] == 1 and j["value"] > 0
    assert abs(j["value"] - j["config"]["objects"] * 576 / (j["ms_per_step"] * 1e-3)) < 1e-6 * j["value"]
    assert j["roofline"]["frac"] > 0 and j["roofline"]["clock"]["probe_fp32_mfma_mhz"] is None
    assert not {"stage_s", "extras", "cpu_baseline", "parity", "vs_cpu_baseline", "cpu_baseline_1thread"} & set(j)
    assert (tmp_path / "final.poses.npy").is_file()


def test_bench_refuses_more_gpus_than_visible():
    import subprocess
    import sys

    root = Path(__file__).resolve().parent.parent
    n = torch.cuda.device_count() + 1
    p = subprocess.run([sys.executable, str(root / "bench.py"), "--gpus", str(n)], capture_output=True, text=True, timeout=600)
    assert p.returncode != 0 and "GPU(s) visible" in (p.stderr + p.stdout)

"""CPU: the host side of BOP's result files (megapose6d_amd/bop_files.py) -- the 6D results CSV as literal text, its name and its round
trip; the detection JSON assembled from ready-made RLE dicts and read back.  The masks' encoding itself is tests/test_rle_contract_cpu.py
(format) and tests/test_gpu_rle.py (kernels)."""
import json

import numpy as np
import pandas as pd
import pytest
import torch

from megapose6d_amd import bop_files as bf
from megapose6d_amd.tcoll import PandasTensorCollection
from megapose6d_amd.types import assert_detections_valid


def _two_poses():
    # every number is a short binary fraction, so its product with 1e3 in float32 and its decimal form are exact
    T = torch.eye(4).repeat(2, 1, 1)
    T[0, :3, :3] = torch.tensor([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    T[0, :3, 3] = torch.tensor([0.5, -0.125, 1.25])
    T[1, :3, :3] = torch.tensor([[0.5, 0.0, 0.25], [0.0, 1.0, 0.0], [-0.25, 0.0, 0.5]])
    T[1, :3, 3] = torch.tensor([0.0, 0.25, 2.0])
    infos = pd.DataFrame(dict(label=["obj_000005", "ycbv-obj_000012"], scene_id=[48, 49], view_id=[1, 733], score=[0.5, 0.25], pose_score=[0.75, 0.125]))
    return PandasTensorCollection(infos, poses=T)


def test_results_csv_is_the_toolkits_text(tmp_path):
    preds = _two_poses()
    path = bf.save_bop_results(tmp_path / "sub" / "a.csv", preds)
    assert path.read_text() == ("scene_id,im_id,obj_id,score,R,t,time\n"
                                "48,1,5,0.75,0.0 -1.0 0.0 1.0 0.0 0.0 0.0 0.0 1.0,500.0 -125.0 1250.0,-1\n"
                                "49,733,12,0.125,0.5 0.0 0.25 0.0 1.0 0.0 -0.25 0.0 0.5,0.0 250.0 2000.0,-1")
    # the detection score instead of the pose score; times per row and per image
    text = bf.save_bop_results(tmp_path / "b.csv", preds, use_pose_score=False, times=[0.5, 2.0]).read_text().splitlines()
    assert text[1].startswith("48,1,5,0.5,") and text[1].endswith(",0.5") and text[2].startswith("49,733,12,0.25,") and text[2].endswith(",2.0")
    text = bf.save_bop_results(tmp_path / "c.csv", preds, times={(48, 1): 1.5, (49, 733): -1}).read_text().splitlines()
    assert text[1].endswith(",1.5") and text[2].endswith(",-1")
    with pytest.raises(ValueError):
        bf.save_bop_results(tmp_path / "d.csv", PandasTensorCollection(preds.infos.drop(columns="pose_score"), poses=preds.poses))


def test_results_name():
    assert bf.bop_results_name("refiner/final", "ycbv", "test") == "refiner-final_ycbv-test.csv"
    assert bf.bop_results_name("megapose_1.0/coarse_rgb", "tless", "test_primesense") == "megapose-1.0-coarse-rgb_tless-test_primesense.csv"


def test_results_csv_round_trip(tmp_path):
    """R comes back bit for bit (`str` of a float reads back to the same double, which holds the float32 exactly).  t is multiplied by
    1e3 in float32 (one rounding, 2^-24 relative), divided by 1e3 in float64 (negligible) and rounded to float32 once more (2^-24):
    within 2^-23 of its magnitude."""
    g = torch.Generator().manual_seed(0)
    n = 40
    poses = torch.eye(4).repeat(n, 1, 1)
    poses[:, :3, :3] = torch.linalg.qr(torch.randn(n, 3, 3, generator=g))[0]
    poses[:, :3, 3] = torch.randn(n, 3, generator=g) * torch.tensor([0.3, 0.3, 1.0])
    infos = pd.DataFrame(dict(label=[f"obj_{i % 21 + 1:06d}" for i in range(n)], scene_id=np.arange(n) // 7 + 48, view_id=np.arange(n) * 3,
                              pose_score=torch.rand(n, generator=g).numpy(), time=np.arange(n) * 0.25))
    back = bf.load_bop_results(bf.save_bop_results(tmp_path / bf.bop_results_name("m", "ycbv", "test"), PandasTensorCollection(infos, poses=poses)))
    assert back.poses.dtype == torch.float32 and torch.equal(back.poses[:, :3, :3], poses[:, :3, :3]) and torch.equal(back.poses[:, 3], poses[:, 3])
    assert bool(((back.poses[:, :3, 3] - poses[:, :3, 3]).abs() <= poses[:, :3, 3].abs() * 2.0 ** -23).all())
    assert back.infos["label"].tolist() == infos["label"].tolist() and back.infos["scene_id"].tolist() == infos["scene_id"].tolist()
    assert back.infos["view_id"].tolist() == infos["view_id"].tolist() and back.infos["time"].tolist() == infos["time"].tolist()
    assert np.array_equal(back.infos["pose_score"].to_numpy(), infos["pose_score"].to_numpy().astype(np.float64))
    with pytest.raises(ValueError):
        (tmp_path / "bad.csv").write_text("scene_id,im_id\n1,2")
        bf.load_bop_results(tmp_path / "bad.csv")


def _detections():
    infos = pd.DataFrame(dict(label=["obj_000002", "obj_000002", "obj_000015"], score=[0.5, 0.25, 0.875], scene_id=[3, 3, 4], view_id=[10, 10, 7],
                              batch_im_id=[0, 0, 1]))
    return PandasTensorCollection(infos, bboxes=torch.tensor([[1.0, 2.0, 4.0, 6.5], [0.0, 0.0, 2.0, 3.0], [0.5, 1.0, 1.5, 3.0]]))


def test_detection_records_from_ready_made_rle(tmp_path):
    segs = [{"size": [3, 2], "counts": [1, 1, 1, 2, 1]}, {"size": [3, 2], "counts": "06"}, {"size": [3, 2], "counts": np.array([6], np.int32)}]
    path = bf.save_bop_detections(tmp_path / "det.json", _detections(), segmentations=segs)
    assert json.loads(path.read_text()) == [
        dict(scene_id=3, image_id=10, category_id=2, bbox=[1.0, 2.0, 3.0, 4.5], score=0.5, time=-1, segmentation={"size": [3, 2], "counts": [1, 1, 1, 2, 1]}),
        dict(scene_id=3, image_id=10, category_id=2, bbox=[0.0, 0.0, 2.0, 3.0], score=0.25, time=-1, segmentation={"size": [3, 2], "counts": "06"}),
        dict(scene_id=4, image_id=7, category_id=15, bbox=[0.5, 1.0, 1.0, 2.0], score=0.875, time=-1, segmentation={"size": [3, 2], "counts": [6]})]
    assert bf.rle_from_string("06") == [0, 6]
    plain = bf.detection_records(_detections())
    assert all("segmentation" not in r for r in plain) and [r["bbox"] for r in plain] == [[1.0, 2.0, 3.0, 4.5], [0.0, 0.0, 2.0, 3.0], [0.5, 1.0, 1.0, 2.0]]
    with pytest.raises(ValueError):
        bf.detection_records(_detections(), segs[:2])


def test_load_detections_without_masks(tmp_path):
    det = _detections()
    path = bf.save_bop_detections(tmp_path / "det.json", det)
    back = bf.load_bop_detections(path)
    assert_detections_valid(back)
    assert "masks" not in back.tensors and back.bboxes.dtype == torch.float32 and torch.equal(back.bboxes, det.bboxes)
    assert list(back.infos.columns) == ["label", "score", "scene_id", "view_id", "batch_im_id", "time", "instance_id"]
    for col in ("label", "score", "scene_id", "view_id", "batch_im_id"):
        assert back.infos[col].tolist() == det.infos[col].tolist(), col
    assert back.infos["instance_id"].tolist() == [0, 1, 0] and back.infos["time"].tolist() == [-1.0] * 3
    # records instead of a path, view_id for image_id, another label format, batch_im_id from the caller's mapping
    records = [dict(scene_id=1, view_id=5, category_id=3, bbox=[0, 0, 2, 2], score=1), dict(scene_id=1, image_id=4, category_id=3, bbox=[1, 1, 1, 1], score=0.5)]
    got = bf.load_bop_detections(records, label_format="ycbv-obj_{:06d}", image_key={(1, 5): 7, (1, 4): 2})
    assert got.infos["label"].tolist() == ["ycbv-obj_000003"] * 2 and got.infos["batch_im_id"].tolist() == [7, 2] and got.infos["view_id"].tolist() == [5, 4]
    assert "time" not in got.infos and got.bboxes.tolist() == [[0.0, 0.0, 2.0, 2.0], [1.0, 1.0, 2.0, 2.0]]
    assert bf.load_bop_detections(records).infos["batch_im_id"].tolist() == [0, 1]                  # file order
    with pytest.raises(ValueError, match="image_key"):
        bf.load_bop_detections(records, image_key={(1, 5): 0})
    assert len(bf.load_bop_detections([])) == 0


def test_a_malformed_rle_names_its_record():
    """what the host can see without decoding: a string that is no RLE string, counts that are no integers, a segmentation without a size"""
    ok = dict(scene_id=1, image_id=2, category_id=3, bbox=[0, 0, 1, 1], score=1.0, segmentation={"size": [3, 2], "counts": [6]})
    for seg in ({"size": [3, 2], "counts": "P"}, {"size": [3, 2], "counts": [1.5, 4.5]}, {"counts": [6]}, [[0, 0, 1, 1, 2, 2]]):
        with pytest.raises(ValueError, match="record 1 "):
            bf.load_bop_detections([ok, dict(ok, segmentation=seg)])
    with pytest.raises(ValueError, match="share one size"):
        bf.rle_to_masks([{"size": [3, 2], "counts": [6]}, {"size": [2, 3], "counts": [6]}], "cpu")

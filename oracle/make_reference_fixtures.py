"""Generate the fixtures that pin the drop-in claims to the REFERENCE's own Python (imported read-only via oracle/ref_import.py).
CONTAINER-ONLY, like oracle/make_golden.py; the outputs are committed so that the pinning tests run anywhere.

    python -m oracle.make_reference_fixtures

Files
  reference_api.json    public signatures of the drop-in classes / functions (CLASSES, FUNCTIONS below), the public names of the
                        modules INTEGRATION.md's monkey-patch block assigns to, and the reference Detector.get_detections tables for
                        the fake-model cases of tests/_ref_api_check.py
  reference_api.npz     the array outputs of those Detector cases (bboxes, masks) and of Detector.image_tensor_from_numpy
  reference_icp.npz     the reference's getXYZ / get_normal / compute_masks / icp_refinement (cv2.inpaint and cv2.ppf_match_3d_ICP
                        replaced by the oracle's stand-ins) on the scenes of tests/_ref_icp_check.py; the full-frame maps as digests
"""
from __future__ import annotations

import inspect
import json
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
GOLD = ROOT / "tests" / "golden"

# (reference module, class) -> methods whose signatures the engine must reproduce
CLASSES = {
    ("megapose.inference.pose_estimator", "PoseEstimator"): ["__init__", "load_SO3_grid", "forward_refiner", "forward_scoring_model",
                                                             "forward_coarse_model", "forward_detection_model", "run_depth_refiner",
                                                             "run_inference_pipeline", "filter_pose_estimates"],
    ("megapose.models.pose_rigid", "PosePredictor"): ["__init__", "crop_inputs", "compute_crops_multiview", "update_pose", "net_forward",
                                                      "render_images_multiview", "normalize_images", "normalize_depth", "forward",
                                                      "forward_coarse_tensor", "forward_coarse"],
    ("megapose.panda3d_renderer.panda3d_batch_renderer", "Panda3dBatchRenderer"): ["__init__", "render", "stop"],
    ("megapose.inference.icp_refiner", "ICPRefiner"): ["__init__", "refine_poses"],
    ("megapose.inference.depth_refiner", "DepthRefiner"): ["refine_poses"],
    ("megapose.datasets.object_dataset", "RigidObject"): ["__init__", "make_symmetry_poses"],
    ("megapose.datasets.object_dataset", "RigidObjectDataset"): ["__init__", "__getitem__", "get_object_by_label", "__len__", "filter_objects"],
    ("megapose.inference.detector", "Detector"): ["__init__", "image_tensor_from_numpy", "get_detections"],
}
FUNCTIONS = {"create_model_pose": ("megapose.training.pose_models_cfg", "create_model_pose"),
             "load_named_model": ("megapose.utils.load_model", "load_named_model"),
             "load_pose_models": ("megapose.inference.utils", "load_pose_models")}
PATCHED_MODULES = ["megapose.panda3d_renderer.panda3d_batch_renderer", "megapose.inference.utils", "megapose.utils.load_model",
                   "megapose.inference.pose_estimator", "megapose.inference.icp_refiner"]


def signature(fn) -> list:
    """[{name, kind, has_default, default | default_repr}] without `self`; plain defaults by value, others by repr (the data directory
    the reference reads from MEGAPOSE_DATA_DIR written as {MEGAPOSE_DATA_DIR})"""
    data_dir = os.environ["MEGAPOSE_DATA_DIR"]
    out = []
    for p in inspect.signature(fn).parameters.values():
        if p.name == "self":
            continue
        d = {"name": p.name, "kind": p.kind.name, "has_default": p.default is not inspect.Parameter.empty}
        if d["has_default"]:
            if p.default is None or type(p.default) in (bool, int, float, str):
                d["default"] = p.default
            else:
                d["default_repr"] = repr(p.default).replace(data_dir, "{MEGAPOSE_DATA_DIR}")
        out.append(d)
    return out


def api_fixture():
    import importlib

    from _ref_api_check import DETECTOR_CASES, FakeMaskRCNN, detector_images, detector_u8

    sigs = {}
    for (mod, cls), methods in CLASSES.items():
        c = getattr(importlib.import_module(mod), cls)
        for m in methods:
            sigs[f"{cls}.{m}"] = signature(getattr(c, m))
    for name, (mod, fn) in FUNCTIONS.items():
        sigs[name] = signature(getattr(importlib.import_module(mod), fn))
    modules = {m: sorted(n for n in dir(importlib.import_module(m)) if not n.startswith("_")) for m in PATCHED_MODULES}

    import megapose.inference.detector as r_det
    from megapose.inference.types import ObservationTensor as RObs

    images = detector_images()
    cases, arrays = [], {}
    for i, (per_image, kw) in enumerate(DETECTOR_CASES):
        case = {"per_image": per_image, "kw": kw}
        try:
            a = r_det.Detector(FakeMaskRCNN(per_image)).get_detections(RObs(images=images), **kw)
        except Exception as e:  # noqa: BLE001
            case["error"] = f"{type(e).__name__}: {e}"
            cases.append(case)
            continue
        da = a.infos.reset_index(drop=True)
        case["n"] = len(da)
        case["columns"] = {c: da[c].tolist() for c in da.columns}
        arrays[f"case{i}_bboxes"] = a.bboxes.float().cpu().numpy()
        if kw.get("output_masks") and sum(per_image):
            arrays[f"case{i}_masks"] = a.masks.cpu().numpy()
        cases.append(case)
    arrays["image_tensor_from_numpy"] = r_det.Detector(FakeMaskRCNN([1])).image_tensor_from_numpy(detector_u8()).numpy()
    return {"signatures": sigs, "module_names": modules, "detector_cases": cases}, arrays


def icp_fixture():
    import megapose.inference.icp_refiner as r_icp
    import megapose.inference.refiner_utils as r_ru

    from _ref_icp_check import array_digest, icp_cases, install_cv2_stand_ins

    install_cv2_stand_ins(r_icp)
    out = {}
    for n, (dm, dr, K, init) in enumerate(icp_cases()):
        fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
        out[f"s{n}_getXYZ"] = array_digest(r_icp.getXYZ(dm, fx, fy, cx, cy))
        for refine in (False, True):
            out[f"s{n}_get_normal_{int(refine)}"] = array_digest(r_icp.get_normal(dm, fx=fx, fy=fy, cx=cx, cy=cy, refine=refine))
        mr, mm = r_ru.compute_masks("threshold", dr, dm, 0.1)
        out[f"s{n}_mask_rendered"], out[f"s{n}_mask_measured"] = np.packbits(mr), np.packbits(mm)
        T_ref, rv_ref = r_icp.icp_refinement(dm, dr, mm, K, init, n_min_points=1000)
        out[f"s{n}_T"], out[f"s{n}_retval"] = np.asarray(T_ref, dtype=np.float32), np.asarray(rv_ref)
    return out


def main():
    from oracle import ref_import

    ref_import.install()
    GOLD.mkdir(parents=True, exist_ok=True)
    meta, arrays = api_fixture()
    (GOLD / "reference_api.json").write_text(json.dumps(meta, indent=1, sort_keys=True) + "\n")
    np.savez_compressed(GOLD / "reference_api.npz", **arrays)
    print("reference_api.json / .npz done")
    np.savez_compressed(GOLD / "reference_icp.npz", **icp_fixture())
    print("reference_icp.npz done")


if __name__ == "__main__":
    main()

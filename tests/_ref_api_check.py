"""Run in a SUBPROCESS by tests/test_reference_api_cpu.py.
(i) diffs every public signature of the drop-in classes against the reference's, (i-b) runs Detector.get_detections on fake-model cases
and compares with the reference's tables, (ii) executes the monkey-patch block of INTEGRATION.md verbatim against modules carrying the
reference modules' public names and checks that each patched attribute now resolves to the engine's object.  The reference side was
recorded by `python -m oracle.make_reference_fixtures` from the reference's own Python: tests/golden/reference_api.json / .npz.
Prints a JSON list of problems (empty = OK)."""
import ast
import inspect
import json
import os
import re
import sys
import types
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
GOLD = ROOT / "tests" / "golden"
# defaults derived from the data directory are compared with the reference's for the same MEGAPOSE_DATA_DIR (main() sets it before
# megapose6d_amd is imported)
DATA_DIR = "megapose_data_dir"

# the cases of the behaviour check; the reference itself raises on an empty frame with one_instance_per_class or detection_th
# (groupby/score on empty columns), so those are not cases
DETECTOR_CASES = [(per_image, kw) for per_image in ([4, 0, 6], [0, 0, 0], [1, 1, 1])
                  for kw in (dict(), dict(detection_th=0.4), dict(output_masks=True, mask_th=0.5), dict(one_instance_per_class=True),
                             dict(detection_th=0.3, output_masks=True, one_instance_per_class=True))
                  if not (sum(per_image) == 0 and (kw.get("one_instance_per_class") or kw.get("detection_th") is not None))]


class FakeMaskRCNN(torch.nn.Module):
    """deterministic stand-in with torchvision's Mask R-CNN output format"""

    def __init__(self, per_image):
        super().__init__()
        self.config = types.SimpleNamespace(label_to_category_id={"ycbv-obj_000001": 1, "ycbv-obj_000002": 2, "ycbv-obj_000005": 3})
        self.per_image = per_image

    def forward(self, images):
        outs = []
        for n, im in enumerate(images):
            k = self.per_image[n]
            g = torch.Generator().manual_seed(100 + n)
            xy = torch.rand(k, 2, generator=g) * 200
            wh = torch.rand(k, 2, generator=g) * 100 + 5
            outs.append(dict(boxes=torch.cat([xy, xy + wh], 1), labels=torch.randint(1, 4, (k,), generator=g),
                             scores=torch.rand(k, generator=g), masks=torch.rand(k, 1, *im.shape[-2:], generator=g)))
        return outs


def detector_images() -> torch.Tensor:
    return torch.from_numpy(np.random.RandomState(0).rand(3, 3, 24, 32).astype(np.float32))


def detector_u8() -> np.ndarray:
    return (np.random.RandomState(1).rand(5, 7, 3) * 255).astype(np.uint8)


def diff(problems, name, ref_params, our_fn):
    """ref_params: the reference's parameters as recorded by oracle/make_reference_fixtures.signature"""
    var = ("VAR_KEYWORD", "VAR_POSITIONAL")
    op = [p for p in inspect.signature(our_fn).parameters.values() if p.name != "self"]
    for i, r in enumerate(ref_params):
        if r["kind"] in var:
            if not any(o.kind.name == r["kind"] for o in op):
                problems.append(f"{name}: missing *{r['name']}")
            continue
        if i >= len(op) or op[i].name != r["name"]:
            problems.append(f"{name}: parameter {i} is {op[i].name if i < len(op) else None!r}, reference has {r['name']!r}")
            continue
        if r["has_default"]:
            d = op[i].default
            if "default_repr" in r:
                if d is inspect.Parameter.empty or repr(d) != r["default_repr"].replace("{MEGAPOSE_DATA_DIR}", DATA_DIR):
                    problems.append(f"{name}: default of {r['name']!r} is {d!r}, reference {r['default_repr']}")
            elif d != r["default"]:
                problems.append(f"{name}: default of {r['name']!r} is {d!r}, reference {r['default']!r}")
        # a default where the reference has none is a superset
    fixed = [r for r in ref_params if r["kind"] not in var]
    for o in op[len(fixed):]:  # engine extensions: must be optional
        if o.kind.name in var:
            continue
        if o.default is inspect.Parameter.empty:
            problems.append(f"{name}: extra parameter {o.name!r} has no default")


def check_signatures(problems, sigs):
    import megapose6d_amd as mp
    from megapose6d_amd import detector as o_det

    ours = {"PoseEstimator": mp.pose_estimator.PoseEstimator, "PosePredictor": mp.pose_rigid.PosePredictor,
            "Panda3dBatchRenderer": mp.renderer.Panda3dBatchRenderer, "ICPRefiner": mp.icp_refiner.ICPRefiner,
            "DepthRefiner": mp.icp_refiner.DepthRefiner, "RigidObject": mp.object_dataset.RigidObject,
            "RigidObjectDataset": mp.object_dataset.RigidObjectDataset, "Detector": o_det.Detector}
    functions = {"create_model_pose": mp.load_model.create_model_pose, "load_named_model": mp.load_model.load_named_model,
                 "load_pose_models": mp.load_model.load_pose_models}
    for name, ref_params in sorted(sigs.items()):
        if name in functions:
            diff(problems, name, ref_params, functions[name])
            continue
        cls, m = name.split(".", 1)
        if not hasattr(ours[cls], m):
            problems.append(f"{name}: missing")
            continue
        diff(problems, name, ref_params, getattr(ours[cls], m))
    for want in list(ours) + list(functions):
        if not any(k == want or k.startswith(want + ".") for k in sigs):
            problems.append(f"{want}: absent from the fixture")


def check_detector(problems, cases, arrays):
    """Detector.get_detections (row f-4) on the fake model vs the reference's tables"""
    from megapose6d_amd import detector as o_det
    from megapose6d_amd.types import ObservationTensor as OObs

    images = detector_images()
    if [(c["per_image"], c["kw"]) for c in cases] != [(p, kw) for p, kw in DETECTOR_CASES]:
        problems.append("Detector cases of the fixture differ from DETECTOR_CASES: regenerate it")
        return
    for i, (per_image, kw) in enumerate(DETECTOR_CASES):
        c = cases[i]
        tag = f"Detector.get_detections per_image={per_image} {kw}"
        if "error" in c:
            problems.append(f"{tag}: the reference raised {c['error']}")
            continue
        try:
            b = o_det.Detector(FakeMaskRCNN(per_image)).get_detections(OObs(images=images), **kw)
        except Exception as e:  # noqa: BLE001
            problems.append(f"{tag}: raised {type(e).__name__}: {e}")
            continue
        db = b.infos.reset_index(drop=True)
        if c["n"] != len(db):
            problems.append(f"{tag}: {len(db)} detections, reference {c['n']}")
            continue
        if c["n"] == 0:   # empty result: pandas gives the reference no instance_id column at all; ours keeps the (empty) column
            db = db.drop(columns=["instance_id"], errors="ignore")
        if sorted(c["columns"]) != sorted(db.columns):
            problems.append(f"{tag}: columns {sorted(db.columns)}, reference {sorted(c['columns'])}")
            continue
        for col, va in c["columns"].items():
            vb = db[col].tolist()
            if col == "score":
                if not np.allclose(va, vb, atol=1e-7):
                    problems.append(f"{tag}: scores differ")
            elif va != vb:
                problems.append(f"{tag}: column {col}: {vb} vs reference {va}")
        if not np.array_equal(arrays[f"case{i}_bboxes"], b.bboxes.cpu().numpy()):
            problems.append(f"{tag}: bboxes differ")
        if kw.get("output_masks") and sum(per_image):
            ref_m, got_m = arrays[f"case{i}_masks"], b.masks.cpu().numpy()
            if ref_m.dtype != got_m.dtype or not np.array_equal(ref_m, got_m):
                problems.append(f"{tag}: masks differ")
    got = o_det.Detector(FakeMaskRCNN([1])).image_tensor_from_numpy(detector_u8()).numpy()
    ref = arrays["image_tensor_from_numpy"]
    if got.dtype != ref.dtype or not np.array_equal(got, ref):
        problems.append("Detector.image_tensor_from_numpy differs")


def check_integration_patch(problems, module_names):
    """INTEGRATION.md monkey-patch block, executed verbatim against stand-in `megapose` modules that carry exactly the public names of
    the reference modules (each bound to a placeholder)"""
    import megapose6d_amd as mp

    md = (ROOT / "INTEGRATION.md").read_text()
    blocks = re.findall(r"```python\n(.*?)```", md, flags=re.S)
    patch = next((b for b in blocks if "sitecustomize" in b), None)
    if patch is None:
        problems.append("INTEGRATION.md: monkey-patch block not found")
        return
    code = "\n".join(l[3:] if l.startswith("   ") else l for l in patch.splitlines())
    for full, names in module_names.items():
        parts = full.split(".")
        for k in range(1, len(parts) + 1):
            name = ".".join(parts[:k])
            if name not in sys.modules:
                sys.modules[name] = types.ModuleType(name)
                if k > 1:
                    setattr(sys.modules[".".join(parts[:k - 1])], parts[k - 1], sys.modules[name])
        for n in names:
            setattr(sys.modules[full], n, type(n, (), {"__module__": full}))
    # every name the patch assigns to must exist in the reference module beforehand (no typo'd attribute)
    aliases = {}
    for node in ast.walk(ast.parse(code)):
        if isinstance(node, ast.Import):
            aliases.update({a.asname or a.name: a.name for a in node.names})
        elif isinstance(node, ast.Assign):
            for t in node.targets:
                if isinstance(t, ast.Attribute) and isinstance(t.value, ast.Name) and aliases.get(t.value.id, "").startswith("megapose."):
                    mod = aliases[t.value.id]
                    if t.attr not in module_names.get(mod, []):
                        problems.append(f"INTEGRATION.md patch assigns {mod}.{t.attr}, which the reference module does not have")
    ns = {}
    try:
        exec(compile(code, "INTEGRATION.md", "exec"), ns)
    except Exception as e:  # noqa: BLE001
        problems.append(f"INTEGRATION.md patch block raised {type(e).__name__}: {e}")
        return
    pbr, iu = sys.modules["megapose.panda3d_renderer.panda3d_batch_renderer"], sys.modules["megapose.inference.utils"]
    lm, pe, icp = sys.modules["megapose.utils.load_model"], sys.modules["megapose.inference.pose_estimator"], sys.modules["megapose.inference.icp_refiner"]
    checks = [(pbr, "Panda3dBatchRenderer", mp.renderer.Panda3dBatchRenderer), (iu, "Panda3dBatchRenderer", mp.renderer.Panda3dBatchRenderer),
              (iu, "create_model_pose", mp.load_model.create_model_pose), (iu, "MeshDataBase", mp.mesh_db.MeshDataBase),
              (pe, "PoseEstimator", mp.pose_estimator.PoseEstimator), (lm, "PoseEstimator", mp.pose_estimator.PoseEstimator),
              (icp, "ICPRefiner", mp.icp_refiner.ICPRefiner), (lm, "ICPRefiner", mp.icp_refiner.ICPRefiner)]
    for mod, attr, want in checks:
        if getattr(mod, attr, None) is not want:
            problems.append(f"after the patch {mod.__name__}.{attr} is not the engine's object")


def main():
    os.environ["MEGAPOSE_DATA_DIR"] = DATA_DIR
    meta = json.loads((GOLD / "reference_api.json").read_text())
    arrays = np.load(GOLD / "reference_api.npz", allow_pickle=False)
    problems = []
    check_signatures(problems, meta["signatures"])
    try:
        check_detector(problems, meta["detector_cases"], arrays)
    except Exception:  # noqa: BLE001
        import traceback

        problems.append("detector behaviour check crashed: " + traceback.format_exc()[-600:])
    check_integration_patch(problems, meta["module_names"])
    print("REF_API_JSON " + json.dumps(problems))


if __name__ == "__main__":
    main()

"""Run in a SUBPROCESS by tests/test_icp_oracles_cpu.py.
Pins oracle/icp_opencv.py to the REFERENCE's own depth-refiner code (src/megapose/inference/icp_refiner.py, refiner_utils.py) wherever
that code does not depend on OpenCV: getXYZ, get_normal, compute_masks and the orchestration of icp_refinement, run by
`python -m oracle.make_reference_fixtures` on the scenes below with the two cv2 calls replaced by the oracle's stand-ins (cv2.inpaint ->
the oracle's hole fill, cv2.ppf_match_3d_ICP -> the oracle's restatement of OpenCV's ICP), are committed as tests/golden/reference_icp.npz
(full-frame maps as digests of their bytes).  Prints a JSON list of problems (empty = OK)."""
import hashlib
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from oracle import icp_opencv as ocv  # noqa: E402
from oracle import raster as orr  # noqa: E402

GOLDEN = ROOT / "tests" / "golden" / "reference_icp.npz"


class _ICP:   # cv2.ppf_match_3d_ICP(iterations, tolerence=, numLevels=) -> .registerModelToScene(src, dst)
    def __init__(self, iterations, tolerence=0.05, rejectionScale=2.5, numLevels=6):
        self.a = (iterations, tolerence, rejectionScale, numLevels)

    def registerModelToScene(self, src, dst):
        return ocv.opencv_icp(src, dst, *self.a)


def install_cv2_stand_ins(r_icp) -> None:
    r_icp.cv2.inpaint = lambda depth, mask, radius, flags: ocv._fill_holes(depth)
    r_icp.cv2.ppf_match_3d_ICP = _ICP


def icp_cases():
    """-> [(depth_measured, depth_rendered at the initial pose, K, initial pose)]: scenes 0-3 and the far-off scene 7"""
    from test_icp_oracles_cpu import make_icp_scenes

    _, scenes = make_icp_scenes(8)
    out = []
    for dm, K, init, gt, mesh, _ in scenes[:4] + [scenes[7]]:
        out.append((dm, orr.render(mesh, init[None], K[None], 480, 640, 2)[2][0], K, init))
    return out


def array_digest(a) -> np.ndarray:
    """sha256 of dtype, shape and bytes (-0.0 folded into +0.0, as np.array_equal does)"""
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "f":
        a = a + a.dtype.type(0)
    h = hashlib.sha256(f"{a.dtype.str}{a.shape}".encode())
    h.update(a.tobytes())
    return np.asarray(h.hexdigest())


def main():
    g = np.load(GOLDEN, allow_pickle=False)
    problems = []
    for n, (dm, dr, K, init) in enumerate(icp_cases()):
        fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]   # numpy float32 scalars, as icp_refinement passes them
        if array_digest(ocv.get_xyz(dm, fx, fy, cx, cy)) != g[f"s{n}_getXYZ"]:
            problems.append(f"scene {n}: getXYZ differs")
        for refine in (False, True):
            if array_digest(ocv.get_normal(dm, fx, fy, cx, cy, refine=refine)) != g[f"s{n}_get_normal_{int(refine)}"]:
                problems.append(f"scene {n}: get_normal(refine={refine}) differs")
        mine = ocv.compute_masks_threshold(dr, dm)
        if not (np.array_equal(np.packbits(mine), g[f"s{n}_mask_measured"]) and np.array_equal(np.packbits(mine), g[f"s{n}_mask_rendered"])):
            problems.append(f"scene {n}: compute_masks differs")
        T_o, rv_o, _ = ocv.icp_refinement(dm, dr, mine, K, init)
        T_ref, rv_ref = g[f"s{n}_T"], int(g[f"s{n}_retval"])
        if rv_ref != rv_o:
            problems.append(f"scene {n}: retval {rv_ref} vs {rv_o}")
        elif rv_o == 0 and not np.array_equal(T_ref, T_o):
            problems.append(f"scene {n}: refined pose differs (max {np.abs(T_ref - T_o).max():.3e})")
    print("REF_ICP_JSON " + json.dumps(problems))


if __name__ == "__main__":
    main()

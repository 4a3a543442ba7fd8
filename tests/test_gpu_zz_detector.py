"""-m gpu: the detector network on the HIP engine (csrc/detector.hip through DetectorMaskRCNN / Detector) against the CPU oracle
(oracle/mask_rcnn.py, a restatement of torchvision 0.12's Mask R-CNN inference -- third party, parity unpinned).
Weights and images are hash-generated on both sides (oracle.mask_rcnn.synthetic_*); the oracle's results come from the committed
compact goldens (tests/golden/detector_*.npz) and, for one small case, from a fresh oracle run on the host CPU.
Tolerances: feature maps 8.2e-6 relative to the scale of the golden's subsample (every 4th row and column, every 16th channel) =
2 x (1.6e-6 + 2.5e-6): the float32 oracle that wrote the goldens is off the float64 oracle by at most 1.6e-6 of that scale, and the engine's
whole trunk from x0 is off the float64 oracle by 8.4e-7 of the FULL map's scale (tests/test_gpu_zz_detector_stages.py, "un-forced"), which
is up to 2.98 x the subsample's (measured against the goldens themselves: the "[golden]" lines of the test output, 1.8e-6);
boxes 5e-2 px, scores 2e-4, labels exact; a couple of detections may swap or drop where two scores tie within round-off.
(The same comparison runs torch-free in scripts/microbench/native_detector_check.cpp; its MI355X log is profiles/r02_detector_native_check.txt.)"""
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"
PYRAMID_TOL = 8.2e-6


def _model(C, mn, mx):
    from megapose6d_amd.mask_rcnn import DetectorMaskRCNN
    from oracle import mask_rcnn as om

    m = DetectorMaskRCNN(input_resize=(mn, mx), n_classes=C)
    m.load_state_dict(om.synthetic_state_dict(C))
    return m.cuda().eval()


def _match(boxes, scores, labels, gb, gs, gl):
    """-> number of golden detections that have a twin (same label, score within 2e-4, box within 5e-2 px) among ours"""
    found = 0
    for b, s, l in zip(gb, gs, gl):
        ok = (labels == l) & (np.abs(scores - s) < 2e-4) & (np.abs(boxes - b).max(axis=1) < 5e-2)
        found += bool(ok.any())
    return found


@pytest.mark.parametrize("case", ["native", "resized", "batch2"])
def test_detector_matches_the_oracle_goldens(case):
    from oracle import mask_rcnn as om

    g = np.load(GOLD / f"detector_{case}.npz")
    n, H, W, mn, mx, C = (int(v) for v in g["config"])
    m = _model(C, mn, mx)
    images = om.synthetic_images(n, H, W).cuda()
    out = m(list(images))
    net = m._net()
    for l in range(2, 7):   # pyramid
        f = net.debug_tensor(f"P{l}").cpu().numpy()
        ref = g[f"P{l}_sub"]
        err = float(np.abs(f[:, ::4, ::4, ::16] - ref).max() / max(1.0, np.abs(ref).max()))
        print(f"[golden] {case}: P{l} err {err:.3e}")
        assert err < PYRAMID_TOL, (l, err)
        assert abs(np.abs(f).mean() - float(g[f"P{l}_absmean"][0])) < 1e-4
    props, pcnt = net.debug_tensor("proposals").cpu().numpy(), net.debug_tensor("proposal_counts").cpu().numpy().ravel()
    assert (pcnt == g["proposal_counts"]).all()   # (measured on the MI355X: every proposal identical; tolerances are what is achieved)
    assert np.abs(props[:, :16] - g["proposals_first64"][:, :16]).max() < 5e-2   # the best proposals, in place
    for i in range(n):
        k = int(g["counts"][i])
        o = out[i]
        assert len(o["boxes"]) == k
        assert o["masks"].shape == (len(o["boxes"]), 1, H, W) and o["labels"].dtype == torch.int64
        found = _match(o["boxes"].cpu().numpy(), o["scores"].cpu().numpy(), o["labels"].cpu().numpy(), g["boxes"][i, :k], g["scores"][i, :k], g["labels"][i, :k])
        assert found >= k - 1, (found, k)   # (one slot of slack for an exact score tie at the cut)
        s = o["scores"].cpu().numpy()
        assert (s[:-1] >= s[1:]).all() and 0 <= float(o["masks"].min()) and float(o["masks"].max()) <= 1
    # deterministic
    again = m(list(images))
    assert all(torch.equal(a["boxes"], b["boxes"]) and torch.equal(a["masks"], b["masks"]) for a, b in zip(out, again))

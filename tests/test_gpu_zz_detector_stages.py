"""-m gpu: csrc/detector.hip stage by stage against the CPU oracle (oracle/mask_rcnn.py), teacher-forced: every oracle stage is fed the
ENGINE's own input to that stage (DetectorNet.debug_tensor), so that a difference is the stage's own fault, not an inherited one.

Stages: preprocess (x0 vs om.transform_images), RPN (om.rpn_proposals on the engine's P2..P6, ranked on the engine's own fp32
objectness logits "keys"), box head (om.box_branch on the engine's P2..P5 and proposals), post-processing (om.postprocess_detections on
the engine's class_logits and proposals) and masks (sigmoid, class select and om.paste_masks on the engine's mask_logits and boxes).
Between those: the trunk (x0 -> pool -> C2 -> C3 -> C4 -> C5 -> L5..L2 -> P2..P5, each step from the engine's own tap; P6 is P5[:, ::2, ::2]
bit for bit), RoIAlign (the roi7 / roi14 taps against a float64 RoIAlign of the engine's P2..P5 on its own proposals / detections), the
mask head (roi14 -> the 28 x 28 logits of every class, before the sigmoid and the class selection) and the RPN objectness logits (the
"keys" tap against om.rpn_proposals without the override, every anchor).  Every element of every live row is compared; borders, pad
columns and the rows past a count must be zero (the mask logits past the count: finite).

Arithmetic: continuous operations (resize weights, convolutions / FC of the heads, softmax, sigmoid, box decoding, bilinear paste) run
in float64 from the engine's fp32 inputs; selection decisions are taken on the fp32 values the kernels ranked (the RPN keys, the mask-box
edges, which om.paste_masks truncates from the fp32 boxes exactly as det_mask_paste_kernel does).  The EXACT cases (constant keys from
zeroed weights) run the oracle in float32: there the fp32 IoU / scores are what the kernels compared, and every comparison is exact.

Tolerances (worst errors of the MI355X run in the test output, "[stage]" lines):
  x0             4e-5 abs   fp32 (x - mean) / std and resize weights vs float64: the fp32 source coordinate sy * (y + 0.5) - 0.5
                            (<= 200 px, ulp 1.5e-5) is off by ~1e-5 px on a resized frame, times pixel steps of the normalised noise
                            image of up to ~4 / px (measured 3.0e-5; 2.4e-7 without a resize)
  boxes          Spec.box_tol / post_box_tol px: 3e-3 for the "clip" case, whose decodes form x1 = pcx - pw / 2 from terms of
                            ~2e4 px (fp32 ulp 2e-3; measured 1.95e-3); RPN 2e-4: its deltas come from the oracle's float64 head
                            convolutions vs fp32 MFMA and scale with anchors of up to 512 px (measured 1.2e-4); detections 4e-5: decoded
                            from the engine's own deltas, fp32 vs float64 decoding only (measured 1.7e-5); the exact cases 0
  scores         3e-7 abs   fp32 sigmoid / softmax of the same logits vs float64 (measured 7.6e-8)
  class logits   6e-6 x max(1, |ref|)  the box head's 12544-term fp32 MFMA dot products vs float64 (measured 3.6e-6)
  masks          2e-6 abs   fp32 bilinear source coordinate (30 / w) * (x + 0.5) - 0.5 (<= 30, ulp 1.9e-6) vs float64, times the
                            step between neighbouring 28 x 28 probabilities (measured 1.2e-6 on the "clip" boxes, 660 px wide)
Bounds of the trunk / RoIAlign / mask head / RPN logit stages: max |got - ref| / max(1, max |ref|) of the compared tensor, = 2 x the worst
error of the MI355X run over all specs (the factor covers split-K partitions that depend on the CU count; the inputs are fixed).  "f32"
is the float32 oracle against the float64 one on the same input (CPU, worst spec): beyond 4 x f32 an error counts as a finding.
  pool           1.4e-6   stem 7 x 7 + max pool from x0 (measured 6.8e-7; f32 6.7e-7)
  C2 C3 C4 C5    9.2e-7 9.6e-7 8.6e-7 7.6e-7   one body stage (3, 4, 6, 3 bottlenecks) from the previous tap (measured 4.6e-7 4.8e-7
                            4.3e-7 3.8e-7; f32 4.7e-7 6.7e-7 8.9e-7 5.0e-7)
  L2..L5         8.8e-7   lateral 1 x 1 of C_k + the upsampled L_(k+1) tap (measured 4.4e-7)
  P_k from L_k   1.3e-6   the 3 x 3 output convolution alone (measured 6.4e-7); "clip": 5.5e-6 (measured 2.71e-6), see below
  P2..P5         1.4e-6   the FPN as one stage from C2..C5 (measured 6.9e-7; f32 5.6e-7); "clip": 5.7e-6 (measured 2.82e-6; f32 5.4e-7)
                            FINDING, localised with the L taps: at 480 x 640 the P2 convolution (K = 2304) has 300 tiles and runs its K loop
                            un-split, one fp32 accumulation of 2304 terms; the smaller frames split K.  A plain sequential fp32 sum in the
                            kernel's K order (kh, kw, c) on the same L2 tap is off float64 by 2.84e-6 of the scale AT THE SAME ELEMENT
                            (c 2, y 109, x 16), with the same median (6.0e-7 abs) and 99.9th percentile (6.8e-6 abs) as the engine's error,
                            and differs from the engine by 8.5e-7: summation-order round-off (the oracle's blocked sums: 3.6e-7), no
                            wrong index.  Spec.fpn_tol carries the bound of that path; the other specs keep the tight one.
  un-forced      (reported) x0 -> P2..P6 in one go: 8.4e-7 on the golden cases, 2.82e-6 on "clip"; tests/test_gpu_zz_detector.py's bound
                            is derived from it
  roi7 roi14     3.5e-7   fp32 bilinear weights and 16-term sum vs float64, coordinates in fp32 on both sides (measured 1.73e-7; f32 1.53e-7)
  mask logits    2.6e-6   four 3 x 3 convolutions, the transposed convolution and the logits from the roi14 tap (measured 1.27e-6 at
                            scale 0.42; f32 4.4e-7)
  RPN logits     2.1e-6   3 x 3 + 1 x 1 head from P2..P6 (measured 1.02e-6 on "clip", 4.7e-7 elsewhere; f32 4.7e-7); "tied": exactly 0.25
Selections are compared rank for rank (tests/support/detector.py match_ranked); a neighbour swap or an entry at the cut is admitted only
where the oracle keys differ by less than KEY_EPS (fp32 round-off of the keys), and at most MAX_EXC of them per list.  A mask may differ
beyond 2e-6 only if one of its box edges lies within 1e-4 px of an integer in float64 (the truncation point), counted the same way.
Exact cases use eps = 0: no exception at all."""
from __future__ import annotations

import contextlib
from dataclasses import dataclass, field
from typing import Dict

import numpy as np
import pytest
import torch

from tests.support import detector as sup

pytestmark = pytest.mark.gpu

X0_TOL = 4e-5
SCORE_TOL = 3e-7
LOGIT_TOL = 6e-6
MASK_TOL = 2e-6
KEY_EPS = 1e-6
TRUNK_TOL = {"pool": 1.4e-6, "C2": 9.2e-7, "C3": 9.6e-7, "C4": 8.6e-7, "C5": 7.6e-7, "L": 8.8e-7, "PL": 1.3e-6, "P": 1.4e-6}
ROI_TOL = 3.5e-7
MASK_LOGIT_TOL = 2.6e-6
RPN_KEY_TOL = 2.1e-6
MAX_EXC = 2
T_IOU = float(np.float32(896) / (np.float32(1024) + np.float32(1024) - np.float32(896)))   # fp32 IoU of two 32 px anchors 4 px apart

# engine option -> the oracle's module constant
OM_CONST = {"rpn_pre_nms_top_n": "RPN_PRE_NMS_TOP_N", "rpn_post_nms_top_n": "RPN_POST_NMS_TOP_N", "rpn_nms_thresh": "RPN_NMS_THRESH",
            "rpn_min_size": "RPN_MIN_SIZE", "box_min_size": "BOX_MIN_SIZE", "box_score_thresh": "BOX_SCORE_THRESH", "box_nms_thresh": "BOX_NMS_THRESH", "box_detections_per_img": "BOX_DETECTIONS_PER_IMG"}


@dataclass
class Spec:
    n: int
    H: int
    W: int
    mn: int
    mx: int
    C: int
    edits: Dict[str, object] = field(default_factory=dict)       # state_dict key -> constant value or per-element list
    overrides: Dict[str, object] = field(default_factory=dict)   # mp_detector_config fields (DetectorMaskRCNN.engine_overrides)
    exact: bool = False                                          # constant keys: oracle in float32, eps = 0, exact boxes
    box_tol: float = 2e-4                                        # RPN proposals, px
    post_box_tol: float = 4e-5                                   # detections (decoded from the engine's own deltas), px
    fpn_tol: Dict[str, float] = field(default_factory=dict)      # TRUNK_TOL entries of a spec whose FPN convolutions run an un-split K loop


def _tied(**ov):
    e = {"rpn.head.cls_logits.weight": 0.0, "rpn.head.cls_logits.bias": 0.25, "rpn.head.bbox_pred.weight": 0.0, "rpn.head.bbox_pred.bias": 0.0,
         "roi_heads.box_predictor.cls_score.weight": 0.0, "roi_heads.box_predictor.cls_score.bias": [0.0, 1.0, 1.0, 1.0, 1.0],
         "roi_heads.box_predictor.bbox_pred.weight": 0.0, "roi_heads.box_predictor.bbox_pred.bias": 0.0}
    o = {"rpn_pre_nms_top_n": 100, "rpn_nms_thresh": T_IOU, "box_nms_thresh": T_IOU}
    o.update(ov)
    return Spec(1, 192, 256, 192, 256, 5, e, o, exact=True, box_tol=0.0, post_box_tol=0.0)


SPECS = {
    # the fixture cases (tests/golden/detector_*.npz), a batch of three, and an odd size whose resize hits the bilinear edge clamps
    "native": Spec(1, 192, 256, 192, 256, 5),
    "resized": Spec(1, 150, 200, 192, 256, 5),
    "batch2": Spec(2, 160, 224, 160, 224, 7),
    "batch3": Spec(3, 160, 224, 160, 224, 3),
    "odd": Spec(1, 151, 203, 192, 256, 5),
    # all objectness keys equal, proposals = anchors, NMS thresholds at the fp32 IoU of adjacent anchors, equal foreground logits:
    # the stable rank order, the per-level top-100 cut (P2..P5 have more anchors, P6 has 36), IoU == thr must not suppress
    "tied": _tied(),
    "cut1": _tied(box_detections_per_img=1),
    "cut5": _tied(box_detections_per_img=5),
    # deltas past DET_XFORM_CLIP at the released detectors' 480 x 640: RPN boxes [ctr + w / 4, ctr + h / 4, W, H] (dx = dy = 31.5,
    # dw = dh = 6 clamped to log(1000 / 16)), some of zero width at the right / bottom border, frame-sized ones pooled from P5; the box
    # head does the same once more (10 * 31.5, 5 * 6 with its weights 10, 10, 5, 5)
    "clip": Spec(1, 480, 640, 480, 640, 3, {"rpn.head.bbox_pred.weight": 0.0, "rpn.head.bbox_pred.bias": [31.5, 31.5, 6.0, 6.0] * 3,
                                            "roi_heads.box_predictor.bbox_pred.weight": 0.0,
                                            "roi_heads.box_predictor.bbox_pred.bias": [315.0, 315.0, 30.0, 30.0] * 3}, box_tol=3e-3, post_box_tol=3e-3,
                 fpn_tol={"PL": 5.5e-6, "P": 5.7e-6}),
    # NMS segments at their capacity (DET_MAX_SEG = 1024) and at one entry
    "seg1024": Spec(1, 192, 256, 192, 256, 5, overrides={"rpn_pre_nms_top_n": 1024, "rpn_post_nms_top_n": 1024}),
    "seg1": Spec(1, 192, 256, 192, 256, 5, overrides={"rpn_pre_nms_top_n": 1, "rpn_post_nms_top_n": 1}),
}
STAGE_SPECS = list(SPECS)
# the trunk's own cases: "tied", "cut*" and "seg*" share weights and sizes with "native"; "small" (P2 16 x 24, P5 2 x 3, P6 1 x 2) has
# maps smaller than the convolution's tile and narrower than the reach of the 3 x 3 window
TRUNK_SPECS = ["native", "resized", "batch2", "batch3", "odd", "clip", "small"]
SPECS["small"] = Spec(1, 64, 96, 64, 96, 3)
# RoIAlign's own case: "clip"'s RPN deltas, identity box deltas and no small-box filter, so that the detections ARE the clipped proposals
# [ctr + w / 4, ctr + h / 4, W, H]: frame-sized ones down to boxes of zero width or height at the right / bottom border (the filters of
# "clip" drop those, and its detections, a quarter of their proposals' size, stop at level 3).  On the CPU oracle: 643 proposals on the
# levels {2: 503, 3: 93, 4: 46, 5: 1}, 318 of zero size; 100 detections on {2: 85, 3: 8, 4: 6, 5: 1}, 44 of zero size.
ROI_SPECS = ["clipdet"]
SPECS["clipdet"] = Spec(1, 480, 640, 480, 640, 3, {"rpn.head.bbox_pred.weight": 0.0, "rpn.head.bbox_pred.bias": [31.5, 31.5, 6.0, 6.0] * 3,
                                                   "roi_heads.box_predictor.bbox_pred.weight": 0.0, "roi_heads.box_predictor.bbox_pred.bias": 0.0},
                        {"rpn_min_size": 0.0, "box_min_size": 0.0})

_SD: Dict[int, Dict[str, torch.Tensor]] = {}
_RUNS: Dict[str, "Run"] = {}


def _state_dict(spec: Spec) -> Dict[str, torch.Tensor]:
    from oracle import mask_rcnn as om

    if spec.C not in _SD:
        _SD[spec.C] = om.synthetic_state_dict(spec.C)
    sd = dict(_SD[spec.C])
    for k, v in spec.edits.items():
        t = torch.empty_like(sd[k])
        t[...] = torch.tensor(v, dtype=torch.float32).view(-1, *([1] * (t.dim() - 1))) if isinstance(v, list) else v
        sd[k] = t
    return sd


@contextlib.contextmanager
def _oracle_config(overrides):
    from oracle import mask_rcnn as om

    saved = {}
    try:
        for k, v in overrides.items():
            name = OM_CONST[k]
            saved[name] = getattr(om, name)
            setattr(om, name, float(np.float32(v)) if isinstance(v, float) else v)
        yield om
    finally:
        for name, v in saved.items():
            setattr(om, name, v)


class Run:
    """one engine forward of a spec, its debug taps on the host, and the oracle stages fed from them (computed on first use)"""

    def __init__(self, spec: Spec):
        from megapose6d_amd.mask_rcnn import DetectorMaskRCNN
        from oracle import mask_rcnn as om

        self.spec = spec
        self.sd = _state_dict(spec)
        m = DetectorMaskRCNN(input_resize=(spec.mn, spec.mx), n_classes=spec.C)
        m.load_state_dict(self.sd)
        m.engine_overrides = dict(spec.overrides)
        self.model = m.cuda().eval()
        self.images = om.synthetic_images(spec.n, spec.H, spec.W)
        self.net = m._net()
        self.D = int(self.net.cfg.box_detections_per_img)
        self.R = int(self.net.cfg.rpn_post_nms_top_n)
        boxes, scores, labels, counts, masks = self.net.forward(self.images.cuda())
        torch.cuda.synchronize()
        self.out = dict(boxes=boxes.cpu(), scores=scores.cpu(), labels=labels.cpu(), counts=counts.cpu(), masks=masks.cpu())
        self.tap = {w: self.net.debug_tensor(w).cpu() for w in ("x0", "P2", "P3", "P4", "P5", "P6", "keys", "proposals", "proposal_scores",
                                                                "proposal_counts", "class_logits", "det_resized", "f_cnt", "mask_logits")}
        self.dt = torch.float32 if spec.exact else torch.float64
        self.sd_d = {k: v.to(self.dt) for k, v in self.sd.items()}
        self.feats = [sup.nhwc_to_nchw(self.tap[f"P{l}"], self.dt) for l in range(2, 7)]
        _, self.sizes, self.orig = om.transform_images(list(self.images), spec.mn, spec.mx)
        self.pcnt = self.tap["proposal_counts"].view(-1).tolist()
        self.survivors = self.tap["f_cnt"].view(-1).tolist()   # candidates that survived their class's NMS, before the cut at D
        self.fcnt = [min(k, self.D) for k in self.survivors]
        self.props = [self.tap["proposals"][i, : self.pcnt[i]].to(self.dt) for i in range(spec.n)]
        self._cache = {}
        self._maps = {}

    @property
    def sd64(self):
        """the float64 weights (the continuous stages run in float64 on the exact specs too)"""
        if self.dt == torch.float64:
            return self.sd_d
        if "sd64" not in self._cache:
            self._cache["sd64"] = {k: v.double() for k, v in self.sd.items()}
        return self._cache["sd64"]

    def map(self, what: str) -> torch.Tensor:
        """a padded-NHWC tap's interior [n, h, w, c] (fp32), its border ring asserted to be zero"""
        if what not in self._maps:
            self._maps[what] = sup.debug_map(self.net, what)
        return self._maps[what]

    def oracle(self, stage: str):
        if stage not in self._cache:
            with _oracle_config(self.spec.overrides) as om, torch.no_grad():
                if stage == "rpn":
                    hw = (int(self.tap["x0"].shape[1]), int(self.tap["x0"].shape[2]))   # the padded batch
                    self._cache[stage] = om.rpn_proposals(self.sd_d, self.feats, self.sizes, hw, objectness_override=self.tap["keys"])
                elif stage == "rpn_free":   # the head's own objectness logits: no override, float64 on every spec
                    hw = (int(self.tap["x0"].shape[1]), int(self.tap["x0"].shape[2]))
                    feats = self.feats if self.dt == torch.float64 else [f.double() for f in self.feats]
                    self._cache[stage] = om.rpn_proposals(self.sd64, feats, self.sizes, hw)[1]["objectness"]
                elif stage == "box":   # one image at a time (the RoIAlign reference holds [rois, 256, 7, 2, 7, 2] sample arrays)
                    lg, rg = [], []
                    for i in range(self.spec.n):
                        a, b = om.box_branch(self.sd_d, [f[i : i + 1] for f in self.feats[:4]], [self.props[i]], [self.sizes[i]])
                        lg.append(a)
                        rg.append(b)
                    self._cache[stage] = torch.cat(lg), torch.cat(rg)
                elif stage == "post":
                    C = self.spec.C
                    rows = torch.cat([self.tap["class_logits"][i * self.R : i * self.R + self.pcnt[i]] for i in range(self.spec.n)]).to(self.dt)
                    self._cache[stage] = om.postprocess_detections(rows[:, :C], rows[:, C : 5 * C], self.props, self.sizes)
        return self._cache[stage]


def _run(name: str) -> Run:
    if name not in _RUNS:
        _RUNS.clear()   # one spec at a time holds its taps (the parametrisation runs spec by spec)
        _RUNS[name] = Run(SPECS[name])
    return _RUNS[name]


def _eps(run: Run) -> float:
    return 0.0 if run.spec.exact else KEY_EPS


def _report(stage, name, **errs):
    print(f"[{stage}] {name}: " + ", ".join(f"{k} {v:.3e}" if isinstance(v, float) else f"{k} {v}" for k, v in errs.items()))


# ---------------------------------------------------------------------------------------------------------------------------------
# stages, parametrised spec-major so that each spec's forward serves its five stages
# ---------------------------------------------------------------------------------------------------------------------------------
STAGES = ["preprocess", "rpn", "box_head", "postprocess", "masks", "trunk", "roi7", "mask_head", "rpn_logits"]
CASES = [(name, stage) for name in SPECS for stage in STAGES
         if (stage == "trunk" and name in TRUNK_SPECS) or (stage != "trunk" and name in STAGE_SPECS) or (stage in ("roi7", "mask_head") and name in ROI_SPECS)]


@pytest.mark.parametrize("name,stage", CASES, ids=[f"{n}-{s}" for n, s in CASES])
def test_detector_stage_matches_the_oracle(name, stage):
    run = _run(name)
    globals()[f"_check_{stage}"](run, name)


def _check_preprocess(run: Run, name: str):
    from oracle import mask_rcnn as om

    spec = run.spec
    batch, sizes, _ = om.transform_images(list(run.images.double()), spec.mn, spec.mx)
    flat, shp, b, _ = sup.raw_debug(run.net, "x0")
    n, Hp, Wp, _ = shp
    full = flat.view(n, Hp + 2 * b, Wp + 2 * b, 4)
    assert tuple(batch.shape) == (n, 3, Hp, Wp), (batch.shape, shp)
    inner = full[:, b : b + Hp, b : b + Wp]
    got = sup.nhwc_to_nchw(inner[..., :3])
    err = (got - batch).abs().max().item()
    _report("x0", name, err=err, resized=sizes[0])
    assert err < X0_TOL, err
    # the pad: the 4th channel everywhere, the border of 3, and the rows / columns past the resized image up to the multiple of 32
    pad = full.clone()
    pad[:, b : b + Hp, b : b + Wp, :3] = 0
    assert (pad == 0).all()
    for i, (h, w) in enumerate(sizes):
        assert (inner[i, h:] == 0).all() and (inner[i, :, w:] == 0).all()


def _check_rpn(run: Run, name: str):
    props, dbg = run.oracle("rpn")
    P, S = run.tap["proposals"], run.tap["proposal_scores"]
    tol, eps = run.spec.box_tol, _eps(run)
    worst_b, worst_s, n_exc = 0.0, 0.0, 0
    for i in range(run.spec.n):
        k = run.pcnt[i]
        rb, rs = props[i].double(), dbg["scores"][i].double()
        gb, gs = P[i, :k].double(), S[i, :k].double()
        exc, msg = sup.match_ranked(lambda a, c: bool((gb[a] - rb[c]).abs().max() <= tol), k, rs.tolist(), eps, gs.tolist())
        assert msg is None, (i, msg, k, len(rb))
        n_exc += exc
        same = [(gb[a] - rb[a]).abs().max().item() <= tol for a in range(k)]
        if k:
            worst_b = max(worst_b, max((gb[a] - rb[a]).abs().max().item() for a in range(k) if same[a]))
            worst_s = max(worst_s, max(abs(gs[a].item() - rs[a].item()) for a in range(k) if same[a]))
        assert (P[i, k:] == 0).all() and (S[i, k:] == 0).all()   # rows past the count
    _report("rpn", name, boxes=worst_b, scores=worst_s, exceptions=n_exc, counts=run.pcnt)
    assert worst_b <= tol and worst_s <= SCORE_TOL, (worst_b, worst_s)
    assert n_exc <= MAX_EXC, n_exc
    if name == "tied":   # the threshold tie was exercised: surviving neighbours overlap at exactly rpn_nms_thresh
        b = P[0, : run.pcnt[0]].numpy()
        iou = sup.iou_f32(b, b)
        assert (iou == np.float32(T_IOU)).sum() > 0


def _levels(boxes: torch.Tensor) -> torch.Tensor:
    """LevelMapper of MultiScaleRoIAlign (ops/poolers.py): k = floor(4 + log2(sqrt(area) / 224) + 1e-6) clamped to [2, 5]"""
    area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    return torch.floor(4 + torch.log2(torch.sqrt(area) / 224) + 1e-6).clamp(2, 5).long()


def _check_box_head(run: Run, name: str):
    logits, reg = run.oracle("box")
    C, R = run.spec.C, run.R
    rows = sup.debug_rows(run.net, "class_logits")
    live = torch.cat([torch.arange(i * R, i * R + run.pcnt[i]) for i in range(run.spec.n)])
    got = rows[live].double()
    ref = torch.cat([logits, reg], 1).double()
    scale = max(1.0, ref.abs().max().item())
    err = (got[:, : 5 * C] - ref).abs().max().item() / scale if len(live) else 0.0
    lv = _levels(torch.cat(run.props).float()) if len(live) else torch.zeros(0)
    _report("box_head", name, rel_err=err, rows=len(live), levels=sorted(set(lv.tolist())))
    assert err <= (0.0 if run.spec.exact else LOGIT_TOL), err
    assert (rows[:, 5 * C :] == 0).all()   # the predictor's pad columns
    if name == "clip":   # frame-sized proposals: RoIAlign must use every level, P5 included
        assert set(lv.tolist()) == {2, 3, 4, 5}, sorted(set(lv.tolist()))


def _check_postprocess(run: Run, name: str):
    dets = run.oracle("post")
    tol, eps = run.spec.post_box_tol, _eps(run)
    O, DR = run.out, run.tap["det_resized"]
    worst_b, worst_s, worst_o, n_exc = 0.0, 0.0, 0.0, 0
    for i, d in enumerate(dets):
        k = run.fcnt[i]
        assert int(O["counts"][i]) == k and len(d["boxes"]) == k and (run.survivors[i] == k or k == run.D), (run.survivors[i], k, len(d["boxes"]))
        rb, rs, rl = d["boxes"].double(), d["scores"].double(), d["labels"]
        gb, gs, gl = DR[i, :k].double(), O["scores"][i, :k].double(), O["labels"][i, :k].long()
        exc, msg = sup.match_ranked(lambda a, c: bool(gl[a] == rl[c]) and bool((gb[a] - rb[c]).abs().max() <= tol), k, rs.tolist(), eps,
                                    gs.tolist())
        assert msg is None, (i, msg, gl[:8].tolist(), rl[:8].tolist())
        n_exc += exc
        # boxes in the original frame: transform.py resize_boxes with the fp32 ratios
        o, s = run.orig[i], run.sizes[i]
        rh, rw = torch.tensor(float(o[0])) / torch.tensor(float(s[0])), torch.tensor(float(o[1])) / torch.tensor(float(s[1]))
        ro = torch.stack((rb[:, 0] * rw, rb[:, 1] * rh, rb[:, 2] * rw, rb[:, 3] * rh), 1)
        go = O["boxes"][i, :k].double()
        for a in range(k):
            if bool(gl[a] == rl[a]) and (gb[a] - rb[a]).abs().max() <= tol:
                worst_b = max(worst_b, (gb[a] - rb[a]).abs().max().item())
                worst_s = max(worst_s, abs(gs[a].item() - rs[a].item()))
                worst_o = max(worst_o, (go[a] - ro[a]).abs().max().item())
        assert (O["boxes"][i, k:] == 0).all() and (O["scores"][i, k:] == 0).all() and (O["labels"][i, k:] == 0).all()
    _report("post", name, boxes=worst_b, boxes_orig=worst_o, scores=worst_s, exceptions=n_exc, counts=run.fcnt)
    assert worst_b <= tol and worst_o <= 1.3 * tol and worst_s <= SCORE_TOL, (worst_b, worst_o, worst_s)   # (ratios <= 1.28)
    assert n_exc <= MAX_EXC, n_exc
    if name in ("cut1", "cut5"):
        D = run.D
        assert run.fcnt == [D], run.fcnt
        if D == 5:   # equal foreground scores: torchvision's stable order walks the candidates proposal by proposal, class by class
            assert O["labels"][0].tolist() == [1, 2, 3, 4, 1], O["labels"][0].tolist()


def _check_masks(run: Run, name: str):
    from oracle import mask_rcnn as om

    spec, D = run.spec, run.D
    rows = sup.debug_rows(run.net, "mask_logits")
    m28 = sup.mask_logits_28(rows, spec.n * D)
    masks = run.out["masks"]
    worst, n_exc, n_cmp = 0.0, 0, 0
    for i in range(spec.n):
        k = run.fcnt[i]
        assert (masks[i, k:] == 0).all()   # rows past the count
        if k == 0:
            continue
        lab = run.out["labels"][i, :k].long()
        logit = m28[i * D : i * D + k].double()[torch.arange(k), lab]
        prob = torch.sigmoid(logit)[:, None]
        boxes = run.out["boxes"][i, :k]                                  # fp32, as the kernel reads them
        ref = om.paste_masks(prob, boxes, (spec.H, spec.W))[:, 0].double()
        err = (masks[i, :k].double() - ref).abs().flatten(1).max(1).values
        # f64 box edges: within 1e-4 px of an integer, fp contraction could move the truncation
        b = boxes.double()
        sc = 30.0 / 28.0
        wh, hh = (b[:, 2] - b[:, 0]) * 0.5 * sc, (b[:, 3] - b[:, 1]) * 0.5 * sc
        xc, yc = (b[:, 2] + b[:, 0]) * 0.5, (b[:, 3] + b[:, 1]) * 0.5
        e = torch.stack([xc - wh, yc - hh, xc + wh, yc + hh], 1)
        near = ((e - e.round()).abs() < 1e-4).any(1)
        bad = err > MASK_TOL
        assert not (bad & ~near).any(), (i, err[bad & ~near][:4].tolist(), torch.where(bad & ~near)[0][:4].tolist())
        n_exc += int((bad & near).sum())
        ok = ~bad
        if ok.any():
            worst = max(worst, err[ok].max().item())
        n_cmp += k
    _report("masks", name, err=worst, masks=n_cmp, exceptions=n_exc)
    assert torch.isfinite(masks).all() and n_exc <= MAX_EXC


def _rel_err(got: torch.Tensor, ref: torch.Tensor):
    """-> (max |got - ref| / max(1, max |ref|), max |ref|): every element, the reference in float64"""
    assert tuple(got.shape) == tuple(ref.shape), (got.shape, ref.shape)
    assert ref.dtype == torch.float64 and torch.isfinite(got).all()
    if ref.numel() == 0:
        return 0.0, 0.0
    top = ref.abs().max().item()
    return (got.double() - ref).abs().max().item() / max(1.0, top), top


def _check_trunk(run: Run, name: str):
    """x0 -> pool -> C2 -> C3 -> C4 -> C5 -> P2..P5 -> P6, every step fed the engine's own tap in float64; then the whole trunk
    un-forced from x0 (reported: the figure the bound of tests/test_gpu_zz_detector.py is derived from)"""
    from oracle import mask_rcnn as om

    sd = run.sd64
    x0 = run.tap["x0"]                       # [n, Hp, Wp, 4]: the resized images AND the engine's zero padding up to the multiple of 32
    n, Hp, Wp, _ = x0.shape
    assert (x0[..., 3] == 0).all()
    x = sup.nhwc_to_nchw(x0[..., :3])
    maps = {w: run.map(w) for w in ("pool", "C2", "C3", "C4", "C5", "L2", "L3", "L4", "L5", "P2", "P3", "P4", "P5", "P6")}
    errs, scales = {}, {}
    with torch.no_grad():
        errs["pool"], scales["pool"] = _rel_err(sup.nhwc_to_nchw(maps["pool"], torch.float32), om.resnet_stem(sd, x))
        prev = "pool"
        for li in range(4):
            w = f"C{li + 2}"
            errs[w], scales[w] = _rel_err(sup.nhwc_to_nchw(maps[w], torch.float32), om.resnet_stage(sd, sup.nhwc_to_nchw(maps[prev]), li))
            prev = w
        cs = [sup.nhwc_to_nchw(maps[f"C{k}"]) for k in range(2, 6)]
        ref = om.fpn(sd, cs)
        for k in range(2, 6):   # the FPN as one stage, from C2..C5
            errs[f"P{k}"], scales[f"P{k}"] = _rel_err(sup.nhwc_to_nchw(maps[f"P{k}"], torch.float32), ref[k - 2])
        for k in range(5, 1, -1):   # and layer by layer: the top-down map from C{k} and the engine's L{k + 1}, P{k} from the engine's L{k}
            top = sup.nhwc_to_nchw(maps[f"L{k + 1}"]) if k < 5 else None
            errs[f"L{k}"], scales[f"L{k}"] = _rel_err(sup.nhwc_to_nchw(maps[f"L{k}"], torch.float32), om.fpn_inner(sd, cs[k - 2], k - 2, top))
            e = (sup.nhwc_to_nchw(maps[f"P{k}"]) - om.fpn_layer(sd, sup.nhwc_to_nchw(maps[f"L{k}"]), k - 2)).abs() / max(1.0, scales[f"P{k}"])
            errs[f"P{k}|L{k}"] = e.max().item()
            if k == 2:   # the distribution of the largest map's error: round-off has a smooth tail, a wrong index has outliers
                errs["P2|L2 median"], errs["P2|L2 p99.9"] = e.median().item(), e.flatten().kthvalue(int(0.999 * e.numel())).values.item()
        free = om.resnet50_fpn(sd, x)
    assert tuple(maps["P2"].shape) == (n, Hp // 4, Wp // 4, 256) and tuple(maps["P5"].shape) == (n, Hp // 32, Wp // 32, 256)
    assert tuple(maps["P6"].shape) == (n, ref[4].shape[2], ref[4].shape[3], 256)
    assert torch.equal(maps["P6"], maps["P5"][:, ::2, ::2])   # LastLevelMaxPool = a stride-2 subsample: bit for bit
    unforced = {f"P{k}": _rel_err(sup.nhwc_to_nchw(maps[f"P{k}"], torch.float32), free[k - 2])[0] for k in range(2, 7)}
    _report("trunk", name, **errs, unforced=max(unforced.values()), P2_hw=tuple(maps["P2"].shape[1:3]), P6_hw=tuple(maps["P6"].shape[1:3]),
            scale_C5=scales["C5"], scale_P2=scales["P2"])
    for w, e in errs.items():
        key = "PL" if "|" in w else w[0] if w[0] in "PL" else w
        assert e <= run.spec.fpn_tol.get(key, TRUNK_TOL[key]), (w, e)


def _check_roi(run: Run, name: str, what: str):
    """the RoIAlign output tap ("roi7": the proposals, "roi14": the detections) against the float64 RoIAlign of the engine's P2..P5"""
    n = run.spec.n
    if what == "roi7":
        P, per, cnt, boxes = 7, run.R, run.pcnt, run.tap["proposals"]
        rows = sup.debug_rows(run.net, "roi7")
        assert rows.shape == (n * per, 49 * 256)
        got = rows.view(n * per, 7, 7, 256)
    else:
        P, per, cnt, boxes = 14, run.D, run.fcnt, run.tap["det_resized"]
        got = run.map("roi14")               # (border ring asserted zero)
        assert tuple(got.shape) == (n * per, 14, 14, 256)
    live_boxes = [boxes[i, : cnt[i]] for i in range(n)]
    live = torch.cat([torch.arange(i * per, i * per + cnt[i]) for i in range(n)])
    dead = torch.ones(n * per, dtype=torch.bool)
    dead[live] = False
    assert (got[dead] == 0).all()            # rows past the count
    ref, lv = sup.multiscale_roi_align_f64([run.tap[f"P{l}"] for l in range(2, 6)], live_boxes, run.sizes, P)
    err, top = _rel_err(got[live], ref)
    b = torch.cat(live_boxes)
    sc = 0.5 ** lv.float()
    narrow = int((((b[:, 2] - b[:, 0]) * sc < 1) | ((b[:, 3] - b[:, 1]) * sc < 1)).sum()) if len(b) else 0   # max(roi_w, 1) / max(roi_h, 1) clamps
    zero = int(((b[:, 2] == b[:, 0]) | (b[:, 3] == b[:, 1])).sum()) if len(b) else 0
    _report("roi", name, what=what, rel_err=err, scale=top, rows=len(live), levels=sorted(set(lv.tolist())), clamped=narrow, zero_size=zero)
    assert err <= ROI_TOL, err
    return got, live, lv, narrow, zero


def _assert_roi_coverage(name: str, what: str, lv, narrow: int, zero: int):
    """what the RoIAlign cases are there for: every pyramid level, and boxes under one cell of their level (max(roi_w, 1), max(roi_h, 1))"""
    if name == "clipdet":
        assert set(lv.tolist()) == {2, 3, 4, 5} and zero > 0, (what, sorted(set(lv.tolist())), zero)
    if name == "clip":   # (its small-box filters leave no box of zero size, and its detections stop at level 3: see "clipdet")
        assert narrow > 0 and (what == "roi14" or set(lv.tolist()) == {2, 3, 4, 5}), (what, sorted(set(lv.tolist())), narrow)


def _check_roi7(run: Run, name: str):
    _, _, lv, narrow, zero = _check_roi(run, name, "roi7")
    _assert_roi_coverage(name, "roi7", lv, narrow, zero)


def _check_mask_head(run: Run, name: str):
    from oracle import mask_rcnn as om

    spec, D = run.spec, run.D
    roi, live, lv, narrow, zero = _check_roi(run, name, "roi14")
    rows = sup.debug_rows(run.net, "mask_logits")
    C = spec.C
    assert rows.shape[0] == spec.n * D * 196 * 4 and (rows[:, C:] == 0).all()   # the pad columns past C
    assert torch.isfinite(rows).all()                                           # rows past the count included
    m28 = sup.mask_logits_28(rows, spec.n * D)
    with torch.no_grad():
        ref = om.mask_head_logits(run.sd64, sup.nhwc_to_nchw(roi[live])) if len(live) else torch.zeros(0, C, 28, 28, dtype=torch.float64)
    err, top = _rel_err(m28[live][:, :C], ref)
    _report("mask_head", name, rel_err=err, scale=top, masks=len(live), classes=C)
    assert err <= MASK_LOGIT_TOL, err
    _assert_roi_coverage(name, "roi14", lv, narrow, zero)


def _check_rpn_logits(run: Run, name: str):
    ref = run.oracle("rpn_free")
    keys = run.tap["keys"]
    err, top = _rel_err(keys, ref)
    _report("rpn_logits", name, rel_err=err, scale=top, anchors=int(keys.shape[1]))
    if name == "tied":   # zeroed weights, bias 0.25: exact
        assert (keys == np.float32(0.25)).all() and (ref == 0.25).all()
    assert err <= RPN_KEY_TOL, err


# ---------------------------------------------------------------------------------------------------------------------------------
# edge cases with their own assertions
# ---------------------------------------------------------------------------------------------------------------------------------
def test_no_detections_when_the_background_wins():
    """background cls_score bias +20 on zeroed weights: every foreground score is ~2e-9 < 0.05; f_cnt = 0, empty outputs, zero masks"""
    from megapose6d_amd.mask_rcnn import DetectorMaskRCNN

    spec = Spec(2, 160, 224, 160, 224, 3, {"roi_heads.box_predictor.cls_score.weight": 0.0,
                                            "roi_heads.box_predictor.cls_score.bias": [20.0, 0.0, 0.0]})
    run = Run(spec)
    assert run.fcnt == [0, 0] and run.out["counts"].tolist() == [0, 0]
    assert all(len(d["boxes"]) == 0 for d in run.oracle("post"))
    assert (run.out["masks"] == 0).all() and torch.isfinite(run.out["masks"]).all()
    assert (run.out["boxes"] == 0).all() and (run.out["scores"] == 0).all()
    m = DetectorMaskRCNN(input_resize=(160, 224), n_classes=3)
    m.load_state_dict(run.sd)
    out = m.cuda().eval()(list(run.images))
    assert all(len(o["boxes"]) == 0 and o["masks"].shape == (0, 1, 160, 224) for o in out)


def test_score_exactly_at_the_threshold_is_dropped():
    """two classes with equal logits score exactly 0.5: box_score_thresh = 0.5 keeps nothing (roi_heads.py: scores > thresh), one fp32
    step below it keeps a detection per proposal and class (up to D)"""
    e = {"roi_heads.box_predictor.cls_score.weight": 0.0, "roi_heads.box_predictor.cls_score.bias": [0.0, 0.0],
         "roi_heads.box_predictor.bbox_pred.weight": 0.0, "roi_heads.box_predictor.bbox_pred.bias": 0.0}   # (boxes = proposals: exact)
    at = Run(Spec(1, 192, 256, 192, 256, 2, e, {"box_score_thresh": 0.5}, exact=True, box_tol=0.0, post_box_tol=0.0))
    assert at.fcnt == [0] and len(at.oracle("post")[0]["boxes"]) == 0
    below = float(np.nextafter(np.float32(0.5), np.float32(0)))
    run = Run(Spec(1, 192, 256, 192, 256, 2, e, {"box_score_thresh": below}, exact=True, box_tol=0.0, post_box_tol=0.0))
    assert run.fcnt[0] > 0
    _check_postprocess(run, "score_below")


def test_top_n_beyond_the_segment_capacity_is_a_clean_error():
    from megapose6d_amd._lib import EngineError
    from megapose6d_amd.mask_rcnn import DetectorMaskRCNN

    for k in ("rpn_pre_nms_top_n", "rpn_post_nms_top_n", "box_detections_per_img"):
        m = DetectorMaskRCNN(input_resize=(192, 256), n_classes=2)
        m.engine_overrides = {k: 1025}
        with pytest.raises(EngineError, match="top-n sizes"):
            m._net()


def test_two_forwards_are_bit_identical():
    run = _run("batch2")
    boxes, scores, labels, counts, masks = run.net.forward(run.images.cuda())
    torch.cuda.synchronize()
    again = dict(boxes=boxes.cpu(), scores=scores.cpu(), labels=labels.cpu(), counts=counts.cpu(), masks=masks.cpu())
    for k, v in run.out.items():
        assert torch.equal(v, again[k]), k
    for w, v in run.tap.items():
        assert torch.equal(v, run.net.debug_tensor(w).cpu()), w


def test_detector_convolutions_stay_on_the_fp32_kernel():
    """every convolution of a detector forward runs on the fp32-MFMA direct kernel: the detector's layers are packed in that form only,
    so no Winograd launch is counted and every convolution row of the profiler is conv_nhwc_f32_mfma (conv_splitk_reduce is the second
    pass of that kernel's split-K launches)"""
    from megapose6d_amd import engine as eng

    run = _run("batch2")
    eng.conv_wino_stats(reset=True)
    eng.conv_wino_bf16_stats(reset=True)
    eng.profile_begin()
    try:
        run.net.forward(run.images.cuda())
    finally:
        prof = eng.profile_end()
    assert eng.conv_wino_stats()[0] == 0.0 and eng.conv_wino_bf16_stats()[0] == 0.0
    convs = [k for k in prof if k.startswith("conv") and k != "conv_splitk_reduce"]
    assert convs and all(k.startswith("conv_nhwc_f32_mfma") for k in convs), sorted(prof)
    assert sum(int(prof[k]["launches"]) for k in convs) >= 80, prof   # the forward has 80 convolution layers (53 ResNet-50, 8 FPN, 10 RPN, 3 box head, 6 mask head)


TAPS = ["x0", "pool", "C2", "C3", "C4", "C5", "L2", "L3", "L4", "L5", "P2", "P3", "P4", "P5", "P6", "keys", "proposals", "proposal_scores",
        "proposal_counts", "roi7", "class_logits", "f_cnt", "det_resized", "roi14", "mask_logits"]


def test_every_published_tap_resolves():
    """every tap DetectorNet.debug_tensor documents, at the smallest frame the detector admits: the buffer lies inside the workspace the
    plan reports, no two taps overlap, n_elements is what (shape4, border, row_stride) imply under the three published layouts, the two
    count taps are int32; unknown and internal names, and a detector that has not run, are clean errors"""
    from megapose6d_amd import _lib
    from megapose6d_amd import engine as eng
    from megapose6d_amd._lib import EngineError

    run = _run("small")
    net, spec = run.net, run.spec
    total = _lib.load().mp_detector_workspace_bytes(net.handle, spec.n, spec.H, spec.W)
    assert 0 < total <= net._ws.numel()
    spans = []
    for what in TAPS:
        flat, (s0, s1, s2, s3), b, rs = net.debug_buffer(what)
        if b:                      # padded NHWC map
            n_el = s0 * (s1 + 2 * b) * (s2 + 2 * b) * s3
        elif s2 == 4:              # box list
            n_el = s0 * s1 * 4
        elif rs > 1:               # row matrix, rows padded to row_stride
            n_el = s0 * rs
        else:                      # flat per-image list / counter
            n_el = s0 * s1
        assert flat.numel() == n_el, (what, flat.numel(), n_el)
        assert flat.dtype == (torch.int32 if what in ("proposal_counts", "f_cnt") else torch.float32), what
        lo = flat.data_ptr() - net._ws.data_ptr()
        assert 0 <= lo and lo + 4 * n_el <= total, (what, lo, n_el, total)
        spans.append((lo, lo + 4 * n_el, what))
    spans.sort()
    for a, b in zip(spans, spans[1:]):
        assert a[1] <= b[0], (a, b)
    for what in ("nope", "cand_box"):
        with pytest.raises(EngineError, match=what):
            net.debug_tensor(what)
    fresh = eng.DetectorNet(run.sd, spec.C, spec.mn, spec.mx)
    with pytest.raises(EngineError, match="no forward"):
        fresh.debug_tensor("x0")
    fresh.close()


def test_missing_or_missized_checkpoint_tensor_is_a_clean_error():
    """a checkpoint without one tensor of each kind the loader treats differently (plain convolution weight, FrozenBatchNorm term, a
    tensor of a merged head, a permuted one), or with a mis-sized one, is an EngineError that names the key; the loader is intact after
    it: the complete checkpoint loads"""
    import re

    from megapose6d_amd import engine as eng
    from megapose6d_amd._lib import EngineError

    sd = _state_dict(Spec(1, 64, 96, 64, 96, 2))
    fc6 = "roi_heads.box_head.fc6.weight"
    broken = [(k, {q: v for q, v in sd.items() if q != k})
              for k in ("backbone.body.layer4.2.conv3.weight", "backbone.body.layer2.0.downsample.1.running_var", "rpn.head.bbox_pred.bias",
                        "roi_heads.mask_predictor.conv5_mask.weight")]
    broken.append((fc6, {**sd, fc6: sd[fc6][:-1]}))   # one row too few
    for key, bad in broken:
        with pytest.raises(EngineError, match=re.escape(key)):
            eng.DetectorNet(bad, 2, 64, 96)
        eng.DetectorNet(sd, 2, 64, 96).close()

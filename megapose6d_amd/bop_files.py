"""BOP's result files: what a run hands to somebody else, and the published detections it starts from.

  * the 6D pose results CSV -- the reference's `convert_results_to_bop` (src/megapose/evaluation/bop.py:100-138) through
    `bop_toolkit_lib.inout.save_bop_results`: `save_bop_results`, `load_bop_results`, `bop_results_name`;
  * the detection / segmentation results JSON in COCO's format -- the reference's `convert_results_to_coco` (bop.py:64-97), and the
    format of BOP's published default detections: `save_bop_detections`, `load_bop_detections`;
  * a mask in those files is COCO's run-length encoding (RLE): `masks_to_rle`, `rle_to_masks` on the device (`engine.rle_encode` /
    `engine.rle_decode`, csrc/rle.hip; the format is stated in csrc/rle_core.h), and the compressed string of pycocotools' `rleToString`
    / `rleFrString` on the host: `rle_to_string`, `rle_from_string` (a few kB per image).

Known deviations.  `pycocotools` and `bop_toolkit` are absent here: both formats are restated from their documentation and pinned
against a host emulation and a numpy restatement (tests/support/rle.py), unpinned against the packages.  The reference's
`convert_results_to_coco` names a polygon helper and writes `view_id`; the files BOP reads and publishes carry RLE masks and `image_id`,
which is what is written here (`view_id` is accepted when reading).  The files are host Python; only the masks touch the device.
"""
from __future__ import annotations

import json
from pathlib import Path
from typing import Any, Dict, List, Mapping, Optional, Sequence, Tuple, Union

import numpy as np
import pandas as pd
import torch

from .tcoll import PandasTensorCollection

BOP_RESULTS_HEADER = "scene_id,im_id,obj_id,score,R,t,time"
_INT32_MAX = (1 << 31) - 1


# --------------------------------------------------------------------------- #
# the compressed string
def rle_to_string(counts: Sequence[int]) -> str:
    """pycocotools' rleToString: from the fourth entry on, an entry is stored as its difference to the entry two before; a number is
    written five bits at a time, lowest first, as chr(48 + bits), with bit 0x20 set while more digits follow; it ends when what is left
    is all sign (0, or -1 with the digit's bit 0x10 set)."""
    counts = [int(c) for c in counts]
    out = []
    for i, x in enumerate(counts):
        if i > 2:
            x -= counts[i - 2]
        more = True
        while more:
            c = x & 0x1F
            x >>= 5
            more = (x != -1) if (c & 0x10) else (x != 0)
            if more:
                c |= 0x20
            out.append(chr(c + 48))
    return "".join(out)


def rle_from_string(s: str) -> List[int]:
    """pycocotools' rleFrString, the inverse of `rle_to_string`.  Raises ValueError for a character outside chr(48) .. chr(111) and for a
    string that ends inside a number."""
    counts: List[int] = []
    i, n = 0, len(s)
    while i < n:
        x, k, more = 0, 0, True
        while more:
            if i >= n:
                raise ValueError("RLE string ends inside a number")
            c = ord(s[i]) - 48
            if not 0 <= c < 64:
                raise ValueError(f"character {s[i]!r} at {i} is not an RLE digit")
            i += 1
            x |= (c & 0x1F) << (5 * k)
            k += 1
            more = bool(c & 0x20)
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts


# --------------------------------------------------------------------------- #
# masks <-> RLE dicts
def masks_to_rle(masks: torch.Tensor, compressed: bool = False) -> List[Dict[str, Any]]:
    """masks [n,h,w] bool or uint8 on the device -> [{"size": [h, w], "counts": list of ints, or the compressed string}] (COCO's RLE
    dict; encoded by `engine.rle_encode`, one read-back of the encoded form)."""
    from . import engine as eng

    if masks.dim() != 3:
        raise ValueError(f"masks must be [n,h,w], got {tuple(masks.shape)}")
    h, w = int(masks.shape[1]), int(masks.shape[2])
    counts, offsets, _, _ = eng.rle_encode(masks)
    counts, offsets = counts.cpu().numpy(), offsets.cpu().numpy()
    lists = [counts[offsets[m]:offsets[m + 1]].tolist() for m in range(len(offsets) - 1)]
    return [{"size": [h, w], "counts": rle_to_string(c) if compressed else c} for c in lists]


def _counts_of(seg: Mapping[str, Any]) -> np.ndarray:
    """the list of one RLE dict as int32; an entry beyond int32 is cut to its end of the range, which keeps the list malformed (h * w
    is below 2^31 - 1)"""
    c = seg["counts"]
    if isinstance(c, bytes):
        c = c.decode("ascii")
    if isinstance(c, str):
        c = rle_from_string(c)
    a = np.asarray(list(c), dtype=object)
    if any(not isinstance(v, (int, np.integer)) or isinstance(v, bool) for v in a):
        raise ValueError("RLE counts must be integers")
    return np.clip(np.asarray([int(v) for v in a], dtype=np.int64), -_INT32_MAX, _INT32_MAX).astype(np.int32)


def rle_to_masks(segmentations: Sequence[Mapping[str, Any]], device) -> Tuple[torch.Tensor, torch.Tensor]:
    """[{"size": [h, w], "counts": list or compressed string}] -> (masks [n,h,w] bool on `device`, status [n] int32: 0, or the bits of
    `engine.rle_decode` for a malformed list, whose mask is all False).  All entries must share one size (ValueError)."""
    from . import engine as eng

    if len(segmentations) == 0:
        raise ValueError("no segmentation: the size of the masks is unknown")
    sizes = {tuple(int(v) for v in s["size"]) for s in segmentations}
    if len(sizes) != 1 or len(next(iter(sizes))) != 2:
        raise ValueError(f"the segmentations must share one size [h, w], got {sorted(sizes)}")
    h, w = next(iter(sizes))
    lists = [_counts_of(s) for s in segmentations]
    offsets = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(l) for l in lists], out=offsets[1:])
    counts = torch.from_numpy(np.concatenate(lists) if lists else np.zeros(0, np.int32)).to(device)
    masks, status = eng.rle_decode(counts, offsets, h, w)
    return masks.bool(), status


# --------------------------------------------------------------------------- #
# detections: the BOP / COCO results JSON
def _obj_id(label: str) -> int:
    return int(str(label).split("_")[-1])


def detection_records(detections: PandasTensorCollection, segmentations: Optional[Sequence[Mapping[str, Any]]] = None) -> List[Dict[str, Any]]:
    """One record per row of `detections` (infos label, score, scene_id, view_id, optionally time; bboxes [n,4] xyxy): scene_id, image_id
    (the view_id), category_id (int(label.split("_")[-1])), bbox [x1, y1, x2 - x1, y2 - y1] as the reference computes it, score, time (-1
    if absent), and segmentation (segmentations[row], a COCO RLE dict) when given."""
    infos = detections.infos
    n = len(infos)
    boxes = detections.bboxes.detach().cpu().tolist()
    if segmentations is not None and len(segmentations) != n:
        raise ValueError(f"{len(segmentations)} segmentations for {n} detections")
    has_time = "time" in infos
    records = []
    for r in range(n):
        row = infos.iloc[r]
        x1, y1, x2, y2 = boxes[r]
        rec = dict(scene_id=int(row.scene_id), image_id=int(row.view_id), category_id=_obj_id(row.label), bbox=[x1, y1, x2 - x1, y2 - y1],
                   score=float(row.score), time=float(row.time) if has_time else -1)
        if segmentations is not None:
            seg = segmentations[r]
            counts = seg["counts"]
            rec["segmentation"] = {"size": [int(v) for v in seg["size"]], "counts": counts if isinstance(counts, str) else [int(c) for c in counts]}
        records.append(rec)
    return records


def save_bop_detections(path: Union[str, Path], detections: PandasTensorCollection, compressed: bool = False,
                        segmentations: Optional[Sequence[Mapping[str, Any]]] = None) -> Path:
    """Write the BOP / COCO results JSON of `detections` (records: `detection_records`).  `segmentation` is written when the collection
    has `masks` ([n,h,w] on the device, encoded by `masks_to_rle`; compressed = the string form of the counts) or when ready-made RLE
    dicts are passed as `segmentations`."""
    if segmentations is None and "masks" in detections.tensors:
        segmentations = masks_to_rle(detections.masks, compressed=compressed) if len(detections) else []
    path = Path(path)
    path.write_text(json.dumps(detection_records(detections, segmentations)))
    return path


def load_bop_detections(path_or_records: Union[str, Path, Sequence[Mapping[str, Any]]], device="cpu", label_format: str = "obj_{:06d}",
                        image_key: Optional[Mapping[Tuple[int, int], int]] = None) -> PandasTensorCollection:
    """A BOP / COCO results JSON (a path, or its parsed list of records; e.g. BOP's published default detections) -> the detections
    collection `PoseEstimator.run_inference_pipeline(detections=...)` takes: infos label (label_format of category_id), score, scene_id,
    view_id (the record's image_id, or view_id), batch_im_id, instance_id (numbered per image and label), time when any record has one;
    bboxes [n,4] float32 xyxy on `device`; masks [n,h,w] bool on `device` when every record has a segmentation (decoded by
    `rle_to_masks`).  batch_im_id numbers the distinct (scene_id, image_id) pairs in file order, or is image_key[(scene_id, image_id)].
    A record with a malformed RLE raises ValueError naming it."""
    from .pose_estimator import add_instance_id

    if isinstance(path_or_records, (str, Path)):
        records = json.loads(Path(path_or_records).read_text())
    else:
        records = list(path_or_records)
    rows, boxes, order = [], [], {}
    for r, rec in enumerate(records):
        if "image_id" not in rec and "view_id" not in rec:
            raise ValueError(f"record {r} has neither image_id nor view_id")
        scene, view = int(rec["scene_id"]), int(rec["image_id"] if "image_id" in rec else rec["view_id"])
        if image_key is not None:
            if (scene, view) not in image_key:
                raise ValueError(f"record {r}: image_key has no entry for scene {scene}, image {view}")
            im = int(image_key[(scene, view)])
        else:
            im = order.setdefault((scene, view), len(order))
        x, y, bw, bh = (float(v) for v in rec["bbox"])
        boxes.append([x, y, x + bw, y + bh])
        row = dict(label=label_format.format(int(rec["category_id"])), score=float(rec["score"]), scene_id=scene, view_id=view, batch_im_id=im)
        if "time" in rec:
            row["time"] = float(rec["time"])
        rows.append(row)
    infos = pd.DataFrame(rows, columns=["label", "score", "scene_id", "view_id", "batch_im_id"] + (["time"] if any("time" in r for r in rows) else []))
    if "time" in infos:
        infos["time"] = infos["time"].fillna(-1.0)
    tensors = dict(bboxes=torch.tensor(boxes, dtype=torch.float32).reshape(-1, 4).to(device))
    if records and all(rec.get("segmentation") is not None for rec in records):
        segs = []
        for r, rec in enumerate(records):
            seg = rec["segmentation"]
            try:
                if not isinstance(seg, Mapping) or len(seg["size"]) != 2:
                    raise ValueError("not an RLE dict with a size [h, w]")
                _counts_of(seg)
            except (ValueError, KeyError, TypeError) as e:
                raise ValueError(f"record {r} (scene {rec.get('scene_id')}, image {rows[r]['view_id']}): malformed RLE: {e}") from e
            segs.append(seg)
        masks, status = rle_to_masks(segs, device)
        bad = torch.nonzero(status).flatten().cpu().tolist()
        if bad:
            r = bad[0]
            raise ValueError(f"record {r} (scene {rows[r]['scene_id']}, image {rows[r]['view_id']}): malformed RLE, status {int(status[r])} "
                             f"(1 no entries, 2 a negative entry, 4 the entries do not sum to h * w)")
        tensors["masks"] = masks
    return add_instance_id(PandasTensorCollection(infos, **tensors))


# --------------------------------------------------------------------------- #
# poses: the BOP results CSV
def bop_results_name(method: str, dataset: str, split: str) -> str:
    """the file name bop_toolkit expects, as the reference builds it (bop.py:192-197): "<method with / and _ turned into ->_<dataset>-<split>.csv" """
    return f"{method.replace('/', '-').replace('_', '-')}_{dataset}-{split}.csv"


def save_bop_results(path: Union[str, Path], predictions: PandasTensorCollection, use_pose_score: bool = True, times=None) -> Path:
    """Write the 6D results CSV of `predictions` (poses [n,4,4] in metres; infos label, scene_id, view_id, pose_score or score, optionally
    time) as `convert_results_to_bop` and bop_toolkit's `save_bop_results` do: the header line, then per row scene_id, im_id (the view_id),
    obj_id (int(label.split("_")[-1])), score (pose_score, or score with use_pose_score=False), R (9 numbers, row-major, separated by
    spaces), t (3 numbers in MILLIMETRES: the translation times 1e3 in the poses' dtype, as the reference multiplies), time.  Numbers are
    written with `str` of the Python float, which reads back to the same bits.  times: None = the infos' `time` column, -1 if there is
    none; a sequence [n]; or a mapping {(scene_id, view_id): seconds}.  Lines are joined by newlines without a trailing one, like the
    toolkit's writer."""
    infos = predictions.infos
    n = len(infos)
    poses = predictions.poses.detach().cpu()
    if poses.shape != (n, 4, 4):
        raise ValueError(f"poses must be [{n},4,4], got {tuple(poses.shape)}")
    R = poses[:, :3, :3].reshape(n, 9).tolist()
    t = (poses[:, :3, 3] * 1e3).tolist()
    score_field = "pose_score" if use_pose_score else "score"
    if n and score_field not in infos:
        raise ValueError(f"predictions.infos has no column {score_field!r}")
    lines = [BOP_RESULTS_HEADER]
    for r in range(n):
        row = infos.iloc[r]
        scene, view = int(row.scene_id), int(row.view_id)
        if times is None:
            time = row.time if "time" in infos else -1
        elif isinstance(times, Mapping):
            time = times[(scene, view)]
        else:
            time = times[r]
        time = -1 if time is None or float(time) == -1 else float(time)
        lines.append(f"{scene},{view},{_obj_id(row.label)},{float(row[score_field])},{' '.join(map(str, R[r]))},{' '.join(map(str, t[r]))},{time}")
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text("\n".join(lines))
    return path


def load_bop_results(path: Union[str, Path], label_format: str = "obj_{:06d}") -> PandasTensorCollection:
    """A 6D results CSV -> a collection with poses [n,4,4] float32 in METRES (t / 1e3 in float64, then rounded once) and infos label
    (label_format of obj_id), scene_id, view_id, score, pose_score (both the file's score), time."""
    lines = [l for l in Path(path).read_text().splitlines() if l.strip()]
    if not lines or lines[0].strip() != BOP_RESULTS_HEADER:
        raise ValueError(f"{path}: the first line must be {BOP_RESULTS_HEADER!r}")
    rows, poses = [], []
    for k, line in enumerate(lines[1:], start=2):
        f = line.split(",")
        if len(f) != 7:
            raise ValueError(f"{path}, line {k}: 7 fields expected, got {len(f)}")
        R, t = np.array(f[4].split(), np.float64), np.array(f[5].split(), np.float64)
        if R.shape != (9,) or t.shape != (3,):
            raise ValueError(f"{path}, line {k}: R must hold 9 numbers and t 3")
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R.reshape(3, 3), t / 1e3
        poses.append(T)
        score = float(f[3])
        rows.append(dict(label=label_format.format(int(f[2])), scene_id=int(f[0]), view_id=int(f[1]), score=score, pose_score=score, time=float(f[6])))
    infos = pd.DataFrame(rows, columns=["label", "scene_id", "view_id", "score", "pose_score", "time"])
    return PandasTensorCollection(infos, poses=torch.from_numpy(np.asarray(poses, np.float64).reshape(-1, 4, 4)).float())

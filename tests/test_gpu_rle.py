"""GPU: the run-length kernels (csrc/rle.hip) through the C ABI and the wrappers.  mp_rle_count, mp_rle_encode and mp_rle_decode against
the host emulation built from the same rules header (tests/rle_emul.cpp), integer for integer, on the shapes and mask kinds of the
contract test with 1, 3 and 300 masks and on a batch of 480 x 640; bool and uint8 inputs, a tensor at an odd byte offset, every
rows_per_segment; areas and boxes against numpy; the round trip; the argument rules (refused before any launch); malformed lists (a
status and a zero mask: validation paths, every offset handed over is in range); and detections written to a BOP file and read back.
Reads nothing outside the tree."""
import numpy as np
import pandas as pd
import pytest
import torch

from tests.support import rle as sr

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _abi_encode(masks_t, rows=0):
    """the three entry points one by one, on tensors of exactly the stated sizes -> numpy counts, offsets, areas, boxes"""
    from megapose6d_amd import _lib
    from megapose6d_amd import engine as eng

    lib = _lib.load()
    n, h, w = masks_t.shape
    ws = torch.empty(max(lib.mp_rle_workspace_bytes(n, h, w, rows), 256), dtype=torch.uint8, device="cuda")
    n_counts = torch.full((n,), -5, dtype=torch.int32, device="cuda")
    areas, boxes = torch.full((n,), -5, dtype=torch.int32, device="cuda"), torch.full((n, 4), -5, dtype=torch.int32, device="cuda")
    _lib.check(lib.mp_rle_count(masks_t.data_ptr(), n, h, w, rows, n_counts.data_ptr(), areas.data_ptr(), boxes.data_ptr(), ws.data_ptr(), ws.numel(),
                                eng._stream()))
    offsets = np.concatenate([[0], np.cumsum(n_counts.cpu().numpy(), dtype=np.int64)]).astype(np.int64)
    counts = torch.full((int(offsets[-1]),), -7, dtype=torch.int32, device="cuda")
    _lib.check(lib.mp_rle_encode(masks_t.data_ptr(), n, h, w, rows, offsets.ctypes.data, counts.data_ptr(), counts.numel(), ws.data_ptr(), ws.numel(),
                                 eng._stream()))
    return counts.cpu().numpy(), offsets, areas.cpu().numpy(), boxes.cpu().numpy()


def _same(got, want, what=""):
    for g, e, name in zip(got, want, ("counts", "offsets", "areas", "boxes")):
        g = g.cpu().numpy() if isinstance(g, torch.Tensor) else g
        assert g.dtype == e.dtype and np.array_equal(g, e), (name, what)


def _kinds_batch(n, h, w):
    return sr.batch([sr.KINDS[i % len(sr.KINDS)] for i in range(n)], h, w)


@pytest.mark.parametrize("h,w", sr.SHAPES)
def test_the_three_entry_points_equal_the_emulation_with_1_and_3_masks(h, w):
    from megapose6d_amd import engine as eng

    for n, kinds in ((1, ["noise"]), (3, ["checker_set", "noise", "run_across_columns"]), (len(sr.KINDS), sr.KINDS)):
        masks = sr.batch(kinds, h, w, seed=n)
        want = sr.emul_encode(masks)
        _same(_abi_encode(_dev(masks)), want, n)
        got = eng.rle_decode(_dev(want[0]), want[1], h, w)
        e_masks, e_status = sr.emul_decode(want[0], want[1], h, w)
        assert got[0].dtype == torch.uint8 and np.array_equal(got[0].cpu().numpy(), e_masks) and np.array_equal(got[1].cpu().numpy(), e_status)
        assert not e_status.any() and np.array_equal(e_masks, (masks != 0).astype(np.uint8))


@pytest.mark.parametrize("h,w", [(3, 5), (63, 65)])
def test_300_masks_in_one_call(h, w):
    from megapose6d_amd import engine as eng

    masks = _kinds_batch(300, h, w)
    want = sr.emul_encode(masks)
    _same(_abi_encode(_dev(masks)), want)
    got = eng.rle_encode(_dev(masks))
    assert got[0].dtype == torch.int32 and got[1].dtype == torch.int64 and got[0].is_cuda and got[1].is_cuda
    _same(got, want)
    back, status = eng.rle_decode(got[0], got[1], h, w)
    assert not bool(status.any()) and torch.equal(back.bool(), _dev(masks) != 0)


@pytest.fixture(scope="module")
def frames():
    """8 masks of 480 x 640: blobs, noise, a checkerboard, full, empty -> (masks, what the emulation gives)"""
    h, w = 480, 640
    masks = np.concatenate([sr.blobs(4, h, w, seed=3), sr.batch(["noise", "checker_unset", "full", "empty"], h, w)])
    return masks, sr.emul_encode(masks)


def test_a_batch_of_480_x_640(frames):
    from megapose6d_amd import engine as eng

    masks, want = frames
    _same(_abi_encode(_dev(masks)), want)
    for m, a, b in zip(masks, want[2], want[3]):                       # areas and boxes against numpy
        area, box = sr.restated_area_box(m)
        assert a == area and b.tolist() == box
    back, status = eng.rle_decode(_dev(want[0]), _dev(want[1]), 480, 640)     # (offsets as a device tensor)
    assert not bool(status.any()) and torch.equal(back.bool(), _dev(masks) != 0)


def test_input_forms_and_segment_sizes(frames):
    from megapose6d_amd import engine as eng

    for masks in (frames[0][:3], sr.batch(sr.KINDS, 64, 64), sr.batch(sr.KINDS, 65, 257)):
        want = sr.emul_encode(masks)
        n, h, w = masks.shape
        for rows in (1, 7, 64, 0):
            _same(eng.rle_encode(_dev(masks), rows_per_segment=rows), want, rows)
        _same(eng.rle_encode(_dev(masks != 0)), want, "bool")
        assert _dev(masks != 0).dtype == torch.bool
        # the same bytes at an odd byte offset: rows of 16 columns that start off a 16-byte boundary take the byte loads
        flat = torch.zeros(masks.size + 1, dtype=torch.uint8, device="cuda")
        flat[1:] = _dev(masks).flatten()
        odd = flat[1:].view(n, h, w)
        assert odd.data_ptr() % 2 == 1 and odd.is_contiguous()
        _same(eng.rle_encode(odd), want, "odd offset")
        out = torch.zeros(masks.size + 1, dtype=torch.uint8, device="cuda")      # (decoding writes 0 / 1 bytes wherever the tensor lies)
        back, _ = eng.rle_decode(_dev(want[0]), want[1], h, w)
        out[1:] = back.flatten()
        assert torch.equal(out[1:].view(n, h, w).bool(), _dev(masks) != 0) and int(out[0]) == 0


def test_areas_boxes_and_the_round_trip_on_random_shapes():
    from megapose6d_amd import engine as eng

    rng = np.random.RandomState(5)
    for h, w in ((17, 31), (40, 16), (5, 100), (33, 48)):
        masks = np.where(rng.uniform(size=(6, h, w)) < 0.08, sr.SET_VALUES[rng.randint(0, 4, size=(6, h, w))], 0).astype(np.uint8)
        masks[5] = 0
        counts, offsets, areas, boxes = eng.rle_encode(_dev(masks))
        for m, a, b in zip(masks, areas.cpu().numpy(), boxes.cpu().numpy()):
            area, box = sr.restated_area_box(m)
            assert a == area and b.tolist() == box
        assert boxes[5].tolist() == [0, 0, -1, -1] and counts[offsets[5]:].tolist() == [h * w]
        back, status = eng.rle_decode(counts, offsets, h, w)
        assert not bool(status.any()) and torch.equal(back.bool(), _dev(masks) != 0)
        _same((counts, offsets, areas, boxes), sr.restated_encode(masks))


def test_bad_arguments_are_refused_before_any_launch():
    from megapose6d_amd import _lib
    from megapose6d_amd import engine as eng

    lib = _lib.load()
    n, h, w = 2, 5, 20
    masks = _dev(sr.batch(["noise", "rectangle"], h, w))
    want = sr.emul_encode(masks.cpu().numpy())
    ws = torch.zeros(lib.mp_rle_workspace_bytes(n, h, w, 0), dtype=torch.uint8, device="cuda")
    out = torch.full((n,), -5, dtype=torch.int32, device="cuda")
    s = eng._stream()

    def count(m=masks.data_ptr(), n=n, h=h, o=out.data_ptr(), wsp=ws.data_ptr(), wsn=ws.numel(), rows=0):
        return lib.mp_rle_count(m, n, h, w, rows, o, None, None, wsp, wsn, s)

    assert count(m=None) != 0 and count(o=None) != 0 and count(wsp=None) != 0 and count(h=0) != 0 and count(n=-1) != 0 and count(rows=-1) != 0
    assert count(wsn=ws.numel() - 256) != 0
    assert b"workspace" in lib.mp_last_error()
    assert lib.mp_rle_workspace_bytes(1, 65536, 32768, 0) == 0 and lib.mp_rle_workspace_bytes(1, 0, 4, 0) == 0       # 2^31 pixels; h = 0
    assert lib.mp_rle_workspace_bytes(1, 46340, 46340, 0) > 0                                                         # just below: only sized
    torch.cuda.synchronize()
    assert out.tolist() == [-5, -5] and not bool(ws.any())
    assert count(n=0) == 0 and count(n=0, m=None, o=None, wsp=None, wsn=0) == 0                                        # n = 0: a no-op
    assert count() == 0
    counts = torch.full((len(want[0]),), -7, dtype=torch.int32, device="cuda")
    off = want[1]

    def encode(m=masks.data_ptr(), n=n, h=h, offsets=off, c=counts.data_ptr(), cap=counts.numel(), wsn=ws.numel()):
        return lib.mp_rle_encode(m, n, h, w, 0, None if offsets is None else offsets.ctypes.data, c, cap, ws.data_ptr(), wsn, s)

    assert encode(m=None) != 0 and encode(offsets=None) != 0 and encode(c=None) != 0 and encode(h=0) != 0
    assert encode(cap=counts.numel() - 1) != 0 and b"capacity" in lib.mp_last_error()
    assert encode(wsn=ws.numel() - 256) != 0
    assert encode(offsets=np.array([1, 3, int(off[2])], np.int64)) != 0 and encode(offsets=np.array([0, int(off[2]), int(off[1])], np.int64)) != 0
    torch.cuda.synchronize()
    assert bool((counts == -7).all())
    assert encode(n=0) == 0 and encode() == 0
    assert np.array_equal(counts.cpu().numpy(), want[0]) and np.array_equal(out.cpu().numpy(), np.diff(off).astype(np.int32))
    # decode
    dmask = torch.full((n, h, w), 9, dtype=torch.uint8, device="cuda")
    status = torch.full((n,), -5, dtype=torch.int32, device="cuda")
    dws = torch.zeros(lib.mp_rle_decode_workspace_bytes(n, h, w, counts.numel()), dtype=torch.uint8, device="cuda")

    def decode(c=counts.data_ptr(), offsets=off, cap=counts.numel(), n=n, h=h, m=dmask.data_ptr(), st=status.data_ptr(), wsn=dws.numel()):
        return lib.mp_rle_decode(c, None if offsets is None else offsets.ctypes.data, cap, n, h, w, m, st, dws.data_ptr(), wsn, s)

    assert decode(c=None) != 0 and decode(offsets=None) != 0 and decode(m=None) != 0 and decode(st=None) != 0 and decode(h=0) != 0
    assert decode(cap=counts.numel() - 1) != 0 and decode(wsn=dws.numel() - 256) != 0
    assert decode(offsets=np.array([0, int(off[2]), int(off[1])], np.int64)) != 0                                      # descending
    torch.cuda.synchronize()
    assert bool((dmask == 9).all()) and status.tolist() == [-5, -5]
    assert decode(n=0) == 0 and decode() == 0
    assert torch.equal(dmask, (masks != 0).to(torch.uint8)) and status.tolist() == [0, 0]
    with pytest.raises(eng.EngineError):
        eng.rle_encode(masks.float())
    with pytest.raises(eng.EngineError):
        eng.rle_decode(counts, np.array([0, counts.numel() + 1]), h, w)


@pytest.mark.parametrize("h,w", [(3, 5), (63, 65)])
def test_malformed_lists_cost_a_status_and_a_zero_mask(h, w):
    from megapose6d_amd import engine as eng

    cases = sr.malformed(h, w)
    good = sr.restated_counts(sr.make_mask("noise", h, w))
    counts, offsets = sr.ragged([good] + [c for c, _ in cases.values()] + [good])
    masks, status = eng.rle_decode(_dev(counts), offsets, h, w)
    e_masks, e_status = sr.emul_decode(counts, offsets, h, w)
    assert status.tolist() == [0] + [st for _, st in cases.values()] + [0] == e_status.tolist()
    assert np.array_equal(masks.cpu().numpy(), e_masks) and not bool(masks[1:-1].any()) and bool(masks[0].any())


@pytest.mark.parametrize("h,w", [(3, 5), (63, 65), (65, 257)])
def test_runs_of_length_zero_inside_a_list(h, w):
    """a column that leaves its run steps into a run of length zero: the one path of the fill that searches"""
    from megapose6d_amd import engine as eng

    lists = sr.zero_run_lists(h, w)
    counts, offsets = sr.ragged(lists)
    masks, status = eng.rle_decode(_dev(counts), offsets, h, w)
    e_masks, e_status = sr.emul_decode(counts, offsets, h, w)
    assert not bool(status.any()) and not e_status.any() and np.array_equal(masks.cpu().numpy(), e_masks)
    for m, l in zip(e_masks, lists):
        assert np.array_equal(m, sr.restated_mask(l, h, w)[0])


@pytest.mark.parametrize("compressed", [False, True])
def test_detections_through_a_bop_file_and_back(tmp_path, compressed):
    import json

    from megapose6d_amd import bop_files as bf
    from megapose6d_amd.tcoll import PandasTensorCollection
    from megapose6d_amd.types import assert_detections_valid

    h, w = 48, 72
    masks = torch.from_numpy(sr.blobs(5, h, w, seed=2)).cuda().bool()
    masks[4] = False                                                   # a detection without a pixel: the list [h * w]
    _, _, _, boxes = sr.restated_encode(masks.cpu().numpy())
    bboxes = torch.from_numpy(boxes.astype(np.float32)).cuda() + torch.tensor([0.0, 0.0, 1.0, 1.0], device="cuda")
    bboxes[4] = torch.tensor([3.5, 4.25, 10.0, 12.75])
    infos = pd.DataFrame(dict(label=["obj_000003", "obj_000011", "obj_000003", "obj_000003", "obj_000021"], score=[0.5, 0.9375, 0.1, 0.7, 0.3],
                              scene_id=[48, 48, 48, 50, 50], view_id=[7, 7, 7, 1, 1], batch_im_id=[0, 0, 0, 1, 1], instance_id=[0, 0, 1, 0, 0]))
    det = PandasTensorCollection(infos, bboxes=bboxes, masks=masks)
    assert_detections_valid(det)
    path = bf.save_bop_detections(tmp_path / "coco_ycbv-test.json", det, compressed=compressed)
    records = json.loads(path.read_text())
    assert len(records) == 5 and all(isinstance(r["segmentation"]["counts"], str if compressed else list) for r in records)
    assert records[4]["segmentation"] == {"size": [h, w], "counts": bf.rle_to_string([h * w]) if compressed else [h * w]}
    assert records[1]["image_id"] == 7 and records[1]["category_id"] == 11 and records[3]["scene_id"] == 50 and records[0]["time"] == -1
    back = bf.load_bop_detections(path, device="cuda")
    assert_detections_valid(back)
    assert back.masks.dtype == torch.bool and back.masks.is_cuda and torch.equal(back.masks, masks)
    # x2 - x1 and x1 + (x2 - x1) are exact on these boxes (quarter pixels below 2^7), and float32 -> JSON -> float32 keeps the bits
    assert back.bboxes.dtype == torch.float32 and torch.equal(back.bboxes, bboxes)
    for col in ("label", "scene_id", "view_id", "batch_im_id", "instance_id"):
        assert back.infos[col].tolist() == infos[col].tolist(), col
    assert np.array_equal(back.infos["score"].to_numpy(), infos["score"].to_numpy())
    # the dict forms themselves
    rle = bf.masks_to_rle(masks, compressed=compressed)
    assert [r["segmentation"] for r in records] == rle
    again, status = bf.rle_to_masks(rle, "cuda")
    assert torch.equal(again, masks) and not bool(status.any())
    # a record with a malformed list is named
    records[2]["segmentation"] = {"size": [h, w], "counts": [5, h * w]}
    with pytest.raises(ValueError, match="record 2 "):
        bf.load_bop_detections(records, device="cuda")

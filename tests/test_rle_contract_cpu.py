"""CPU: the contract of COCO's run-length encoding as csrc/rle_core.h states it -- the host emulation of the kernels (tests/rle_emul.cpp,
built on the header) against an independent numpy restatement written from the contract's text (tests/support/rle.py), exactly; the
worked example and the string table as literal values; malformed lists; and the emulation under the sanitizers."""
import subprocess

import numpy as np
import pytest

from megapose6d_amd import bop_files as bf
from tests.support import rle as sr

STRING_TABLE = [([15], "?"), ([0, 15], "0?"), ([10, 1, 4], ":14"), ([2, 5, 2, 2, 1, 3], "252MO1"), ([307200], "PP\\9"),
                ([1000, 5, 995, 7, 300000], "Xo05So02moS9")]


def _lists(counts, offsets):
    return [counts[offsets[m]:offsets[m + 1]].tolist() for m in range(len(offsets) - 1)]


def test_worked_example_and_limits():
    m = np.array([[0, 1], [1, 1], [0, 0]], np.uint8)
    assert sr.restated_counts(m) == [1, 1, 1, 2, 1]
    counts, offsets, areas, boxes = sr.emul_encode(m[None])
    assert counts.tolist() == [1, 1, 1, 2, 1] and offsets.tolist() == [0, 5] and areas.tolist() == [3] and boxes.tolist() == [[0, 0, 1, 1]]
    assert sr.limits() == dict(max_pixels=2 ** 31 - 2, default_rows=32, unit=16)
    # empty is [h * w], full is [0, h * w], the checkerboard that starts set on 3 x 5 has h * w + 1 = 16 entries
    assert sr.emul_encode(sr.batch(["empty", "full", "checker_set"], 3, 5))[0].tolist() == [15] + [0, 15] + [0] + [1] * 15


@pytest.mark.parametrize("h,w", sr.SHAPES)
def test_emulation_equals_restatement_on_every_kind_and_segment_size(h, w):
    masks = sr.batch(sr.KINDS, h, w)
    want = sr.restated_encode(masks)
    for rows in sorted({0, 1, 2, 7, h, h + 3}):
        got = sr.emul_encode(masks, rows)
        for g, e, name in zip(got, want, ("counts", "offsets", "areas", "boxes")):
            assert np.array_equal(g, e), (name, rows)
    counts, offsets = want[0], want[1]
    for l in _lists(counts, offsets):
        assert sum(l) == h * w and len(l) <= h * w + 1 and l[0] >= 0 and all(c >= 1 for c in l[1:])
    # the kinds do what their names say at this shape
    by_kind = dict(zip(sr.KINDS, _lists(counts, offsets)))
    assert by_kind["empty"] == [h * w] and by_kind["full"] == [0, h * w]
    assert by_kind["first_pixel"][0] == 0 and by_kind["last_pixel"][-1] == 1
    if h % 2 == 1 or w == 1:     # the walk then alternates at every pixel: the longest possible list
        assert len(by_kind["checker_set"]) == h * w + 1
    if h > 1 and w > 1:
        # h even: the bottom of a column and the top of the next are both set or both unset, so runs of 2 cross every boundary
        assert (2 in by_kind["checker_set"]) == (h % 2 == 0)
        x = (w - 1) // 2
        assert by_kind["run_across_columns"] == [x * h + h - 1, 2, h * w - (x * h + h - 1) - 2]
        assert by_kind["transition_at_column"] == ([(w // 2) * h, h, h * w - (w // 2 + 1) * h] if w // 2 + 1 < w else [(w // 2) * h, h])
    # decoding: emulation against restatement, and the round trip
    masks_e, status = sr.emul_decode(counts, offsets, h, w)
    assert not status.any() and np.array_equal(masks_e, (masks != 0).astype(np.uint8))
    for m, l in zip(masks, _lists(counts, offsets)):
        back, st = sr.restated_mask(l, h, w)
        assert st == 0 and np.array_equal(back, (m != 0).astype(np.uint8))


def test_string_table_and_round_trips():
    for counts, s in STRING_TABLE:
        assert bf.rle_to_string(counts) == s and sr.restated_to_string(counts) == s, counts
        assert bf.rle_from_string(s) == counts and sr.restated_from_string(s) == counts, s
    # every case of the contract test, and lists whose deltas are negative (the fourth entry on is stored against the entry two before)
    lists = [[5, 100, 3, 2, 1, 50], [0, 70000, 1, 3, 69000, 2], [40000, 1, 1, 39999]]
    for h, w in sr.SHAPES:
        counts, offsets = sr.restated_encode(sr.batch(sr.KINDS, h, w))[:2]
        lists += _lists(counts, offsets)
    assert any(l[i] < l[i - 2] for l in lists for i in range(3, len(l)))
    for l in lists:
        s = bf.rle_to_string(l)
        assert s == sr.restated_to_string(l) and all(48 <= ord(c) < 112 for c in s)
        assert bf.rle_from_string(s) == l and sr.restated_from_string(s) == l
    with pytest.raises(ValueError):
        bf.rle_from_string("P")          # bit 0x20 set: a digit must follow
    with pytest.raises(ValueError):
        bf.rle_from_string("1 2")


@pytest.mark.parametrize("h,w", [(3, 5), (63, 65)])
def test_malformed_lists_give_a_status_and_a_zero_mask(h, w):
    cases = sr.malformed(h, w)
    good = sr.restated_counts(sr.make_mask("rectangle", h, w))
    lists = [good] + [c for c, _ in cases.values()] + [good]
    counts, offsets = sr.ragged(lists)
    masks, status = sr.emul_decode(counts, offsets, h, w)
    assert status.tolist() == [0] + [s for _, s in cases.values()] + [0]
    for m, (l, st) in zip(masks[1:-1], cases.values()):
        assert not m.any() and sr.restated_mask(l, h, w)[1] == st
    want = (sr.make_mask("rectangle", h, w) != 0).astype(np.uint8)
    assert np.array_equal(masks[0], want) and np.array_equal(masks[-1], want)      # the neighbours of a malformed list are untouched


def test_emulation_refuses_bad_arguments():
    import ctypes as C

    lib = sr.load()
    m = np.zeros((1, 2, 2), np.uint8)
    out = np.zeros(8, np.int32)
    off = np.array([0, 1], np.int64)
    assert lib.rle_count_emul(sr._p(m), C.c_int(1), C.c_int(0), C.c_int(2), C.c_int(0), sr._p(out), None, None) != 0
    assert lib.rle_count_emul(sr._p(m), C.c_int(1), C.c_int(65536), C.c_int(32768), C.c_int(0), sr._p(out), None, None) != 0    # 2^31 pixels
    assert lib.rle_encode_emul(sr._p(m), C.c_int(1), C.c_int(2), C.c_int(2), C.c_int(0), sr._p(off), sr._p(out), C.c_longlong(0)) != 0
    assert lib.rle_decode_emul(sr._p(out), sr._p(np.array([0, 9], np.int64)), C.c_longlong(8), C.c_int(1), C.c_int(2), C.c_int(2), sr._p(m),
                               sr._p(out)) != 0


def test_emulation_under_the_sanitizers(tmp_path):
    """the emulation as a stand-alone program (tests/rle_asan_main.cpp) under the address and undefined-behaviour sanitizers, on arrays of
    exactly the call's sizes: a neighbour read before the first pixel, a store past a list's end or a search past the ends would be
    caught here.  The program compares every call with what the plain build returned."""
    n_calls = 0
    with open(tmp_path / "calls.bin", "wb") as f:
        for (h, w), rows in (((1, 1), 0), ((1, 67), 1), ((67, 1), 7), ((3, 5), 2), ((63, 65), 0), ((63, 65), 66)):
            masks = sr.batch(sr.KINDS, h, w)
            counts, offsets, areas, boxes = sr.emul_encode(masks, rows)
            f.write(np.array([0, len(masks), h, w, rows, len(counts)], np.int32).tobytes())
            f.write(masks.tobytes() + offsets.tobytes() + counts.tobytes() + areas.tobytes() + boxes.tobytes())
            n_calls += 1
        for h, w in ((3, 5), (63, 65)):
            lists = [c for c, _ in sr.malformed(h, w).values()] + [sr.restated_counts(sr.make_mask("noise", h, w))]
            counts, offsets = sr.ragged(lists)
            masks, status = sr.emul_decode(counts, offsets, h, w)
            f.write(np.array([1, len(lists), h, w, 0, len(counts)], np.int32).tobytes())
            f.write(offsets.tobytes() + counts.tobytes() + masks.tobytes() + status.tobytes())
            n_calls += 1
    exe = tmp_path / "rle_asan"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    str(sr.CSRC), "-I", str(sr.TESTS), "-o", str(exe), str(sr.TESTS / "rle_asan_main.cpp")], check=True)
    run = subprocess.run([str(exe), str(tmp_path / "calls.bin")], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and run.stdout.strip() == f"{n_calls} calls, 0 bad", (run.stdout, run.stderr[-2000:])


@pytest.mark.parametrize("h,w", [(3, 5), (63, 65), (65, 257)])
def test_runs_of_length_zero_inside_a_list(h, w):
    lists = sr.zero_run_lists(h, w)
    counts, offsets = sr.ragged(lists)
    masks, status = sr.emul_decode(counts, offsets, h, w)
    assert not status.any() and masks[:3].any() and not masks[3].any()
    for m, l in zip(masks, lists):
        want, st = sr.restated_mask(l, h, w)
        assert st == 0 and np.array_equal(m, want)

"""CPU: the value of every multi-region workspace size function, pinned to the values of the commit BEFORE the layouts moved onto the
shared carver (`WsCarver`, csrc/common.h).  The size functions are pure host code, so the library answers them without a device.

`tests/golden/workspace_bytes.json` is a list of [function, arguments, bytes].  It was recorded from a build of that earlier commit, never
from the code under test:

    python tests/test_workspace_bytes_cpu.py path/to/the/earlier/libmp_engine.so

writes the file from CASES below.  A layout that gains, loses or resizes a region without the size function's value being meant to
change fails here; a value that is meant to change needs a new recording from a library whose value is trusted, and a reason.

Per function: the zero-slack shape that tests/test_gpu_workspace_contract.py names (its "tight" cases), shapes where a region is no
multiple of 256 bytes, a zero count where the function accepts one, and refused arguments (0).  mp_icp_nn_workspace_bytes refuses
nothing.  An argument given as a list is a host int32 array (the prefix array / the point counts the function reads).
"""
import ctypes as C
import json
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "workspace_bytes.json"

_TEASER = [[n, h, w, stride, sel] for sel in (0, 1, 2) for stride in (1, 100, 1024) for n, h, w in ((3, 24, 32), (1, 0, 0))]
CASES = {
    "mp_icp_nn_workspace_bytes": [[1, 1, 3, 3], [2, 5, 37, 53], [1, 0, 8, 8], [3, 7, 480, 640], [4, 2, 512, 512], [1, 3, 1, 1]],
    "mp_teaser_workspace_bytes_ex": _TEASER + [[0, 24, 32, 100, 0], [7, 1, 1, 33, 2], [300, 5, 7, 65, 2], [65535, 0, 0, 1, 1],
                                               [-1, 24, 32, 100, 0], [3, 24, 32, 0, 0], [3, 24, 32, 1025, 0], [3, 24, 32, 100, 3],
                                               [3, 24, 32, 100, -1], [3, -1, 32, 100, 0], [1, 32768, 32768, 100, 0]],
    "mp_teaser_workspace_bytes": [[3, 24, 32], [1, 37, 53], [0, 24, 32], [5, 0, 0], [-1, 24, 32], [1, 32768, 32768]],
    "mp_max_clique_workspace_bytes": [[n, stride] for stride in (1, 100, 1024) for n in (1, 3, 257)] + [[0, 100], [-1, 100], [3, 0], [3, 1025]],
    "mp_rle_workspace_bytes": [[32, 63, 65, 0], [1, 1, 1, 0], [10, 65, 257, 0], [10, 65, 257, 7], [3, 480, 640, 1], [5, 33, 17, 1000], [0, 63, 65, 0],
                               [-1, 63, 65, 0], [1, 0, 65, 0], [1, 63, 65, -1], [1, 65536, 65536, 0], [1 << 20, 1024, 1024, 1]],
    "mp_rle_decode_workspace_bytes": [[32, 63, 65, 4096], [1, 1, 1, 1], [10, 65, 257, 1234], [3, 480, 640, 100001], [0, 63, 65, 10], [4, 63, 65, 0],
                                      [4, 63, 65, -1], [-1, 63, 65, 10], [1, 63, 0, 10], [1 << 20, 1024, 1024, 10]],
    "mp_tsdf_extract_workspace_bytes": [[16, 32, 32], [2, 2, 2], [33, 17, 9], [96, 96, 64], [512, 512, 512], [1, 32, 32], [16, 32, 513], [1024, 1024, 1024]],
    "mp_mesh_select_workspace_bytes": [[262146, 262144], [3, 1], [1000, 1999], [4097, 8193], [0, 0], [0, 5], [7, 0], [-1, 5], [5, -1], [(1 << 29) + 1, 5]],
    "mp_mesh_cluster_workspace_bytes": [[128, 126, 64, 2, 1], [3, 1, 1, 1, 1], [1000, 1999, 7, 5, 3], [50, 96, 33, 17, 9], [100000, 200000, 64, 64, 64],
                                        [0, 0, 4, 4, 4], [5, 0, 512, 512, 512], [-1, 5, 4, 4, 4], [5, 5, 0, 4, 4], [5, 5, 513, 4, 4],
                                        [5, 5, 512, 512, 513]],
    "mp_surface_sample_scratch_bytes": [[1, [0, 64], 64, 0], [1, [0, 1], 1, 0], [3, [0, 257, 322, 334], 65, 0], [3, [0, 257, 322, 334], 65, 64],
                                        [2, [0, 5000, 5001], 1000, 128], [1, [0, 64], 64, 2048], [0, [0], 64, 0], [1, [0, 0], 64, 0], [1, [0, 64], 0, 0],
                                        [1, [0, 64], 64, 63], [2, [0, 64, 10], 64, 0], [1, [-1, 64], 64, 0], [1, [0, (1 << 22) + 1], 64, 0]],
    "mp_model_info_scratch_bytes": [[1, [1], 0], [1, [100], 0], [3, [257, 65, 8], 0], [3, [257, 65, 8], 64], [2, [5000, 1], 1024], [63, [10] * 63, 0],
                                    [64, [10] * 64, 128], [0, [], 0], [1, [0], 0], [2, [5, -1], 0], [1, [100], 63], [1, [100], 1088]],
}
ITEMS = [(fn, args) for fn, cases in CASES.items() for args in cases]


def _call(lib, fn, args):
    from megapose6d_amd import _lib

    restype, argtypes = _lib.SIGNATURES[fn]
    f = getattr(lib, fn)
    f.restype, f.argtypes = restype, argtypes
    keep = [(C.c_int32 * max(len(a), 1))(*a) if isinstance(a, list) else a for a in args]
    return int(f(*[C.cast(a, C.c_void_p) if isinstance(a, C.Array) else a for a in keep]))


def record(lib_path):
    """the few lines that record the fixture, from a library built at the commit before the change under test"""
    lib = C.CDLL(str(lib_path))
    GOLDEN.write_text("[\n" + ",\n".join(json.dumps([fn, args, _call(lib, fn, args)]) for fn, args in ITEMS) + "\n]\n")


@pytest.fixture(scope="module")
def golden():
    rows = json.loads(GOLDEN.read_text())
    assert [(fn, args) for fn, args, _ in rows] == ITEMS, "the fixture was not recorded from this module's CASES"
    return {(fn, json.dumps(args)): want for fn, args, want in rows}


@pytest.fixture(scope="module")
def lib():
    from megapose6d_amd import _lib

    return _lib.load()


def test_the_fixture_covers_every_function_with_a_zero_slack_an_odd_and_a_refused_shape(golden):
    by_fn = {fn: [golden[(fn, json.dumps(a))] for a in cases] for fn, cases in CASES.items()}
    assert len(by_fn) == 11
    for fn, values in by_fn.items():
        assert any(v > 0 for v in values), fn
        assert fn == "mp_icp_nn_workspace_bytes" or 0 in values, (fn, "no refused argument set")
        assert len(set(values)) >= 4, fn
    # the values checked by hand on a CPU-only process before the change
    assert golden[("mp_tsdf_extract_workspace_bytes", "[16, 32, 32]")] == 82432
    assert golden[("mp_teaser_workspace_bytes_ex", "[3, 24, 32, 100, 2]")] == 641024
    # the zero-slack shapes: the last region is a whole number of 256-byte units, so no padding hides a missing byte
    assert golden[("mp_rle_workspace_bytes", "[32, 63, 65, 0]")] % 256 == 0 and 32 * 2 * 4 == 256
    assert golden[("mp_surface_sample_scratch_bytes", "[1, [0, 64], 64, 0]")] % 256 == 0 and 64 * 8 == 512
    assert golden[("mp_mesh_cluster_workspace_bytes", "[128, 126, 64, 2, 1]")] % 256 == 0 and 128 * 52 == 26 * 256
    # the TEASER functions: three selections x strides 1, 100, 1024
    assert {(a[3], a[4]) for a in CASES["mp_teaser_workspace_bytes_ex"][:18]} == {(s, k) for s in (1, 100, 1024) for k in (0, 1, 2)}
    # the short form is the long one at stride 1024, k-core
    for n, h, w in CASES["mp_teaser_workspace_bytes"]:
        if [n, h, w, 1024, 0] in CASES["mp_teaser_workspace_bytes_ex"]:
            assert golden[("mp_teaser_workspace_bytes", json.dumps([n, h, w]))] == golden[("mp_teaser_workspace_bytes_ex", json.dumps([n, h, w, 1024, 0]))]


@pytest.mark.parametrize("fn", list(CASES))
def test_size_function_returns_what_it_returned_before_the_carver(fn, golden, lib):
    for args in CASES[fn]:
        assert _call(lib, fn, args) == golden[(fn, json.dumps(args))], (fn, args)


if __name__ == "__main__":
    sys.path.insert(0, str(ROOT))
    record(sys.argv[1])
    print(f"{len(ITEMS)} rows -> {GOLDEN}")

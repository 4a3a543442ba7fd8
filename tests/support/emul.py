"""TEST SUPPORT: the host emulations (tests/*_emul.cpp on the arithmetic headers of megapose6d_amd/csrc) as shared libraries, built on
first use under tests/_build, and the pointer / array helpers of their ctypes wrappers."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path
from typing import Dict, Optional, Sequence

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
CSRC = ROOT / "megapose6d_amd" / "csrc"
TESTS = ROOT / "tests"
_libs: Dict[str, C.CDLL] = {}


def build(lib_name: str, sources: Sequence[Path], fma: bool = True) -> C.CDLL:
    """tests/_build/lib<lib_name>.so of sources[0]; the other sources are what it includes: the library is rebuilt when any of them is
    newer.  No contraction in either case (the headers spell out every fmaf); fma=False also keeps fmaf from becoming an instruction."""
    if lib_name not in _libs:
        lib = TESTS / "_build" / f"lib{lib_name}.so"
        if not lib.is_file() or lib.stat().st_mtime < max(Path(s).stat().st_mtime for s in sources):
            lib.parent.mkdir(exist_ok=True)
            tmp = lib.with_suffix(".tmp.so")
            subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", *(["-mfma"] if fma else []), "-fno-fast-math", "-shared", "-fPIC",
                            "-I", str(CSRC), "-I", str(TESTS), "-o", str(tmp), str(sources[0])], check=True)
            tmp.replace(lib)
        _libs[lib_name] = C.CDLL(str(lib))
    return _libs[lib_name]


def _p(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, np.float32)


def _i32(a):
    return None if a is None else np.ascontiguousarray(a, np.int32)

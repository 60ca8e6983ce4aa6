"""CPU-side checks of the gallery-scale retrieval bindings: ``mvae_match_colsq``, ``mvae_match_rnorm``,
``mvae_match_ex``, ``mvae_pair_scores`` and ``mvae_match_merge`` are declared in ``include/mvae.h``,
bound in ``magic_amd/_lib.py`` with the header's arity and exported by the library;
``mvae_match_opts`` mirrors the header's struct; the additions leave the ABI version at 7."""
import ctypes
import os
import re

from magic_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mvae_match_colsq", "mvae_match_rnorm", "mvae_match_ex", "mvae_pair_scores", "mvae_match_merge")
FIELDS = ["rl", "rk", "key_base", "carry", "dist_ld", "thr_val", "thr_idx", "ahead"]


def header():
    src = open(os.path.join(ROOT, "include", "mvae.h")).read()
    return src, re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_entry_points_are_declared_bound_and_exported():
    _, code = header()
    lib = _lib.load()
    for name in NAMES:
        m = re.search(r"\bint %s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, f"{name} is not declared in include/mvae.h"
        assert name in _lib._SIGS and name in _lib.EXPORTED and hasattr(lib, name), name
        assert len(_lib._SIGS[name][0]) == len(m.group(1).split(",")), name
        assert _lib._SIGS[name][1] is ctypes.c_int


def test_match_opts_layout():
    """rl, rk, key_base, carry, dist_ld, thr_val, thr_idx, ahead in the header's order; LP64: 64
    bytes, offsets 0, 8, 16, 24, 32, 40, 48, 56."""
    o = _lib.mvae_match_opts
    assert [n for n, _ in o._fields_] == FIELDS
    assert ctypes.sizeof(o) == 64
    assert [getattr(o, n).offset for n in FIELDS] == [0, 8, 16, 24, 32, 40, 48, 56]
    _, code = header()
    body = re.search(r"typedef struct mvae_match_opts \{(.*?)\} mvae_match_opts;", code, flags=re.S).group(1)
    assert re.findall(r"(\w+)\s*[;,]", body) == FIELDS
    # the pointer argument of mvae_match_ex is that struct
    assert _lib._SIGS["mvae_match_ex"][0][7] is ctypes.POINTER(o)


def test_abi_version_stays_7():
    raw, _ = header()
    assert int(re.search(r"#define MVAE_ABI_VERSION (\d+)", raw).group(1)) == _lib.ABI_VERSION == 7
    assert _lib.load().mvae_abi_version() == 7

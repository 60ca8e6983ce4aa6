"""CPU-side checks of the retrieval entry points' bindings: ``mvae_embed_images`` and ``mvae_match``
are declared in ``include/mvae.h``, bound in ``magic_amd/_lib.py`` with the header's arity, and the
binding's ABI version is the header's (7)."""
import ctypes
import os
import re

from magic_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    src = open(os.path.join(ROOT, "include", "mvae.h")).read()
    return src, re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_abi_version_is_7_and_matches_header():
    raw, _ = header()
    assert int(re.search(r"#define MVAE_ABI_VERSION (\d+)", raw).group(1)) == _lib.ABI_VERSION == 7
    assert _lib.load().mvae_abi_version() == 7


def test_retrieval_entry_points_are_bound_with_the_header_arity():
    _, code = header()
    lib = _lib.load()
    for name in ("mvae_embed_images", "mvae_match"):
        assert name in _lib.EXPORTED and hasattr(lib, name)
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1)
        assert len(_lib._SIGS[name][0]) == len(args.split(",")), name
        assert _lib._SIGS[name][1] is ctypes.c_int


def test_images_descriptor_layout():
    """table, height, width, idx, divisor in the header's order (LP64: 8 + 4 + 4 + 8 + 4, padded)."""
    f = [n for n, _ in _lib.mvae_images._fields_]
    assert f == ["table", "height", "width", "idx", "divisor"]
    assert (ctypes.sizeof(_lib.mvae_images), _lib.mvae_images.idx.offset, _lib.mvae_images.divisor.offset) == (32, 16, 24)
    _, code = header()
    body = re.search(r"typedef struct mvae_images \{(.*?)\} mvae_images;", code, flags=re.S).group(1)
    names = re.findall(r"(\w+)\s*[;,]", body)
    assert names == ["table", "height", "width", "idx", "divisor"]

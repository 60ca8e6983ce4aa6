"""CPU-side checks of the verified-retrieval entry points: ``mvae_rerank_work_bytes``, ``mvae_rerank``
and ``mvae_overlap_place`` are declared in ``include/mvae.h``, bound in ``magic_amd/_lib.py`` with the
header's arity and exported; every invalid argument is ``MVAE_EINVAL`` with a message that begins
with the entry point's name, before anything touches a device (the pointers here point nowhere);
the additions leave the ABI version at 7."""
import ctypes
import os
import re

import pytest

from magic_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
P = 0x10000  # a 16-byte aligned address that is never dereferenced


def header():
    src = open(os.path.join(ROOT, "include", "mvae.h")).read()
    return src, re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_entry_points_are_declared_bound_and_exported():
    _, code = header()
    lib = _lib.load()
    for name, res in (("mvae_rerank_work_bytes", ctypes.c_size_t), ("mvae_rerank", ctypes.c_int),
                      ("mvae_overlap_place", ctypes.c_int)):
        m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, f"{name} is not declared in include/mvae.h"
        assert name in _lib._SIGS and name in _lib.EXPORTED and hasattr(lib, name), name
        assert len(_lib._SIGS[name][0]) == len(m.group(1).split(",")), name
        assert _lib._SIGS[name][1] is res


def test_abi_version_stays_7():
    raw, _ = header()
    assert int(re.search(r"#define MVAE_ABI_VERSION (\d+)", raw).group(1)) == _lib.ABI_VERSION == 7
    assert _lib.load().mvae_abi_version() == 7


def rerank_args(**kw):
    a = dict(locks=P, keys=P + 0x1000, height=20, width=20, lock_idx=None, cand=P + 0x5000, N=4, R=3,
             coef=P + 0x2000, n_rot=8, key_out=P + 0x3000, area_out=P + 0x6000, pose_out=None, from_out=None,
             work=P + 0x4000, stream=None)
    a.update(kw)
    return tuple(a.values())


def place_args(**kw):
    a = dict(locks=P, keys=P + 0x1000, height=20, width=20, lock_idx=None, key_idx=None, count=4, coef=P + 0x2000,
             n_rot=8, pose=P + 0x5000, overlay_out=P + 0x3000, stats_out=P + 0x6000, stream=None)
    a.update(kw)
    return tuple(a.values())


RERANK_CASES = {
    "null locks": dict(locks=None),
    "null keys": dict(keys=None),
    "null cand": dict(cand=None),
    "null coef": dict(coef=None),
    "null key_out": dict(key_out=None),
    "null area_out": dict(area_out=None),
    "N 0": dict(N=0),
    "N negative": dict(N=-3),
    "R 0": dict(R=0),
    "R 65": dict(R=65),
    "n_rot 0": dict(n_rot=0),
    "n_rot above 2^24": dict(n_rot=(1 << 24) + 1),
    "height 0": dict(height=0),
    "height 257": dict(height=257),
    "width 0": dict(width=0),
    "width 257": dict(width=257),
    "coef misaligned": dict(coef=P + 0x2004),
    "work misaligned": dict(work=P + 0x4004),
    "work null": dict(work=None),
}

PLACE_CASES = {
    "null locks": dict(locks=None),
    "null keys": dict(keys=None),
    "null coef": dict(coef=None),
    "null pose": dict(pose=None),
    "both outputs null": dict(overlay_out=None, stats_out=None),
    "count 0": dict(count=0),
    "count negative": dict(count=-3),
    "n_rot 0": dict(n_rot=0),
    "n_rot above 2^24": dict(n_rot=(1 << 24) + 1),
    "height 0": dict(height=0),
    "height 257": dict(height=257),
    "width 0": dict(width=0),
    "width 257": dict(width=257),
    "coef misaligned": dict(coef=P + 0x2004),
}


@pytest.mark.parametrize("case", sorted(RERANK_CASES))
def test_rerank_invalid_arguments_are_einval_with_a_message(case):
    lib = _lib.load()
    rc = lib.mvae_rerank(*rerank_args(**RERANK_CASES[case]))
    assert rc == EINVAL, (case, rc)
    msg = lib.mvae_last_error(None).decode()
    assert msg.startswith("mvae_rerank"), (case, msg)
    with pytest.raises(_lib.MVAEError, match="mvae_rerank"):
        _lib.check(lib, None, rc)


@pytest.mark.parametrize("case", sorted(PLACE_CASES))
def test_place_invalid_arguments_are_einval_with_a_message(case):
    lib = _lib.load()
    rc = lib.mvae_overlap_place(*place_args(**PLACE_CASES[case]))
    assert rc == EINVAL, (case, rc)
    msg = lib.mvae_last_error(None).decode()
    assert msg.startswith("mvae_overlap_place"), (case, msg)
    with pytest.raises(_lib.MVAEError, match="mvae_overlap_place"):
        _lib.check(lib, None, rc)


def test_messages_name_the_argument():
    lib = _lib.load()
    for case, word in (("null cand", "null"), ("N 0", "N"), ("R 65", "R"), ("n_rot 0", "n_rot"),
                       ("height 257", "height"), ("coef misaligned", "aligned"), ("work misaligned", "aligned"),
                       ("work null", "work")):
        assert lib.mvae_rerank(*rerank_args(**RERANK_CASES[case])) == EINVAL
        assert word in lib.mvae_last_error(None).decode(), case
    for case, word in (("null pose", "null"), ("both outputs null", "both"), ("count 0", "count"),
                       ("n_rot 0", "n_rot"), ("width 257", "width"), ("coef misaligned", "aligned")):
        assert lib.mvae_overlap_place(*place_args(**PLACE_CASES[case])) == EINVAL
        assert word in lib.mvae_last_error(None).decode(), case


def test_work_bytes():
    """The overlap partials of the N R pairs, the two index lists, the unordered areas and poses: at
    least what ``mvae_overlap_work_bytes`` asks for N R pairs plus 24 bytes a pair, a multiple of 8; 0
    for arguments the call refuses."""
    lib = _lib.load()
    for N, R, n_rot in ((1, 1, 1), (1, 64, 360), (5, 3, 8), (960, 16, 360), (130, 64, 8), (100000, 7, 72)):
        b = lib.mvae_rerank_work_bytes(N, R, n_rot, 100, 100)
        ov = lib.mvae_overlap_work_bytes(N * R, n_rot, 100, 100)
        assert ov > 0 and b % 8 == 0 and b >= ov + 24 * N * R, (N, R, n_rot, b, ov)
    for bad in ((0, 3, 8, 20, 20), (4, 0, 8, 20, 20), (4, 65, 8, 20, 20), (4, 3, 0, 20, 20), (4, 3, 8, 0, 20),
                (4, 3, 8, 20, 257), (-1, 3, 8, 20, 20)):
        assert lib.mvae_rerank_work_bytes(*bad) == 0, bad

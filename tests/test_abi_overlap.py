"""CPU-side checks of the maximum-overlap entry points: ``mvae_overlap_work_bytes`` and
``mvae_overlap_pairs`` are declared in ``include/mvae.h``, bound in ``magic_amd/_lib.py`` with the
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
    for name, res in (("mvae_overlap_work_bytes", ctypes.c_size_t), ("mvae_overlap_pairs", ctypes.c_int)):
        m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, f"{name} is not declared in include/mvae.h"
        assert name in _lib._SIGS and name in _lib.EXPORTED and hasattr(lib, name), name
        assert len(_lib._SIGS[name][0]) == len(m.group(1).split(",")), name
        assert _lib._SIGS[name][1] is res


def test_abi_version_stays_7():
    raw, _ = header()
    assert int(re.search(r"#define MVAE_ABI_VERSION (\d+)", raw).group(1)) == _lib.ABI_VERSION == 7
    assert _lib.load().mvae_abi_version() == 7


def args(**kw):
    a = dict(locks=P, keys=P + 0x1000, height=20, width=20, lock_idx=None, key_idx=None, count=4, coef=P + 0x2000,
             n_rot=8, area_out=P + 0x3000, pose_out=None, work=P + 0x4000, stream=None)
    a.update(kw)
    return tuple(a.values())


CASES = {
    "null locks": dict(locks=None),
    "null keys": dict(keys=None),
    "null coef": dict(coef=None),
    "null area_out": dict(area_out=None),
    "count 0": dict(count=0),
    "count negative": dict(count=-3),
    "n_rot 0": dict(n_rot=0),
    "height 0": dict(height=0),
    "height 257": dict(height=257),
    "width 0": dict(width=0),
    "width 257": dict(width=257),
    "coef misaligned": dict(coef=P + 0x2004),
    "work null": dict(work=None),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_invalid_arguments_are_einval_with_a_message(case):
    lib = _lib.load()
    rc = lib.mvae_overlap_pairs(*args(**CASES[case]))
    assert rc == EINVAL, (case, rc)
    msg = lib.mvae_last_error(None).decode()
    assert msg.startswith("mvae_overlap_pairs"), (case, msg)
    with pytest.raises(_lib.MVAEError, match="mvae_overlap_pairs"):
        _lib.check(lib, None, rc)


def test_messages_name_the_argument():
    lib = _lib.load()
    for case, word in (("null coef", "null"), ("count 0", "count"), ("n_rot 0", "n_rot"), ("height 257", "height"),
                       ("coef misaligned", "aligned"), ("work null", "work")):
        assert lib.mvae_overlap_pairs(*args(**CASES[case])) == EINVAL
        assert word in lib.mvae_last_error(None).decode(), case


def test_work_bytes():
    """One 8-byte partial per pair and chunk of angles: at least 8 bytes per pair, at most 8 n_rot;
    0 for arguments the call refuses."""
    lib = _lib.load()
    for count, n_rot in ((1, 1), (1, 360), (300, 8), (960, 360), (100000, 72)):
        b = lib.mvae_overlap_work_bytes(count, n_rot, 100, 100)
        assert b % 8 == 0 and 8 * count <= b <= 8 * count * n_rot, (count, n_rot, b)
    assert lib.mvae_overlap_work_bytes(1, 360, 100, 100) == 8 * 360  # one pair: a workgroup per angle
    for bad in ((0, 8, 20, 20), (4, 0, 20, 20), (4, 8, 0, 20), (4, 8, 20, 257)):
        assert lib.mvae_overlap_work_bytes(*bad) == 0

"""CPU-side checks of the cross-pair entry points: ``mvae_make_batch_x``, the six ``*_xpairs`` twins
and ``mvae_debug_xpairs_bits`` are declared in ``include/mvae.h``, bound in ``magic_amd/_lib.py``
with the header's arity and exported; ``mvae_xpairs`` has the layout the header states; the
additions leave the ABI version at 7; ``mvae_make_batch_x`` refuses its invalid arguments with
``MVAE_EINVAL`` and a message of its own name before anything touches a device (the pointers
here point nowhere)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from magic_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
P = 0x10000  # a 16-byte aligned address that is never dereferenced

XPAIRS = ["mvae_forward_xpairs", "mvae_train_step_xpairs", "mvae_predict_xpairs", "mvae_predict_encode_xpairs",
          "mvae_transform_xpairs", "mvae_reconstruct_xpairs"]
NEW = ["mvae_make_batch_x"] + XPAIRS + ["mvae_debug_xpairs_bits"]


def header():
    src = open(os.path.join(ROOT, "include", "mvae.h")).read()
    return src, re.sub(r"/\*.*?\*/", "", src, flags=re.S)


@pytest.mark.parametrize("name", NEW)
def test_entry_points_are_declared_bound_and_exported(name):
    _, code = header()
    lib = _lib.load()
    m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, code)
    assert m, f"{name} is not declared in include/mvae.h"
    assert name in _lib._SIGS and name in _lib.EXPORTED and hasattr(lib, name), name
    assert len(_lib._SIGS[name][0]) == len(m.group(1).split(",")), name
    assert _lib._SIGS[name][1] is ctypes.c_int


@pytest.mark.parametrize("name", XPAIRS)
def test_twins_take_the_descriptor_where_pairs_take_theirs(name):
    """Each twin has the arity of its ``*_pairs`` entry point, the descriptor in the same place."""
    twin = _lib._SIGS[name][0]
    own = _lib._SIGS[name.replace("_xpairs", "_pairs")][0]
    assert len(twin) == len(own)
    assert twin[1] is ctypes.POINTER(_lib.mvae_xpairs) and own[1] is ctypes.POINTER(_lib.mvae_pairs)
    assert twin[2:] == own[2:]


def test_debug_entry_point_adds_one_argument():
    assert len(_lib._SIGS["mvae_debug_xpairs_bits"][0]) == len(_lib._SIGS["mvae_debug_pairs_bits"][0]) + 1
    assert len(_lib._SIGS["mvae_make_batch_x"][0]) == len(_lib._SIGS["mvae_make_batch"][0]) + 1


def test_abi_version_stays_7():
    raw, _ = header()
    assert int(re.search(r"#define MVAE_ABI_VERSION (\d+)", raw).group(1)) == _lib.ABI_VERSION == 7
    assert _lib.load().mvae_abi_version() == 7


def test_xpairs_layout(tmp_path):
    """56 bytes, ``key_idx`` at offset 48, ``p`` first: the ctypes mirror and the C compiler agree."""
    x = _lib.mvae_xpairs
    got = (ctypes.sizeof(x), x.key_idx.offset, x.p.offset, ctypes.sizeof(_lib.mvae_pairs))
    assert got == (56, 48, 0, 48)
    if shutil.which("gcc") is None:
        return
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\n'
                   'int main(){printf("%%zu %%zu %%zu %%zu", sizeof(mvae_xpairs), offsetof(mvae_xpairs, key_idx),'
                   ' offsetof(mvae_xpairs, p), sizeof(mvae_pairs));}\n' % os.path.join(ROOT, "include", "mvae.h"))
    exe = tmp_path / "s"
    subprocess.check_call(["gcc", str(src), "-o", str(exe)])
    assert got == tuple(int(v) for v in subprocess.check_output([str(exe)]).split())


def args(**kw):
    a = dict(locks=P, keys=P + 0x1000, height=20, width=20, lock_idx=P + 0x2000, key_idx=P + 0x3000,
             coef=P + 0x4000, batch=64, divisor=255.0, x_out=P + 0x10000, stream=None)
    a.update(kw)
    return tuple(a.values())


CASES = {
    "null locks": (dict(locks=None), "null"),
    "null keys": (dict(keys=None), "null"),
    "null lock_idx": (dict(lock_idx=None), "null"),
    "coef misaligned": (dict(coef=P + 0x4004), "16-byte"),
    "divisor 0": (dict(divisor=0.0), "divisor"),
    "divisor negative": (dict(divisor=-255.0), "divisor"),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_make_batch_x_invalid_arguments_are_einval_with_a_message(case):
    lib = _lib.load()
    kw, word = CASES[case]
    rc = lib.mvae_make_batch_x(*args(**kw))
    assert rc == EINVAL, (case, rc)
    msg = lib.mvae_last_error(None).decode()
    assert msg.startswith("mvae_make_batch_x") and word in msg, (case, msg)
    with pytest.raises(_lib.MVAEError, match="mvae_make_batch_x"):
        _lib.check(lib, None, rc)

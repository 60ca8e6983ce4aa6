"""mvae_debug_tower refuses its invalid arguments with MVAE_EINVAL and a message naming the entry,
before any HIP call (no GPU needed: the pointers are never followed); the addition leaves the ABI
version at 7."""
import ctypes
import os
import re

from magic_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ("mode", "S", "n", "ld", "opt", "in0", "in1", "xs", "arg_in", "out0", "out1", "outb", "arg_out")


def test_debug_tower_rejects_bad_arguments():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    ok = dict(mode=0, S=4, n=1, ld=16, opt=0, in0=p, in1=p, xs=p, arg_in=p, out0=p, out1=p, outb=p, arg_out=p)
    bad = [dict(mode=4), dict(mode=-1), dict(S=6), dict(S=0), dict(S=104), dict(n=0), dict(n=16385),
           dict(ld=15), dict(opt=1), dict(in0=None), dict(in1=None), dict(out0=None), dict(arg_out=None),
           dict(out1=None, outb=None),
           dict(mode=1, ld=63), dict(mode=1, ld=64, opt=0), dict(mode=1, ld=64, opt=2 << 1),
           dict(mode=1, ld=64, opt=-1), dict(mode=1, ld=64, opt=1, out0=None),
           dict(mode=1, ld=64, opt=3 << 1, outb=None), dict(mode=1, ld=64, opt=1, arg_out=None),
           dict(mode=2, ld=64, opt=1), dict(mode=2, ld=63), dict(mode=2, ld=64, arg_in=None),
           dict(mode=2, ld=64, in1=None), dict(mode=2, ld=64, out0=None, outb=None),
           dict(mode=3, opt=-1), dict(mode=3, opt=(1 << 20) + 1), dict(mode=3, xs=None), dict(mode=3, arg_in=None),
           dict(mode=3, out1=None), dict(mode=3, ld=8)]
    for b in bad:
        a = {**ok, **b}
        rc = lib.mvae_debug_tower(*[a[k] for k in ARGS], None)
        assert rc == -1, (b, rc)   # MVAE_EINVAL
        assert lib.mvae_last_error(None).startswith(b"mvae_debug_tower: "), b


def test_abi_version_unchanged():
    raw = open(os.path.join(ROOT, "include", "mvae.h")).read()
    assert int(re.search(r"#define MVAE_ABI_VERSION (\d+)", raw).group(1)) == _lib.ABI_VERSION == 7
    assert "mvae_debug_tower" in _lib.EXPORTED

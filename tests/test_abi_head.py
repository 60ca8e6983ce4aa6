"""mvae_debug_head refuses its invalid arguments with MVAE_EINVAL and a message naming the entry,
before any HIP call (no GPU needed: the pointers are never followed); the addition leaves the ABI
version at 7."""
import ctypes
import os
import re

from magic_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTRS = ("ms", "eps", "areas", "rowpart", "dzdec", "z", "zp", "rowfwd", "colsq", "coldot", "draw", "part",
        "cnt", "out", "rowvals", "dist", "losses", "dhead", "hp")


def _args(p, **kw):
    a = _lib.mvae_head_args()
    base = dict(mode=0, B=2, L=8, Bg=2, ldz=16, ldh=16, off=0, zmask=6, z_planes=3, h_planes=3, cs_mode=0,
                nblk=3, metric=0, recip=0, w=1.0, seed=1, counter=0, **{k: p for k in PTRS})
    for k, v in {**base, **kw}.items():
        setattr(a, k, v)
    return a


def test_debug_head_rejects_bad_arguments():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64 + 16)
    p = (ctypes.addressof(buf) + 15) & ~15        # 16-byte aligned
    q = p + 4                                     # 4-byte aligned only
    F, C, M, R, W = _lib.HEAD_FWD, _lib.HEAD_COLSTATS, _lib.HEAD_METRIC, _lib.HEAD_LOSS, _lib.HEAD_BWD
    every = [dict(mode=m, **b) for m in (F, C, M, R, W)
             for b in (dict(B=0), dict(L=0), dict(B=-1), dict(Bg=1))]
    bad = [dict(mode=5), dict(mode=-1)] + every + [
        # forward
        dict(mode=F, ldz=7), dict(mode=F, zmask=1), dict(mode=F, zmask=8), dict(mode=F, z_planes=2),
        dict(mode=F, z_planes=-1), dict(mode=F, ms=None), dict(mode=F, rowfwd=None), dict(mode=F, z=None),
        dict(mode=F, zp=None), dict(mode=F, eps=None, off=1), dict(mode=F, eps=None, off=-1),
        dict(mode=F, eps=None, Bg=8, off=7),
        dict(mode=F, ms=q), dict(mode=F, eps=q), dict(mode=F, z=q), dict(mode=F, zp=q), dict(mode=F, rowfwd=q),
        dict(mode=F, L=5, ldz=8, rowfwd=q),
        # column statistics
        dict(mode=C, ldz=7), dict(mode=C, cs_mode=2), dict(mode=C, cs_mode=-1), dict(mode=C, z=None),
        dict(mode=C, part=None), dict(mode=C, out=None), dict(mode=C, cs_mode=1, colsq=None),
        dict(mode=C, cs_mode=1, draw=None),
        # metric
        dict(mode=M, ldz=7), dict(mode=M, metric=2), dict(mode=M, nblk=-1), dict(mode=M, z=None),
        dict(mode=M, rowfwd=None), dict(mode=M, rowpart=None), dict(mode=M, colsq=None),
        dict(mode=M, rowvals=None), dict(mode=M, dist=None), dict(mode=M, draw=None), dict(mode=M, rowfwd=q),
        dict(mode=M, L=64, ldz=64, z=q),
        # loss reduce
        dict(mode=R, rowvals=None), dict(mode=R, losses=None), dict(mode=R, rowvals=q),
        # backward
        dict(mode=W, ldh=15), dict(mode=W, metric=-1), dict(mode=W, h_planes=2), dict(mode=W, ms=None),
        dict(mode=W, dzdec=None), dict(mode=W, draw=None), dict(mode=W, colsq=None), dict(mode=W, coldot=None),
        dict(mode=W, hp=None), dict(mode=W, dhead=None, h_planes=0), dict(mode=W, eps=None, off=1),
        dict(mode=W, ms=q), dict(mode=W, eps=q), dict(mode=W, dzdec=q), dict(mode=W, dhead=q), dict(mode=W, hp=q)]
    for b in bad:
        rc = lib.mvae_debug_head(ctypes.byref(_args(p, **b)), None)
        assert rc == -1, (b, rc)   # MVAE_EINVAL
        assert lib.mvae_last_error(None).startswith(b"mvae_debug_head: "), b
    assert lib.mvae_debug_head(None, None) == -1
    assert lib.mvae_last_error(None).startswith(b"mvae_debug_head: ")


def test_abi_version_unchanged():
    raw = open(os.path.join(ROOT, "include", "mvae.h")).read()
    assert int(re.search(r"#define MVAE_ABI_VERSION (\d+)", raw).group(1)) == _lib.ABI_VERSION == 7
    assert "mvae_debug_head" in _lib.EXPORTED

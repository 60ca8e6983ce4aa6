"""mvae_debug_epi refuses its invalid arguments with MVAE_EINVAL and a message naming the entry,
before any HIP call (no GPU needed: the pointers are never followed); the addition leaves the ABI
version at 7."""
import ctypes
import os
import re

from magic_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTRS = ("A", "B", "du", "cp", "x", "xp", "dyn", "xbits", "y", "rowpart", "aux", "auxp")
A, D, E = _lib.EPI_ACT, _lib.EPI_DACT, _lib.EPI_BCE


def _args(p, **kw):
    a = _lib.mvae_epi_args()
    base = dict(M=300, N=392, K=21, lda=24, ldb=392, bt=0, prec=1, variant=0, x3=0, epi=E, act=0, ldc=392,
                ncp=1, ldx=392, ldbits=49, ldy=392, rp_ld=0, rp_off=0, split_c0=0, ld_aux=392, remap_split=0,
                remap_shift=0, padw=0, scale=1.0, pc=300 * 392, **{k: p for k in PTRS})
    for k, v in {**base, **kw}.items():
        setattr(a, k, v)
    return a


def test_debug_epi_rejects_bad_arguments():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64 + 16)
    p = (ctypes.addressof(buf) + 15) & ~15
    every = [dict(epi=m, **b) for m in (A, D, E)
             for b in (dict(M=0), dict(N=0), dict(K=0), dict(M=-1), dict(lda=20), dict(ldb=391),
                       dict(bt=1, ldb=20), dict(bt=2), dict(ldc=391), dict(ncp=2), dict(ncp=-1),
                       dict(du=None, ncp=0), dict(cp=None), dict(pc=300 * 392 - 1), dict(A=None), dict(B=None),
                       dict(prec=3), dict(prec=-1), dict(variant=1), dict(variant=9), dict(variant=14),
                       dict(variant=-1), dict(x3=3), dict(act=2), dict(padw=3), dict(padw=-1))]
    bad = [dict(epi=0), dict(epi=4), dict(epi=5), dict(epi=-1)] + every + [
        # the BCE head
        dict(x=None), dict(ldx=391), dict(rowpart=None), dict(rp_ld=3), dict(rp_ld=5, rp_off=2),
        dict(rp_off=1), dict(rp_off=-1, rp_ld=8), dict(ldy=391), dict(padw=1),
        dict(dyn=None), dict(dyn=None, xbits=None), dict(dyn=None, xp=None), dict(xp=None), dict(ldbits=48),
        dict(split_c0=128), dict(split_c0=-256), dict(split_c0=512), dict(split_c0=256, N=383, ldb=392),
        dict(split_c0=256, prec=0), dict(split_c0=256, bt=1, ldb=24), dict(split_c0=256, M=127),
        # dgrad
        dict(epi=D, aux=None, auxp=None), dict(epi=D, ld_aux=391), dict(epi=D, remap_split=-1),
        dict(epi=D, remap_shift=-1), dict(epi=D, remap_split=10, remap_shift=11),
        dict(epi=D, padw=1, N=390, ld_aux=391), dict(epi=D, padw=1, N=390, ldc=390), dict(epi=D, split_c0=256),
        # activation
        dict(epi=A, padw=2, N=390, ldc=391), dict(epi=A, padw=2, N=390, ldc=390), dict(epi=A, split_c0=256)]
    for b in bad:
        rc = lib.mvae_debug_epi(ctypes.byref(_args(p, **b)), None)
        assert rc == -1, (b, rc)   # MVAE_EINVAL
        assert lib.mvae_last_error(None).startswith(b"mvae_debug_epi: "), b
    assert lib.mvae_debug_epi(None, None) == -1
    assert lib.mvae_last_error(None).startswith(b"mvae_debug_epi: ")


def test_abi_version_unchanged():
    raw = open(os.path.join(ROOT, "include", "mvae.h")).read()
    assert int(re.search(r"#define MVAE_ABI_VERSION (\d+)", raw).group(1)) == _lib.ABI_VERSION == 7
    assert "mvae_debug_epi" in _lib.EXPORTED
    fields = re.search(r"typedef struct mvae_epi_args \{(.*?)\} mvae_epi_args;", raw, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = [n.strip(" *") for decl in fields.split(";") if decl.strip()
             for n in re.sub(r"^\s*(const\s+)?(unsigned\s+)?(long long|\w+)", "", decl.strip()).split(",")]
    assert names == [f[0] for f in _lib.mvae_epi_args._fields_]

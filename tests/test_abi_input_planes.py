"""mvae_debug_input_planes (include/mvae.h) without a GPU: it refuses its invalid arguments with
MVAE_EINVAL and a message naming the entry before any HIP call (the pointers are never followed), and
the addition leaves the ABI version at 7."""
import ctypes
import os
import re

from magic_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTRS = ("x", "locks", "keys", "idx", "key_idx", "coef", "xs", "planes", "xbits", "xbf", "xbw", "dyn")


def _args(p, **kw):
    """A valid call of `route` (B 64, 8 x 8 images, three planes, the lock rows on the flag), overridden."""
    B, D, ldx, ldbits = 64, 64, 72, 16
    rows = 3 * B * ldx
    base = dict(route=kw.get("route", 0), B=B, H=8, W=8, ldx=ldx, np=3, f32mask=0, f32dyn_mask=2, ldbits=ldbits,
                no_xbw=0, slot=0, divisor=255.0, plane_stride=rows + 16, x_elems=3 * B * D, xs_elems=rows,
                planes_elems=2 * (rows + 16) + rows, xbits_elems=B * ldbits, **{k: p for k in PTRS})
    a = _lib.mvae_input_args()
    for k, v in {**base, **kw}.items():
        setattr(a, k, v)
    return a


def test_debug_input_planes_rejects_bad_arguments():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64 + 16)
    p = (ctypes.addressof(buf) + 15) & ~15        # 16-byte aligned
    q, q8 = p + 4, p + 8                          # 4-byte / 8-byte aligned only
    rows = 3 * 64 * 72
    every = [dict(route=r, **b) for r in range(4) for b in (
        dict(B=0), dict(H=0), dict(W=-1), dict(np=2), dict(np=-1), dict(np=4), dict(slot=2), dict(slot=-1),
        dict(f32mask=8), dict(f32dyn_mask=8), dict(f32dyn_mask=-1), dict(ldx=63), dict(dyn=None), dict(planes=None),
        dict(planes=q), dict(xs=None), dict(xs=q8), dict(xs_elems=rows - 1), dict(plane_stride=rows - 1),
        dict(planes_elems=2 * (rows + 16) + rows - 1), dict(np=1, planes_elems=rows - 1),
        dict(ldbits=7), dict(xbits_elems=64 * 16 - 1), dict(B=65536), dict(H=4097, W=4097))]
    bad = [dict(route=4), dict(route=-1)] + every + [
        # the plane path
        dict(x=None), dict(x_elems=3 * 64 * 64 - 1), dict(f32mask=2, f32dyn_mask=0, xs=None),
        dict(np=0, f32mask=7, f32dyn_mask=0, xs_elems=rows - 1),
        # the bits routes: no fp32-precision form, no unconditional rows, every buffer, the launchers' shapes
        *[dict(route=r, **b) for r in (1, 2, 3) for b in (
            dict(np=0), dict(f32mask=2), dict(f32mask=7, f32dyn_mask=0), dict(xbits=None), dict(xbf=None),
            dict(xbw=None), dict(B=63, x_elems=10 ** 9), dict(B=32), dict(H=3, W=3), dict(H=2, W=6, ldx=16),
            dict(ldx=68), dict(ldx=76))],
        dict(route=1, x=None), dict(route=1, x=q), dict(route=1, x=q8), dict(route=1, x_elems=3 * 64 * 64 - 1),
        dict(route=2, locks=None), dict(route=2, keys=None), dict(route=2, idx=None), dict(route=2, coef=None),
        dict(route=2, locks=q), dict(route=2, keys=q), dict(route=2, coef=q8), dict(route=2, divisor=0.0),
        dict(route=3, locks=None), dict(route=3, idx=None), dict(route=3, locks=q), dict(route=3, divisor=-1.0)]
    for b in bad:
        rc = lib.mvae_debug_input_planes(ctypes.byref(_args(p, **b)), None)
        assert rc == -1, (b, rc)   # MVAE_EINVAL
        assert lib.mvae_last_error(None).startswith(b"mvae_debug_input_planes: "), (b, lib.mvae_last_error(None))
    assert lib.mvae_debug_input_planes(None, None) == -1
    assert lib.mvae_last_error(None).startswith(b"mvae_debug_input_planes: ")


def test_refusals_name_their_reason():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64 + 16)
    p = (ctypes.addressof(buf) + 15) & ~15
    who = b"mvae_debug_input_planes: "
    for kw, msg in ((dict(route=7), b"route must be in [0, 3]"), (dict(np=2), b"np must be 0, 1 or 3"),
                    (dict(slot=2), b"slot must be 0 or 1"), (dict(f32mask=9), b"f32mask and f32dyn_mask"),
                    (dict(route=1, np=0), b"np 0 is the plane path's"), (dict(route=2, f32mask=2), b"f32mask is the plane"),
                    (dict(ldx=60), b"ldx is smaller than a row"), (dict(ldbits=7), b"ldbits is smaller than a row"),
                    (dict(xs=None), b"xs is NULL"), (dict(planes_elems=5), b"planes_elems is smaller"),
                    (dict(route=1, B=32), b"shape or alignment the route does not serve"),
                    (dict(route=3, locks=p + 4), b"shape or alignment the route does not serve")):
        assert lib.mvae_debug_input_planes(ctypes.byref(_args(p, **kw)), None) == -1, kw
        assert lib.mvae_last_error(None).startswith(who + msg), (kw, lib.mvae_last_error(None))


def test_abi_version_unchanged():
    raw = open(os.path.join(ROOT, "include", "mvae.h")).read()
    assert int(re.search(r"#define MVAE_ABI_VERSION (\d+)", raw).group(1)) == _lib.ABI_VERSION == 7
    assert "mvae_debug_input_planes" in _lib.EXPORTED
    assert re.search(r"int mvae_debug_input_planes\(const mvae_input_args\* args, void\* stream\);", raw)
    fields = re.search(r"typedef struct mvae_input_args \{(.*?)\} mvae_input_args;", raw, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = [n.strip(" *") for decl in fields.split(";") if decl.strip()
             for n in re.sub(r"^\s*(const\s+)?(unsigned\s+)?(long long|\w+)", "", decl.strip()).split(",")]
    assert names == [f[0] for f in _lib.mvae_input_args._fields_]

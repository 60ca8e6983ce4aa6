"""mvae_debug_gemm_ex (include/mvae.h) without a GPU: it refuses its invalid arguments with MVAE_EINVAL
and a message naming the entry before any HIP call (the pointers are never followed); the addition
leaves the ABI version at 7; and the cases of tests/gemm_cases.py are what they say -- each one's plan,
asked of mvae_debug_plan (host arithmetic only), lands on the kernel, tile, split and epilogue form the
GPU pins of tests/test_gpu_gemm_batch.py rely on."""
import ctypes
import os
import re

import pytest

from magic_amd import _lib
from tests import gemm_cases as G
from tests.gemm_cases import E8, F32, PLANE, RING, VALU, X3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args(p, **kw):
    c = dict(G.make("base", 300, 260, 576, at=1, variant=13, split=2))
    shared = kw.pop("shared", False)
    if shared:
        c = dict(G.make("base", 300, 260, 512, at=1, variant=13, split=2, sA=256 * 304, bits=1, bits_shared=1))
    c.update(A=p, B=p, C=p)
    c.update(kw)
    a = _lib.mvae_gemm_args()
    for k, v in c.items():
        if k != "name":
            setattr(a, k, v)
    return a


def test_debug_gemm_ex_rejects_bad_arguments():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64 + 16)
    p = (ctypes.addressof(buf) + 15) & ~15
    base = G.make("base", 300, 260, 576, at=1, variant=13, split=2)
    bad = [dict(A=None), dict(B=None), dict(C=None),
           dict(M=0), dict(N=0), dict(K=0), dict(batch=0), dict(M=-1), dict(batch=-2),
           dict(at=2), dict(bt=-1),
           dict(lda=299), dict(at=0, lda=575), dict(ldb=259), dict(bt=1, ldb=575), dict(ldc=259),
           dict(sA=-1), dict(sB=-8), dict(sC=-4),
           dict(a_elems=base["a_elems"] - 1), dict(b_elems=base["b_elems"] - 1), dict(c_elems=base["c_elems"] - 1),
           dict(batch=3), dict(a_elems=0), dict(c_elems=-1),
           dict(sC=299 * base["ldc"] + 259), dict(sC=0),          # the output windows overlap
           dict(prec=3), dict(prec=-1), dict(variant=16), dict(variant=-1), dict(x3=3), dict(x3=-1),
           dict(tm=128), dict(tm=-192), dict(epi=2), dict(epi=3), dict(epi=-1), dict(act=2), dict(act=-1),
           dict(bits=3), dict(bits=-1), dict(group=-2), dict(a_off=8), dict(a_off=-1), dict(b_off=8), dict(b_off=-1),
           dict(split=-1),
           dict(bits=1, prec=0), dict(bits=2, prec=0), dict(bits=1, variant=9),   # bits in fp32
           dict(bits_shared=1), dict(bits_shared=2, bits=1), dict(bits_shared=-1, bits=1),
           dict(shared=True, bits=0), dict(shared=True, prec=0),
           dict(shared=True, sA=255 * 304), dict(shared=True, sA=256 * 304 + 8),
           # (at = 0: the same buffers as M 512 x K 300 with sA still a multiple of 64 lda)
           dict(shared=True, at=0, M=512, K=300, sC=512 * base["ldc"] + 16, c_elems=10 ** 9),
           # A's run-time flag: f32x only (the base case is bf16)
           dict(a_dyn=1), dict(a_dyn=2), dict(a_dyn=1, prec=0), dict(a_dyn=1, prec=2, variant=9),
           dict(a_dyn=3, prec=2), dict(a_dyn=-1, prec=2)]
    for b in bad:
        rc = lib.mvae_debug_gemm_ex(ctypes.byref(_args(p, **b)), None, None)
        assert rc == -1, (b, rc)   # MVAE_EINVAL
        assert lib.mvae_last_error(None).startswith(b"mvae_debug_gemm_ex: "), (b, lib.mvae_last_error(None))
    assert lib.mvae_debug_gemm_ex(None, None, None) == -1
    assert lib.mvae_last_error(None).startswith(b"mvae_debug_gemm_ex: ")


def test_abi_version_unchanged():
    raw = open(os.path.join(ROOT, "include", "mvae.h")).read()
    assert int(re.search(r"#define MVAE_ABI_VERSION (\d+)", raw).group(1)) == _lib.ABI_VERSION == 7
    assert "mvae_debug_gemm_ex" in _lib.EXPORTED
    fields = re.search(r"typedef struct mvae_gemm_args \{(.*?)\} mvae_gemm_args;", raw, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = [n.strip(" *") for decl in fields.split(";") if decl.strip()
             for n in re.sub(r"^\s*(const\s+)?(unsigned\s+)?(long long|\w+)", "", decl.strip()).split(",")]
    assert names == [f[0] for f in _lib.mvae_gemm_args._fields_]
    assert names == list(G.FIELDS) + ["A", "B", "C", "a_dyn"]   # (a_dyn: appended; a zero keeps the old behaviour)


# ------------------------------------------------------------------ the plane-pair cases (test_gpu_gemm_pairs.py)

@pytest.fixture(scope="module")
def pair_plans():
    """name -> (case, its plan without a flag, its plan with one)."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    base = (ctypes.addressof(buf) + 15) & ~15
    out = {}
    for c in G.PAIR_CASES:
        ps = []
        for a_dyn in (0, 1):
            a, o = G.plan_args(_lib.mvae_plan_args(), dict(c, a_dyn=a_dyn), base), _lib.mvae_plan_out()
            assert lib.mvae_debug_plan(ctypes.byref(a), ctypes.byref(o)) == 0, (c["name"], lib.mvae_last_error(None))
            ps.append({f[0]: getattr(o, f[0]) for f in _lib.mvae_plan_out._fields_})
        out[c["name"]] = (c, ps[0], ps[1])
    return out


def test_pair_cases_reach_every_f32x_family(pair_plans):
    """Plane; ring at 256 and 192 rows; the plane-stacked kernel in both forms (tile N 128 at 256 and 192
    rows, 256x256); eight-phase on planes and on both bits forms -- each with both at (k-contiguous A alone
    on 192 rows), both bt, unsplit and a split whose last slice is one partial k-tile, at batch 2. A flag
    on A changes none of these forced plans."""
    want = {"pairs_plane": (PLANE, 128, 128), "pairs_ring256": (RING, 256, 128), "pairs_ring192": (RING, 192, 128),
            "pairs_x3f1_256": (X3, 256, 128), "pairs_x3f1_192": (X3, 192, 128), "pairs_x3f2": (X3, 256, 256),
            "pairs_e8": (E8, 256, 256), "pairs_e8_bits_lds": (E8, 256, 256), "pairs_e8_bits_reg": (E8, 256, 256)}
    seen = {}
    for name, (c, p, pd) in pair_plans.items():
        if name.startswith("pairs_planner"):     # unforced: whatever the planner picks, a 256-row kernel
            assert (c["variant"], c["split"]) == (0, 0) and p["kernel"] in (RING, X3, E8) and pd["kernel"] == p["kernel"]
            continue
        fam = max((k for k in want if name.startswith(k + "_at")), key=len)
        assert (p["kernel"], p["tm"], p["tn"]) == want[fam], (name, p)
        assert c["prec"] == G.PREC_F32X and c["batch"] == 2 and not p["refused"]
        assert p["split"] == c["split"] and p == pd, (name, p, pd)
        assert _partial_last(c, p) == ("tail_slice" in name) and (p["split"] == 1) == ("unsplit" in name), (name, p)
        assert (c["bits"] == 1) == ("bits_lds" in name) and (c["bits"] == 2) == ("bits_reg" in name)
        seen.setdefault(fam, set()).add((c["at"], c["bt"], p["split"] > 1))
    assert set(seen) == set(want)
    for fam, s in seen.items():
        ats = (0,) if "192" in fam else (0, 1)
        assert s == {(at, bt, sp) for at in ats for bt in (0, 1) for sp in (False, True)}, fam


# ------------------------------------------------------------------ the cases are what they say

@pytest.fixture(scope="module")
def plans():
    """name -> (case, its plan by mvae_debug_plan)."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    base = (ctypes.addressof(buf) + 15) & ~15
    out = {}
    for c in G.CASES:
        a, o = G.plan_args(_lib.mvae_plan_args(), c, base), _lib.mvae_plan_out()
        assert lib.mvae_debug_plan(ctypes.byref(a), ctypes.byref(o)) == 0, (c["name"], lib.mvae_last_error(None))
        out[c["name"]] = (c, {f[0]: getattr(o, f[0]) for f in _lib.mvae_plan_out._fields_})
    return out


def _bk(p):
    return 32 if p["kernel"] in (F32, VALU) else 64   # the k-tile of the kernel that runs


def _empty_last(c, p):
    return p["split"] > 1 and (p["split"] - 1) * p["kchunk"] >= c["K"]


def _partial_last(c, p):
    return p["split"] > 1 and 0 < c["K"] - (p["split"] - 1) * p["kchunk"] < _bk(p)


def test_no_case_is_refused_and_forces_hold(plans):
    assert 90 <= len(plans) <= 130
    for name, (c, p) in plans.items():
        assert not p["refused"], name
        if c["split"] > 0:
            assert p["split"] == c["split"], name
        assert p["ntm"] == -(-c["M"] // p["tm"]) and p["ntn"] == -(-c["N"] // p["tn"]), name
        assert p["kchunk"] % _bk(p) == 0 and p["kchunk"] * p["split"] >= c["K"], name
        if c["tm"] and p["kernel"] in (RING, X3):
            assert p["tm"] == c["tm"], name


def test_case_names_tell_the_kernel(plans):
    prefix = {"f32": F32, "valu": VALU, "plane": PLANE, "ring_to_plane": PLANE, "ring": RING, "x3": X3, "e8": E8}
    for name, (c, p) in plans.items():
        fam = max((k for k in prefix if name.startswith(k)), key=len)
        assert p["kernel"] == prefix[fam], (name, _lib.KERNEL_NAMES[p["kernel"]])
        if "empty_slice" in name:
            assert _empty_last(c, p), (name, p)
        if "tail_slice" in name:
            assert _partial_last(c, p), (name, p)
        if "one_tile_slices" in name:
            assert p["split"] > 1 and p["kchunk"] == _bk(p) and p["split"] * p["kchunk"] == c["K"], (name, p)
        if name.startswith("ring") and name[4:7] in ("256", "192"):
            assert f"ring{p['tm']}x{p['tn']}" == name.split("_")[0], (name, p)


def test_batched_cases_reach_every_kernel_and_edge(plans):
    b = [(c, p) for c, p in plans.values() if c["batch"] >= 2]
    assert any(c["batch"] >= 3 for c, _ in b)
    kernels = (F32, VALU, PLANE, RING, X3, E8)
    assert {p["kernel"] for _, p in b} == set(kernels)
    assert {(p["tm"], p["tn"]) for _, p in b if p["kernel"] == RING} == {(256, 256), (256, 128), (192, 256), (192, 128)}
    assert {(p["tm"], p["tn"]) for _, p in b if p["kernel"] == X3} == {(256, 256), (256, 128), (192, 128)}
    for reg in (1, 2):
        assert all(any(p["kernel"] == E8 and c["bits"] == reg and c["bits_shared"] == s for c, p in b) for s in (0, 1))
    for k in kernels:
        of = [(c, p) for c, p in b if p["kernel"] == k]
        name = _lib.KERNEL_NAMES[k]
        assert any(p["split"] > 1 for _, p in of), name
        assert any(p["split"] == 1 for _, p in of), name
        assert any(_empty_last(c, p) for c, p in of), name
        assert any(_partial_last(c, p) for c, p in of), name
        assert any(c["epi"] == 1 and p["split"] == 1 for c, p in of) and any(c["epi"] == 1 and p["split"] > 1 for c, p in of), name
        # overlapping A windows (the weight gradients' form) and windows back to back
        assert any(c["sA"] < G.a_shape(c)[0] * c["lda"] for c, _ in of), name
    for k in (RING, X3, E8):
        assert any(c["group"] > 0 and p["ntm"] % c["group"] != 0 and p["ntn"] >= 2 for c, p in b if p["kernel"] == k)
        assert any(c["group"] > 0 and p["split"] > 1 for c, p in b if p["kernel"] == k)


def test_the_planner_itself_emits_empty_slices(plans):
    """Unforced (variant 0, split 0): fp32, M 64, N 40, at = 1, batch 2 -- the latent head's weight-gradient
    class. K 796: split 6 of kchunk 160, slice 5 starts at 800 >= K. K 1589: two empty slices."""
    c, p = plans["f32_planner_empty_slice"]
    assert (c["variant"], c["split"], c["batch"]) == (0, 0, 2)
    assert (p["kernel"], p["split"], p["kchunk"]) == (F32, 6, 160) and _empty_last(c, p)
    c, p = plans["f32_planner_two_empty_slices"]
    assert (c["variant"], c["split"]) == (0, 0) and p["kernel"] == F32
    assert (p["split"] - 2) * p["kchunk"] >= c["K"], p


def test_the_alignment_fallbacks_are_taken_one_at_a_time(plans):
    # the eight-phase kernel's 16-byte epilogue: cases that differ in sC % 4 alone ...
    (c1, p1), (c0, p0) = plans["e8_unsplit_vec"], plans["e8_unsplit_novec"]
    assert {k: v for k, v in c1.items() if k not in ("name", "sC", "c_elems")} == \
           {k: v for k, v in c0.items() if k not in ("name", "sC", "c_elems")}
    assert c1["sC"] % 4 == 0 and c0["sC"] % 4 != 0 and c1["ldc"] % 4 == 0
    assert (p1["kernel"], p1["vec_epilogue"], p0["kernel"], p0["vec_epilogue"]) == (E8, 1, E8, 0)
    # ... and, for a slab launch (rows of N floats, M N between two slabs), in N alone: N % 4 != 0 is the
    # one way to it, since N % 4 == 0 makes M N % 4 == 0 -- both forms of it here, output strides aligned
    (c1, p1), (c0, p0), (c2, p2) = plans["e8_slabs_vec"], plans["e8_slabs_novec"], plans["e8_slabs_novec_odd"]
    assert (c1["M"], c1["K"], c1["split"], c1["ldc"]) == (c0["M"], c0["K"], c0["split"], c0["ldc"])
    assert c1["M"] * c1["N"] % 4 == 0 and c0["N"] % 4 != 0 and c0["M"] * c0["N"] % 4 == 0
    assert c2["M"] * c2["N"] % 4 != 0
    assert all(c["sC"] % 4 == 0 and c["ldc"] % 4 == 0 for c in (c0, c1, c2))
    assert (p1["kernel"], p1["vec_epilogue"], p0["kernel"], p0["vec_epilogue"]) == (E8, 1, E8, 0)
    assert (p2["kernel"], p2["vec_epilogue"]) == (E8, 0)
    assert p1["split"] == p0["split"] == p2["split"] == 2
    # a forced ring number lands on the plane kernel: by a batch stride, or by the image's alignment
    for name, key in (("ring_to_plane_sA", "sA"), ("ring_to_plane_sB", "sB")):
        c, p = plans[name]
        assert c[key] % 8 != 0 and c["a_off"] == c["b_off"] == 0 and p["kernel"] == PLANE
    for name, key in (("ring_to_plane_a_off", "a_off"), ("ring_to_plane_b_off", "b_off")):
        c, p = plans[name]
        assert c[key] != 0 and c["sA"] % 8 == 0 and c["sB"] % 8 == 0 and p["kernel"] == PLANE
    # ... and the same cases without the one thing stay on a 256-row kernel
    c, p = plans["ring_any_shape_empty_slice"]
    assert {k: v for k, v in c.items() if k != "name"} == \
           {k: v for k, v in plans["ring_to_plane_a_off"][0].items() if k not in ("name", "a_off")} | {"a_off": 0}
    assert (p["kernel"], p["tm"], p["tn"], p["split"]) == (RING, 256, 128, 4)
    c, p = plans["ring_any_shape_t192"]
    assert (p["kernel"], p["tm"], p["tn"], p["split"]) == (RING, 192, 128, 4)
    # the split-K reductions: 16-byte (N, ldc, sC multiples of 4, at least 2^18 elements) and scalar
    c, p = plans["ring_group2_slabs"]
    assert c["M"] * c["N"] >= 1 << 18 and c["N"] % 4 == 0 and c["ldc"] % 4 == 0 and c["sC"] % 4 == 0
    assert plans["ring_group2_slabs_odd_sC"][0]["sC"] % 4 != 0

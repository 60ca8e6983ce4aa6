"""The GEMM planner against its recorded decisions (no GPU needed: mvae_debug_plan is host code and
never follows a pointer). tests/golden/gemm_plans.npz holds the plan of every case of
make_golden.gemm_plan_cases() as the library made it before the planner became one function
(DESIGN.md 5q): kernel, tile, grid, split, epilogue form, workspace. Every column of every case must
still come out the same; the invariants below hold over the same cases."""
import ctypes
import os

import numpy as np
import pytest

from magic_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_plans.npz")
F32, VALU, PLANE, RING, X3, E8 = 1, 2, 3, 4, 5, 6
STORE, ACT, DACT, BCE, SIGMOID, BCEB, DACTB = range(7)
PTRS = ("Ap", "Bp", "C", "cp", "aux", "auxp", "x", "xp", "y", "ws")


@pytest.fixture(scope="module")
def plans():
    """(input columns by name, recorded plans by name, this library's plans by name, in_names)."""
    z = np.load(GOLDEN)
    in_names, out_names = [str(n) for n in z["in_names"]], [str(n) for n in z["out_names"]]
    assert in_names == [f[0] for f in _lib.mvae_plan_args._fields_]
    assert out_names == [f[0] for f in _lib.mvae_plan_out._fields_]
    cases, want = z["cases"], z["plans"]
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    base = (ctypes.addressof(buf) + 15) & ~15
    got = np.zeros_like(want)
    a, o = _lib.mvae_plan_args(), _lib.mvae_plan_out()
    for i, row in enumerate(cases.tolist()):
        for k, v in zip(in_names, row):
            setattr(a, k, (None, base, base + 4)[v] if k in PTRS else v)
        assert lib.mvae_debug_plan(ctypes.byref(a), ctypes.byref(o)) == 0, (i, lib.mvae_last_error(None))
        got[i] = [getattr(o, k) for k in out_names]
    col = lambda m, names: {n: m[:, j].astype(np.int64) for j, n in enumerate(names)}  # noqa: E731
    c = col(cases, in_names)
    c["max_ws"] = cases[:, in_names.index("max_ws")]  # (unsigned: 2^64 - 1 is "unlimited")
    return c, col(want, out_names), col(got, out_names), in_names


def test_plans_match_the_recorded_ones(plans):
    c, want, got, in_names = plans
    assert len(want["kernel"]) > 3000
    for i in range(len(want["kernel"])):
        for k in want:
            if want[k][i] != got[k][i]:
                case = {n: int(c[n][i]) for n in in_names}
                raise AssertionError(f"case {i} column {k}: recorded {want[k][i]}, now {got[k][i]}; "
                                     f"recorded kernel {_lib.KERNEL_NAMES[int(want['kernel'][i])]}; case {case}")


def test_the_cases_reach_every_kernel_and_rule(plans):
    """The recorded cases flip what the planner's rules decide (each both ways)."""
    c, want, _, _ = plans
    assert set(want["kernel"].tolist()) == {F32, VALU, PLANE, RING, X3, E8}
    assert set(want["tm"].tolist()) == {64, 128, 192, 256} and set(want["staging"].tolist()) == {0, 1, 2}
    assert {0, 1} == set(want["lds_epilogue"].tolist()) == set(want["vec_epilogue"].tolist())
    assert set(want["epi_launched"].tolist()) == set(range(7))
    assert {0, 1} == set(want["refused"].tolist()) == set(want["valu_fits"].tolist())
    free = (c["variant"] == 0) & (c["valu"] == 0) & (c["prec"] > 0)
    big = (c["M"] >= 256) & (c["N"] >= 256)
    assert (free & big & (want["kernel"] == E8)).any() and (free & big & (want["kernel"] == RING)).any()
    assert (free & big & (want["kernel"] == PLANE)).any()  # K <= 64 and few tiles
    assert (free & (c["abits"] == 1) & (want["kernel"] == RING)).any()  # a plane of 2^32 elements


def test_plan_invariants(plans):
    c, _, p, _ = plans
    M, N, K, batch = c["M"], c["N"], c["K"], c["batch"]
    need = np.where(p["split"] > 1, batch * p["split"] * M * N, 0)
    assert (p["ws_elems"] == need).all()
    fixed = np.isin(c["epi"], (BCE, SIGMOID))
    assert (p["split"][fixed & (c["split"] == 0)] == 1).all()
    assert (p["ntm"] == -(-M // p["tm"])).all() and (p["ntn"] == -(-N // p["tn"])).all()
    assert (p["kchunk"] * p["split"] >= K).all()
    # the eight-phase kernel addresses a plane by 32-bit element offsets
    ea = np.where(c["at"] == 1, K, M) * c["lda"]
    eb = np.where(c["bt"] == 1, N, K) * c["ldb"]
    e8 = p["kernel"] == E8
    assert (ea[e8] < 2**32).all() and (eb[e8] < 2**32).all() and (ea >= 2**32).any() and (eb >= 2**32).any()
    assert ((p["tm"][e8] == 256) & (p["tn"][e8] == 256) & (p["lds_epilogue"][e8] == 1)).all()
    # 192-row tiles: a k-contiguous A, not the BCE head / sigmoid
    t192 = p["tm"] == 192
    assert t192.any() and (c["at"][t192] == 0).all() and not fixed[t192].any()
    assert np.isin(p["kernel"][t192], (RING, X3)).all()
    # a split beyond the workspace is refused (hipErrorInvalidValue), forced or not: the column is
    # gemm_plan_refused (gemm_plan.h), the one function gemm_run and mvae_debug_plan both call
    max_ws = np.where(c["ws"] == 0, 0, c["max_ws"]).astype(np.float64)
    over = (p["split"] > 1) & (need.astype(np.float64) > max_ws)
    assert (p["refused"] == over).all()
    assert (c["split"][over] > 1).all()  # (the planner itself never exceeds it)
    forced = c["split"] > 0
    assert (p["split"][forced] == c["split"][forced]).all()
    # kernels by precision; the launched epilogue
    assert np.isin(p["kernel"][(c["prec"] == 0) & (c["valu"] == 0) & (c["variant"] != 9)], (F32,)).all()
    assert (p["kernel"][(c["valu"] == 1) | (c["variant"] == 9)] == VALU).all()
    assert (p["epi_launched"][p["split"] > 1] == STORE).all()
    assert (c["epi"][p["epi_launched"] == BCEB] == BCE).all() and (c["epi"][p["epi_launched"] == DACTB] == DACT).all()
    assert (p["vec_epilogue"] <= p["lds_epilogue"]).all()
    assert (p["valu_fits"][c["variant"] != 0] == 0).all()


def test_the_recorded_plans_hold_empty_slices(plans):
    """kchunk is a whole number of k-tiles, so kchunk * split may pass K by whole slices: the planner's own
    splits (nothing forced) include plans whose last slices start at or past K. The kernels write a zero
    slab there (tests/test_gpu_gemm_batch.py); DESIGN.md 5t."""
    c, _, p, _ = plans
    empty = (p["split"] > 1) & ((p["split"] - 1) * p["kchunk"] >= c["K"])
    assert (empty & (c["split"] == 0)).any()

"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports every
symbol ``include/mvae.h`` declares (no compute without a GPU)."""
import ctypes
import os
import re

import pytest

from magic_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    src = open(os.path.join(ROOT, "include", "mvae.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mvae_[a-z_0-9]+)\s*\(", src)))


def test_library_loads_and_exports_header():
    lib = _lib.load()
    syms = header_symbols()
    assert len(syms) >= 19
    for s in syms:
        assert hasattr(lib, s), s
    assert set(syms) == set(_lib.EXPORTED), set(syms) ^ set(_lib.EXPORTED)
    assert lib.mvae_abi_version() == _lib.ABI_VERSION


def test_struct_layout_matches_header(tmp_path):
    """ctypes mirrors of mvae_cfg / mvae_tensor agree with the C compiler's layout."""
    import shutil
    import subprocess
    got = (ctypes.sizeof(_lib.mvae_cfg), _lib.mvae_cfg.seed.offset, ctypes.sizeof(_lib.mvae_tensor))
    if shutil.which("gcc") is None:
        assert got == (112, 104, 72)
        return
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\n'
                   'int main(){printf("%%zu %%zu %%zu", sizeof(mvae_cfg), offsetof(mvae_cfg, seed),'
                   ' sizeof(mvae_tensor));}\n' % os.path.join(ROOT, "include", "mvae.h"))
    exe = tmp_path / "s"
    subprocess.check_call(["gcc", str(src), "-o", str(exe)])
    want = tuple(int(v) for v in subprocess.check_output([str(exe)]).split())
    assert got == want


def test_create_rejects_bad_config_without_gpu_work():
    lib = _lib.load()
    c = _lib.mvae_cfg()
    c.image_size = 0
    h = ctypes.c_void_p()
    rc = lib.mvae_create(ctypes.byref(c), 0, ctypes.byref(h))
    assert rc < 0 and h.value is None
    assert b"positive" in lib.mvae_last_error(None)
    assert lib.mvae_create(None, 0, ctypes.byref(h)) < 0


REMOVED_OPTIONS = ["deint_fuse=1", "deint_fuse_diag=1", "deint_variant=8", "e8_prio=1", "diag_skip_deint=1",
                   "diag_shadow_deint=1", "diag_shadow_at=1", "diag_chain=1",
                   "conv2_half=0", "conv2_nw=4", "conv2_tpb=2", "conv2_fpw=4", "conv2_wg=4"]


@pytest.mark.parametrize("option", REMOVED_OPTIONS)
def test_create_rejects_removed_options(option):
    """The rejected experiments' create options are gone: each name is an unknown option now
    (MVAE_EINVAL, a null handle). Options are parsed before the first HIP call, so no GPU is needed."""
    lib = _lib.load()
    c = _lib.mvae_cfg()
    c.image_size, c.batch, c.global_batch = 10, 4, 4
    c.n_enc = 2
    c.enc[0], c.enc[1] = 12, 10
    c.dec[0], c.dec[1] = 10, 12
    c.latent = 3
    c.deform_weight = 1.0
    c.lr[0], c.lr[1] = 1e-3, 1e-3
    c.beta1, c.beta2, c.epsilon = 0.9, 0.999, 1e-8
    h = ctypes.c_void_p()
    rc = lib.mvae_create_ex(ctypes.byref(c), 0, option.encode(), ctypes.byref(h))
    assert rc == -1 and h.value is None  # MVAE_EINVAL
    err = lib.mvae_last_error(None)
    assert b"unknown option" in err and option.encode() in err, err


@pytest.mark.parametrize("bit", [1, 2, 4, 8, 16, 32, 64, 128])
def test_bench_gemm_refuses_removed_diagnostics(bit):
    """mvae_bench_gemm's variant bits 12-19 selected kernel timing diagnostics that are gone: each is
    MVAE_EINVAL with the entry's name in the message, at argument validation (before any allocation
    or HIP call, so no GPU is needed)."""
    lib = _lib.load()
    ms = ctypes.c_float()
    rc = lib.mvae_bench_gemm(256, 256, 64, 0, 0, 1, 16 | (bit << 12), 1, None, ctypes.byref(ms))
    assert rc == -1  # MVAE_EINVAL
    assert b"mvae_bench_gemm" in lib.mvae_last_error(None)


@pytest.mark.parametrize("bit", [1, 2, 3, 4, 5, 6])
def test_debug_conv2_refuses_removed_kernel_forms(bit):
    """mvae_debug_conv2's mfma bits 1-6 selected the conv2 kernel forms that are gone (the full-channel
    forward / data-gradient kernel and its shapes, the 4-wave weight gradient): each is MVAE_EINVAL
    with the entry's name in the message, at argument validation -- the pointers here are fakes that
    nothing may read, so no GPU is needed."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    for mode in (0, 1, 2):
        rc = lib.mvae_debug_conv2(6, 1, mode, 1 | (1 << bit), p, p, p, None)
        assert rc == -1  # MVAE_EINVAL
        assert b"mvae_debug_conv2" in lib.mvae_last_error(None)


def test_engine_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from magic_amd.engine import Engine
    from magic_amd.config import preset
    with pytest.raises(_lib.MVAELibraryError):
        Engine(preset("8c", image_size=10, batch=4))


def test_missing_library_is_an_error(tmp_path):
    with pytest.raises(_lib.MVAELibraryError):
        _lib.load(str(tmp_path / "nope.so"))


def test_build_id_ties_library_to_sources():
    """libmvae.so carries the hash of the sources it was built from; the loader refuses a
    library whose id differs from the sources on disk (a stale or foreign build)."""
    from magic_amd.build import source_files, source_hash
    lib = _lib.load()
    assert lib.mvae_build_id().decode() == source_hash()
    assert any(p.endswith("mvae_api.cpp") for p in source_files())
    assert any(p.endswith(os.path.join("include", "mvae.h")) for p in source_files())
    with pytest.raises(_lib.MVAELibraryError, match="stale"):
        _lib.verify_build(lib, expected="0" * 16)


def test_build_id_ignores_stray_files_and_names_missing_sources(tmp_path, monkeypatch):
    """Only the compiled sources enter the build id (a stray file under csrc/ does not make the
    library "stale"); a missing source raises MVAELibraryError naming it, not a bare OSError."""
    from magic_amd import build
    lib = _lib.load()
    stray = os.path.join(build.CSRC, "zz_stray_editor_file.orig")
    with open(stray, "w") as f:
        f.write("not a source\n")
    try:
        assert _lib.verify_build(lib) == build.source_hash()
    finally:
        os.remove(stray)
    monkeypatch.setattr(build, "SOURCES", build.SOURCES + ["does_not_exist.hip"])
    with pytest.raises(_lib.MVAELibraryError, match="does_not_exist.hip"):
        _lib.verify_build(lib)


def test_every_native_source_is_in_the_build():
    """Every *.cpp, *.hip and *.h under csrc/ is named in SOURCES or HEADERS, so a new file cannot
    be compiled from, or included, while staying outside the build id."""
    from magic_amd import build
    named = {os.path.normpath(os.path.join(build.CSRC, f)) for f in build.SOURCES + build.HEADERS}
    on_disk = {os.path.join(build.CSRC, f) for f in os.listdir(build.CSRC)
               if f.endswith((".cpp", ".hip", ".h"))}
    assert on_disk and not sorted(on_disk - named)
    assert all(os.path.isfile(p) for p in named)

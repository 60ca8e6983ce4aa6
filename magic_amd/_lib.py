"""ctypes binding of ``libmvae.so`` (the C ABI declared in ``include/mvae.h``).

The library is the product path: nothing here falls back to a CPU or PyTorch
implementation. If the shared object is missing or cannot be loaded, importing the
engine raises ``MVAELibraryError`` with the reason.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MVAE_LIB", os.path.join(HERE, "libmvae.so"))

MVAE_MAX_ENC = 8
MARKER_GRID = 4096   # mvae_region_marker workgroups = MARKER_GRID + region (mvae_internal.h)
ABI_VERSION = 7

ACT = {"tanh": 0, "elu": 1}
METRIC = {"cosine": 0, "sqdiff": 1}
PREC = {"f32": 0, "bf16": 1, "f32x": 2}

KIND_PARAM, KIND_GRAD1, KIND_GRAD2, KIND_M1, KIND_V1, KIND_M2, KIND_V2 = range(7)
(BUF_PARAMS, BUF_GRADS, BUF_ADAM, BUF_LOSSES, BUF_COLSQ, BUF_COLDOT, BUF_DIST, BUF_GRADS_DEC,
 BUF_DEAD, BUF_EPS, BUF_DYN) = range(11)


class MVAELibraryError(RuntimeError):
    pass


class MVAEError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libmvae error {code}: {msg}")
        self.code = code


class mvae_cfg(C.Structure):
    _fields_ = [
        ("image_size", C.c_int), ("batch", C.c_int), ("global_batch", C.c_int),
        ("n_enc", C.c_int), ("enc", C.c_int * MVAE_MAX_ENC), ("dec", C.c_int * 2),
        ("latent", C.c_int), ("act", C.c_int), ("metric", C.c_int), ("reciprocal", C.c_int),
        ("deform_weight", C.c_float), ("lr", C.c_float * 2),
        ("beta1", C.c_float), ("beta2", C.c_float), ("epsilon", C.c_float),
        ("precision", C.c_int), ("seed", C.c_uint64), ("conv", C.c_int),
    ]


class mvae_pairs(C.Structure):
    """A batch described by its sources (``include/mvae.h``): device pointers and sizes."""
    _fields_ = [("locks", C.c_void_p), ("keys", C.c_void_p), ("height", C.c_int), ("width", C.c_int),
                ("idx", C.c_void_p), ("coef", C.c_void_p), ("divisor", C.c_float)]


class mvae_xpairs(C.Structure):
    """``mvae_pairs`` with a key index of its own (``include/mvae.h``): row b is lock ``p.idx[b]`` and
    key ``key_idx[b]``."""
    _fields_ = [("p", mvae_pairs), ("key_idx", C.c_void_p)]


class mvae_images(C.Structure):
    """Single images of one uint8 table (``include/mvae.h``): device pointers and sizes."""
    _fields_ = [("table", C.c_void_p), ("height", C.c_int), ("width", C.c_int), ("idx", C.c_void_p),
                ("divisor", C.c_float)]


class mvae_match_opts(C.Structure):
    """Options of ``mvae_match_ex`` (``include/mvae.h``): a zeroed one is ``mvae_match``."""
    _fields_ = [("rl", C.c_void_p), ("rk", C.c_void_p), ("key_base", C.c_int64), ("carry", C.c_int),
                ("dist_ld", C.c_int64), ("thr_val", C.c_void_p), ("thr_idx", C.c_void_p), ("ahead", C.c_void_p)]


HEAD_FWD, HEAD_COLSTATS, HEAD_METRIC, HEAD_LOSS, HEAD_BWD = range(5)


class mvae_head_args(C.Structure):
    """Arguments of ``mvae_debug_head`` (``include/mvae.h``): sizes and device pointers; a zeroed
    field is a NULL / 0 argument."""
    _fields_ = [("mode", C.c_int), ("B", C.c_int), ("L", C.c_int), ("Bg", C.c_int), ("ldz", C.c_int),
                ("ldh", C.c_int), ("off", C.c_int), ("zmask", C.c_int), ("z_planes", C.c_int),
                ("h_planes", C.c_int), ("cs_mode", C.c_int), ("nblk", C.c_int), ("metric", C.c_int),
                ("recip", C.c_int), ("w", C.c_float), ("seed", C.c_uint64), ("counter", C.c_uint64),
                ("ms", C.c_void_p), ("eps", C.c_void_p), ("areas", C.c_void_p), ("rowpart", C.c_void_p),
                ("dzdec", C.c_void_p), ("z", C.c_void_p), ("zp", C.c_void_p), ("rowfwd", C.c_void_p),
                ("colsq", C.c_void_p), ("coldot", C.c_void_p), ("draw", C.c_void_p), ("part", C.c_void_p),
                ("cnt", C.c_void_p), ("out", C.c_void_p), ("rowvals", C.c_void_p), ("dist", C.c_void_p),
                ("losses", C.c_void_p), ("dhead", C.c_void_p), ("hp", C.c_void_p)]


EPI_ACT, EPI_DACT, EPI_BCE = 1, 2, 3


class mvae_epi_args(C.Structure):
    """Arguments of ``mvae_debug_epi`` (``include/mvae.h``): sizes and device pointers; a zeroed
    field is a NULL / 0 argument."""
    _fields_ = [("M", C.c_int), ("N", C.c_int), ("K", C.c_int), ("lda", C.c_int), ("ldb", C.c_int),
                ("bt", C.c_int), ("prec", C.c_int), ("variant", C.c_int), ("x3", C.c_int), ("epi", C.c_int),
                ("act", C.c_int), ("ldc", C.c_int), ("ncp", C.c_int), ("ldx", C.c_int), ("ldbits", C.c_int),
                ("ldy", C.c_int), ("rp_ld", C.c_int), ("rp_off", C.c_int), ("split_c0", C.c_int),
                ("ld_aux", C.c_int), ("remap_split", C.c_int), ("remap_shift", C.c_int), ("padw", C.c_int),
                ("scale", C.c_float), ("pc", C.c_longlong),
                ("A", C.c_void_p), ("B", C.c_void_p), ("du", C.c_void_p), ("cp", C.c_void_p),
                ("x", C.c_void_p), ("xp", C.c_void_p), ("dyn", C.c_void_p), ("xbits", C.c_void_p),
                ("y", C.c_void_p), ("rowpart", C.c_void_p), ("aux", C.c_void_p), ("auxp", C.c_void_p)]


class mvae_plan_args(C.Structure):
    """Arguments of ``mvae_debug_plan`` (``include/mvae.h``): everything a GEMM's kernel choice reads.
    The pointers are never followed (only their alignment is read)."""
    _fields_ = ([(n, C.c_int) for n in ("M", "N", "K", "batch", "at", "bt", "lda", "ldb", "ldc", "prec", "nA", "nB",
                                        "dynA", "epi", "c32", "xdyn", "padw", "ld_aux", "ldx", "ldy", "abits", "x3",
                                        "tm", "split", "valu", "variant")] +
                [(n, C.c_longlong) for n in ("pA", "pB", "sA", "sB", "sC", "pc")] + [("max_ws", C.c_ulonglong)] +
                [(n, C.c_void_p) for n in ("Ap", "Bp", "C", "cp", "aux", "auxp", "x", "xp", "y", "ws")])


class mvae_plan_out(C.Structure):
    """What ``mvae_debug_plan`` reports: the kernel (``KERNEL_NAMES``) and its launch plan."""
    _fields_ = ([(n, C.c_int) for n in ("kernel", "staging", "tm", "tn", "ntm", "ntn", "group", "split", "kchunk",
                                        "lds_epilogue", "vec_epilogue", "epi_launched", "valu_fits", "refused")] +
                [("ws_elems", C.c_ulonglong)])


class mvae_gemm_args(C.Structure):
    """Arguments of ``mvae_debug_gemm_ex`` (``include/mvae.h``): one batched GEMM on caller buffers; a
    zeroed field is its default."""
    _fields_ = ([(n, C.c_int) for n in ("M", "N", "K", "batch", "at", "bt", "lda", "ldb", "ldc", "prec", "variant",
                                        "x3", "tm", "split", "group", "epi", "act", "bits", "bits_shared", "a_off",
                                        "b_off")] +
                [(n, C.c_longlong) for n in ("sA", "sB", "sC", "a_elems", "b_elems", "c_elems")] +
                [(n, C.c_void_p) for n in ("A", "B", "C")] + [("a_dyn", C.c_int)])


class mvae_input_args(C.Structure):
    """Arguments of ``mvae_debug_input_planes`` (``include/mvae.h``): one route of batch input on caller
    buffers; a zeroed field is a NULL / 0 argument."""
    _fields_ = ([(n, C.c_int) for n in ("route", "B", "H", "W", "ldx", "np", "f32mask", "f32dyn_mask", "ldbits",
                                        "no_xbw", "slot")] + [("divisor", C.c_float)] +
                [(n, C.c_longlong) for n in ("plane_stride", "x_elems", "xs_elems", "planes_elems", "xbits_elems")] +
                [(n, C.c_void_p) for n in ("x", "locks", "keys", "idx", "key_idx", "coef", "xs", "planes", "xbits",
                                           "xbf", "xbw", "dyn")])


KERNEL_NAMES = {1: "f32", 2: "valu", 3: "plane", 4: "ring", 5: "x3", 6: "e8"}


class mvae_tensor(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("data", C.c_void_p), ("rows", C.c_int),
                ("cols", C.c_int), ("ld", C.c_int), ("trained_by", C.c_int)]


_SIGS = {
    "mvae_abi_version": ([], C.c_int),
    "mvae_build_id": ([], C.c_char_p),
    "mvae_create": ([C.POINTER(mvae_cfg), C.c_int, C.POINTER(C.c_void_p)], C.c_int),
    "mvae_create_ex": ([C.POINTER(mvae_cfg), C.c_int, C.c_char_p, C.POINTER(C.c_void_p)], C.c_int),
    "mvae_destroy": ([C.c_void_p], C.c_int),
    "mvae_last_error": ([C.c_void_p], C.c_char_p),
    "mvae_param_count": ([C.c_void_p], C.c_int),
    "mvae_param_info": ([C.c_void_p, C.c_int, C.c_int, C.POINTER(mvae_tensor)], C.c_int),
    "mvae_buffer": ([C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)], C.c_int),
    "mvae_get_step": ([C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)], C.c_int),
    "mvae_set_step": ([C.c_void_p, C.c_int64, C.c_int64], C.c_int),
    "mvae_set_shard": ([C.c_void_p, C.c_int64], C.c_int),
    "mvae_get_rng": ([C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)], C.c_int),
    "mvae_set_rng": ([C.c_void_p, C.c_uint64, C.c_uint64], C.c_int),
    "mvae_sync_params": ([C.c_void_p, C.c_void_p], C.c_int),
    "mvae_forward": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "mvae_metric": ([C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "mvae_backward": ([C.c_void_p, C.c_void_p], C.c_int),
    "mvae_backward_part": ([C.c_void_p, C.c_int, C.c_void_p], C.c_int),
    "mvae_backward_nparts": ([C.c_void_p], C.c_int),
    "mvae_grad_range": ([C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)], C.c_int),
    "mvae_set_option": ([C.c_void_p, C.c_char_p, C.c_int], C.c_int),
    "mvae_adam": ([C.c_void_p, C.c_void_p], C.c_int),
    "mvae_train_step": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                         C.c_void_p], C.c_int),
    "mvae_predict": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "mvae_predict_encode": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "mvae_predict_finish": ([C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "mvae_transform": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "mvae_reconstruct": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "mvae_generate": ([C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p], C.c_int),
    "mvae_make_batch": ([C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                         C.c_float, C.c_void_p, C.c_void_p], C.c_int),
    "mvae_forward_pairs": ([C.c_void_p, C.POINTER(mvae_pairs), C.c_void_p, C.c_void_p], C.c_int),
    "mvae_train_step_pairs": ([C.c_void_p, C.POINTER(mvae_pairs), C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_void_p], C.c_int),
    "mvae_predict_pairs": ([C.c_void_p, C.POINTER(mvae_pairs), C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "mvae_predict_encode_pairs": ([C.c_void_p, C.POINTER(mvae_pairs), C.c_void_p, C.c_void_p], C.c_int),
    "mvae_transform_pairs": ([C.c_void_p, C.POINTER(mvae_pairs), C.c_void_p, C.c_void_p], C.c_int),
    "mvae_reconstruct_pairs": ([C.c_void_p, C.POINTER(mvae_pairs), C.c_void_p, C.c_void_p, C.c_void_p],
                               C.c_int),
    "mvae_make_batch_x": ([C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                           C.c_float, C.c_void_p, C.c_void_p], C.c_int),
    "mvae_forward_xpairs": ([C.c_void_p, C.POINTER(mvae_xpairs), C.c_void_p, C.c_void_p], C.c_int),
    "mvae_train_step_xpairs": ([C.c_void_p, C.POINTER(mvae_xpairs), C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p], C.c_int),
    "mvae_predict_xpairs": ([C.c_void_p, C.POINTER(mvae_xpairs), C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "mvae_predict_encode_xpairs": ([C.c_void_p, C.POINTER(mvae_xpairs), C.c_void_p, C.c_void_p], C.c_int),
    "mvae_transform_xpairs": ([C.c_void_p, C.POINTER(mvae_xpairs), C.c_void_p, C.c_void_p], C.c_int),
    "mvae_reconstruct_xpairs": ([C.c_void_p, C.POINTER(mvae_xpairs), C.c_void_p, C.c_void_p, C.c_void_p],
                                C.c_int),
    "mvae_embed_images": ([C.c_void_p, C.POINTER(mvae_images), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p],
                          C.c_int),
    "mvae_match": ([C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p,
                    C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "mvae_match_colsq": ([C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p], C.c_int),
    "mvae_match_rnorm": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "mvae_match_ex": ([C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int,
                       C.POINTER(mvae_match_opts), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "mvae_pair_scores": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                          C.c_void_p], C.c_int),
    "mvae_match_merge": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p,
                          C.c_void_p, C.c_void_p], C.c_int),
    "mvae_overlap_work_bytes": ([C.c_int64, C.c_int, C.c_int, C.c_int], C.c_size_t),
    "mvae_overlap_pairs": ([C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int64,
                            C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "mvae_rerank_work_bytes": ([C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int], C.c_size_t),
    "mvae_rerank": ([C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int,
                     C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
                    C.c_int),
    "mvae_overlap_place": ([C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int64,
                            C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "mvae_timing_enable": ([C.c_void_p, C.c_int], C.c_int),
    "mvae_timing_select": ([C.c_void_p, C.c_int], C.c_int),
    "mvae_timing_marker": ([C.c_void_p, C.c_int, C.c_int], C.c_int),
    "mvae_timing_regions": ([C.c_void_p], C.c_int),
    "mvae_timing_name": ([C.c_void_p, C.c_int], C.c_char_p),
    "mvae_timing_read": ([C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int64)], C.c_int),
    "mvae_timing_reset": ([C.c_void_p], C.c_int),
    "mvae_bench_gemm": ([C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                         C.c_void_p, C.POINTER(C.c_float)], C.c_int),
    "mvae_bench_deint": ([C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_float)], C.c_int),
    "mvae_debug_conv2": ([C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                          C.c_void_p], C.c_int),
    "mvae_debug_tower": ([C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "mvae_debug_pairs_bits": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float,
                               C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                               C.c_void_p, C.c_void_p, C.c_int, C.c_void_p], C.c_int),
    "mvae_debug_xpairs_bits": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p], C.c_int),
    "mvae_debug_gemm": ([C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                         C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                         C.c_int, C.c_void_p], C.c_int),
    "mvae_debug_chain": ([C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int,
                          C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int),
                          C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_void_p], C.c_int),
    "mvae_debug_head": ([C.POINTER(mvae_head_args), C.c_void_p], C.c_int),
    "mvae_debug_epi": ([C.POINTER(mvae_epi_args), C.c_void_p], C.c_int),
    "mvae_debug_plan": ([C.POINTER(mvae_plan_args), C.POINTER(mvae_plan_out)], C.c_int),
    "mvae_debug_gemm_ex": ([C.POINTER(mvae_gemm_args), C.POINTER(mvae_plan_out), C.c_void_p], C.c_int),
    "mvae_debug_input_planes": ([C.POINTER(mvae_input_args), C.c_void_p], C.c_int),
}

EXPORTED = tuple(_SIGS)

_lib = None


def load(path: str | None = None):
    """Load and type the library once. Raises MVAELibraryError if it is unavailable."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise MVAELibraryError(
            f"{p} not found: build it with `python -m magic_amd.build` (hipcc, gfx950). "
            "There is no CPU fallback for the product path.")
    # torch first: it carries the process's HIP runtime (same soname as ours), so the
    # library binds to the runtime that owns torch's device pointers and streams.
    import torch  # noqa: F401
    try:
        lib = C.CDLL(p)
    except OSError as e:
        raise MVAELibraryError(f"cannot load {p}: {e}") from e
    for name, (args, res) in _SIGS.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = res
    v = lib.mvae_abi_version()
    if v != ABI_VERSION:
        raise MVAELibraryError(f"ABI version mismatch: library {v}, binding {ABI_VERSION}")
    verify_build(lib)
    if path is None:
        _lib = lib
    return lib


def verify_build(lib, expected: str | None = None) -> str:
    """The library's build id must equal the hash of the sources on disk (magic_amd/build.py
    source_hash): a libmvae.so built from other sources (stale, or shipped from another tree)
    is refused. Returns the id."""
    from .build import source_hash
    got = lib.mvae_build_id().decode()
    try:
        want = expected if expected is not None else source_hash()
    except FileNotFoundError as e:
        raise MVAELibraryError(
            f"cannot verify libmvae.so (build id {got}): source file missing ({e.filename}); the "
            "library is only loaded from a tree holding the sources it was built from") from e
    if got != want:
        raise MVAELibraryError(
            f"libmvae.so build id {got} does not match the sources on disk ({want}): the library "
            "is stale; rebuild it with `python -m magic_amd.build`")
    return got


def check(lib, ctx, rc):
    if rc != 0:
        msg = lib.mvae_last_error(ctx)
        raise MVAEError(rc, msg.decode() if msg else "")
    return rc


# ------------------------------------------------------------------------- DLPack
# Zero-copy torch views of context-owned device memory (params, grads, Adam slots):
# a DLManagedTensor (device kDLROCM) wrapped in a "dltensor" PyCapsule.
class _DLDevice(C.Structure):
    _fields_ = [("device_type", C.c_int32), ("device_id", C.c_int32)]


class _DLDataType(C.Structure):
    _fields_ = [("code", C.c_uint8), ("bits", C.c_uint8), ("lanes", C.c_uint16)]


class _DLTensor(C.Structure):
    _fields_ = [("data", C.c_void_p), ("device", _DLDevice), ("ndim", C.c_int32),
                ("dtype", _DLDataType), ("shape", C.POINTER(C.c_int64)),
                ("strides", C.POINTER(C.c_int64)), ("byte_offset", C.c_uint64)]


class _DLManagedTensor(C.Structure):
    pass


_DELETER = C.CFUNCTYPE(None, C.POINTER(_DLManagedTensor))
_DLManagedTensor._fields_ = [("dl_tensor", _DLTensor), ("manager_ctx", C.c_void_p),
                             ("deleter", _DELETER)]

_KDLROCM = 10
_KDLFLOAT = 2
_PyCapsule_New = C.pythonapi.PyCapsule_New
_PyCapsule_New.restype = C.py_object
_PyCapsule_New.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p]


def device_view(ptr: int, shape, strides, device: int, keepalive: list):
    """torch.float32 tensor aliasing device memory at ``ptr`` (owned by a libmvae context).

    ``keepalive`` must outlive the tensor (the engine keeps it); the view must not be used
    after the context is destroyed."""
    import torch
    nd = len(shape)
    shp = (C.c_int64 * nd)(*shape)
    std = (C.c_int64 * nd)(*strides)
    mt = _DLManagedTensor()
    mt.dl_tensor.data = ptr
    mt.dl_tensor.device = _DLDevice(_KDLROCM, device)
    mt.dl_tensor.ndim = nd
    mt.dl_tensor.dtype = _DLDataType(_KDLFLOAT, 32, 1)
    mt.dl_tensor.shape = shp
    mt.dl_tensor.strides = std
    mt.dl_tensor.byte_offset = 0
    mt.manager_ctx = None
    mt.deleter = _DELETER()  # NULL: memory belongs to the context
    keepalive.extend([shp, std, mt])
    cap = _PyCapsule_New(C.addressof(mt), b"dltensor", None)
    return torch.utils.dlpack.from_dlpack(cap)

"""The cases of the batched-GEMM pins (tests/test_abi_gemm_ex.py on the CPU, tests/test_gpu_gemm_batch.py
on the GPU): plain dicts of the fields of mvae_gemm_args (include/mvae.h) plus a name, pointers left out.

What the table is for: every GEMM family decodes a workgroup number into a batch element, a split-K
slice and a tile (tile_of_t, gemm_common.h) and offsets its operands, its output or slabs and its
BitMat by them. The cases put a batch of 2 or 3 with strides of every alignment class on each of the
six kernels and the four ring tiles, force splits whose last slice is empty or one partial k-tile,
walk the tiles in ragged bands, and take each alignment fallback that is keyed on a batch stride.
test_abi_gemm_ex.py asserts, through mvae_debug_plan, that the cases reach what they are named for.
"""
F32, VALU, PLANE, RING, X3, E8 = 1, 2, 3, 4, 5, 6
PREC_F32, PREC_BF16, PREC_F32X = 0, 1, 2

FIELDS = ("M", "N", "K", "batch", "at", "bt", "lda", "ldb", "ldc", "prec", "variant", "x3", "tm", "split", "group",
          "epi", "act", "bits", "bits_shared", "a_off", "b_off", "sA", "sB", "sC", "a_elems", "b_elems", "c_elems")


def round8(v):
    return (v + 7) // 8 * 8


def a_shape(c):
    """(rows, columns) of one batch element's stored A."""
    return (c["K"], c["M"]) if c["at"] else (c["M"], c["K"])


def b_shape(c):
    return (c["N"], c["K"]) if c["bt"] else (c["K"], c["N"])


def make(name, M, N, K, *, batch=2, at=0, bt=0, prec=PREC_BF16, variant=0, x3=0, tm=0, split=0, group=0, epi=0,
         act=0, bits=0, bits_shared=0, a_off=0, b_off=0, lda=None, ldb=None, ldc=None, sA=None, sB=None, sC=None,
         dsA=0, dsB=0, dsC=0):
    """A case with the step's defaults where nothing is said: rows padded to 8 elements, ldc one chunk
    wider than a row, the A and B windows back to back, 16 elements between the C windows. dsA / dsB /
    dsC are added to those default strides."""
    c = dict(name=name, M=M, N=N, K=K, batch=batch, at=at, bt=bt, prec=prec, variant=variant, x3=x3, tm=tm,
             split=split, group=group, epi=epi, act=act, bits=bits, bits_shared=bits_shared, a_off=a_off, b_off=b_off)
    ar, ac = a_shape(c)
    br, bc = b_shape(c)
    c["lda"] = round8(ac) if lda is None else lda
    c["ldb"] = round8(bc) if ldb is None else ldb
    c["ldc"] = round8(N) + 8 if ldc is None else ldc
    c["sA"] = (ar * c["lda"] if sA is None else sA) + dsA
    c["sB"] = (br * c["ldb"] if sB is None else sB) + dsB
    c["sC"] = (M * c["ldc"] + 16 if sC is None else sC) + dsC
    c["a_elems"] = (batch - 1) * c["sA"] + ar * c["lda"]
    c["b_elems"] = (batch - 1) * c["sB"] + br * c["ldb"]
    c["c_elems"] = (batch - 1) * c["sC"] + M * c["ldc"]
    # the host fill writes each window's rows whole: overlapping windows share their row structure
    assert c["sA"] >= ar * c["lda"] or c["sA"] % c["lda"] == 0, name
    assert c["sB"] >= br * c["ldb"] or c["sB"] % c["ldb"] == 0, name
    return c


def _cases():
    out = []
    add = lambda *a, **k: out.append(make(*a, **k))  # noqa: E731

    # ---- the fp32 MFMA kernel (128x128 tiles, k-tiles of 32) and the fp32 VALU kernel (64x64, k-chunks of 32)
    for fam, v in (("f32", 4), ("valu", 9)):
        kw = dict(prec=PREC_F32, variant=v)
        add(f"{fam}_unsplit", 130, 70, 100, split=1, **kw)
        add(f"{fam}_unsplit_at_bt_b3", 130, 70, 100, batch=3, at=1, bt=1, split=1, **kw)
        add(f"{fam}_empty_slice", 130, 70, 288, at=1, split=4, **kw)          # kchunk 96: slice 3 starts at K
        add(f"{fam}_empty_slice_b3", 130, 70, 288, batch=3, bt=1, split=4, **kw)
        add(f"{fam}_tail_slice", 130, 70, 208, bt=1, split=3, **kw)           # kchunk 96: slice 2 is k 192..207
        add(f"{fam}_tail_slice_at", 130, 70, 208, at=1, split=3, **kw)
        add(f"{fam}_one_tile_slices", 130, 70, 96, split=3, **kw)             # every slice one k-tile
        add(f"{fam}_odd_strides", 130, 70, 100, split=2, lda=101, ldb=71, ldc=73, dsA=1, dsB=3, dsC=1, **kw)
        add(f"{fam}_act_split", 130, 70, 288, at=1, split=4, epi=1, act=1, **kw)
        add(f"{fam}_act", 130, 70, 100, split=1, epi=1, **kw)
        # the encoder weight gradients' form: at = 1, K = 2B stored rows of which the two windows share B
        add(f"{fam}_wgrad_overlap", 64, 40, 128, at=1, split=2, sA=64 * 64, dsC=3, **kw)
        add(f"{fam}_wgrad_overlap_b3", 70, 40, 256, batch=3, at=1, split=4, sA=128 * 72, **kw)
    # unforced: the planner's own plans with empty trailing slices (the latent head's weight-gradient class)
    add("f32_planner_empty_slice", 64, 40, 796, at=1, prec=PREC_F32)             # split 6, kchunk 160
    add("f32_planner_two_empty_slices", 64, 40, 1589, at=1, prec=PREC_F32)       # split 12
    add("valu_planner_split", 64, 40, 796, at=1, prec=PREC_F32, variant=9)

    # ---- the 128x128 plane kernel (k-tiles of 64), bf16 and f32x
    for fam, pr in (("plane_bf16", PREC_BF16), ("plane_f32x", PREC_F32X)):
        kw = dict(prec=pr, variant=4)
        add(f"{fam}_unsplit", 130, 70, 100, split=1, **kw)
        add(f"{fam}_empty_slice", 130, 70, 576, at=1, split=4, **kw)          # kchunk 192: slice 3 starts at K
        add(f"{fam}_tail_slice", 130, 70, 400, bt=1, split=3, **kw)           # kchunk 192: slice 2 is k 384..399
        add(f"{fam}_odd_strides", 130, 70, 200, batch=3, split=2, lda=201, ldb=71, ldc=73, dsA=1, dsB=3, dsC=1, **kw)
    add("plane_bf16_unsplit_at_bt_b3", 130, 70, 100, batch=3, at=1, bt=1, split=1, variant=4)
    add("plane_bf16_act_split", 130, 70, 576, at=1, split=4, epi=1, variant=4)
    add("plane_f32x_act", 130, 70, 100, bt=1, split=1, epi=1, act=1, prec=PREC_F32X, variant=4)
    add("plane_bf16_wgrad_overlap", 130, 70, 256, at=1, split=2, sA=128 * 136, variant=4)
    # a forced ring number that the batch strides or the image's alignment send to the plane kernel
    add("ring_to_plane_sA", 300, 260, 576, at=1, variant=3, split=4, dsA=4)
    add("ring_to_plane_sB", 300, 260, 576, variant=3, split=1, dsB=4)
    add("ring_to_plane_a_off", 300, 260, 576, at=1, variant=3, split=4, a_off=3)
    add("ring_to_plane_b_off", 300, 260, 576, variant=13, split=1, b_off=4)

    # ---- the ring kernels at 256 / 192 rows and tile N 256 / 128, bf16 and f32x
    for tmr, tn in ((256, 256), (256, 128), (192, 256), (192, 128)):
        fam = f"ring{tmr}x{tn}"
        at = 1 if tmr == 256 else 0   # (192-row tiles: a k-contiguous A)
        kw = dict(variant=12 if tn == 256 else 11, tm=tmr)
        add(f"{fam}_unsplit", 300, 260, 200, at=at, split=1, **kw)
        add(f"{fam}_empty_slice", 300, 260, 576, at=at, split=4, **kw)
        add(f"{fam}_tail_slice_b3", 300, 260, 400, batch=3, at=at, bt=1, split=3, **kw)
        add(f"{fam}_f32x_empty_slice", 300, 260, 576, at=at, split=4, prec=PREC_F32X, **kw)
    add("ring_any_shape_empty_slice", 300, 260, 576, at=1, variant=3, split=4)         # 256x128 at split 4
    add("ring_any_shape_t192", 300, 260, 576, variant=3, tm=192, split=4)              # 192x128 at split 4
    add("ring_wgrad_overlap", 300, 260, 512, at=1, variant=3, split=2, sA=256 * 304, dsC=2)
    add("ring_act_split", 300, 260, 400, variant=11, tm=256, split=3, epi=1, act=1)
    add("ring_act", 300, 260, 200, variant=12, tm=192, split=1, epi=1)
    add("ring_one_tile_slices", 300, 260, 192, at=1, variant=3, split=3)
    add("ring_planner", 300, 260, 1100, at=1, variant=3)                                # the planner's split

    # ---- the plane-stacked x3 kernels (f32x, three-plane operands)
    kw = dict(prec=PREC_F32X, x3=1, variant=11)
    add("x3_256x128_unsplit", 300, 260, 200, at=1, split=1, **kw)
    add("x3_256x128_empty_slice", 300, 260, 576, at=1, split=4, **kw)
    add("x3_256x128_tail_slice_b3", 300, 260, 400, batch=3, bt=1, tm=256, split=3, **kw)
    add("x3_192x128_empty_slice", 300, 260, 576, tm=192, split=4, **kw)
    add("x3_192x128_tail_slice", 300, 260, 400, tm=192, split=3, **kw)
    add("x3_256x256_empty_slice", 300, 260, 576, at=1, split=4, prec=PREC_F32X, x3=2, variant=12, tm=256)
    add("x3_act_split", 300, 260, 400, at=1, split=3, epi=1, **kw)
    add("x3_act", 300, 260, 200, tm=192, split=1, epi=1, act=1, **kw)
    add("x3_wgrad_overlap", 300, 260, 512, at=1, split=2, sA=256 * 304, **kw)

    # ---- the eight-phase kernel: planes
    kw = dict(variant=13)
    add("e8_unsplit_vec", 300, 260, 200, split=1, **kw)
    add("e8_unsplit_novec", 300, 260, 200, split=1, dsC=2, **kw)                # sC % 4 != 0: element-wise epilogue
    add("e8_slabs_vec", 300, 260, 576, split=2, **kw)
    # slab rows are N floats and a slab M N: element-wise slab stores where N % 4 != 0 (M N % 4 != 0 implies it)
    add("e8_slabs_novec", 300, 257, 576, split=2, **kw)
    add("e8_slabs_novec_odd", 301, 257, 576, split=2, **kw)
    add("e8_empty_slice", 300, 260, 576, at=1, split=4, **kw)
    add("e8_empty_slice_b3", 300, 260, 576, batch=3, bt=1, split=4, **kw)
    add("e8_tail_slice", 300, 260, 400, at=1, split=3, **kw)
    add("e8_f32x_empty_slice", 300, 260, 576, at=1, split=4, prec=PREC_F32X, **kw)
    add("e8_f32x_tail_slice", 300, 260, 400, split=3, prec=PREC_F32X, **kw)
    add("e8_act_split", 300, 260, 400, split=3, epi=1, act=1, **kw)
    add("e8_act", 300, 260, 200, at=1, split=1, epi=1, **kw)
    add("e8_wgrad_overlap", 300, 260, 512, at=1, split=2, sA=256 * 304, **kw)
    add("e8_one_tile_slices", 300, 260, 192, split=3, **kw)
    # ---- ... and its two bits paths (A of 0/1 values), one BitMat per element or the step's shared one
    for reg in (1, 2):
        fam = "e8_bits_lds" if reg == 1 else "e8_bits_reg"
        kw = dict(variant=13, bits=reg)
        add(f"{fam}_unsplit", 300, 260, 200, split=1, **kw)
        add(f"{fam}_empty_slice", 300, 260, 576, at=1, split=4, **kw)
        add(f"{fam}_tail_slice_b3", 300, 260, 400, batch=3, split=3, **kw)
        add(f"{fam}_f32x_empty_slice", 300, 260, 576, at=1, split=4, prec=PREC_F32X, **kw)
        add(f"{fam}_act", 520, 260, 200, at=1, split=1, epi=1, **kw)
        # layer 0's weight gradient: at = 1, the windows share half their stored rows, one BitMat of all of
        # them with batch element 1 a k-tile offset into every strip
        add(f"{fam}_shared_overlap", 300, 260, 512, at=1, split=2, sA=256 * 304, bits_shared=1, **kw)
        add(f"{fam}_shared_b3_empty_slice", 520, 260, 576, batch=3, at=1, split=4, sA=64 * 520, bits_shared=1, **kw)
        add(f"{fam}_shared_back_to_back", 300, 260, 192, at=1, split=1, bits_shared=1, **kw)
    add("e8_bits_planner", 300, 260, 576, at=1, bits=2)                          # variant 0: the bits prefer E8

    # ---- tile order: bands of `group` m-tiles, the last band ragged (ntm 3)
    for g in (1, 2, 4):
        add(f"ring_group{g}", 600, 700, 130, at=1, variant=11, tm=256, split=1, group=g)       # 3 x 6 tiles
    add("ring_group2_slabs", 600, 700, 130, at=1, variant=11, tm=256, split=2, group=2)
    add("ring_group2_slabs_odd_sC", 600, 700, 130, at=1, variant=11, tm=256, split=2, group=2, dsC=1)
    add("ring192x256_group3",600, 700, 130, variant=12, tm=192, split=1, group=3)                  # 4 x 3 tiles
    add("e8_group2", 600, 700, 130, variant=13, split=1, group=2)                               # 3 x 3 tiles
    add("e8_group2_slabs_b3", 600, 700, 130, batch=3, at=1, variant=13, split=2, group=2)
    add("e8_bits_group2", 600, 700, 130, at=1, variant=13, split=1, group=2, bits=2)
    add("x3_group2", 600, 700, 130, at=1, prec=PREC_F32X, x3=1, variant=11, tm=256, split=1, group=2)
    add("x3_group2_slabs", 600, 700, 130, at=1, prec=PREC_F32X, x3=1, variant=11, tm=256, split=2, group=2)
    return out


CASES = _cases()
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def _pair_cases():
    """The cases of the plane-pair pins (tests/test_gpu_gemm_pairs.py): the f32x families at the table's
    smallest shapes that reach each kernel, batch 2, both at and both bt, unsplit and a forced split whose
    last slice is one partial k-tile (kchunk 192, K 400: k 384..399). A 192-row tile needs a k-contiguous
    A: those families run at = 0 alone."""
    fams = [("pairs_plane", 130, 70, dict(variant=4), (0, 1)),
            ("pairs_ring256", 300, 260, dict(variant=11, tm=256), (0, 1)),
            ("pairs_ring192", 300, 260, dict(variant=11, tm=192), (0,)),
            ("pairs_x3f1_256", 300, 260, dict(variant=11, x3=1, tm=256), (0, 1)),
            ("pairs_x3f1_192", 300, 260, dict(variant=11, x3=1, tm=192), (0,)),
            ("pairs_x3f2", 300, 260, dict(variant=12, x3=2, tm=256), (0, 1)),
            ("pairs_e8", 300, 260, dict(variant=13), (0, 1)),
            ("pairs_e8_bits_lds", 300, 260, dict(variant=13, bits=1), (0, 1)),
            ("pairs_e8_bits_reg", 300, 260, dict(variant=13, bits=2), (0, 1))]
    out = []
    for fam, M, N, kw, ats in fams:
        for at in ats:
            for bt in (0, 1):
                out.append(make(f"{fam}_at{at}_bt{bt}_unsplit", M, N, 200, at=at, bt=bt, split=1, prec=PREC_F32X, **kw))
                out.append(make(f"{fam}_at{at}_bt{bt}_tail_slice", M, N, 400, at=at, bt=bt, split=3, prec=PREC_F32X,
                                **kw))
    # unforced: the planner's own choice, which weighs a flag on A (fewer plane pairs expected)
    out.append(make("pairs_planner_at1", 300, 260, 576, at=1, prec=PREC_F32X))
    out.append(make("pairs_planner_bits", 300, 260, 576, at=1, prec=PREC_F32X, bits=2))
    return out


PAIR_CASES = _pair_cases()
PAIR_BY_NAME = {c["name"]: c for c in PAIR_CASES}
assert len(PAIR_BY_NAME) == len(PAIR_CASES) and not set(PAIR_BY_NAME) & set(BY_NAME)


def fill_args(a, c, **ptrs):
    """The case's fields (and the pointers given) into an mvae_gemm_args; a_dyn (A's run-time flag) is 0
    where the case does not name it."""
    for k in FIELDS:
        setattr(a, k, c[k])
    a.a_dyn = c.get("a_dyn", 0)
    for k, v in ptrs.items():
        setattr(a, k, v)
    return a


def plan_args(a, c, base):
    """The case as mvae_debug_plan's arguments (host arithmetic only): fake pointers at `base` (16-byte
    aligned) with the images' low four bits, an unlimited aligned workspace."""
    planes = 3 if c["prec"] == PREC_F32X else 1
    for k in ("M", "N", "K", "batch", "at", "bt", "lda", "ldb", "ldc", "prec", "epi", "x3", "tm", "split", "variant",
              "sA", "sB", "sC"):
        setattr(a, k, c[k])
    a.nA = a.nB = planes
    a.c32 = 1
    a.abits = 1 if c["bits"] else 0
    a.dynA = 1 if c.get("a_dyn", 0) else 0
    a.pA, a.pB = round8(c["a_elems"]), round8(c["b_elems"])
    a.max_ws = 2 ** 64 - 1
    a.Ap, a.Bp = base + 2 * c["a_off"], base + 2 * c["b_off"]
    a.C = a.ws = base
    return a

"""Conv-encoder variant (BASELINE config 5) on the HIP path vs the oracle
(oracle/conv_oracle.py, itself pinned against torch.autograd in tests/test_conv_oracle.py;
parity with the reference is unpinned by nature: the reference has no conv VAE).

f32 / f32x (tower in fp32 VALU kernels): the north-star bar, 1e-4 max-norm relative per
tensor, cancellation-aware as in test_gpu_parity.py. bf16 (tower conv2 on bf16 MFMA,
fp32 accumulate): the documented bf16 tolerance of test_gpu_parity.py (losses 2e-3,
distance 2e-2, gradients 5e-2)."""
import numpy as np
import pytest
import torch

from magic_amd.config import MVAEConfig, preset
from oracle import mvae_oracle as O
from tests.gpu_helpers import gpu_phases, make_inputs, make_params, oracle_cfg, to_dev
from tests.test_gpu_parity import FLAVOURS, _engine, check_step

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def tiny_conv(act, metric, recip, w, **kw):
    base = dict(image_size=12, batch=6, enc=(40, 24), dec=(28, 20), latent=6, act=act,
                metric=metric, reciprocal=recip, deform_weight=w, lr=(1e-3, 1e-4), conv=True)
    base.update(kw)
    return MVAEConfig(**base)


@pytest.mark.parametrize("flav", FLAVOURS)
def test_conv_step_f32(flav):
    check_step(tiny_conv(*flav), density=0.3)


@pytest.mark.parametrize("S,B", [(20, 4), (16, 9)])
def test_conv_step_f32_sizes(S, B):
    check_step(tiny_conv("tanh", "sqdiff", True, 10.0, image_size=S, batch=B), density=0.3)


def test_conv_step_f32x():
    check_step(tiny_conv("tanh", "cosine", False, 10.0, image_size=20, batch=4, precision="f32x"),
               density=0.3)


@pytest.mark.parametrize("S,B", [(12, 6), (20, 4), (100, 2)])
def test_conv_step_bf16_mfma(S, B):
    """conv2 forward / data gradient / weight gradient on the bf16 MFMA kernels (each kernel is
    exact to 2e-6 given bf16-rounded operands: test_conv2_kernel). The metric gradient of the
    conv2 layer sums lock and key contributions of opposite sign (squared difference), so
    at a few tiny images its bf16 error relative to the cancelled value reaches ~0.1: its W
    and b are held to 0.15 there, everything else to the documented 5e-2."""
    cfg = tiny_conv("tanh", "sqdiff", True, 10.0, image_size=S, batch=B, precision="bf16",
                    enc=(500, 64) if S == 100 else (40, 24))
    check_step(cfg, density=0.3, tol=5e-2, loss_tol=2e-3, dist_tol=2e-2, adam=False,
               g2_tol={"enc_conv2_W": 0.15, "enc_conv2_b": 0.15} if S < 100 else None)


def test_conv_full_image_f32():
    """100x100 images (the benched geometry: 50x50x64 after pool 1, 40000 features)."""
    check_step(tiny_conv("tanh", "sqdiff", True, 10.0, image_size=100, batch=2, enc=(64,)),
               density=0.3, adam=False)


def test_conv_step_deterministic():
    cfg = tiny_conv("tanh", "cosine", False, 10.0, image_size=20, batch=8, precision="bf16")
    out = []
    for _ in range(2):
        eng = _engine(cfg)
        try:
            eng.load_params(make_params(cfg))
            X, areas, eps = make_inputs(cfg, cfg.batch, density=0.3)
            _, _, g1, g2 = gpu_phases(eng, X, areas, eps)
            out.append((g1, g2))
        finally:
            eng.close()
    for k in out[0][0]:
        np.testing.assert_array_equal(out[0][0][k], out[1][0][k], err_msg=k)


def test_conv_transform_matches_oracle():
    cfg = tiny_conv("elu", "cosine", False, 100.0, image_size=16, batch=5)
    eng = _engine(cfg)
    try:
        P = make_params(cfg)
        eng.load_params(P)
        X, _, _ = make_inputs(cfg, cfg.batch, density=0.3)
        mu = eng.transform(to_dev(X)).cpu().numpy()
        oc = oracle_cfg(cfg)
        _, mu_o, _, _ = O.encode({k: v.astype(np.float64) for k, v in P.items()},
                                 X[:, 0::3].astype(np.float64), oc)
        assert np.abs(mu - mu_o).max() <= 1e-4 * np.abs(mu_o).max()
        names = list(eng.params())
        assert names[:4] == ["enc_conv1_W", "enc_conv1_b", "enc_conv2_W", "enc_conv2_b"]
        assert tuple(eng.params()["enc_conv2_W"].shape) == (1600, 64)
    finally:
        eng.close()


def test_conv_c5conv_preset_runs():
    """The benched configuration's shape (C5CONV: 8e encoder, L=2000, conv tower) at a batch
    the oracle handles: bf16 tolerance."""
    cfg = preset("8e", image_size=100, batch=4, metric="sqdiff", reciprocal=True,
                 precision="bf16", conv=True)
    check_step(cfg, density=0.1, tol=5e-2, loss_tol=2e-3, dist_tol=2e-2, adam=False)


# ------------------------------------------------------------------ conv2 kernels in isolation
def _bf16(a):
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32)


def _conv2_ref(mode, x, y, S1, B):
    """float64 restatement with the kernel's operand rounding already applied to x, y. The im2col
    matrix is built one image at a time (S1 = 50 is 32 MB per image), summed in float64."""
    from oracle import conv_oracle as CV
    x = x.astype(np.float64).reshape(-1, S1, S1, 64)
    y = y.astype(np.float64)
    if mode in (0, 1):
        y = y.reshape(1601, 64)
        W, b = (y[:1600], y[1600]) if mode == 0 else (CV.rot_weights(y[:1600], 64), 0.0)
        out, mag = np.empty_like(x), np.empty_like(x)
        for i in range(x.shape[0]):
            cols = CV.im2col(x[i:i + 1])
            out[i] = cols @ W + b
            mag[i] = np.abs(cols) @ np.abs(W)
        return (np.maximum(out, 0) if mode == 0 else out), mag
    d = y.reshape(-1, S1, S1, 64)
    out, mag = np.zeros((2, 1601, 64)), np.zeros((2, 1601, 64))
    for g in range(2):
        for r in range(2 * B):
            j = 2 * B * g + r
            cols = CV.im2col(x[j if j < 2 * B else j - B][None]).reshape(-1, 1600)
            dd = d[j].reshape(-1, 64)
            out[g, :1600] += cols.T @ dd
            out[g, 1600] += dd.sum(0)
            mag[g, :1600] += np.abs(cols).T @ np.abs(dd)
            mag[g, 1600] += np.abs(dd).sum(0)
    return out, mag


def _conv2_case(mode, mfma, S1, B, chunks=0, repeat=1):
    """One mvae_debug_conv2 case against _conv2_ref: returns max|error| / max sum|terms|. With
    repeat > 1 the later launches must equal the first bitwise."""
    from magic_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(S1 * 10 + mode)
    img = S1 * S1 * 64
    nx = (3 * B if mode in (0, 2) else 4 * B) * img
    x = np.maximum(rng.standard_normal(nx), -0.2).astype(np.float32)   # relu-ish, with zeros
    if mode == 2:
        y = (rng.standard_normal(4 * B * img) * (rng.random(4 * B * img) < 0.3)).astype(np.float32)
        nout = 2 * 1601 * 64
    else:
        y = (rng.standard_normal(1601 * 64) * 0.05).astype(np.float32)
        nout = (3 * B if mode == 0 else 4 * B) * img
    xd, yd = to_dev(x), to_dev(y)
    outs = []
    for _ in range(repeat):
        out = torch.zeros(nout, device="cuda")
        rc = lib.mvae_debug_conv2(S1, B, mode, mfma | (chunks << 8), xd.data_ptr(), yd.data_ptr(),
                                  out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.mvae_last_error(None)
        outs.append(out.cpu().numpy())
    for o in outs[1:]:
        np.testing.assert_array_equal(o.view(np.uint32), outs[0].view(np.uint32))
    xr, yr = (_bf16(x), _bf16(y)) if mfma else (x, y)
    if mfma and mode != 2:
        yr = np.concatenate([_bf16(y[:1600 * 64]), y[1600 * 64:]])   # the bias stays fp32
    ref, mag = _conv2_ref(mode, xr, yr, S1, B)
    got = outs[0].astype(np.float64).reshape(ref.shape)
    err = np.abs(got - ref).max() / max(np.abs(mag).max(), 1e-30)
    print(f"conv2 mode={mode} mfma={mfma} S1={S1} B={B} chunks={chunks}: err/mag={err:.3e}")
    return err


@pytest.mark.parametrize("mfma", [0, 1], ids=["valu_f32", "mfma_bf16"])
@pytest.mark.parametrize("mode", [0, 1, 2], ids=["fwd", "dgrad", "wgrad"])
@pytest.mark.parametrize("S1,B", [(6, 2), (10, 3), (50, 1)])
def test_conv2_kernel(mode, mfma, S1, B):
    err = _conv2_case(mode, mfma, S1, B)
    assert err <= 2e-6, err


@pytest.mark.parametrize("mfma", [0, 1], ids=["valu_f32", "mfma_bf16"])
@pytest.mark.parametrize("mode", [0, 1, 2], ids=["fwd", "dgrad", "wgrad"])
@pytest.mark.parametrize("S1,B", [(2, 2), (4, 3), (18, 1), (24, 1), (40, 1), (48, 1)])
def test_conv2_kernel_ragged_and_tiny(mode, mfma, S1, B):
    """Sizes whose row bands do not divide the image, and the two smallest legal images. From the
    launchers: channel-half forward / data gradient bands hbr = min(S1, 512 // S1), weight
    gradient row blocks R = min(S1, 256 // S1), fp32 VALU kernels 8 x 8 tiles.

      S1   hbr bands      R row blocks    8 x 8 tiles
       2   2 (whole)      2 (whole)       1, 2 of 8 rows / columns used; image < the 5 x 5 kernel, S2 = 1
       4   4 (whole)      4 (whole)       1, 4 of 8 used; image < the 5 x 5 kernel
      18   18 (whole)     14 + 4          3 x 3, edge tiles 2 wide
      24   21 + 3         10 + 10 + 4     3 x 3, full
      40   3 x 12 + 4     6 x 6 + 4       5 x 5, full
      48   4 x 10 + 8     9 x 5 + 3       6 x 6, full
    """
    err = _conv2_case(mode, mfma, S1, B)
    assert err <= 2e-6, err


@pytest.mark.parametrize("mfma", [0, 1], ids=["valu_f32", "mfma_bf16"])
@pytest.mark.parametrize("S1,B,chunks", [(18, 3, 2), (18, 3, 4), (50, 2, 3), (6, 5, 4)])
def test_conv2_wgrad_chunk_loop(mfma, S1, B, chunks):
    """Several images per weight-gradient chunk (mvae_debug_conv2 bits 8-19), ipc = ceil(2B / chunks);
    image j of a chunk, row block b: the kernels' j0 + b / nrb, (b % nrb) * R walk.
      (18, 3, 2): ipc 3, two ragged row blocks (14 + 4) per image;
      (18, 3, 4): ipc 2, chunks of 2, 2, 2 images and one empty chunk;
      (50, 2, 3): ipc 2 with 10 row blocks per image (the benchmark's loop shape: 20 row blocks per
                  chunk, the prefetch crossing the image boundary), chunks of 2, 2, 0 images;
      (6, 5, 4):  ipc 3, chunks of 3, 3, 3 and a last one of a single image.
    The debug entry prefills the slab with NaN bits, so an empty chunk must write its zeros. Two
    launches are bitwise equal (slabs are reduced in a fixed order)."""
    err = _conv2_case(2, mfma, S1, B, chunks=chunks, repeat=2)
    assert err <= 2e-6, err


@pytest.mark.parametrize("mfma,S1,B", [(0, 6, 17), (1, 6, 33)], ids=["valu_f32", "mfma_bf16"])
def test_conv2_wgrad_default_chunks_ipc2(mfma, S1, B):
    """The step's own chunk counts past their caps: VALU nchunk2 = 32 at B = 17 (ipc 2, 17 chunks of
    two images, 15 empty), MFMA nchunk2m = 64 at B = 33 (33 chunks of two, 31 empty)."""
    err = _conv2_case(2, mfma, S1, B, repeat=2)
    assert err <= 2e-6, err


# ------------------------------------------------------------------ whole steps at the new shapes
@pytest.mark.parametrize("S", [4, 8, 36])
def test_conv_step_f32_small_and_ragged(S):
    """The smallest legal images (S1 = 2, 4: smaller than the 5 x 5 kernel; S2 = 1 at S = 4) and a
    ragged one (S1 = 18) through a whole f32 step."""
    check_step(tiny_conv("tanh", "sqdiff", True, 10.0, image_size=S, batch=3), density=0.3)


def test_conv_step_f32_two_images_per_chunk():
    """B = 17: the VALU weight gradient's nchunk2 = 32 < 2B, two images per chunk inside a step."""
    check_step(tiny_conv("tanh", "sqdiff", True, 10.0, image_size=12, batch=17), density=0.3)


@pytest.mark.parametrize("options", ["conv2_nchunk=2"])
def test_conv_step_bf16_options(options):
    """bf16 at S1 = 18 (ragged weight-gradient row blocks) with three images per chunk (create option
    conv2_nchunk=2): the tolerances of test_conv_step_bf16_mfma."""
    cfg = tiny_conv("tanh", "sqdiff", True, 10.0, image_size=36, batch=3, precision="bf16", options=options)
    check_step(cfg, density=0.3, tol=5e-2, loss_tol=2e-3, dist_tol=2e-2, adam=False,
               g2_tol={"enc_conv2_W": 0.15, "enc_conv2_b": 0.15})

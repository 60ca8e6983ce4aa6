"""``mvae_embed_images``: any number of single images of one uint8 table encoded to their latent
mean / log-sigma. The direct kernel's bit buffers against the step's de-interleave of a host-built
X (bitwise), the embeddings against the float64 oracle, the lock-block rows against
``transform_pairs`` (bitwise), ragged counts, the materialising configurations, the absence of side
effects on training, and argument validation."""
import ctypes as C

import numpy as np
import pytest
import torch

from magic_amd import _lib
from magic_amd.config import preset
from oracle import mvae_oracle as O
from tests.gpu_helpers import make_inputs, make_params, max_rel, oracle_cfg, to_dev

pytestmark = pytest.mark.gpu

TOL = {"f32": 1e-4, "f32x": 1e-4, "bf16": 2e-2}  # the project's TOL; the documented bf16 distance tolerance
N_IMG = 5


def table(n, S, kind, seed):
    """n images: ``bin255`` / ``bin1`` values {0, hi} with ~30 % foreground, ``grey`` any byte"""
    rng = np.random.default_rng(seed)
    if kind == "grey":
        return rng.integers(0, 256, (n, S, S)).astype(np.uint8)
    return ((rng.random((n, S, S)) < 0.3) * (255 if kind == "bin255" else 1)).astype(np.uint8)


def draw_idx(count, n, seed):
    """indices with repeats that hold 0 and n - 1"""
    idx = np.random.default_rng(seed).integers(0, n, count).astype(np.int32)
    idx[0], idx[-1] = 0, n - 1
    if count > 2:
        idx[1] = idx[0]
    return idx


# ------------------------------------------------------------------ 1. bit buffers
def debug_bits(mode, T, idx, B, div, no_xbw, x=None):
    """mvae_debug_pairs_bits mode 2 (the embedding kernel, idx [3B] into T) or mode 3 (the step's
    de-interleave of the host's x) on zero-filled buffers -> dict of host tensors"""
    lib = _lib.load()
    S = T.shape[1]
    D = S * S
    ldx, ldbits = D + 8, (D // 8 + 15) // 16 * 16
    ceil = lambda a, b: (a + b - 1) // b  # noqa: E731
    z = lambda n, dt: torch.zeros(n, dtype=dt, device="cuda")  # noqa: E731
    out = dict(xbf=z(ceil(3 * B, 256) * ceil(D + 1, 64) * 512, torch.int32),
               xbw=z(ceil(D + 1, 256) * ceil(3 * B, 64) * 512, torch.int32),
               xbits=z(B * ldbits, torch.uint8), dyn=z(4, torch.int32), plane=z(3 * B * ldx, torch.int16))
    t, i = to_dev(T), to_dev(idx)
    xd = to_dev(x) if x is not None else None
    rc = lib.mvae_debug_pairs_bits(t.data_ptr(), None, i.data_ptr(), None, B, S, float(div), mode, int(no_xbw),
                                   xd.data_ptr() if xd is not None else None, out["xbf"].data_ptr(),
                                   out["xbw"].data_ptr(), out["xbits"].data_ptr(), ldbits, out["dyn"].data_ptr(),
                                   out["plane"].data_ptr(), ldx, torch.cuda.current_stream().cuda_stream)
    _lib.check(lib, None, rc)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def host_x(T, idx, B, div):
    """The pass as X: stacked row c B + b is image idx[c B + b]; blocks 0, 1, 2 are X's channels
    1, 0, 2 (rotated lock, lock, key)."""
    D = T.shape[1] * T.shape[2]
    img = T.reshape(len(T), D)[idx].astype(np.float32) / np.float32(div)  # [3B, D]
    x = np.empty((B, D, 3), np.float32)
    for c, ch in enumerate((1, 0, 2)):
        x[:, :, ch] = img[c * B:(c + 1) * B]
    return x.reshape(B, 3 * D)


BIT_SHAPES = [(64, 8), (64, 12), (64, 16), (128, 20), (192, 20), (320, 12), (64, 100)]


@pytest.mark.parametrize("kind,div", [("bin255", 255.0), ("bin1", 1.0), ("grey", 255.0)])
@pytest.mark.parametrize("B,S", BIT_SHAPES, ids=[f"B{b}_S{s}" for b, s in BIT_SHAPES])
def test_bit_buffers_equal_deint_of_host_x(B, S, kind, div):
    """The embedding kernel (mode 2) writes the BitMats, target bits, flag words and (grey) plane 0
    that the step's de-interleave to bits writes from an X the host builds from the same images."""
    T = table(N_IMG, S, kind, seed=S)
    idx = draw_idx(3 * B, N_IMG, seed=B + S)
    x = host_x(T, idx, B, div)
    for no_xbw in (0, 1):
        ref = debug_bits(3, T, idx, B, div, no_xbw, x=x)
        got = debug_bits(2, T, idx, B, div, no_xbw)
        assert ref["xbf"].any() and ref["xbits"].any()
        assert bool(ref["dyn"][2]) == (kind == "grey")
        assert ref["plane"].any() == (kind == "grey")
        for k in ("xbf", "xbits", "dyn", "plane") + (() if no_xbw else ("xbw",)):
            assert torch.equal(got[k], ref[k]), (k, no_xbw)


# ------------------------------------------------------------------ 2. against the oracle
def engine(cfg, P=None):
    from magic_amd.engine import Engine
    eng = Engine(cfg, 0)
    eng.load_params(P if P is not None else make_params(cfg))
    return eng


def oracle_embed(cfg, P, T, idx=None, div=255.0):
    """float64 mean and log-sigma of the images"""
    x = T.reshape(len(T), -1).astype(np.float64) / div
    if idx is not None:
        x = x[idx]
    P64 = {k: np.asarray(v, np.float64) for k, v in P.items()}
    _, mu, s, _ = O.encode(P64, x, oracle_cfg(cfg))
    return mu, s


def check_oracle(cfg, T, idx, label=""):
    P = make_params(cfg)
    eng = engine(cfg, P)
    try:
        mu, ls = eng.embed(to_dev(T), None if idx is None else to_dev(idx), log_sigma=True)
        torch.cuda.synchronize()
        mu_o, s_o = oracle_embed(cfg, P, T, idx)
        e_mu, e_s = max_rel(mu.cpu().numpy(), mu_o), max_rel(ls.cpu().numpy(), s_o)
        print(f"embed vs oracle {label}{cfg.precision}: mean {e_mu:.3e} log-sigma {e_s:.3e}")
        assert e_mu <= TOL[cfg.precision] and e_s <= TOL[cfg.precision], (e_mu, e_s)
        return mu, ls
    finally:
        eng.close()


@pytest.mark.parametrize("kind", ["bin255", "grey"])
@pytest.mark.parametrize("prec", ["f32", "f32x", "bf16"])
@pytest.mark.parametrize("S", [8, 20])
@pytest.mark.parametrize("name", ["8c", "11a"])
def test_embed_matches_oracle(name, S, prec, kind):
    """Mean and log-sigma of 3B + 5 images (two passes, the second ragged) against O.encode."""
    cfg = preset(name, image_size=S, batch=64, precision=prec)
    T = table(7, S, kind, seed=S + 1)
    check_oracle(cfg, T, draw_idx(3 * 64 + 5, 7, seed=3))


# ------------------------------------------------------------------ 3. lock-block rows
@pytest.mark.parametrize("prec,B", [("bf16", 64), ("f32x", 64), ("f32x", 128)])
def test_lock_block_rows_equal_transform_pairs(prec, B):
    """The images in stacked rows [B, 2B) -- the block mvae_transform copies from -- equal, bit for
    bit, transform_pairs of a PairBatch with those images as locks: the same rows in the same
    place through the same GEMMs."""
    from magic_amd.overlap_input import PairBatch, rotation_coefficients
    S = 20
    cfg = preset("8c", image_size=S, batch=B, precision=prec)
    T = table(N_IMG, S, "bin255", seed=5)
    idx = draw_idx(3 * B, N_IMG, seed=6)
    eng = engine(cfg)
    try:
        eng.timing_enable(True)
        emb = eng.embed(to_dev(T), to_dev(idx)).clone()
        torch.cuda.synchronize()
        # (f32x at 3B < 256 rows runs its layer-0 GEMMs off the plane kernels: no bits, through X)
        assert ("images_bits" in eng.timing_read()) == (prec == "bf16" or B == 128)
        coef = rotation_coefficients(np.linspace(0, 6, B).astype(np.float32), S, S)
        pb = PairBatch(to_dev(T), to_dev(T[::-1].copy()), to_dev(idx[B:2 * B].copy()), to_dev(coef))
        ref = eng.transform(pb)
        torch.cuda.synchronize()
        assert torch.equal(emb[B:2 * B], ref)
    finally:
        eng.close()


# ------------------------------------------------------------------ 4. ragged counts
@pytest.mark.parametrize("with_idx", [False, True], ids=["table_order", "idx"])
def test_ragged_counts(with_idx):
    """Any count: the rows of the full embedding, nothing written past row count - 1."""
    B, S, full = 64, 8, 7 * 64 + 1
    cfg = preset("8c", image_size=S, batch=B, precision="bf16")
    T = table(full, S, "bin255", seed=9)
    idx = draw_idx(full, full, seed=10) if with_idx else None
    eng = engine(cfg)
    try:
        Td = to_dev(T)
        idx_d = to_dev(idx) if with_idx else None
        ref_mu, ref_ls = (t.clone() for t in eng.embed(Td, idx_d, log_sigma=True))
        assert torch.isfinite(ref_mu).all() and ref_mu.abs().max() > 0
        for count in (1, 3 * B - 1, 3 * B, 3 * B + 5, full):
            mu = torch.full((full + 3, cfg.latent), -7.0, device="cuda")
            ls = torch.full((full + 3, cfg.latent), -9.0, device="cuda")
            eng.embed(Td if with_idx else Td[:count], idx_d[:count] if with_idx else None, out=(mu[:count], ls[:count]), log_sigma=True)
            torch.cuda.synchronize()
            assert torch.equal(mu[:count], ref_mu[:count]) and torch.equal(ls[:count], ref_ls[:count]), count
            assert (mu[count:] == -7.0).all() and (ls[count:] == -9.0).all(), count
    finally:
        eng.close()


# ------------------------------------------------------------------ 5. materialising configurations
MATERIALISING = {
    "f32": dict(precision="f32"),
    "conv": dict(conv=True, image_size=8, precision="f32x"),
    "bits0": dict(options="bits=0"),
    "batch16": dict(batch=16),
    "image5": dict(image_size=5),
}


@pytest.mark.parametrize("case", sorted(MATERIALISING))
def test_materialising_configurations(case):
    """Configurations the direct kernel does not serve take the X scratch: against the oracle."""
    kw = dict(image_size=20, batch=64, precision="bf16")
    kw.update(MATERIALISING[case])
    cfg = preset("8c", **kw)
    T = table(7, cfg.image_size, "bin255", seed=11)
    idx = draw_idx(3 * cfg.batch + 5, 7, seed=12)
    P = make_params(cfg)
    eng = engine(cfg, P)
    try:
        eng.timing_enable(True)
        mu, ls = eng.embed(to_dev(T), to_dev(idx), log_sigma=True)
        torch.cuda.synchronize()
        regions = {k: v[1] for k, v in eng.timing_read().items()}
        assert regions.get("images_make_x") == 2 and "images_bits" not in regions, regions
        mu_o, s_o = oracle_embed(cfg, P, T, idx)
        e_mu, e_s = max_rel(mu.cpu().numpy(), mu_o), max_rel(ls.cpu().numpy(), s_o)
        print(f"embed vs oracle {case}: mean {e_mu:.3e} log-sigma {e_s:.3e}")
        assert e_mu <= TOL[cfg.precision] and e_s <= TOL[cfg.precision], (e_mu, e_s)
    finally:
        eng.close()


@pytest.mark.parametrize("prec", ["bf16", "f32x"])
def test_misaligned_table_materialises_the_same_bits(prec):
    """A table view starting 1 byte into its storage takes the X scratch; the aligned table takes
    the direct kernel: the two routes are equal bitwise, and both meet the oracle."""
    B, S, n = 128, 20, 7  # (3B >= 256 rows: the f32x layer-0 GEMMs run the plane kernels, so bits are on)
    cfg = preset("11a", image_size=S, batch=B, precision=prec)
    T = table(n, S, "grey", seed=13)
    idx = draw_idx(3 * B + 5, n, seed=14)
    P = make_params(cfg)
    eng = engine(cfg, P)
    try:
        eng.timing_enable(True)
        buf = torch.zeros(n * S * S + 8, dtype=torch.uint8, device="cuda")
        off = buf[1:1 + n * S * S].view(n, S, S)
        off.copy_(to_dev(T))
        assert off.data_ptr() % 8 == 1
        got = [t.clone() for t in eng.embed(off, to_dev(idx), log_sigma=True)]
        torch.cuda.synchronize()
        r1 = {k: v[1] for k, v in eng.timing_read().items()}
        assert r1.get("images_make_x") == 2 and "images_bits" not in r1, r1
        eng.timing_reset()
        ref = eng.embed(to_dev(T), to_dev(idx), log_sigma=True)
        torch.cuda.synchronize()
        r2 = {k: v[1] for k, v in eng.timing_read().items()}
        assert r2.get("images_bits") == 2 and "images_make_x" not in r2, r2
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
        mu_o, s_o = oracle_embed(cfg, P, T, idx)
        assert max_rel(ref[0].cpu().numpy(), mu_o) <= TOL[prec] and max_rel(ref[1].cpu().numpy(), s_o) <= TOL[prec]
    finally:
        eng.close()


# ------------------------------------------------------------------ 6. no side effects
@pytest.mark.parametrize("prec", ["bf16", "f32x"])
def test_embed_between_steps_changes_nothing(prec):
    """Three training steps (the second batch grey) with embed calls of a grey and a binary table
    between them: losses and final parameters bitwise those of the three steps alone; the RNG
    counters do not move in embed."""
    B, S = 64, 20
    cfg = preset("8c", image_size=S, batch=B, precision=prec)
    P = make_params(cfg)
    steps = [make_inputs(cfg, B, seed=20 + k, density=0.2, grey=(k == 1)) for k in range(3)]
    Tg, Tb = to_dev(table(9, S, "grey", seed=30)), to_dev(table(200, S, "bin255", seed=31))
    res = []
    for with_embed in (False, True):
        eng = engine(cfg, P)
        rec = []
        for k, (X, areas, _) in enumerate(steps):
            losses = torch.zeros(5, device="cuda")
            eng.train_step(to_dev(X), to_dev(areas), None, losses_out=losses)
            rec.append(losses)
            if with_embed:
                rng = eng.get_rng()
                for T in ([Tg], [Tb, Tg], [Tb])[k]:  # one, two (both slot parities), one
                    assert torch.isfinite(eng.embed(T)).all()
                assert eng.get_rng() == rng
        torch.cuda.synchronize()
        res.append((rec, {k: v.clone() for k, v in eng.params().items()}, eng.get_rng()))
        eng.close()
    (rec_a, p_a, rng_a), (rec_b, p_b, rng_b) = res
    assert rng_a == rng_b
    for a, b in zip(rec_a, rec_b):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    for k in p_a:
        assert torch.equal(p_a[k], p_b[k]), k


# ------------------------------------------------------------------ 7. validation
def test_validation():
    cfg = preset("8c", image_size=20, batch=64, precision="bf16")
    eng = engine(cfg)
    try:
        T = to_dev(table(4, 20, "bin255", seed=1))
        out = torch.zeros(4, cfg.latent, device="cuda")

        def call(desc, count=4, mean=out):
            return eng.lib.mvae_embed_images(eng.ctx, desc, count, mean.data_ptr() if mean is not None else None,
                                             None, eng.stream)

        def images(**kw):
            im = _lib.mvae_images()
            im.table, im.height, im.width, im.idx, im.divisor = T.data_ptr(), 20, 20, None, 255.0
            for k, v in kw.items():
                setattr(im, k, v)
            return im

        cases = {
            "null descriptor": lambda: call(None),
            "null table": lambda: call(C.byref(images(table=None))),
            "null output": lambda: call(C.byref(images()), mean=None),
            "count 0": lambda: call(C.byref(images()), count=0),
            "height": lambda: call(C.byref(images(height=21))),
            "width": lambda: call(C.byref(images(width=10))),
            "divisor 0": lambda: call(C.byref(images(divisor=0.0))),
            "divisor < 0": lambda: call(C.byref(images(divisor=-1.0))),
        }
        for name, fn in cases.items():
            rc = fn()
            assert rc == -1, name
            msg = eng.lib.mvae_last_error(eng.ctx).decode()
            assert msg.startswith("mvae_embed_images:"), (name, msg)
        with pytest.raises(ValueError):
            eng.embed(T.float())
        with pytest.raises(ValueError):
            eng.embed(T, torch.zeros(3, dtype=torch.int64, device="cuda"))
        # ... and the engine still embeds
        assert call(C.byref(images())) == 0
        torch.cuda.synchronize()
        assert out.abs().max() > 0
    finally:
        eng.close()

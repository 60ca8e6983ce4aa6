"""The latent head (mvae_kernels.hip: latent_fwd, colstats, metric, loss_reduce, latent_bwd) restated
in float64 numpy, one function per kernel, from the comments above each kernel and
oracle/mvae_oracle.py (forward, metric, loss_sums, backward). tests/test_head_ref.py pins this
restatement to float64 torch autograd and to the oracle; tests/test_gpu_head.py holds the kernels
to it.

Every function takes the kernel's own inputs and returns, next to each output, its magnitude
``mag``: the sum of the absolute values of the terms that are added to form the output, taken down
to the kernel's inputs (a z that the kernel recomputes counts as |mu| + |sigma eps|, not as |z|: its
rounding error is relative to those terms, and an output built from z inherits it). A product of
sums has the product of their mags. The fp32 bar is ``|gpu - ref| <= 2e-6 * mag``.

Where an output is a nonlinear function f of a quantity with magnitude m (the reciprocal distance,
the squared residual), the first-order propagation |f'| * m is used and the rounding of f's own
arithmetic is added, so one relative 2e-6 covers both.

Row blocks are the kernels': ms [3B][2L] = [rot | lock | key] rows of [mu | s]; eps [3][B][L] in the
reference's slot order (lock, rot, key).
"""
from __future__ import annotations

import numpy as np

L2_EPS = 1e-12
EPS_SLOT = (1, 0, 2)   # internal block (rot, lock, key) -> eps slot (lock, rot, key)

f64 = lambda a: np.asarray(a, np.float64)


def reparam(ms, eps, B, L):
    """z, mag, mu, s, sigma, eps per internal block: each [3][B][L]."""
    ms = f64(ms).reshape(3, B, 2 * L)
    eps = f64(eps).reshape(3, B, L)[list(EPS_SLOT)]
    mu, s = ms[:, :, :L], ms[:, :, L:]
    sig = np.sqrt(np.exp(s))
    z = mu + sig * eps
    return dict(z=z, mag=np.abs(mu) + np.abs(sig * eps), mu=mu, s=s, sig=sig, eps=eps)


def latent_fwd(ms, eps, B, L):
    """z [3][B][L] (rot, lock, key) and rowfwd [B][3] = {sum 1 + s - mu^2 - exp s (lock), sum (z_lock -
    z_rot)^2, sum (z_lock - z_key)^2}, each with its mag."""
    r = reparam(ms, eps, B, L)
    z, zm, mu, s = r["z"], r["mag"], r["mu"][1], r["s"][1]
    kl = 1 + s - mu ** 2 - np.exp(s)
    kl_mag = np.abs(1 + s) + mu ** 2 + np.exp(s)
    fd, sq = (z[1] - z[0]) ** 2, (z[1] - z[2]) ** 2
    fd_mag, sq_mag = (zm[1] + zm[0]) ** 2, (zm[1] + zm[2]) ** 2
    row = np.stack([kl.sum(1), fd.sum(1), sq.sum(1)], 1)
    row_mag = np.stack([kl_mag.sum(1), fd_mag.sum(1), sq_mag.sum(1)], 1)
    return dict(z=z, z_mag=zm, rowfwd=row, rowfwd_mag=row_mag, kl=kl, kl_mag=kl_mag)


def chunk_rows(B, rows=128):
    return [(r0, min(r0 + rows, B)) for r0 in range(0, B, rows)]


def colsq(zl, zk):
    """column sums of squares [2L] of the lock | key rows ([B][L] each, the kernel's fp32 z); all terms
    are positive, so mag = value. Also the 128-row chunk partials [nchunk][2L]."""
    sq = np.concatenate([f64(zl) ** 2, f64(zk) ** 2], 1)
    part = np.stack([sq[a:b].sum(0) for a, b in chunk_rows(sq.shape[0])])
    return dict(out=sq.sum(0), mag=sq.sum(0), part=part, part_mag=part)


def norms(cs, L):
    """r_lock, r_key = 1 / sqrt(max(colsq, eps)) and the gradient masks colsq >= eps"""
    cs = f64(cs)
    r = 1.0 / np.sqrt(np.maximum(cs, L2_EPS))
    m = (cs >= L2_EPS).astype(np.float64)
    return r[:L], r[L:], m[:L], m[L:]


def coldot(zl, zk, cs, draw):
    """out [L] = sum_b draw_b n_lock n_key from the given colsq [2L]"""
    zl, zk, draw = f64(zl), f64(zk), f64(draw)
    rl, rk, _, _ = norms(cs, zl.shape[1])
    t = draw[:, None] * (zl * rl) * (zk * rk)
    ch = chunk_rows(zl.shape[0])
    return dict(out=t.sum(0), mag=np.abs(t).sum(0), part=np.stack([t[a:b].sum(0) for a, b in ch]),
                part_mag=np.stack([np.abs(t[a:b]).sum(0) for a, b in ch]))


def metric(zl, zk, rowfwd, rowpart, areas, cs, metric, recip, w, Bg):
    """rowvals [B][4] = {R, K, F, T}, dist [B], draw [B] with mags; raw / raw_mag the distance before the
    reciprocal. metric: 0 cosine, 1 squared difference (rowfwd[:, 2], taken as given). areas None: 0."""
    zl, zk, rowfwd = f64(zl), f64(zk), f64(rowfwd)
    B, L = zl.shape
    inv = 1.0 / Bg
    a = np.zeros(B) if areas is None else f64(areas)
    if metric == 0:
        rl, rk, _, _ = norms(cs, L)
        t = (zl * rl) * (zk * rk)
        raw, raw_mag = t.sum(1), np.abs(t).sum(1)
    else:
        raw = rowfwd[:, 2].copy()
        raw_mag = np.abs(raw)
    if recip:
        dist = 1.0 / raw
        dist_mag = raw_mag / raw ** 2          # |d(1/raw)| = |d raw| / raw^2; covers the division's rounding
    else:
        dist, dist_mag = raw, raw_mag
    res = dist - a
    res_mag = dist_mag + np.abs(a)
    T = res ** 2
    T_mag = 2 * np.abs(res) * res_mag + res ** 2 + 2e-6 * res_mag ** 2   # (the last: second order, res ~ 0)
    g = 2.0 * res * inv
    g_mag = 2.0 * res_mag * inv
    if recip:
        draw = -g * dist * dist                # tf.reciprocal grad: -dy * y^2
        draw_mag = g_mag * dist ** 2 + 2 * np.abs(g * dist) * dist_mag + np.abs(draw)
    else:
        draw, draw_mag = g, g_mag
    rp = f64(rowpart).reshape(B, -1)
    rowvals = np.stack([rp.sum(1), -0.5 * rowfwd[:, 0], w * rowfwd[:, 1], T], 1)
    rowvals_mag = np.stack([np.abs(rp).sum(1), np.abs(0.5 * rowfwd[:, 0]), np.abs(w * rowfwd[:, 1]), T_mag], 1)
    return dict(rowvals=rowvals, rowvals_mag=rowvals_mag, dist=dist, dist_mag=dist_mag, draw=draw,
                draw_mag=draw_mag, raw=raw, raw_mag=raw_mag)


def loss_reduce(rowvals, Bg):
    """losses[5] = {cost, training_loss, r_l, l_l, d_l} and mag = inv_bg sum |rowvals|"""
    rv = f64(rowvals)
    s, m = rv.sum(0) / Bg, np.abs(rv).sum(0) / Bg
    return dict(losses=np.array([s[0] + s[1] + s[2], s[3], s[0], s[1], s[2]]),
                mag=np.array([m[0] + m[1] + m[2], m[3], m[0], m[1], m[2]]))


def latent_bwd(ms, eps, dzdec, draw, cs, cd, B, L, metric, w, Bg):
    """dhead [4][B][2L]: rows [rot g1 | lock g1 | lock g2 | key g2], columns [dmu | ds], and its mag. The
    cosine's colsq [2L] and coldot [L] are taken as given (cs, cd)."""
    r = reparam(ms, eps, B, L)
    z, zm, mu, s, sig, e = r["z"], r["mag"], r["mu"], r["s"], r["sig"], r["eps"]
    inv = 1.0 / Bg
    dd, dr = f64(dzdec).reshape(B, L), f64(draw).reshape(B, 1)
    de = 2.0 * w * (z[1] - z[0]) * inv
    de_mag = 2.0 * abs(w) * (zm[1] + zm[0]) * inv
    dz1, dz1_mag = dd + de, np.abs(dd) + de_mag
    if metric == 1:
        dz2 = 2.0 * dr * (z[1] - z[2])
        dz3 = -dz2
        dz2_mag = dz3_mag = 2.0 * np.abs(dr) * (zm[1] + zm[2])
    else:
        rl, rk, ml, mk = norms(cs, L)
        c = f64(cd)
        nl, nk, nl_mag, nk_mag = z[1] * rl, z[2] * rk, zm[1] * rl, zm[2] * rk
        dz2 = rl * (dr * nk - nl * c * ml)
        dz3 = rk * (dr * nl - nk * c * mk)
        dz2_mag = rl * (np.abs(dr) * nk_mag + nl_mag * np.abs(c) * ml)
        dz3_mag = rk * (np.abs(dr) * nl_mag + nk_mag * np.abs(c) * mk)
    # the same two magnitudes with |z| for mag(z): NOT a bound (z is recomputed in fp32 and its error
    # is relative to |mu| + |sigma eps|, so where z cancels they fall below it); test_gpu_head.py
    # prints the kernels' ratio under them next to the asserted one
    za = np.abs(z)
    if metric == 1:
        lit2 = lit3 = 2.0 * np.abs(dr) * (za[1] + za[2])
    else:
        lit2 = rl * (np.abs(dr) * za[2] * rk + za[1] * rl * np.abs(c) * ml)
        lit3 = rk * (np.abs(dr) * za[1] * rl + za[2] * rk * np.abs(c) * mk)
    lit = [np.concatenate([a, 0.5 * a * np.abs(e[k]) * sig[k]], 1) for a, k in ((lit2, 1), (lit3, 2))]
    ex = np.exp(s[1])
    dmu = [-de, dz1 + mu[1] * inv, dz2, dz3]
    dmu_mag = [de_mag, dz1_mag + np.abs(mu[1]) * inv, dz2_mag, dz3_mag]
    ds = [-0.5 * de * e[0] * sig[0], 0.5 * dz1 * e[1] * sig[1] + 0.5 * (ex - 1) * inv,
          0.5 * dz2 * e[1] * sig[1], 0.5 * dz3 * e[2] * sig[2]]
    ds_mag = [0.5 * de_mag * np.abs(e[0]) * sig[0], 0.5 * dz1_mag * np.abs(e[1]) * sig[1] + 0.5 * (ex + 1) * inv,
              0.5 * dz2_mag * np.abs(e[1]) * sig[1], 0.5 * dz3_mag * np.abs(e[2]) * sig[2]]
    out = np.stack([np.concatenate([a, b], 1) for a, b in zip(dmu, ds)])
    mag = np.stack([np.concatenate([a, b], 1) for a, b in zip(dmu_mag, ds_mag)])
    return dict(dhead=out, mag=mag, z=z, z_mag=zm, g2_mag_abs_z=np.stack(lit))


# ------------------------------------------------------------------------- bf16 planes
def bf16_bits(a):
    """round-to-nearest-even bf16 bit patterns of an fp32 array"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def planes(a, n):
    """the n bf16 planes of the exact split of fp32 a: plane t = bf16(a - plane 0 - .. - plane t-1),
    every residual an exact fp32 difference"""
    r = np.ascontiguousarray(a, np.float32).copy()
    out = []
    for _ in range(n):
        b = bf16_bits(r)
        out.append(b)
        r = r - (b.astype(np.uint32) << 16).view(np.float32)
    return np.stack(out) if out else np.zeros((0,) + r.shape, np.uint16)

"""The internal N(0,1) sampler of the HIP step restated in numpy: Philox4x32-10 (Salmon,
Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) + Box-Muller.

Written from the generator's definition: one round multiplies counter words 0 and 2 by the
two round constants, and the new counter is (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0); the key
words are bumped by the Weyl constants between rounds; ten rounds.

``eps_reference`` is the eps tensor ``[3, B, L]`` (lock, rotated lock, key) the library draws
for call ``counter`` when the caller passes no eps (``mvae_forward(..., eps = NULL)``):

  global element of (slot s, row b, column i)   g = (s * Bg + off + b) * L + i
  Philox block / lane                           q = g >> 2, g & 3
  counter words                                 (q lo, q hi, counter lo, counter hi)
  key words                                     (seed lo, seed hi)
  uniforms                                      u = (float32(word) + 0.5f) * 2^-32, in float32
  lanes 0, 1                                    sqrt(-2 ln u(w0)) * (cos, sin)(2 pi u(w1))
  lanes 2, 3                                    the same of words 2, 3

The uniforms are formed in float32 exactly as the kernel forms them (so a word that rounds to
u = 1.0 gives radius 0 here too); the logarithm, square root and sine / cosine are float64, so
the only difference to the kernel is the error of its hardware transcendentals.
"""
from __future__ import annotations

import numpy as np

M0 = np.uint64(0xD2511F53)   # multiplier of counter word 0
M1 = np.uint64(0xCD9E8D57)   # multiplier of counter word 2
W0 = np.uint64(0x9E3779B9)   # key word 0 increment (golden ratio)
W1 = np.uint64(0xBB67AE85)   # key word 1 increment (sqrt(3) - 1)
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)

EVAL_STREAM = 1 << 63  # inference draws (predict / reconstruct): bit 63 of the call counter


def philox4x32_10(counter4, key2):
    """Philox4x32-10. counter4: four arrays (or scalars) of 32-bit words, key2: two; any integer
    type, broadcast against each other. Returns four uint64 arrays holding 32-bit words."""
    c = [np.asarray(w, dtype=np.uint64) & MASK for w in counter4]
    k = [np.asarray(w, dtype=np.uint64) & MASK for w in key2]
    shape = np.broadcast(*c, *k).shape
    c = [np.broadcast_to(w, shape).copy() for w in c]
    k = [np.broadcast_to(w, shape).copy() for w in k]
    for _ in range(10):
        p0 = M0 * c[0]  # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = M1 * c[2]
        c = [(p1 >> S32) ^ c[1] ^ k[0], p1 & MASK, (p0 >> S32) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + W0) & MASK, (k[1] + W1) & MASK]
    return c


def uniform_f32(word):
    """(float32(word) + 0.5f) * 2^-32 with every step rounded to float32: in (0, 1]."""
    f = np.asarray(word, dtype=np.uint64).astype(np.float32)  # round to nearest even, as v_cvt_f32_u32
    return (f + np.float32(0.5)) * np.float32(2.0 ** -32)


def normals_of_blocks(q, seed: int, counter: int):
    """float64 [..., 4]: the four normals of Philox blocks ``q`` of call ``counter``."""
    q = np.asarray(q, dtype=np.uint64)
    seed, counter = int(seed), int(counter)
    w = philox4x32_10((q & MASK, q >> S32, counter & 0xFFFFFFFF, counter >> 32),
                      (seed & 0xFFFFFFFF, seed >> 32))
    out = np.empty(q.shape + (4,), np.float64)
    for j in range(2):
        u1 = uniform_f32(w[2 * j]).astype(np.float64)
        u2 = uniform_f32(w[2 * j + 1]).astype(np.float64)
        rad = np.sqrt(-2.0 * np.log(u1))
        out[..., 2 * j] = rad * np.cos(2.0 * np.pi * u2)
        out[..., 2 * j + 1] = rad * np.sin(2.0 * np.pi * u2)
    return out


def eps_reference(seed: int, counter: int, Bg: int, L: int, off: int = 0, B: int | None = None):
    """float64 [3, B, L]: rows off .. off + B - 1 of the eps of call ``counter`` for a global
    batch of ``Bg`` rows (B None: all of them)."""
    B = Bg - off if B is None else B
    s = np.arange(3, dtype=np.uint64)[:, None, None]
    b = np.arange(B, dtype=np.uint64)[None, :, None]
    i = np.arange(L, dtype=np.uint64)[None, None, :]
    g = (s * np.uint64(Bg) + np.uint64(off) + b) * np.uint64(L) + i
    q, inv = np.unique(g >> np.uint64(2), return_inverse=True)
    n = normals_of_blocks(q, seed, counter)
    return n[inv.reshape(g.shape), (g & np.uint64(3)).astype(np.int64)]

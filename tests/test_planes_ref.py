"""tests/planes_ref.py (and the split it rests on, tests/epi_ref.py split_planes) against values written
out by hand: the exact three-plane split of the pixel values, round-to-nearest-even at the ties, the form
launch_deinterleave picks at the shapes tests/test_gpu_input_planes.py runs, and what each route writes
for the smallest batches of each kind."""
import numpy as np

from tests import planes_ref as P
from tests.epi_ref import split_planes


def f32(bits):
    return np.array(bits, np.uint32).view(np.float32)


def value(planes):
    """the float64 sum of bf16 planes [n][...]"""
    return sum((p.astype(np.uint32) << 16).view(np.float32).astype(np.float64) for p in planes)


# fp32 bits -> the three planes. u = 2^-23. 0x3F80xxxx is 1 + xxxx u with bf16 ulp 2^16 u:
#  low half 0x7FFF rounds down, remainder (2^15 - 1) u -> plane 1 = 2^-8 (eight ones round up), plane 2 = -u
#  low half 0x8000 is the tie: down under an even bit 16 (remainder 2^-8), up under an odd one (-2^-8)
#  low half 0x8001 rounds up, remainder -(2^15 - 1) u -> plane 1 = -2^-8, plane 2 = +u
# 0x3FFF8000 ties upward into the next binade (2.0). The negative values mirror the positive ones.
TIES = {0x3F807FFF: (0x3F80, 0x3B80, 0xB400), 0x3F808000: (0x3F80, 0x3B80, 0x0000),
        0x3F808001: (0x3F81, 0xBB80, 0x3400), 0x3F817FFF: (0x3F81, 0x3B80, 0xB400),
        0x3F818000: (0x3F82, 0xBB80, 0x0000), 0x3F818001: (0x3F82, 0xBB80, 0x3400),
        0x3FFF8000: (0x4000, 0xBB80, 0x0000),
        0xBF807FFF: (0xBF80, 0xBB80, 0x3400), 0xBF808000: (0xBF80, 0xBB80, 0x0000),
        0xBF808001: (0xBF81, 0x3B80, 0xB400), 0xBF817FFF: (0xBF81, 0xBB80, 0x3400),
        0xBF818000: (0xBF82, 0x3B80, 0x0000), 0xBF818001: (0xBF82, 0x3B80, 0xB400),
        0xBFFF8000: (0xC000, 0x3B80, 0x0000)}


def test_pixel_values_split_exactly():
    k = np.arange(256, dtype=np.float32)
    for div in (255.0, 1.0):
        v = k / np.float32(div)
        s = split_planes(v, 3)
        assert np.array_equal(value(s), v.astype(np.float64)), div
    s = split_planes(k / np.float32(255.0), 3)
    assert int((s[2] != 0).sum()) == 254 and not s[2][0] and not s[2][255]   # 0 and 1 alone stop early
    assert int((s[1] != 0).sum()) == 254
    assert not split_planes(k, 3)[1:].any()                                   # a byte is a bf16 value


def test_ties_round_to_even_as_written_by_hand():
    bits = list(TIES)
    s = split_planes(f32(bits), 3)
    assert s.T.tolist() == [list(TIES[b]) for b in bits]
    assert {b & 0xFFFF for b in bits} == {0x7FFF, 0x8000, 0x8001} and {b >> 16 & 1 for b in bits} == {0, 1}
    assert np.array_equal(value(s), f32(bits).astype(np.float64))
    # the residual of each value, split on its own: the same planes 1 and 2, then nothing left
    r1 = (f32(bits).astype(np.float64) - value(s[:1])).astype(np.float32)
    assert np.array_equal(r1.astype(np.float64), f32(bits).astype(np.float64) - value(s[:1]))
    again = split_planes(r1, 3)
    assert np.array_equal(again[:2], s[1:]) and not again[2].any()


def test_form_chooser_at_the_pinned_shapes():
    for D in (8, 64, 2304, 8072):
        assert P.form(D, D, True) == P.form(D, D + 8, True) == P.OCT
    for D in (4, 100, 1028):
        assert P.form(D, D, True) == P.form(D, D + 4, True) == P.QUAD
    assert P.form(64, 68, True) == P.QUAD          # ldx = D + 4
    for D in (1, 25, 259):
        assert P.form(D, D, True) == P.form(D, (D + 7) // 8 * 8, True) == P.SCALAR
    assert P.form(64, 64, False) == P.SCALAR       # x one float past a 16-byte boundary
    assert P.form(64, 65, True) == P.SCALAR        # ldx = D + 1
    assert P.form(100, 104, False) == P.SCALAR


def _x(B, D, rows):
    """X [B][3 D] from stacked rows [3B][D] (rot | lock | key)"""
    R = np.asarray(rows, np.float32).reshape(3, B, D)
    return np.stack([R[1], R[0], R[2]], axis=2).reshape(B, 3 * D)


def test_route0_writes_what_the_header_says():
    B, D, ldx = 1, 8, 16
    exact = _x(B, D, [[0, 1, 0, 0, 1, 1, 0, 0], [1, 0, 0, 0, 0, 0, 0, 1], [0.5, 0, 0, 0, 0, 0, 0, 0]])
    r = P.route0(exact, B, D, ldx, 2, 3, 0, 2, 0)
    assert r["form"] == P.OCT and r["dyn"].tolist() == [0, 0, 1, 0]
    assert r["planes"][1][0, :, :D].all() and not r["planes"][1][0, :, D:].any() and not r["planes"][1][1:].any()
    assert not r["xs"][1].any()                                       # the target rows only with the flag
    assert r["xbits"][0].tolist() == [[0x81, 0]] and r["xbits"][1].tolist() == [[True, False]]
    assert r["planes"][0][0, 2, 0] == 0x3F00
    grey = exact.copy()
    grey[0, 3 * 7 + 2] = np.float32(7) / np.float32(255)              # the key's last pixel
    r = P.route0(grey, B, D, ldx, 2, 3, 0, 2, 1)
    assert r["dyn"].tolist() == [0, 1, 0, 1]
    assert r["planes"][1][:, :, :D].all() and not r["planes"][1][:, :, D:].any()
    assert r["xs"][1].tolist() == [[False] * 16, [True] * 8 + [False] * 8, [False] * 16]
    assert r["planes"][0][1:, :2].any() == 0 and r["planes"][0][1, 2, 7] != 0 and r["planes"][0][2, 2, 7] != 0
    # one plane: the flag still rises, no residual plane; f32mask rows always; no plane image: no flag
    r = P.route0(grey, B, D, ldx, 2, 1, 2, 0, 0)
    assert r["dyn"].tolist() == [1, 0, 1, 0] and r["planes"][1].sum() == 3 * D and r["xs"][1][1, :D].all()
    r = P.route0(grey, B, D, ldx, 2, 0, 7, 0, 0)
    assert r["dyn"].tolist() == [0, 0, 1, 0] and not r["planes"][1].any() and r["xs"][1][:, :D].all()
    # the other forms: no bits, the not-binary word raised for a 0/1 batch too
    binary = _x(B, D, [[0, 1, 0, 0, 1, 1, 0, 0], [1, 0, 0, 0, 0, 0, 0, 1], [1, 0, 0, 0, 0, 0, 0, 0]])
    for kw, f in ((dict(x_aligned=False), P.SCALAR), (dict(), P.OCT)):
        r = P.route0(binary, B, D, ldx, 2, 3, 0, 2, 0, **kw)
        assert r["form"] == f and r["dyn"].tolist() == [0, 0, int(f != P.OCT), 0]
        assert r["xbits"][1].any() == (f == P.OCT)
    assert P.route0(binary, B, D, 12, 2, 3, 0, 2, 0)["form"] == P.QUAD


def test_bits_routes_write_planes_for_grey_batches_only():
    B, D, ldx = 1, 8, 16
    binary = _x(B, D, [[0, 1, 0, 0, 1, 1, 0, 0], [1, 0, 0, 0, 0, 0, 0, 1], [1, 0, 0, 0, 0, 0, 0, 0]])
    r = P.bits_route(binary, B, D, ldx, 2, 3, 2, 0)
    assert r["dyn"].tolist() == [0, 0, 0, 0] and not r["planes"][1].any() and not r["xs"][1].any()
    assert r["xbits"][1].tolist() == [[True, False]]
    half = binary.copy()
    half[0, 2] = 0.5                                                  # exact, not 0 / 1
    r = P.bits_route(half, B, D, ldx, 2, 3, 2, 1)
    assert r["dyn"].tolist() == [0, 0, 0, 1] and r["planes"][1][:, :, :D].all() and not r["planes"][0][1:].any()
    assert r["xs"][1][1, :D].all() and r["xs"][1].sum() == D
    half[0, 2] = np.float32(1) / np.float32(255)
    r = P.bits_route(half, B, D, ldx, 2, 1, 0, 0)
    assert r["dyn"].tolist() == [1, 0, 1, 0] and r["planes"][1].sum() == 3 * D and not r["xs"][1].any()

"""The restatement ``tests/rerank_ref.py`` against literal loops on 6 x 6 images: the area and pose of
every pair by trying every rotation and shift pixel by pixel, the stable order by counting, the
overlay and the stats one pixel at a time. CPU only."""
import numpy as np

from oracle.input_oracle import rotate_nearest, rotation_coefficients
from tests.rerank_ref import pair_table, place_ref, rerank_ref, stable_order

S = 6


def tables():
    rng = np.random.default_rng(4)
    L = ((rng.random((4, S, S)) < 0.4) * 255).astype(np.uint8)
    K = ((rng.random((5, S, S)) < 0.4) * 255).astype(np.uint8)
    L[3] = 0            # an empty lock: every area 0
    K[4] = K[1]         # two identical keys at different indices
    coef = rotation_coefficients(np.array([0.0, 0.7, np.pi / 2, 4.0]), S, S)
    return L, K, coef


def literal_pair(lock, key, coef):
    lb = lock >= 128
    best, pose = 0, (0, 0, 0)
    for r in range(len(coef)):
        kr = rotate_nearest((key >= 128).astype(np.uint8), coef[r])
        for dy in range(-(S - 1), S):
            for dx in range(-(S - 1), S):
                ov = 0
                for y in range(S):
                    for x in range(S):
                        if 0 <= y - dy < S and 0 <= x - dx < S and lb[y, x] and kr[y - dy, x - dx]:
                            ov += 1
                if ov > best:
                    best, pose = ov, (r, dy, dx)
    return best, pose


def test_pair_table_is_the_literal_maximum():
    L, K, coef = tables()
    area, pose = pair_table(L, K, coef)
    for i in range(len(L)):
        for j in range(len(K)):
            a, p = literal_pair(L[i], K[j], coef)
            assert area[i, j] == a and tuple(pose[i, j]) == p, (i, j)
    assert (area[3] == 0).all() and (pose[3] == 0).all()
    np.testing.assert_array_equal(area[:, 4], area[:, 1])


def literal_ranks(area_row):
    return [sum(1 for f, b in enumerate(area_row) if b > a or (b == a and f < e)) for e, a in enumerate(area_row)]


def test_stable_order_is_the_counted_rank():
    rng = np.random.default_rng(1)
    for r in (1, 3, 7, 64):
        areas = rng.integers(-1, 4, (9, r))  # few values: many ties, empties among them
        order = stable_order(areas)
        for row, o in zip(areas, order):
            ranks = literal_ranks(row.tolist())
            assert sorted(ranks) == list(range(r))           # a permutation
            assert [ranks[c] for c in o] == list(range(r))   # column o[t] has rank t


def test_rerank_ref_rows():
    L, K, coef = tables()
    area, pose = pair_table(L, K, coef)
    cand = np.array([[1, 4, 1, 0, 2],       # key 1 twice and its twin 4: equal areas, columns kept
                     [3, -1, 2, -1, 0],     # empties in the middle
                     [-1, -1, -1, -1, -1],  # a row of empties
                     [4, 3, 2, 1, 0]])      # the empty lock: all 0, the model's order stays
    lock_idx = [2, 0, 1, 3]
    key, ar, ps, src = rerank_ref(cand, area, pose, lock_idx)
    for i in range(4):
        row = [-1 if c < 0 else int(area[lock_idx[i], c]) for c in cand[i]]
        ranks = literal_ranks(row)
        for e, t in enumerate(ranks):
            c = cand[i, e]
            assert src[i, t] == e and key[i, t] == (c if c >= 0 else -1) and ar[i, t] == row[e]
            assert tuple(ps[i, t]) == (tuple(pose[lock_idx[i], c]) if c >= 0 else (0, 0, 0))
        assert all(ar[i, t] >= ar[i, t + 1] for t in range(4))
    twins = [t for t in range(5) if key[0, t] in (1, 4)]
    assert [int(src[0, t]) for t in twins] == [0, 1, 2] and twins == [twins[0], twins[0] + 1, twins[0] + 2]
    assert key[1, 3:].tolist() == [-1, -1] and src[1, 3:].tolist() == [1, 3]
    assert src[2].tolist() == [0, 1, 2, 3, 4] and (ar[2] == -1).all() and (ps[2] == 0).all()
    assert key[3].tolist() == [4, 3, 2, 1, 0] and (ar[3] == 0).all()
    k0, a0, _, _ = rerank_ref(cand[:3], area, pose)  # lock_idx None: lock i
    assert a0[0, 0] == max(area[0, c] for c in cand[0])


def literal_place(lock, key, coef, pose):
    r, dy, dx = pose
    lb = lock >= 128
    if not (0 <= r < len(coef)) or abs(dy) >= S or abs(dx) >= S:
        return lb.astype(np.uint8), [int(lb.sum()), -1, -1, -1]
    kr = rotate_nearest((key >= 128).astype(np.uint8), coef[r])
    over = np.zeros((S, S), np.uint8)
    st = [0, 0, 0, 0]
    for y in range(S):
        for x in range(S):
            p = bool(kr[y - dy, x - dx]) if 0 <= y - dy < S and 0 <= x - dx < S else False
            over[y, x] = (1 if lb[y, x] else 0) | (2 if p else 0)
            st[0] += int(lb[y, x])
            st[1] += int(kr[y, x])
            st[2] += int(p)
            st[3] += int(lb[y, x] and p)
    return over, st


def test_place_ref_is_the_literal_overlay():
    L, K, coef = tables()
    area, pose = pair_table(L, K, coef)
    poses = [tuple(pose[0, 1]), tuple(pose[2, 3]), (1, S - 1, -(S - 1)), (3, -(S - 1), S - 1), (2, 0, 0),
             (-1, 0, 0), (len(coef), 0, 0), (0, S, 0), (0, 0, -S)]
    for n, p in enumerate(poses):
        i, j = n % 3, (n * 2) % 5
        over, st = place_ref(L[i], K[j], coef, p)
        lo, ls = literal_place(L[i], K[j], coef, p)
        np.testing.assert_array_equal(over, lo)
        assert st.tolist() == ls, p
    # at the pose of the maximum the shared pixels are the area
    for i, j in ((0, 1), (2, 3), (1, 0)):
        assert place_ref(L[i], K[j], coef, pose[i, j])[1][3] == area[i, j]

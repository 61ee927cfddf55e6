"""The host model of tests/failure_support.py against tables written by hand from the elimination tree (separator k has
level trailing_ones(k); its parent is the separator one level up whose subtree holds it), and its float64 KKT residual
against a dense assembly of the same system. No GPU."""
import numpy as np
import pytest

import failure_support as fs

LEVELS_16 = [0, 1, 0, 2, 0, 1, 0, 3, 0, 1, 0, 2, 0, 1, 0]
CONTAMINATED_8 = {0: [0, 1, 3], 1: [1, 3], 2: [2, 1, 3], 3: [3], 4: [4, 5, 3], 5: [5, 3], 6: [6, 5, 3]}
CONTAMINATED_16 = {0: [0, 1, 3, 7], 1: [1, 3, 7], 2: [2, 1, 3, 7], 3: [3, 7], 4: [4, 5, 3, 7], 5: [5, 3, 7],
                   6: [6, 5, 3, 7], 7: [7], 8: [8, 9, 11, 7], 9: [9, 11, 7], 10: [10, 9, 11, 7], 11: [11, 7],
                   12: [12, 13, 11, 7], 13: [13, 11, 7], 14: [14, 13, 11, 7]}


def test_levels():
    assert [fs.level(k) for k in range(15)] == LEVELS_16
    assert [fs.level(k) for k in range(7)] == LEVELS_16[:7]
    assert fs.level(31) == 5 and fs.level(47) == 4 and fs.level(55) == 3


@pytest.mark.parametrize("N,table", [(8, CONTAMINATED_8), (16, CONTAMINATED_16)])
def test_contaminated(N, table):
    assert {k: fs.contaminated(k, N) for k in range(N - 1)} == table
    for k, seps in table.items():  # one per level from level(k) to K - 1, ending at the top separator N / 2 - 1
        assert [fs.level(s) for s in seps] == list(range(fs.level(k), fs.tree_depth(N)))
        assert seps[-1] == N // 2 - 1


def test_padded_horizons_use_the_device_tree():
    assert fs.device_horizon(5) == 8 and fs.device_horizon(13) == 16 and fs.device_horizon(16) == 16
    assert fs.tree_depth(5) == 3 and fs.tree_depth(13) == 4 and fs.tree_depth(2) == 1
    assert {k: fs.contaminated(k, 5) for k in range(4)} == {k: CONTAMINATED_8[k] for k in range(4)}
    assert {k: fs.contaminated(k, 13) for k in range(12)} == {k: CONTAMINATED_16[k] for k in range(12)}
    assert fs.contaminated(0, 2) == [0] and fs.contaminated(2, 4) == [2, 1]


def test_separators_to_test():
    assert fs.separators_to_test(16) == list(range(15)) and fs.separators_to_test(13) == list(range(12))
    assert fs.separators_to_test(5) == [0, 1, 2, 3] and fs.separators_to_test(2) == [0]
    # first tile, the interior tile 16 .. 23, the last tile without knot N - 1, the top separator 15 (level 3: 23)
    assert fs.separators_to_test(32) == list(range(8)) + [15] + list(range(16, 31))
    # first tile, interior tile 32 .. 39, last tile; level 3: 55, level 4: 47, the top separator 31
    assert fs.separators_to_test(64) == list(range(8)) + [31] + list(range(32, 40)) + [47, 55] + list(range(56, 63))
    for N in (32, 64):  # both halves of every pair (s0 / s2, t0 / t1), the last and the top separator, every level
        ks = fs.separators_to_test(N)
        assert N - 2 in ks and N // 2 - 1 in ks
        assert {fs.level(k) for k in ks} == set(range(fs.tree_depth(N)))
        assert {k % 8 for k in ks} == set(range(8))


def test_count_bounds_cover_every_schedule_name():
    names = {"reduced", "reduced-fused2", "reduced-tree", "reduced-records", "knot-lean", "knot-strict", "knot-keep",
             "generic-reduced", "generic-reduced-records", "generic-lean", "generic-strict", "generic-keep",
             "reduced-compact-records"}
    assert set(fs.COUNT_BOUNDS) == names
    for name in names:
        assert fs.count_bound(name, 0, 16) == 4 and fs.count_bound(name, 7, 16) == 1 and fs.count_bound(name, 3, 5) == 1


def problem(n, m, N, seed=3):
    rng = np.random.default_rng(seed)
    return dict(A=rng.standard_normal((N, n * n)), B=rng.standard_normal((N, n * m)), Q=rng.uniform(1, 2, (N, n)),
                R=rng.uniform(1, 2, (N, m)), q=rng.standard_normal((N, n)), r=rng.standard_normal((N, m)),
                d=rng.standard_normal((N, n)), x0=rng.standard_normal(n))


def test_must_flag():
    n, m, N = 3, 2, 4
    g = problem(n, m, N)
    args = lambda h: (n, m, N, h["A"], h["B"], h["Q"], h["R"])
    assert not fs.must_flag(*args(g))
    for field, knot, value, want in [("A", 0, np.nan, True), ("A", N - 2, np.inf, True), ("B", 1, -np.inf, True),
                                     ("A", N - 1, np.nan, False), ("B", N - 1, np.nan, False), ("R", N - 1, np.nan, False),
                                     ("R", N - 1, -1.0, False), ("Q", N - 1, 0.0, True), ("Q", N - 1, np.inf, True),
                                     ("Q", 0, -1.0, True), ("R", N - 2, np.nan, True), ("R", 0, 0.0, True),
                                     ("Q", 2, 1e-310, False)]:
        h = {k: v.copy() for k, v in g.items()}
        h[field][knot][-1] = value
        assert fs.must_flag(*args(h)) == want, (field, knot, value)
    for pl in fs.unused_placements(n, m, N):
        assert pl.knot == N - 1 and pl.field in ("A", "B", "R", "r", "d")
    assert fs.matrix_entries(4, 3) == [3, 8] and fs.matrix_entries(4, 1) == [3, 0]


def dense_kkt(g):
    """K and b of the system in the order lambda_k, x_k, u_k per knot (no u at the last knot), assembled entry by entry"""
    N, n = g["Q"].shape
    m = g["R"].shape[1]
    zb = 2 * n + m
    nv = zb * N - m
    K, b = np.zeros((nv, nv)), np.zeros(nv)
    lam = lambda k: slice(zb * k, zb * k + n)
    x = lambda k: slice(zb * k + n, zb * k + 2 * n)
    u = lambda k: slice(zb * k + 2 * n, zb * k + zb)
    K[lam(0), x(0)] = -np.eye(n); K[x(0), lam(0)] = -np.eye(n); b[lam(0)] = -g["x0"]
    for k in range(N):
        K[x(k), x(k)] = np.diag(g["Q"][k]); b[x(k)] = -g["q"][k]
        if k < N - 1:
            A = g["A"][k].reshape(n, n).T
            B = g["B"][k].reshape(m, n).T
            K[u(k), u(k)] = np.diag(g["R"][k]); b[u(k)] = -g["r"][k]
            K[lam(k + 1), x(k)] = A; K[x(k), lam(k + 1)] = A.T
            K[lam(k + 1), u(k)] = B; K[u(k), lam(k + 1)] = B.T
            K[lam(k + 1), x(k + 1)] = -np.eye(n); K[x(k + 1), lam(k + 1)] = -np.eye(n)
            b[lam(k + 1)] = -g["d"][k]
    return K, b


@pytest.mark.parametrize("n,m,N", [(2, 1, 3), (3, 2, 4), (1, 1, 2)])
def test_kkt_relative_residual(n, m, N):
    g = problem(n, m, N)
    K, b = dense_kkt(g)
    z = np.linalg.solve(K, b)
    want = np.linalg.norm(K @ z - b) / np.linalg.norm(b)
    got = fs.kkt_relative_residual(g, z)
    assert got <= 1e-13 and abs(got - want) <= 1e-14
    for i in range(z.size):  # every variable is seen
        zz = z.copy()
        zz[i] += 1.0
        r = fs.kkt_relative_residual(g, zz)
        assert abs(r - np.linalg.norm(K @ zz - b) / np.linalg.norm(b)) <= 1e-12 * r and r > 1e-3
    zz = z.copy()
    zz[0] = np.nan
    assert not fs.kkt_relative_residual(g, zz) <= fs.REL_TOL
    # a weight whose reciprocal overflows is data like any other to the residual
    h = {k: v.copy() for k, v in g.items()}
    h["Q"][N - 1, n - 1] = 1e-310
    Kh, bh = dense_kkt(h)
    assert abs(fs.kkt_relative_residual(h, z) - np.linalg.norm(Kh @ z - bh) / np.linalg.norm(bh)) <= 1e-14

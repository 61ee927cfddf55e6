"""GPU: the dense helpers (ndlqr_hip_gemm / potrf_lower / potrs_lower / trsv_lower, csrc/hip_dense.hip with the kernels
of csrc/kernels_dense.hpp) and the Matrix* / clap_* wrappers of csrc/linalg.c at the sizes where their launches change:
more than one block of 256 elements or 64 right-hand sides, a ragged last block, more rows than the 256 threads of the
Cholesky, leading dimensions beyond the row count, k = 0, scratch growth and concurrent callers. Every result is held
to the restatement of tests/dense_support.py bit for bit over the whole buffer, padding included: the units are built
without contraction, the kernels spell the reference's operation order and fp64 + - x / sqrt are correctly rounded, so
a differing bit is a finding about the code."""
import ctypes as C
import threading

import numpy as np
import pytest

import dense_support as ds
from test_gpu_stages import mat  # (a Matrix points into the buffer returned with it: keep that buffer while the Matrix is used)

pytestmark = pytest.mark.gpu
dp = C.POINTER(C.c_double)
INVALID = -1  # NDLQR_ERR_INVALID


def P(a):
    return None if a is None else a.ctypes.data_as(dp)


def hip_gemm(L, tA, tB, m, n, k, alpha, A, lda, B, ldb, beta, Cb, ldc):
    """ndlqr_hip_gemm on copies: (return code, C afterwards); asserts that A and B come back as they went in."""
    a, b, c = A.copy(), B.copy(), Cb.copy()
    err = L.ndlqr_hip_gemm(tA, tB, m, n, k, alpha, P(a), lda, P(b), ldb, beta, P(c), ldc)
    assert np.array_equal(ds.bits(a), ds.bits(A)) and np.array_equal(ds.bits(b), ds.bits(B))
    return err, c


def hip_potrf(L, n, A, lda):
    a = A.copy()
    return L.ndlqr_hip_potrf_lower(n, P(a), lda), a


def hip_tri(L, which, n, nrhs, Lb, ldl, Bb, ldb):
    low, b = Lb.copy(), Bb.copy()
    if which == 0:
        err = L.ndlqr_hip_potrs_lower(n, nrhs, P(low), ldl, P(b), ldb)
    else:
        err = L.ndlqr_hip_trsv_lower(n, nrhs, P(low), ldl, P(b), ldb, 1 if which == 2 else 0)
    assert np.array_equal(ds.bits(low), ds.bits(Lb))
    return err, b


# ------------------------------------------------------------------------------------------- scratch growth (first: see below)
def test_scratch_growth_keeps_results(ndlqr):
    """A 5x4x7 product, then (96,96,96) -- 27 648 doubles, three doublings of a new scratch of 4096 -- then 5x4x7 again,
    on a fresh thread: all three bit-equal to the restatement, the first and the third to each other. (The scratches
    are pooled per process and handed to whichever thread asks; this test stands first in the file so that in a run of
    the suite no earlier call of these helpers has grown one, and test_threads_* below grows several new ones.)"""
    L = ndlqr.lib()
    small = ds.gemm_case(5, 4, 7, 0, 0, True)
    big = ds.gemm_case(96, 96, 96, 1, 0, False)
    got = []

    def work():
        for c, (m, n, k), tA in ((small, (5, 4, 7), 0), (big, (96, 96, 96), 1), (small, (5, 4, 7), 0)):
            got.append(hip_gemm(L, tA, 0, m, n, k, 0.7, c["A"], c["lda"], c["B"], c["ldb"], -1.3, c["C"], c["ldc"]))

    t = threading.Thread(target=work)
    t.start()
    t.join()
    assert [e for e, _ in got] == [0, 0, 0]
    want_small = ds.gemm_ref(0, 0, 5, 4, 7, 0.7, small["A"], small["lda"], small["B"], small["ldb"], -1.3, small["C"], small["ldc"])
    want_big = ds.gemm_ref(1, 0, 96, 96, 96, 0.7, big["A"], big["lda"], big["B"], big["ldb"], -1.3, big["C"], big["ldc"])
    ds.assert_bits(got[0][1], want_small, small["ldc"], 5, 4, "first 5x4x7")
    ds.assert_bits(got[1][1], want_big, big["ldc"], 96, 96, "96x96x96")
    ds.assert_bits(got[2][1], want_small, small["ldc"], 5, 4, "5x4x7 after the growth")
    ds.assert_bits(got[2][1], got[0][1], small["ldc"], 5, 4, "first against third")


# ------------------------------------------------------------------------------------------- the three kernels
@pytest.mark.parametrize("m,n,k", ds.GEMM_SHAPES)
def test_gemm_bits(ndlqr, m, n, k):
    L = ndlqr.lib()
    for tA, tB in ds.GEMM_TRANSPOSES:
        for padded in (False, True):
            c = ds.gemm_case(m, n, k, tA, tB, padded)
            for alpha, beta in ds.GEMM_SCALARS:
                err, got = hip_gemm(L, tA, tB, m, n, k, alpha, c["A"], c["lda"], c["B"], c["ldb"], beta, c["C"], c["ldc"])
                assert err == 0
                want = ds.gemm_ref(tA, tB, m, n, k, alpha, c["A"], c["lda"], c["B"], c["ldb"], beta, c["C"], c["ldc"])
                ds.assert_bits(got, want, c["ldc"], m, n,
                               "gemm (%d,%d,%d) tA=%d tB=%d padded=%d alpha=%g beta=%g" % (m, n, k, tA, tB, padded, alpha, beta))


@pytest.mark.parametrize("n", ds.POTRF_SIZES)
def test_potrf_bits(ndlqr, n):
    """Success and every failure case, each failure followed by a successful factorisation on the same thread (the
    failure word of the leased scratch is reused)."""
    L = ndlqr.lib()
    for padded in (False, True):
        good, lda = ds.potrf_case(n, padded)
        info, want = ds.potrf_expected(n, padded)
        assert info == 0
        err, got = hip_potrf(L, n, good, lda)
        assert err == 0
        ds.assert_bits(got, want, lda, n, n, "potrf n=%d lda=%d" % (n, lda))
        for failure in ds.potrf_failures(n):
            bad, _ = ds.potrf_case(n, padded, failure)
            finfo, fwant = ds.potrf_expected(n, padded, failure)
            assert finfo > 0
            err, got = hip_potrf(L, n, bad, lda)
            assert err == -1, (failure, err)
            ds.assert_bits(got, fwant, lda, n, n, "potrf n=%d lda=%d failing at pivot %d (%s)" % (n, lda, finfo - 1, failure))
            err, got = hip_potrf(L, n, good, lda)
            assert err == 0, "success after the failure %s" % failure
            ds.assert_bits(got, want, lda, n, n, "potrf n=%d lda=%d after the failure %s" % (n, lda, failure))


@pytest.mark.parametrize("n", ds.POTRS_N)
def test_potrs_and_trsv_bits(ndlqr, n):
    L = ndlqr.lib()
    for nrhs in ds.POTRS_NRHS:
        Lb, ldl, Bb, ldb = ds.potrs_case(n, nrhs)
        for which in ds.POTRS_WHICH:
            err, got = hip_tri(L, which, n, nrhs, Lb, ldl, Bb, ldb)
            assert err == 0
            want = ds.potrs_ref(n, nrhs, Lb, ldl, Bb, ldb, which)
            ds.assert_bits(got, want, ldb, n, nrhs, "n=%d nrhs=%d which=%d" % (n, nrhs, which))


# ------------------------------------------------------------------------------------------- refusals
def test_argument_refusals_leave_operands_unchanged(ndlqr):
    """lda < rows, ldc < m, a dimension <= 0, a null operand: NDLQR_ERR_INVALID before any launch, every operand bit for
    bit as it was."""
    L = ndlqr.lib()
    assert ndlqr.api.ERR_INVALID == INVALID
    m, n, k = 5, 4, 7
    c = ds.gemm_case(m, n, k, 0, 0, True)
    A, B, Cb, lda, ldb, ldc = c["A"], c["B"], c["C"], c["lda"], c["ldb"], c["ldc"]
    ct = ds.gemm_case(m, n, k, 1, 1, True)
    calls = [
        (0, 0, m, n, k, A, m - 1, B, ldb, Cb, ldc),      # lda < rows of A
        (0, 0, m, n, k, A, lda, B, k - 1, Cb, ldc),      # ldb < rows of B
        (0, 0, m, n, k, A, lda, B, ldb, Cb, m - 1),      # ldc < m
        (1, 1, m, n, k, ct["A"], k - 1, ct["B"], ct["ldb"], ct["C"], ct["ldc"]),   # transposed: A is stored k x m
        (1, 1, m, n, k, ct["A"], ct["lda"], ct["B"], n - 1, ct["C"], ct["ldc"]),   # ... and B n x k
        (0, 0, m, 0, k, A, lda, B, ldb, Cb, ldc), (0, 0, m, -1, k, A, lda, B, ldb, Cb, ldc),
        (0, 0, 0, n, k, A, lda, B, ldb, Cb, ldc), (0, 0, m, n, -1, A, lda, B, ldb, Cb, ldc),
        (0, 0, m, n, k, None, lda, B, ldb, Cb, ldc), (0, 0, m, n, k, A, lda, None, ldb, Cb, ldc),
        (0, 0, m, n, k, A, lda, B, ldb, None, ldc),
    ]
    for tA, tB, mm, nn, kk, a, la, b, lb, cc, lc in calls:
        a2, b2, c2 = [None if x is None else x.copy() for x in (a, b, cc)]
        assert L.ndlqr_hip_gemm(tA, tB, mm, nn, kk, 0.7, P(a2), la, P(b2), lb, -1.3, P(c2), lc) == INVALID
        for x, y in ((a, a2), (b, b2), (cc, c2)):
            assert x is None or np.array_equal(ds.bits(x), ds.bits(y))
    n = 6
    good, lda = ds.potrf_case(n, True)
    for nn, buf, ld in ((n, good, n - 1), (0, good, lda), (-2, good, lda), (n, None, lda)):
        b2 = None if buf is None else buf.copy()
        assert L.ndlqr_hip_potrf_lower(nn, P(b2), ld) == INVALID
        assert buf is None or np.array_equal(ds.bits(buf), ds.bits(b2))
    n, nrhs = 40, 65
    Lb, ldl, Bb, ldb = ds.potrs_case(n, nrhs)
    for nn, nr, low, ll, b, lb in ((n, nrhs, Lb, n - 1, Bb, ldb), (n, nrhs, Lb, ldl, Bb, n - 1), (0, nrhs, Lb, ldl, Bb, ldb),
                                   (n, 0, Lb, ldl, Bb, ldb), (n, -3, Lb, ldl, Bb, ldb), (n, nrhs, None, ldl, Bb, ldb),
                                   (n, nrhs, Lb, ldl, None, ldb)):
        for which in ds.POTRS_WHICH:
            l2, b2 = [None if x is None else x.copy() for x in (low, b)]
            if which == 0:
                err = L.ndlqr_hip_potrs_lower(nn, nr, P(l2), ll, P(b2), lb)
            else:
                err = L.ndlqr_hip_trsv_lower(nn, nr, P(l2), ll, P(b2), lb, which - 1)
            assert err == INVALID
            for x, y in ((low, l2), (b, b2)):
                assert x is None or np.array_equal(ds.bits(x), ds.bits(y))


# ------------------------------------------------------------------------------------------- threads
THREADS, CALLS = 8, 40


def _thread_ops(t):
    """The five calls thread t repeats (CALLS / 5 rounds): shapes of its own, the third and the fifth beyond 4096
    doubles of operands for most threads (and by different amounts), in an order rotated by t so that the scratches
    grow at different moments. Each op: (kind, arguments, expected return, expected buffer, (ld, rows, cols))."""
    ops = []
    m, n, k = 10 + 3 * t, 7 + 2 * t, 5 + t
    c = ds.gemm_case(m, n, k, t & 1, (t >> 1) & 1, True)
    args = (t & 1, (t >> 1) & 1, m, n, k, 0.7, c["A"], c["lda"], c["B"], c["ldb"], -1.3, c["C"], c["ldc"])
    ops.append(("gemm", args, 0, ds.gemm_ref(*args), (c["ldc"], m, n)))
    pn = 20 + 9 * t                               # 20 .. 83: (n + 3) n doubles, beyond 4096 from t = 5
    buf, lda = ds.potrf_case(pn, True, "neg%d" % (pn // 2) if t % 3 == 2 else None)
    info, want = ds.potrf_ref(pn, buf, lda)
    ops.append(("potrf", (pn, buf, lda), -1 if info else 0, want, (lda, pn, pn)))
    m, n, k = 64 + 8 * t, 50 + t, 30              # 6620 .. 14 290 doubles
    c = ds.gemm_case(m, n, k, 0, 1, False)
    args = (0, 1, m, n, k, 1.0, c["A"], c["lda"], c["B"], c["ldb"], 0.0, c["C"], c["ldc"])
    ops.append(("gemm", args, 0, ds.gemm_ref(*args), (c["ldc"], m, n)))
    sn, nrhs = 20 + 9 * t, 3 + 10 * t
    Lb, ldl, Bb, ldb = ds.potrs_case(sn, nrhs)
    ops.append(("tri", (t % 3, sn, nrhs, Lb, ldl, Bb, ldb), 0, ds.potrs_ref(sn, nrhs, Lb, ldl, Bb, ldb, t % 3), (ldb, sn, nrhs)))
    sn, nrhs = 30 + t, 66 + 9 * t                 # two or three blocks of right-hand sides
    Lb, ldl, Bb, ldb = ds.potrs_case(sn, nrhs)
    ops.append(("tri", (0, sn, nrhs, Lb, ldl, Bb, ldb), 0, ds.potrs_ref(sn, nrhs, Lb, ldl, Bb, ldb, 0), (ldb, sn, nrhs)))
    return ops[t % 5:] + ops[:t % 5]


def test_threads_share_the_scratch_pool(ndlqr):
    """Eight host threads (ctypes releases the GIL: they are inside the helpers, and their scratch leases, at the same
    time), released by a barrier, forty calls each of a fixed mix of gemm, potrf and potrs / trsv at shapes of their
    own: every result bit-equal to the serial restatement. One process, eight streams."""
    L = ndlqr.lib()
    plans = [_thread_ops(t) for t in range(THREADS)]
    results = [[] for _ in range(THREADS)]
    errors = []
    barrier = threading.Barrier(THREADS)
    run = {"gemm": lambda a: hip_gemm(L, *a), "potrf": lambda a: hip_potrf(L, *a), "tri": lambda a: hip_tri(L, *a)}

    def work(t):
        try:
            barrier.wait(timeout=60)
            for call in range(CALLS):
                kind, args, _, _, _ = plans[t][call % 5]
                results[t].append(run[kind](args))
        except Exception as exc:  # (reported below, in the main thread)
            errors.append((t, repr(exc)))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(THREADS)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for t in range(THREADS):
        assert len(results[t]) == CALLS
        for call, (err, got) in enumerate(results[t]):
            kind, _, want_err, want, (ld, rows, cols) = plans[t][call % 5]
            assert err == want_err, (t, call, kind, err)
            ds.assert_bits(got, want, ld, rows, cols, "thread %d call %d (%s)" % (t, call, kind))


# ------------------------------------------------------------------------------------------- Matrix* / clap_* wrappers
def _rng(*key):
    return np.random.default_rng([77] + [int(x) for x in key])


def _flat(a):
    """Column-major flat copy of a 2-D array: what a Matrix of mat() holds."""
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).T).ravel()


def _assert_flat(buf, want2d, what):
    rows, cols = want2d.shape
    ds.assert_bits(buf, _flat(want2d), rows, rows, cols, what)


@pytest.mark.parametrize("name", ["MatrixAddition", "clap_MatrixAddition"])
def test_matrix_addition(ndlqr, name):
    """B += alpha A at 20 x 20: 400 elements, two blocks."""
    L = ndlqr.lib()
    rng = _rng(1)
    a, b = rng.standard_normal((20, 20)), rng.standard_normal((20, 20))
    a[3, 4], b[3, 4], b[5, 6] = 0.0, -0.0, -0.0
    for alpha in (0.7, -1.0, 0.0):
        A, Ab = mat(ndlqr, a)
        B, Bb = mat(ndlqr, b)
        assert getattr(L, name)(C.byref(A), C.byref(B), alpha) == 0
        _assert_flat(Bb, b + np.float64(alpha) * a, "%s alpha=%g" % (name, alpha))
        _assert_flat(Ab, a, "%s: A" % name)


@pytest.mark.parametrize("alpha", [2.5, -1.0, 0.0])
def test_clap_matrix_scale(ndlqr, alpha):
    """A *= alpha, one multiplication per entry as in the reference: -0.0 for +0.0 * -1, +-inf stays +-inf (times 0 it is
    NaN, whose sign the arithmetic standard leaves open: NaN is asserted there, the other entries bit for bit)."""
    L = ndlqr.lib()
    a = _rng(2).standard_normal((20, 20))
    a[0, 0], a[1, 0], a[7, 13], a[19, 19] = 0.0, -0.0, 0.0, -0.0
    A, Ab = mat(ndlqr, a)
    assert L.clap_MatrixScale(C.byref(A), alpha) == 0
    _assert_flat(Ab, a * np.float64(alpha), "clap_MatrixScale alpha=%g" % alpha)
    a[2, 2], a[3, 17] = np.inf, -np.inf
    A, Ab = mat(ndlqr, a)
    assert L.clap_MatrixScale(C.byref(A), alpha) == 0
    got = Ab.reshape(20, 20).T
    with np.errstate(invalid="ignore"):
        want = a * np.float64(alpha)
    if alpha == 0.0:
        assert np.isnan(got[2, 2]) and np.isnan(got[3, 17]), (got[2, 2], got[3, 17])
        got = got.copy()
        got[2, 2] = got[3, 17] = want[2, 2] = want[3, 17] = 0.0
    else:
        assert got[2, 2] == np.inf * alpha and got[3, 17] == -np.inf * alpha, (got[2, 2], got[3, 17])
    _assert_flat(_flat(got), want, "clap_MatrixScale with infinities, alpha=%g" % alpha)


@pytest.mark.parametrize("n", [1, 17, 300])
def test_clap_add_diagonal(ndlqr, n):
    """diag(A) += alpha through the strided ldc = n + 1 product; the off-diagonal entries (NaN and -0.0 among them) stay
    bit for bit."""
    L = ndlqr.lib()
    a = _rng(3, n).standard_normal((n, n))
    if n > 1:
        a[0, n - 1], a[n - 1, 0], a[1, 0] = np.nan, -0.0, np.inf
    A, Ab = mat(ndlqr, a)
    assert L.clap_AddDiagonal(C.byref(A), 0.3) == 0
    want = a.copy()
    want[np.diag_indices(n)] = np.diag(a) + np.float64(0.3)
    _assert_flat(Ab, want, "clap_AddDiagonal n=%d" % n)


def test_clap_multiply_and_transpose_multiply(ndlqr):
    """(33,31,40): five blocks, the last ragged."""
    L = ndlqr.lib()
    m, n, k = 33, 31, 40
    for tA, tB in ds.GEMM_TRANSPOSES:
        c = ds.gemm_case(m, n, k, tA, tB, False)
        a, b, c0 = (ds.view(c["A"], c["lda"], c["Ar"], c["Ac"]), ds.view(c["B"], c["ldb"], c["Br"], c["Bc"]),
                    ds.view(c["C"], c["ldc"], m, n))
        want = ds.gemm_ref(tA, tB, m, n, k, 0.7, c["A"], c["lda"], c["B"], c["ldb"], -1.3, c["C"], c["ldc"])
        for name in ("clap_MatrixMultiply", "MatrixMultiply"):
            A, keepA = mat(ndlqr, a)
            B, keepB = mat(ndlqr, b)
            Cm, Cb = mat(ndlqr, c0)
            ret = getattr(L, name)(C.byref(A), C.byref(B), C.byref(Cm), bool(tA), bool(tB), 0.7, -1.3)
            assert name == "MatrixMultiply" or ret == 0
            ds.assert_bits(Cb, want, m, m, n, "%s tA=%d tB=%d" % (name, tA, tB))
    c = ds.gemm_case(m, n, k, 1, 0, False)
    A, keepA = mat(ndlqr, ds.view(c["A"], c["lda"], k, m))
    B, keepB = mat(ndlqr, ds.view(c["B"], c["ldb"], k, n))
    Cm, Cb = mat(ndlqr, ds.view(c["C"], c["ldc"], m, n))
    assert L.clap_MatrixTransposeMultiply(C.byref(A), C.byref(B), C.byref(Cm)) == 0
    want = ds.gemm_ref(1, 0, m, n, k, 1.0, c["A"], c["lda"], c["B"], c["ldb"], 0.0, c["C"], c["ldc"])
    ds.assert_bits(Cb, want, m, m, n, "clap_MatrixTransposeMultiply")


@pytest.mark.parametrize("name", ["MatrixSymmetricMultiply", "clap_SymmetricMatrixMultiply"])
def test_symmetric_multiply_reads_the_lower_triangle(ndlqr, name):
    """n = 33: NaN in the strict upper triangle of Asym gives the bits of the mirrored matrix, which are the product's."""
    L = ndlqr.lib()
    n, cols = 33, 31
    rng = _rng(4)
    full = rng.standard_normal((n, n))
    full = np.tril(full) + np.tril(full, -1).T
    x, c0 = rng.standard_normal((n, cols)), rng.standard_normal((n, cols))
    lower = full.copy()
    lower[np.triu_indices(n, 1)] = np.nan
    want = ds.gemm_ref(0, 0, n, cols, n, 0.7, _flat(full), n, _flat(x), n, -1.3, _flat(c0), n)
    outs = []
    for sym in (lower, full):
        A, Ab = mat(ndlqr, sym)
        X, keepX = mat(ndlqr, x)
        Cm, Cb = mat(ndlqr, c0)
        ret = getattr(L, name)(C.byref(A), C.byref(X), C.byref(Cm), 0.7, -1.3)
        assert name == "MatrixSymmetricMultiply" or ret == 0
        _assert_flat(Ab, sym, "%s: Asym" % name)
        ds.assert_bits(Cb, want, n, n, cols, name)
        outs.append(Cb)
    ds.assert_bits(outs[0], outs[1], n, n, cols, "NaN triangle against mirrored triangle")


def test_cholesky_factorize_and_solve_wrappers(ndlqr):
    """n = 257 (a second step of the 256 threads) and 65 right-hand sides (a second block), through the four Matrix*
    entry points and the two clap_* ones; the info fields for one success and one failure."""
    L = ndlqr.lib()
    n, nrhs = 257, 65
    good, _ = ds.potrf_case(n, False)
    _, want = ds.potrf_expected(n, False)
    failure = "neg%d" % (n // 2)
    bad, _ = ds.potrf_case(n, False, failure)
    _, fwant = ds.potrf_expected(n, False, failure)
    as2d = lambda buf: buf.reshape(n, n).T  # noqa: E731
    for name in ("MatrixCholeskyFactorize", "MatrixCholeskyFactorizeWithInfo", "clap_CholeskyFactorize"):
        for src, expect, code in ((good, want, 0), (bad, fwant, -1)):
            A, Ab = mat(ndlqr, as2d(src))
            if name.endswith("WithInfo"):
                info = ndlqr.api.CholeskyInfo(b"\0", 7, b"\0", None, 0)
                ret = L.MatrixCholeskyFactorizeWithInfo(C.byref(A), C.byref(info))
                assert (info.lib, info.uplo, info.success) == (b"H", b"L", ret)
            else:
                ret = getattr(L, name)(C.byref(A))
            assert ret == code, (name, ret)   # (clap_kCholeskySuccess = 0, clap_kCholeskyFail = -1)
            ds.assert_bits(Ab, expect, n, n, n, "%s returning %d" % (name, code))
    rhs = _rng(5).standard_normal((n, nrhs))
    xwant = ds.potrs_ref(n, nrhs, want, n, _flat(rhs), n, 0)
    for name in ("MatrixCholeskySolve", "MatrixCholeskySolveWithInfo", "clap_CholeskySolve"):
        A, Ab = mat(ndlqr, as2d(want))
        B, Bb = mat(ndlqr, rhs)
        if name.endswith("WithInfo"):
            info = ndlqr.api.CholeskyInfo(b"L", 0, b"H", None, 1)
            ret = L.MatrixCholeskySolveWithInfo(C.byref(A), C.byref(B), C.byref(info))
        else:
            ret = getattr(L, name)(C.byref(A), C.byref(B))
        assert ret == 0
        ds.assert_bits(Bb, xwant, n, n, nrhs, name)
        ds.assert_bits(Ab, want, n, n, n, "%s: the factor" % name)


@pytest.mark.parametrize("transposed", [False, True])
def test_clap_lower_tri_back_sub(ndlqr, transposed):
    L = ndlqr.lib()
    n, nrhs = 40, 65
    Lb, ldl, Bb, ldb = ds.potrs_case(n, nrhs)
    low, rhs = ds.view(Lb, ldl, n, n), ds.view(Bb, ldb, n, nrhs)
    Lm, keepL = mat(ndlqr, low)
    B, Bbuf = mat(ndlqr, rhs)
    assert L.clap_LowerTriBackSub(C.byref(Lm), C.byref(B), transposed) == 0
    want = ds.potrs_ref(n, nrhs, _flat(low), n, _flat(rhs), n, 2 if transposed else 1)
    ds.assert_bits(Bbuf, want, n, n, nrhs, "clap_LowerTriBackSub transposed=%d" % transposed)


@pytest.mark.parametrize("rows,cols", [(4, 4), (3, 5), (5, 3)])
def test_matrix_copy_diagonal(ndlqr, rows, cols):
    """Host only: dest = diag(src), everything else cleared; src shorter than, equal to and longer than the diagonal."""
    L = ndlqr.lib()
    diag = min(rows, cols)
    for length in (diag - 1, diag, diag + 2):
        src = np.arange(1.0, length + 1.0)
        D, Db = mat(ndlqr, np.full((rows, cols), 9.0))
        S, Sb = mat(ndlqr, src)
        L.MatrixCopyDiagonal(C.byref(D), C.byref(S))
        want = np.zeros((rows, cols))
        for i in range(min(length, diag)):
            want[i, i] = src[i]
        _assert_flat(Db, want, "MatrixCopyDiagonal %dx%d from %d entries" % (rows, cols, length))
        assert np.array_equal(Sb, src)

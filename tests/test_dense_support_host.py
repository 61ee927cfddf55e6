"""CPU: the test infrastructure of tests/dense_support.py checks itself -- (1) the restatements of dense_gemm,
dense_potrf and dense_potrs compute the operation they name (against an extended-precision evaluation and np.linalg;
these bounds only guard the restatement against being a different operation, the bar for the device is bit equality),
(2) the bit comparison finds and locates every kind of error a wrong launch or kernel would leave, one injected at a
time into the restatement's own output, (3) the Python level loop that drives the oracle's stage calls reproduces the
oracle's own solve bit for bit at every shape of the stage table."""
import numpy as np
import pytest

import dense_support as ds

EPS = np.finfo(np.float64).eps
LD = np.longdouble


def _ld(buf, ld, rows, cols):
    return ds.view(buf, ld, rows, cols).astype(LD)


# ------------------------------------------------------------------------------------------- (1) the restatements
@pytest.mark.parametrize("m,n,k", ds.GEMM_SHAPES)
def test_gemm_restatement_is_the_product(m, n, k):
    """|restatement - extended precision| <= (k + 2) eps (|alpha| |op(A)| |op(B)| + |beta| |C|) entry by entry: k products
    and sums, the scaling by alpha and the one by beta, each rounded once (the usual k eps |A| |B| bound)."""
    worst = 0.0
    for tA, tB in ds.GEMM_TRANSPOSES:
        for padded in (False, True):
            c = ds.gemm_case(m, n, k, tA, tB, padded)
            for alpha, beta in ds.GEMM_SCALARS:
                out = ds.gemm_ref(tA, tB, m, n, k, alpha, c["A"], c["lda"], c["B"], c["ldb"], beta, c["C"], c["ldc"])
                C0 = _ld(c["C"], c["ldc"], m, n)
                if k > 0:
                    A = _ld(c["A"], c["lda"], c["Ar"], c["Ac"])
                    B = _ld(c["B"], c["ldb"], c["Br"], c["Bc"])
                    A, B = (A.T if tA else A), (B.T if tB else B)
                else:
                    A, B = np.zeros((m, 0), dtype=LD), np.zeros((0, n), dtype=LD)
                exact = LD(alpha) * (A @ B) + LD(beta) * C0
                bound = (k + 2) * EPS * (abs(LD(alpha)) * (np.abs(A) @ np.abs(B)) + abs(LD(beta)) * np.abs(C0))
                err = np.abs(ds.view(out, c["ldc"], m, n).astype(LD) - exact)
                assert np.all(err <= bound), (tA, tB, padded, alpha, beta)
                worst = max(worst, float(np.max(err / np.maximum(bound, np.finfo(LD).tiny))))
                # the padding and the operands are not touched
                pad = np.ones(out.size, dtype=bool)
                pad[(np.arange(m)[:, None] + c["ldc"] * np.arange(n)[None, :]).ravel()] = False
                assert np.array_equal(ds.bits(out)[pad], ds.bits(c["C"])[pad])
    print("gemm (%d,%d,%d): largest error / bound = %.3f" % (m, n, k, worst))


@pytest.mark.parametrize("n", ds.POTRF_SIZES)
def test_potrf_restatement_is_the_cholesky_factor(n):
    """|A - L L'| <= (n + 1) eps |L| |L'| entry by entry, the residual formed in extended precision (the backward error
    bound of the Cholesky factorisation), and ||L - np.linalg.cholesky(A)|| <= n eps cond(A) ||L|| (two backward-stable
    factorisations of one matrix). The strict upper triangle and the padding come back as they went in."""
    for padded in (False, True):
        buf, lda = ds.potrf_case(n, padded)
        info, out = ds.potrf_expected(n, padded)
        assert info == 0
        A = np.tril(ds.view(buf, lda, n, n))
        A = A + np.tril(A, -1).T
        L = np.tril(ds.view(out, lda, n, n))
        Ll = L.astype(LD)
        resid = np.abs(A.astype(LD) - Ll @ Ll.T)
        bound = (n + 1) * EPS * (np.abs(Ll) @ np.abs(Ll.T))
        assert np.all(resid <= bound)
        diff = np.linalg.norm(L - np.linalg.cholesky(A), 2)
        nbound = n * EPS * np.linalg.cond(A) * np.linalg.norm(L, 2)
        assert diff <= nbound
        keep = np.ones(out.size, dtype=bool)
        rows, cols = np.tril_indices(n)
        keep[rows + lda * cols] = False
        assert np.array_equal(ds.bits(out)[keep], ds.bits(buf)[keep])
        print("potrf n=%d lda=%d: residual / bound = %.3f, |L - numpy| = %.3e (bound %.3e)"
              % (n, lda, float(np.max(resid / bound)), diff, nbound))


@pytest.mark.parametrize("n", ds.POTRF_SIZES)
def test_potrf_restatement_failures(n):
    """A failure returns the 1-based pivot and leaves columns < j finished (equal to the successful factorisation of the
    leading block), column j updated and not scaled, the rest untouched."""
    for padded in (False, True):
        for failure in ds.potrf_failures(n):
            buf, lda = ds.potrf_case(n, padded, failure)
            info, out = ds.potrf_expected(n, padded, failure)
            j = int(failure[3:]) if failure.startswith("neg") else n // 2
            assert info == j + 1, (failure, info)
            got, src = ds.view(out, lda, n, n), ds.view(buf, lda, n, n)
            if j > 0:  # the leading j x j block is SPD: its columns are those of its own factorisation, rows below included
                sub_info, sub = ds.potrf_ref(j, buf, lda)
                assert sub_info == 0
                assert np.array_equal(ds.bits(np.tril(ds.view(sub, lda, j, j))), ds.bits(np.tril(got[:j, :j])))
                head = np.linalg.cholesky(np.tril(src[:j, :j]) + np.tril(src[:j, :j], -1).T)
                below = np.linalg.solve(head, src[j:, :j].T).T   # L[j:, :j] = A[j:, :j] L_head^-T
                assert np.allclose(got[j:, :j], below, rtol=1e-10, atol=1e-10)
            pivot = got[j, j]
            assert not (pivot > 0.0)
            if failure == "zero":
                assert pivot == 0.0
            if failure == "nan":
                assert np.isnan(pivot)
            want_col = src[j:, j] - got[j:, :j] @ got[j, :j]   # updated, not scaled
            mask = ~np.isnan(want_col)
            assert np.allclose(got[j:, j][mask], want_col[mask], rtol=1e-10, atol=1e-10)
            assert np.array_equal(ds.bits(got[:, j + 1:]), ds.bits(src[:, j + 1:]))  # the rest untouched


def _substitute_ld(L, B, transposed):
    """Row-oriented (dot product) substitution in extended precision: another algorithm than the restatement's."""
    n = L.shape[0]
    X = B.astype(LD).copy()
    T = (L.T if transposed else L).astype(LD)
    order = range(n - 1, -1, -1) if transposed else range(n)
    for i in order:
        sl = slice(i + 1, n) if transposed else slice(0, i)
        X[i] = (X[i] - T[i, sl] @ X[sl]) / T[i, i]
    return X


@pytest.mark.parametrize("n", ds.POTRS_N)
@pytest.mark.parametrize("nrhs", [1, 65])
def test_potrs_restatement_solves(n, nrhs):
    """max over the right-hand sides of ||x - x_ld||_inf / ||x_ld||_inf <= n eps cond_inf per substitution (a substitution
    is backward stable with backward error n eps |L|; the two of which = 0 add: the first one's error goes through the
    second solve, hence cond(L') (1 + cond(L)))."""
    Lb, ldl, Bb, ldb = ds.potrs_case(n, nrhs)
    L = np.tril(ds.view(Lb, ldl, n, n))
    B = ds.view(Bb, ldb, n, nrhs)
    cL, cLt = np.linalg.cond(L, np.inf), np.linalg.cond(L.T, np.inf)
    for which in ds.POTRS_WHICH:
        out = ds.potrs_ref(n, nrhs, Lb, ldl, Bb, ldb, which)
        X = ds.view(out, ldb, n, nrhs)
        if which == 0:
            exact, cond = _substitute_ld(L, _substitute_ld(L, B, False), True), cLt * (1 + cL)
        elif which == 1:
            exact, cond = _substitute_ld(L, B, False), cL
        else:
            exact, cond = _substitute_ld(L, B, True), cLt
        err = float(np.max(np.max(np.abs(X.astype(LD) - exact), axis=0) / np.max(np.abs(exact), axis=0)))
        bound = n * EPS * cond
        print("potrs n=%d nrhs=%d which=%d: relative error %.3e (bound %.3e)" % (n, nrhs, which, err, bound))
        assert err <= bound
        plain = (np.linalg.solve(L @ L.T, B), np.linalg.solve(L, B), np.linalg.solve(L.T, B))[which]
        assert np.allclose(X, plain, rtol=1e-9, atol=1e-12)
        pad = np.ones(out.size, dtype=bool)
        pad[(np.arange(n)[:, None] + ldb * np.arange(nrhs)[None, :]).ravel()] = False
        assert np.array_equal(ds.bits(out)[pad], ds.bits(Bb)[pad])


def test_nan_outside_the_operands_influences_nothing():
    """The restatements read neither the padding nor the strict upper triangle: other values there, the same bits."""
    n, nrhs = 40, 65
    Lb, ldl, Bb, ldb = ds.potrs_case(n, nrhs)
    L2 = np.where(np.isnan(Lb), 7.0, Lb)
    for which in ds.POTRS_WHICH:
        a = ds.potrs_ref(n, nrhs, Lb, ldl, Bb, ldb, which)
        b = ds.potrs_ref(n, nrhs, L2, ldl, Bb, ldb, which)
        assert ds.compare(a, b, ldb, n, nrhs) is None
    buf, lda = ds.potrf_case(64, True)
    other = np.where(np.isnan(buf), -3.0, buf)
    ia, a = ds.potrf_ref(64, buf, lda)
    ib, b = ds.potrf_ref(64, other, lda)
    low = np.tril_indices(64)
    assert ia == ib == 0 and np.array_equal(ds.bits(ds.view(a, lda, 64, 64)[low]), ds.bits(ds.view(b, lda, 64, 64)[low]))


# ------------------------------------------------------------------------------------------- (2) the comparison
def test_compare_passes_equal_buffers_with_nan_and_signed_zero():
    a = np.array([1.0, -0.0, 0.0, np.nan, np.inf, -np.inf])
    assert ds.compare(a, a.copy(), 3, 3, 2) is None
    ds.assert_bits(a, a.copy(), 3, 3, 2)


def _gemm_two_blocks():
    m, n, k = 17, 16, 9
    c = ds.gemm_case(m, n, k, 0, 0, True)
    want = ds.gemm_ref(0, 0, m, n, k, 0.7, c["A"], c["lda"], c["B"], c["ldb"], -1.3, c["C"], c["ldc"])
    return m, n, c, want


def test_compare_names_one_ulp():
    m, n, c, want = _gemm_two_blocks()
    got = want.copy()
    off = 7 + c["ldc"] * 11
    got[off] = np.nextafter(got[off], np.inf)
    f = ds.compare(got, want, c["ldc"], m, n)
    assert (f["count"], f["where"], f["row"], f["col"], f["element"], f["offset"]) == (1, "entry", 7, 11, 7 + m * 11, off)
    assert abs(int(f["got_bits"], 16) - int(f["want_bits"], 16)) == 1
    with pytest.raises(AssertionError, match=r"row 7, col 11, element 194"):
        ds.assert_bits(got, want, c["ldc"], m, n, "one ulp")


def test_compare_names_a_signed_zero():
    want = ds.pack(np.array([[1.0, 0.0], [2.0, 3.0], [4.0, 5.0]]), 4)
    got = want.copy()
    got[4] = -0.0
    assert got[4] == want[4]  # equal as numbers
    f = ds.compare(got, want, 4, 3, 2)
    assert (f["count"], f["where"], f["row"], f["col"]) == (1, "entry", 0, 1)
    assert (f["got_bits"], f["want_bits"]) == ("8000000000000000", "0000000000000000")


def test_compare_names_a_padding_double():
    m, n, c, want = _gemm_two_blocks()
    got = want.copy()
    off = (m + 2) + c["ldc"] * 3   # the third padding row of column 3: NaN before and a NaN of another payload after
    assert np.isnan(want[off])
    got.view(np.uint64)[off] ^= np.uint64(1)
    assert np.isnan(got[off])
    f = ds.compare(got, want, c["ldc"], m, n)
    assert (f["count"], f["where"], f["row"], f["col"], f["element"], f["offset"]) == (1, "padding", m + 2, 3, None, off)
    got = want.copy()
    got[off] = 0.0
    assert ds.compare(got, want, c["ldc"], m, n)["where"] == "padding"


def test_compare_names_a_missing_second_block():
    """(17,16,9) has 272 elements: a launch of one block of 256 leaves elements 256..271 at their input values."""
    m, n, c, want = _gemm_two_blocks()
    got = want.copy()
    gv, cv = ds.view(got, c["ldc"], m, n), ds.view(c["C"], c["ldc"], m, n)
    for e in range(256, m * n):
        gv[e % m, e // m] = cv[e % m, e // m]
    f = ds.compare(got, want, c["ldc"], m, n)
    assert (f["count"], f["where"], f["element"], f["row"], f["col"]) == (m * n - 256, "entry", 256, 256 % m, 256 // m)


def test_compare_names_unscaled_rows_of_a_cholesky_column():
    """n = 300: a column loop that takes one step of 256 threads leaves rows >= j + 256 of column j unscaled (and not
    updated); the first such row is row 256 of column 0."""
    n = 300
    for padded in (False, True):
        buf, lda = ds.potrf_case(n, padded)
        _, want = ds.potrf_expected(n, padded)
        got = want.copy()
        gv, wv = ds.view(got, lda, n, n), ds.view(want, lda, n, n)
        for j in range(n - 256):
            gv[j + 256:, j] = wv[j + 256:, j] * wv[j, j]   # (scaled back: what the division had found)
        f = ds.compare(got, want, lda, n, n)
        assert (f["where"], f["row"], f["col"], f["element"]) == ("entry", 256, 0, 256)
        assert f["count"] == (n - 256) * (n - 255) // 2


def test_compare_names_unsolved_right_hand_sides():
    """nrhs = 65: a launch of one block of 64 leaves right-hand side 64 as it came."""
    n, nrhs = 40, 65
    Lb, ldl, Bb, ldb = ds.potrs_case(n, nrhs)
    for which in ds.POTRS_WHICH:
        want = ds.potrs_ref(n, nrhs, Lb, ldl, Bb, ldb, which)
        got = want.copy()
        ds.view(got, ldb, n, nrhs)[:, 64:] = ds.view(Bb, ldb, n, nrhs)[:, 64:]
        f = ds.compare(got, want, ldb, n, nrhs)
        assert (f["count"], f["where"], f["row"], f["col"], f["element"]) == (n, "entry", 0, 64, 64 * n)


def test_compare_names_a_transposed_read():
    """L[i, j] read for L[j, i] in the transposed sweep: with NaN in the strict upper triangle every entry above the
    last becomes NaN; with the triangle mirrored (a symmetric-looking L) nothing would show, so the cases keep NaN
    there."""
    n, nrhs = 40, 3
    Lb, ldl, Bb, ldb = ds.potrs_case(n, nrhs)
    want = ds.potrs_ref(n, nrhs, Lb, ldl, Bb, ldb, 2)
    got = Bb.copy()
    X, Lv = ds.view(got, ldb, n, nrhs), ds.view(Lb, ldl, n, n)
    with np.errstate(all="ignore"):
        for j in range(n - 1, -1, -1):
            xj = X[j, :] / Lv[j, j]
            X[j, :] = xj
            X[:j, :] = X[:j, :] - Lv[:j, j][:, None] * xj[None, :]   # the wrong triangle
    f = ds.compare(got, want, ldb, n, nrhs)
    assert (f["where"], f["row"], f["col"], f["count"]) == ("entry", 0, 0, (n - 1) * nrhs)
    assert np.isnan(f["got"]) and not np.isnan(f["want"])


def test_compare_reports_a_length_mismatch():
    f = ds.compare(np.zeros(5), np.zeros(6), 3, 3, 2)
    assert f is not None and f["where"] == "shape"


# ------------------------------------------------------------------------------------------- (3) the stage schedule
@pytest.mark.parametrize("n,m,N", ds.STAGE_SHAPES)
def test_oracle_stage_schedule_reproduces_oracle_solve(ndlqr, oracle, n, m, N):
    """The oracle side of the lockstep replay of test_gpu_stage_shapes.py -- stage_schedule driven through oracle_apply --
    ends with the factors and the solution of oracle.solve (the oracle's own level loop, one thread), bit for bit."""
    _, prob = ds.stage_problem(ndlqr, n, m, N)
    want_soln, want_fact, _, fails = oracle.solve(prob, 1, want_fact=True)
    assert fails == 0
    o = oracle.solver(prob)
    calls = 0
    for _, _, ops in ds.stage_schedule(N):
        for op in ops:
            ds.oracle_apply(oracle.L, o.h, op)
            calls += 1
    assert ds.compare(o.fact(), want_fact, want_fact.size, want_fact.size, 1) is None
    assert ds.compare(o.soln(), want_soln, want_soln.size, want_soln.size, 1) is None
    assert oracle.L.oracle_chol_failures(o.h) == 0
    res, bnorm = oracle.kkt_residual(prob, o.soln()[: prob.nvars])
    assert res <= 1e-9 * max(1.0, bnorm)
    print("stage schedule (%d,%d,%d): %d stage calls" % (n, m, N, calls))

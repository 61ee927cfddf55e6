"""Restatements, case tables and the comparison routine for the dense Matrix* / clap_* helpers (ndlqr_hip_gemm,
ndlqr_hip_potrf_lower, ndlqr_hip_potrs_lower, ndlqr_hip_trsv_lower: csrc/kernels_dense.hpp) and the stage schedule that
drives the stage functions of csrc/stages.c in lockstep with the oracle. Test infrastructure; no GPU and no import of
the package.

The restatements are float64 numpy in the kernels' operation order: vectorised over the independent index (rows, or
right-hand sides) and sequential over the dependent one, so every element sees the kernel's exact sequence of correctly
rounded + - x / sqrt (numpy's elementwise ufuncs do not fuse a product into a sum). They work on column-major buffers
with an explicit leading dimension -- a buffer holds ld * (cols - 1) + rows doubles -- and never touch what lies
between the rows of a column and the leading dimension (the padding), nor the strict upper triangle of a triangular
operand. The device is held to them bit for bit: compare() looks at every double of the buffer as a uint64.
"""
import functools

import numpy as np

NAN = np.float64(np.nan)


# ------------------------------------------------------------------------------------------- buffers
def buf_len(ld, rows, cols):
    return ld * (cols - 1) + rows


def view(buf, ld, rows, cols):
    """(rows, cols) view of the column-major buffer `buf` with leading dimension `ld` (writes go to `buf`)."""
    assert buf.dtype == np.float64 and buf.ndim == 1 and buf.size >= buf_len(ld, rows, cols) and ld >= rows
    return np.lib.stride_tricks.as_strided(buf, shape=(rows, cols), strides=(8, 8 * ld), writeable=True)


def pack(a, ld, fill=NAN):
    """Column-major buffer of the 2-D array `a` with leading dimension `ld`; the padding holds `fill`."""
    a = np.asarray(a, dtype=np.float64)
    rows, cols = a.shape
    buf = np.full(buf_len(ld, rows, cols), fill, dtype=np.float64)
    view(buf, ld, rows, cols)[:, :] = a
    return buf


# ------------------------------------------------------------------------------------------- restatements
def gemm_ref(tA, tB, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc):
    """dense_gemm: acc = C * beta, then for p ascending acc = acc + (alpha * a) * b. Returns the new C buffer."""
    out = C.copy()
    Cv = view(out, ldc, m, n)
    with np.errstate(all="ignore"):
        acc = Cv * np.float64(beta)
        if k > 0:
            Av = view(A, lda, k, m).T if tA else view(A, lda, m, k)   # op(A): (m, k)
            Bv = view(B, ldb, n, k).T if tB else view(B, ldb, k, n)   # op(B): (k, n)
            for p in range(k):
                acc = acc + (np.float64(alpha) * Av[:, p])[:, None] * Bv[p, :][None, :]
    Cv[:, :] = acc
    return out


def potrf_ref(n, A, lda):
    """dense_potrf: per column j, acc = acc - A[i,k] * A[j,k] for k ascending (rows i >= j), then the pivot test
    !(p > 0), then the division by sqrt(p). Returns (info, buffer): info = 0, or j + 1 with the matrix as the kernel
    leaves it -- columns < j finished, column j updated and not scaled, the rest untouched."""
    out = A.copy()
    Av = view(out, lda, n, n)
    with np.errstate(all="ignore"):
        for j in range(n):
            acc = Av[j:, j].copy()
            for k in range(j):
                acc = acc - Av[j:, k] * Av[j, k]
            Av[j:, j] = acc
            pivot = Av[j, j]
            if not (pivot > 0.0):
                return j + 1, out
            Av[j:, j] = acc / np.sqrt(pivot)
    return 0, out


def potrs_ref(n, nrhs, L, ldl, B, ldb, which):
    """dense_potrs: column-oriented forward substitution (which != 2), then the transposed one (which != 1), every
    right-hand side on its own. Returns the new B buffer."""
    out = B.copy()
    X = view(out, ldb, n, nrhs)
    Lv = view(L, ldl, n, n)
    with np.errstate(all="ignore"):
        if which != 2:
            for j in range(n):
                xj = X[j, :] / Lv[j, j]
                X[j, :] = xj
                X[j + 1:, :] = X[j + 1:, :] - Lv[j + 1:, j][:, None] * xj[None, :]
        if which != 1:
            for j in range(n - 1, -1, -1):
                xj = X[j, :] / Lv[j, j]
                X[j, :] = xj
                X[:j, :] = X[:j, :] - Lv[j, :j][:, None] * xj[None, :]
    return out


# ------------------------------------------------------------------------------------------- comparison
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def compare(got, want, ld, rows, cols):
    """Bit comparison of two column-major buffers over every double, padding included. None when they are equal; else
    a dict that locates the difference: `count` differing doubles, and of the first one (in buffer order) `offset`,
    `row`, `col`, `where` ('entry' or 'padding'), `element` (row + rows * col, the kernels' element number; None in
    the padding), `got`, `want` and their bits in hex."""
    got = np.ascontiguousarray(got, dtype=np.float64)
    want = np.ascontiguousarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return dict(count=-1, where="shape", offset=None, row=None, col=None, element=None, got=got.shape, want=want.shape,
                    got_bits=None, want_bits=None)
    diff = np.flatnonzero(bits(got) != bits(want))
    if diff.size == 0:
        return None
    off = int(diff[0])
    row, col = off % ld, off // ld
    inside = row < rows and col < cols
    return dict(count=int(diff.size), where="entry" if inside else "padding", offset=off, row=row, col=col,
                element=row + rows * col if inside else None, got=float(got[off]), want=float(want[off]),
                got_bits="%016x" % int(bits(got)[off]), want_bits="%016x" % int(bits(want)[off]))


def describe(found):
    if found is None:
        return "equal"
    if found["where"] == "shape":
        return "buffers of %s and %s doubles" % (found["got"], found["want"])
    return ("%d doubles differ; first at offset %d = %s (row %d, col %d%s): got %r [%s], want %r [%s]"
            % (found["count"], found["offset"], found["where"], found["row"], found["col"],
               "" if found["element"] is None else ", element %d" % found["element"],
               found["got"], found["got_bits"], found["want"], found["want_bits"]))


def assert_bits(got, want, ld, rows, cols, what=""):
    found = compare(got, want, ld, rows, cols)
    assert found is None, "%s: %s" % (what, describe(found))


# ------------------------------------------------------------------------------------------- case tables
GEMM_SHAPES = [(5, 4, 7), (16, 16, 0), (17, 16, 9), (1, 300, 3), (300, 1, 3), (33, 31, 40)]
GEMM_TRANSPOSES = [(0, 0), (0, 1), (1, 0), (1, 1)]
GEMM_SCALARS = [(0.7, -1.3), (1.0, 0.0), (0.0, 1.0)]
POTRF_SIZES = [1, 2, 64, 255, 256, 257, 300]
POTRS_N = [1, 40, 257]
POTRS_NRHS = [1, 64, 65, 130]
POTRS_WHICH = [0, 1, 2]


def _seed(*key):
    return np.random.default_rng([abs(int(x)) for x in key])


def gemm_case(m, n, k, tA, tB, padded):
    """Operands of one product: dict with A, B, C (buffers), lda, ldb, ldc and the stored shapes. padded: lda = Ar + 3,
    ldb = Br + 2, ldc = m + 5 with NaN in the padding rows; else the leading dimensions are the row counts. k = 0 gives
    one-double operands A and B that nothing may read (NaN)."""
    rng = _seed(1, m, n, k, tA, tB, padded)
    Ar, Ac = (k, m) if tA else (m, k)
    Br, Bc = (n, k) if tB else (k, n)
    lda, ldb, ldc = (Ar + 3, Br + 2, m + 5) if padded else (max(Ar, 1), max(Br, 1), m)
    if k > 0:
        A = pack(rng.standard_normal((Ar, Ac)), lda)
        B = pack(rng.standard_normal((Br, Bc)), ldb)
    else:
        A = np.full(1, NAN)
        B = np.full(1, NAN)
    C = pack(rng.standard_normal((m, n)), ldc)
    return dict(A=A, B=B, C=C, lda=lda, ldb=ldb, ldc=ldc, Ar=Ar, Ac=Ac, Br=Br, Bc=Bc)


def spd(n, rng):
    """G G' + n I."""
    G = rng.standard_normal((n, n))
    return G @ G.T + n * np.eye(n)


def potrf_failures(n):
    """Names of the failure cases at size n: the diagonal entry at j made negative for j in {0, n // 2, n - 1}, one
    exactly zero pivot (a zero row and column) and one NaN on the diagonal."""
    return ["neg%d" % j for j in sorted({0, n // 2, n - 1})] + ["zero", "nan"]


def potrf_case(n, padded, failure=None):
    """(buffer, lda): an SPD matrix in its lower triangle, NaN in the strict upper triangle (and in the padding when
    padded: lda = n + 3). `failure`: one of potrf_failures(n)."""
    rng = _seed(2, n, padded)
    a = spd(n, rng)
    if failure is not None:
        if failure.startswith("neg"):
            j = int(failure[3:])
            a[j, j] = -a[j, j]
        elif failure == "zero":
            j = n // 2
            a[j, :] = 0.0
            a[:, j] = 0.0
        elif failure == "nan":
            j = n // 2
            a[j, j] = NAN
        else:
            raise ValueError(failure)
    a[np.triu_indices(n, 1)] = NAN
    lda = n + 3 if padded else n
    return pack(a, lda), lda


@functools.lru_cache(maxsize=None)
def _potrf_expected(n, padded, failure):
    buf, lda = potrf_case(n, padded, failure)
    info, out = potrf_ref(n, buf, lda)
    out.setflags(write=False)
    return info, out


def potrf_expected(n, padded, failure=None):
    """(info, buffer) of potrf_ref on potrf_case(n, padded, failure); computed once, read-only."""
    return _potrf_expected(n, bool(padded), failure)


def potrs_case(n, nrhs):
    """(L, ldl, B, ldb): a lower Cholesky factor with ldl = n + 3 and right-hand sides with ldb = n + 2, NaN in the
    padding and in the strict upper triangle of L."""
    rng = _seed(3, n, nrhs)
    low = np.linalg.cholesky(spd(n, rng))
    low[np.triu_indices(n, 1)] = NAN
    return pack(low, n + 3), n + 3, pack(rng.standard_normal((n, nrhs)), n + 2), n + 2


# ------------------------------------------------------------------------------------------- stage schedule
STAGE_SHAPES = [(2, 1, 2), (3, 2, 4), (5, 7, 8), (6, 3, 8), (12, 4, 16), (17, 3, 4)]
STAGE_SEED = 2024


def stage_schedule(N):
    """The level-synchronous schedule of a solve as a list of phases (name, level, ops): every op is a tuple of plain
    integers that the two drivers -- oracle_apply below, the drop-in stage functions in test_gpu_stage_shapes.py --
    turn into one stage call each. Factor phase per level: the inner products of every separator of the level into every
    level from it upwards, the separator Cholesky, the solve of the upper levels' columns by it, the Schur update of
    every knot at every upper level; then the solution phase per level with the right-hand side in their place."""
    K = N.bit_length() - 1
    assert N == 1 << K and K >= 1
    phases = [("leaves", -1, [("leaf", k) for k in range(N)])]
    for level in range(K):
        leaves = range(1 << (K - level - 1))
        uppers = range(level + 1, K)
        phases.append(("inner", level, [("inner", leaf, level, up) for leaf in leaves for up in range(level, K)]))
        phases.append(("chol", level, [("chol", leaf, level) for leaf in leaves]))
        phases.append(("cholsolve", level, [("cholsolve", leaf, level, up) for leaf in leaves for up in uppers]))
        phases.append(("schur", level, [("schur", k, level, up) for k in range(N) for up in uppers]))
    for level in range(K):
        leaves = range(1 << (K - level - 1))
        phases.append(("rhs-inner", level, [("rhs-inner", leaf, level) for leaf in leaves]))
        phases.append(("rhs-cholsolve", level, [("rhs-cholsolve", leaf, level) for leaf in leaves]))
        phases.append(("rhs-schur", level, [("rhs-schur", k, level) for k in range(N)]))
    return phases


def oracle_apply(OL, h, op):
    """One op of stage_schedule on the oracle solver `h` (OL: the oracle library)."""
    kind = op[0]
    if kind == "leaf":
        OL.oracle_solve_leaf(h, op[1])
    elif kind in ("inner", "cholsolve", "rhs-inner", "rhs-cholsolve", "chol"):
        leaf, level = op[1], op[2]
        index = OL.oracle_index_from_leaf(leaf, level)
        if kind == "inner":
            OL.oracle_inner_product(h, 0, index, level, op[3])
        elif kind == "chol":
            OL.oracle_factor_separator(h, leaf, level)
        elif kind == "cholsolve":
            OL.oracle_solve_chol_factor(h, index, level, op[3])
        elif kind == "rhs-inner":
            OL.oracle_inner_product(h, 1, index, level, 0)
        else:
            OL.oracle_solve_chol_rhs(h, index, level)
    elif kind in ("schur", "rhs-schur"):
        k, level = op[1], op[2]
        index = OL.oracle_index_at_level(k, level)
        calc = OL.oracle_should_calc_lambda(index, level, k)
        if kind == "schur":
            OL.oracle_update_schur(h, 0, index, k, level, op[3], calc)
        else:
            OL.oracle_update_schur(h, 1, index, k, level, 0, calc)
    else:
        raise ValueError(op)


def stage_problem(ndlqr, n, m, N):
    """(arrays of generate_synthetic, support.Problem) of the stage shape (n, m, N) at the fixed seed."""
    from support import Problem
    g = ndlqr.generate_synthetic(n, m, N, STAGE_SEED)
    return g, Problem(n, m, N, g["A"], g["B"], g["Q"], g["R"], g["q"], g["r"], g["d"], g["x0"])

"""GPU: the stage functions of csrc/stages.c (ndlqr_SolveLeaf, ndlqr_FactorInnerProduct, ndlqr_SolveCholeskyFactor,
ndlqr_UpdateShurFactor, with the separator Cholesky and its solves through the Matrix* helpers) driven through the
whole level-synchronous schedule from Python, in lockstep with the oracle's stage calls, at shapes beyond the 6-3-8
fixture: more inputs than states, more than 16 states, the shortest horizon, every level of a 16-knot tree. After the
leaves, after every phase of every level and at the end the factor and solution slabs of the drop-in solver equal the
oracle's (the dense helpers keep the reference's operation order, so equal means equal values in every entry); the
index functions agree for every argument the schedule uses; the solution meets the parity contract."""
import ctypes as C

import numpy as np
import pytest

import dense_support as ds

pytestmark = pytest.mark.gpu
dp = C.POINTER(C.c_double)


def _dropin_solver(L, g, n, m, N):
    """The reference's call sequence: ndlqr_NewLQRProblem, ndlqr_InitializeLQRData per knot, ndlqr_InitializeLQRProblem,
    ndlqr_NewNdLqrSolver, ndlqr_InitializeWithLQRProblem. Returns (solver, problem)."""
    prob = L.ndlqr_NewLQRProblem(n, m, N)
    assert prob
    ptr = lambda a: a.ctypes.data_as(dp)  # noqa: E731
    keep = []
    for k in range(N):
        arrs = [np.ascontiguousarray(g[f][k], dtype=np.float64) for f in ("Q", "R", "q", "r", "A", "B", "d")]
        keep += arrs
        Q, R, q, r, A, B, d = arrs
        assert L.ndlqr_InitializeLQRData(prob.contents.lqrdata[k], ptr(Q), ptr(R), ptr(q), ptr(r), 0.0, ptr(A), ptr(B), ptr(d)) == 0
    x0 = np.ascontiguousarray(g["x0"], dtype=np.float64)
    assert L.ndlqr_InitializeLQRProblem(prob, ptr(x0), prob.contents.lqrdata) == 0
    solver = L.ndlqr_NewNdLqrSolver(n, m, N)
    assert solver
    assert L.ndlqr_InitializeWithLQRProblem(prob, solver) == 0
    return solver, prob


class DropIn:
    """One op of dense_support.stage_schedule through the drop-in stage functions, with the index functions checked
    against the oracle's for the arguments of that op."""

    def __init__(self, ndlqr, L, OL, solver):
        self.nd, self.L, self.OL, self.solver, self.s = ndlqr, L, OL, solver, solver.contents
        self.tree = C.byref(self.s.tree)

    def _factor(self, nddata, index, level):
        f = C.POINTER(self.nd.NdFactor)()
        assert self.L.ndlqr_GetNdFactor(nddata, index, level, C.byref(f)) == 0
        return f.contents

    def _info(self, leaf, level):
        info = C.POINTER(self.nd.api.CholeskyInfo)()
        assert self.L.ndlqr_GetSFactorization(self.s.cholfacts, leaf, level, C.byref(info)) == 0
        return info

    def _separator(self, leaf, level):
        index = self.L.ndlqr_GetIndexFromLeaf(self.tree, leaf, level)
        assert index == self.OL.oracle_index_from_leaf(leaf, level), (leaf, level)
        return index

    def _knot(self, k, level):
        index = self.L.ndlqr_GetIndexAtLevel(self.tree, k, level)
        assert index == self.OL.oracle_index_at_level(k, level), (k, level)
        calc = self.L.ndlqr_ShouldCalcLambda(self.tree, index, k)
        assert bool(calc) == bool(self.OL.oracle_should_calc_lambda(index, level, k)), (index, level, k)
        return index, calc

    def apply(self, op):
        L, s = self.L, self.s
        kind = op[0]
        if kind == "leaf":
            assert L.ndlqr_SolveLeaf(self.solver, op[1]) == 0
        elif kind == "inner":
            _, leaf, level, upper = op
            assert L.ndlqr_FactorInnerProduct(s.data, s.fact, self._separator(leaf, level), level, upper) == 0
        elif kind == "chol":
            _, leaf, level = op
            sep = self._factor(s.fact, self._separator(leaf, level) + 1, level)
            info = self._info(leaf, level)
            assert L.MatrixCholeskyFactorizeWithInfo(C.byref(sep.lambda_), info) == 0
            assert (info.contents.success, info.contents.lib, info.contents.uplo) == (0, b"H", b"L")
        elif kind == "cholsolve":
            _, leaf, level, upper = op
            assert L.ndlqr_SolveCholeskyFactor(s.fact, self._info(leaf, level), self._separator(leaf, level), level, upper) == 0
        elif kind == "schur":
            _, k, level, upper = op
            index, calc = self._knot(k, level)
            assert L.ndlqr_UpdateShurFactor(s.fact, s.fact, index, k, level, upper, calc) == 0
        elif kind == "rhs-inner":
            _, leaf, level = op
            assert L.ndlqr_FactorInnerProduct(s.data, s.soln, self._separator(leaf, level), level, 0) == 0
        elif kind == "rhs-cholsolve":
            _, leaf, level = op
            index = self._separator(leaf, level)
            sep = self._factor(s.fact, index + 1, level)
            rhs = self._factor(s.soln, index + 1, 0)
            assert L.MatrixCholeskySolveWithInfo(C.byref(sep.lambda_), C.byref(rhs.lambda_), self._info(leaf, level)) == 0
        elif kind == "rhs-schur":
            _, k, level = op
            index, calc = self._knot(k, level)
            assert L.ndlqr_UpdateShurFactor(s.fact, s.soln, index, k, level, 0, calc) == 0
        else:
            raise ValueError(op)


@pytest.mark.parametrize("n,m,N", ds.STAGE_SHAPES)
def test_stage_schedule_in_lockstep_with_the_oracle(ndlqr, oracle, n, m, N):
    L, OL = ndlqr.lib(), oracle.L
    g, pyprob = ds.stage_problem(ndlqr, n, m, N)
    solver, prob = _dropin_solver(L, g, n, m, N)
    s = solver.contents
    o = oracle.solver(pyprob)
    drop = DropIn(ndlqr, L, OL, solver)
    fact = lambda: s.fact.contents.numpy()  # noqa: E731
    soln = lambda: s.soln.contents.numpy()  # noqa: E731
    assert fact().size == o.fact().size and soln().size == o.soln().size
    assert np.array_equal(soln(), o.soln()), "the assembled right-hand side"
    calls = 0
    for name, level, ops in ds.stage_schedule(N):
        for op in ops:
            drop.apply(op)
            ds.oracle_apply(OL, o.h, op)
        calls += len(ops)
        assert np.array_equal(fact(), o.fact()), "factors after phase %s of level %d" % (name, level)
        assert np.array_equal(soln(), o.soln()), "solution after phase %s of level %d" % (name, level)
    assert OL.oracle_chol_failures(o.h) == 0
    assert np.array_equal(fact(), o.fact()) and np.array_equal(soln(), o.soln())
    x = np.zeros(pyprob.nvars)
    assert L.ndlqr_CopySolution(solver, x.ctypes.data_as(dp)) == pyprob.nvars
    assert np.array_equal(x, o.soln()[: pyprob.nvars])
    res, bnorm = oracle.kkt_residual(pyprob, x)
    print("stage shape (%d,%d,%d): %d stage calls, KKT residual %.3e (bar %.3e)" % (n, m, N, calls, res, 1e-9 * max(1.0, bnorm)))
    assert res <= 1e-9 * max(1.0, bnorm)
    L.ndlqr_FreeNdLqrSolver(solver)
    L.ndlqr_FreeLQRProblem(prob)

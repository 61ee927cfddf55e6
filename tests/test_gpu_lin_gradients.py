"""Gradients through the solve with linear inequality constraints on the device (ndlqr_SolveBatchLinAdjoint,
ndlqr_BatchConstraintGradients, lqr_solve_constrained) against lin_grad_support.py: the numpy
restatement of the adjoint iteration in float64 and in longdouble, and the direct solve of the active-set system. The cases
are those of lin_support.case: batch 3, shapes (6,3), (12,4), (7,9), (20,5), horizons 2, 5, 8, 16, rho = 1, alpha = 1.6;
default and strict mode; g seeded standard normal over the whole packed vector.

Four of the 48 forwards end as status 2 at rho = 1 -- problems 1 and 2 of (12,4,2), problems 0 and 2 of (20,5,2)
(lin_grad_support.NOT_CONVERGED). The value checks leave out exactly these four; on them the statuses and the finiteness of
the outputs are checked.

Bars. First iterations, per field and entry: the forward's multiple (test_gpu_lin.first_mult, imported) x the float64
restatement's own error on the same case, at least 16 eps of the field's largest entry -- the re-solve is the forward's,
on the same factorisation. Converged adjoint: |K w + G'nu - g| and |G_A w| to lin_support.kkt_bar built from the adjoint's
residual row, |w - w_direct| to |M_A^-1|_inf times the sum of the two. Constraint gradients: recomputed in numpy from the
device's own z*, w, mu, nu and codes, 2 eps (|mu w| + |nu z|) per entry in default mode, bit for bit in strict mode."""
import functools

import numpy as np
import pytest

import cost_support as cs
import lin_grad_support as lg
import lin_support as ls
from test_gpu_lin import SET, constrained_solver, fields, first_mult, modes, ratio_of

pytestmark = pytest.mark.gpu

EPS = lg.EPS
CASES = lg.CASES
LD = np.longdouble


def solved(ndlqr, cases, flags, **kw):
    bs = constrained_solver(ndlqr, cases, flags, **kw)
    iters, status = bs.solve_constrained(max_iter=2000, **SET)
    return bs, iters, status


def adj_set(**kw):
    return dict(dict(alpha=ls.ALPHA, eps_abs=1e-8, eps_rel=1e-8), **kw)


@functools.lru_cache(maxsize=None)
def first_ld(n, m, N):
    """the first three iterates of the longdouble adjoint restatement, per problem of the case (None: forward status 2)"""
    out = []
    for c in lg.case(n, m, N):
        trace = []
        if c["ref"]["status"] == 1:
            lg.adjoint_admm(c["p"], c["C"], c["D"], c["lo"], c["hi"], c["codes"], c["g"], max_iter=3, dtype=LD, trace=trace)
        out.append(trace or None)
    return out


# ---------------------------------------------------------------------------- 1: codes and the first iterations
def first_adjoint_ratios(ndlqr, n, m, N, flags):
    """largest device error / the float64 restatement's own error over the adjoint's v, nu and the fields of w after
    max_iter = 1, 2, 3 (the codes are compared on the way, on all problems)"""
    cases = lg.case(n, m, N)
    exact = first_ld(n, m, N)
    G = np.stack([c["g"] for c in cases])
    bs, _, fstatus = solved(ndlqr, cases, flags)
    worst = 0.0
    for it in (1, 2, 3):
        iters, status = bs.solve_constrained_adjoint(G, max_iter=it, **adj_set())
        codes = bs.constraint_codes()
        W, nu, v = bs.adjoint(), bs.constraint_adjoint_multipliers(), bs.constraint_adjoint_iterate()
        assert np.isfinite(W).all() and np.isfinite(nu).all() and np.isfinite(v).all()
        for i, c in enumerate(cases):
            assert np.array_equal(codes[i], c["codes"]), (n, m, N, i, int((codes[i] != c["codes"]).sum()))
            if lg.skipped(n, m, N, i):
                assert fstatus[i] == 2
                continue
            assert iters[i] == it and status[i] == 2, (iters, status)
            e, f = exact[i][it - 1], c["adj_first"][it - 1]
            fixed = c["codes"] >= 2
            got = dict(v=v[i], nu=nu[i], **fields(W[i], n, m, N))
            ref = dict(v=e["v"], nu=np.where(fixed, ls.RHO * e["y"], 0), **fields(e["z"], n, m, N))
            own = dict(v=f["v"], nu=np.where(fixed, ls.RHO * f["y"], 0), **fields(f["z"], n, m, N))
            worst = max(worst, ratio_of(got, ref, own))
    bs.close()
    return worst


@pytest.mark.parametrize("n,m,N", CASES)
def test_codes_and_first_iterations_per_entry(ndlqr, n, m, N):
    ratios = {flags: first_adjoint_ratios(ndlqr, n, m, N, flags) for flags in modes(ndlqr)}
    for flags, ratio in ratios.items():
        print("adjoint first iterations", (n, m, N), "flags", flags, "largest error / restatement's own: %.2f" % ratio)
    for flags, ratio in ratios.items():
        assert ratio <= first_mult(ndlqr, flags), (flags, ratio)


# ---------------------------------------------------------------------------- 2: the converged adjoint
@pytest.mark.parametrize("n,m,N", CASES)
def test_converged_adjoint(ndlqr, n, m, N):
    cases = lg.case(n, m, N)
    G = np.stack([c["g"] for c in cases])
    for flags in modes(ndlqr):
        bs, _, fstatus = solved(ndlqr, cases, flags)
        iters, status = bs.solve_constrained_adjoint(G, max_iter=2000, **adj_set())
        W, nu, res = bs.adjoint(), bs.constraint_adjoint_multipliers(), bs.constraint_adjoint_residuals()
        bs.close()
        print("converged adjoint", (n, m, N), "flags", flags, "device", list(iters), list(status), "restatement",
              [c["adj"]["iters"] if "adj" in c else None for c in cases])
        assert np.isfinite(W).all() and np.isfinite(nu).all() and np.isfinite(res).all()
        for i, c in enumerate(cases):
            if lg.skipped(n, m, N, i):
                assert fstatus[i] == 2 and status[i] in (1, 2)
                continue
            a = c["adj"]
            assert status[i] == a["status"] == 1 and abs(int(iters[i]) - a["iters"]) <= 2, (i, iters, status, a["iters"])
            bar = lg.adjoint_bar(c, W[i], res[i])
            K, _ = ls.kkt_ld({k: np.asarray(c["p"][k], dtype=LD) for k in cs.NAMES})
            wl = W[i].astype(LD)
            stat = float(np.abs(K @ wl + ls.perturbation(c["p"], c["C"], c["D"], nu[i].astype(LD)) - c["g"]).max())
            rows = ls.rows_of(c["p"], c["C"], c["D"], wl)
            feas = float(np.abs(rows[c["codes"] >= 2]).max(initial=0.0))
            err = float(np.abs(W[i] - c["w_direct"]).max())
            print("  problem", i, "stationarity %.3e (bar %.3e) |G_A w| %.3e (bar %.3e) |w - w_direct| %.3e (bar %.3e)"
                  % (stat, bar["stationarity"], feas, bar["feasibility"], err, bar["w"]))
            assert stat <= bar["stationarity"], (stat, bar)
            assert feas <= bar["feasibility"], (feas, bar)
            assert err <= bar["w"], (err, bar)
            assert np.array_equal(nu[i][c["codes"] < 2], np.zeros(int((c["codes"] < 2).sum())))


# ---------------------------------------------------------------------------- 3: the constraint gradients, entry by entry
def math_rows(flat, p, width):
    """[.., N, p*width] column-major per knot -> [.., N, p, width]"""
    return flat.reshape(*flat.shape[:-1], width, p).swapaxes(-1, -2)


@pytest.mark.parametrize("n,m,N", [(6, 3, 5), (12, 4, 8), (7, 9, 16), (20, 5, 2)])
def test_constraint_gradients_per_entry(ndlqr, n, m, N):
    cases = lg.case(n, m, N)
    p = m + 2
    G = np.stack([c["g"] for c in cases])
    for flags in modes(ndlqr):
        strict = bool(flags & ndlqr.FLAG_STRICT_FP)
        bs, _, _ = solved(ndlqr, cases, flags)
        bs.solve_constrained_adjoint(G, max_iter=2000, **adj_set())
        Z, W, mu, nu, codes = bs.solutions(), bs.adjoint(), bs.constraint_multipliers(), bs.constraint_adjoint_multipliers(), bs.constraint_codes()
        got = bs.constraint_gradients()
        s1, s2 = bs.constraint_gradients(summed=True), bs.constraint_gradients(summed=True)
        bs.close()
        for k in ("C", "D", "lo", "hi"):
            assert np.isfinite(got[k]).all() and np.array_equal(s1[k], s2[k]), k  # (two calls: the same bits)
        gC, gD = math_rows(got["C"], p, n), math_rows(got["D"], p, m)
        total = {k: np.zeros_like(s1[k]) for k in s1}
        terms = {k: np.zeros_like(s1[k]) for k in s1}
        for i, c in enumerate(cases):
            for k in total:  # (the per-problem results added in order)
                total[k] = total[k] + got[k][i]
                terms[k] = terms[k] + np.abs(got[k][i])
            if lg.skipped(n, m, N, i):
                continue
            act = codes[i] >= 2
            _, x, u = cs.split(Z[i], n, m, N)
            _, wx, wu = cs.split(W[i], n, m, N)
            mu_, nu_ = np.where(act, mu[i], 0.0), np.where(act, nu[i], 0.0)
            for name, dev, wj, zj in (("C", gC[i], wx, x), ("D", gD[i], wu, u)):
                t = mu_[:, :, None] * wj[:, None, :]
                s = nu_[:, :, None] * zj[:, None, :]
                ref = np.where(act[:, :, None], -(t + s), 0.0)
                if name == "D":
                    ref[N - 1] = 0.0
                    assert np.array_equal(dev[N - 1], np.zeros_like(dev[N - 1]))
                assert np.array_equal(dev[~act], np.zeros_like(dev[~act])), name  # (unbounded and free rows: exactly zero)
                if strict:
                    assert np.array_equal(dev, ref), (name, float(np.abs(dev - ref).max()))
                else:
                    assert (np.abs(dev - ref) <= 2 * EPS * (np.abs(t) + np.abs(s))).all(), (name, float(np.abs(dev - ref).max()))
            assert np.array_equal(got["lo"][i], np.where(codes[i] == 2, nu[i], 0.0))
            assert np.array_equal(got["hi"][i], np.where(codes[i] == 3, nu[i], 0.0))
            assert act.any()
        for k in total:
            assert (np.abs(s1[k] - total[k]) <= cs.BATCH * EPS * terms[k]).all(), k


# ---------------------------------------------------------------------------- 4: state rules
def test_the_forward_is_untouched(ndlqr):
    n, m, N = 12, 4, 8
    cases = lg.case(n, m, N)
    G = np.stack([c["g"] for c in cases])
    C, D, lo, hi = ls.flat_rows(cases)
    for flags in modes(ndlqr):
        a, it_a, st_a = solved(ndlqr, cases, flags)
        b, it_b, st_b = solved(ndlqr, cases, flags)
        before = (a.solutions(), a.constraint_multipliers(), a.constraint_residuals(), a.constraint_reduction(), a.factor_count())
        iters, status = a.solve_constrained_adjoint(G, max_iter=2000, **adj_set())
        assert (status == 1).all()
        a.constraint_gradients(); a.constraint_gradients(summed=True); a.adjoint()
        after = (a.solutions(), a.constraint_multipliers(), a.constraint_residuals(), a.constraint_reduction(), a.factor_count())
        assert before[4] == after[4]
        for k in range(3):
            assert np.array_equal(before[k], after[k]), k
        for k in before[3]:
            assert np.array_equal(before[3][k], after[3][k]), k
        # a second adjoint: the same bits; ndlqr_SolveBatchAdjoint keeps refusing
        W1, nu1 = a.adjoint(), a.constraint_adjoint_multipliers()
        a.solve_constrained_adjoint(G, max_iter=2000, **adj_set())
        assert np.array_equal(a.adjoint(), W1) and np.array_equal(a.constraint_adjoint_multipliers(), nu1)
        assert a.solve_adjoint(G) != 0 and a.L.ndlqr_hip_last_error().decode().startswith("ndlqr_hip_solve_adjoint: ")
        assert "ndlqr_hip_solve_constrained" in a.L.ndlqr_hip_last_error().decode()
        # a warm-started forward after the adjoint equals one without it, in iterates and in counts
        for bs in (a, b):
            bs.set_constraint_bounds(1.05 * lo, 1.05 * hi)
        ra = a.solve_constrained(max_iter=2000, warm_start=True, **SET)
        rb = b.solve_constrained(max_iter=2000, warm_start=True, **SET)
        assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1]), (ra, rb)
        assert np.array_equal(a.solutions(), b.solutions()) and a.factor_count() == b.factor_count()
        ia, ib = a.constraint_reduction(), b.constraint_reduction()
        assert np.array_equal(ia["v"], ib["v"]) and np.array_equal(ia["y"], ib["y"])
        a.close(); b.close()


def test_a_forward_that_is_not_finite(ndlqr):
    n, m, N = 6, 3, 8
    cases = lg.case(n, m, N)
    G = np.stack([c["g"] for c in cases])
    bad = [dict(c) for c in cases]
    bad[1] = dict(bad[1], p=dict(bad[1]["p"], q=bad[1]["p"]["q"].copy()))
    bad[1]["p"]["q"][3, 2] = np.nan
    for flags in modes(ndlqr):
        good, _, _ = solved(ndlqr, cases, flags)
        it_g, st_g = good.solve_constrained_adjoint(G, max_iter=2000, **adj_set())
        Wg, gg = good.adjoint(), good.constraint_gradients()
        good.close()
        bs, _, fstatus = solved(ndlqr, bad, flags)
        assert fstatus[1] == 3
        iters, status = bs.solve_constrained_adjoint(G, max_iter=2000, **adj_set())
        assert status[1] == 3 and iters[1] == 0 and list(status[[0, 2]]) == [1, 1] and list(iters[[0, 2]]) == list(it_g[[0, 2]])
        W, got, summed, res = bs.adjoint(), bs.constraint_gradients(), bs.constraint_gradients(summed=True), bs.constraint_adjoint_residuals()
        bs.close()
        assert np.array_equal(W[1], np.zeros_like(W[1])) and np.array_equal(res[1], np.zeros(4))
        for k in got:
            assert np.array_equal(got[k][1], np.zeros_like(got[k][1])), k
            assert np.isfinite(summed[k]).all(), k
            for i in (0, 2):  # the others bit for bit as without it
                assert np.array_equal(got[k][i], gg[k][i]), (k, i)
        for i in (0, 2):
            assert np.array_equal(W[i], Wg[i])


def test_wide_bounds_give_the_plain_adjoint(ndlqr):
    """Bounds so wide that no row is active: every bounded row is free, nu = 0 and the converged w is the adjoint of the
    unconstrained problem, K w = g. Bar: |K^-1|_inf times the stationarity bound of lin_support.kkt_bar built from the
    adjoint's residual row, plus the same for the plain adjoint's own rounding (its residual row is zero)."""
    n, m, N = 6, 3, 8
    cases = lg.case(n, m, N)
    G = np.stack([c["g"] for c in cases])
    wide = np.full((cs.BATCH, N, m + 2), 1e4)
    for flags in modes(ndlqr):
        # (the plain adjoint needs a solver that keeps its factorisation; the constrained solve keeps its own either way)
        keep = ndlqr.FLAG_KEEP_FACT if flags & ndlqr.FLAG_STRICT_FP else ndlqr.FLAG_KEEP_RECORDS
        bs, _, fstatus = solved(ndlqr, cases, flags | keep, lo=-wide, hi=wide)
        assert (fstatus == 1).all()
        iters, status = bs.solve_constrained_adjoint(G, max_iter=2000, **adj_set())
        assert (status == 1).all(), (iters, status)
        W, nu, res, codes = bs.adjoint(), bs.constraint_adjoint_multipliers(), bs.constraint_adjoint_residuals(), bs.constraint_codes()
        assert (codes == 1).all() and np.array_equal(nu, np.zeros_like(nu))
        assert bs.solve() == 0 and bs.solve_adjoint(G) == 0, bs.L.ndlqr_hip_last_error().decode()
        Wp = bs.adjoint()
        with pytest.raises(RuntimeError, match="ndlqr_hip_constraint_gradients: no constrained adjoint"):
            bs.constraint_gradients()  # (a plain adjoint never feeds them)
        bs.close()
        for i, c in enumerate(cases):
            K, _ = cs.dense_kkt(c["p"])
            inv = float(np.abs(np.linalg.inv(K)).sum(axis=1).max())
            bar = inv * (ls.kkt_bar(c["p"], c["C"], c["D"], W[i], res[i])["stationarity"]
                         + ls.kkt_bar(c["p"], c["C"], c["D"], Wp[i], np.zeros(4))["stationarity"])
            err = float(np.abs(W[i] - Wp[i]).max())
            print("wide bounds", flags, i, "iterations", iters[i], "|w - w_plain| %.3e bar %.3e" % (err, bar))
            assert err <= bar, (err, bar)


# ---------------------------------------------------------------------------- 5: refusals by name
def test_refusals_by_name(ndlqr):
    n, m, N = 6, 3, 5
    cases = lg.case(n, m, N)
    G = np.stack([c["g"] for c in cases])
    C, D, lo, hi = ls.flat_rows(cases)
    adjoint = "ndlqr_hip_solve_constrained_adjoint: "
    not_latest = adjoint + "the resident solution is not that of the latest constrained solve"
    grads = "ndlqr_hip_constraint_gradients: "
    # not in constrained mode
    bs = ndlqr.BatchSolver(n, m, N, cs.BATCH)
    bs.initialize_flat_dense(*cs.flat([c["p"] for c in cases]))
    with pytest.raises(RuntimeError, match=adjoint + "the solver is not in constrained mode"):
        bs.solve_constrained_adjoint(G)
    with pytest.raises(RuntimeError, match=grads + "the solver is not in constrained mode"):
        bs.constraint_gradients()
    bs.close()
    bs = constrained_solver(ndlqr, cases)
    # before any constrained solve; after a plain solve
    with pytest.raises(RuntimeError, match=not_latest):
        bs.solve_constrained_adjoint(G)
    bs.solve_constrained(max_iter=2000, **SET)
    assert bs.solve() == 0
    with pytest.raises(RuntimeError, match=not_latest):
        bs.solve_constrained_adjoint(G)
    # bad settings
    bs.solve_constrained(max_iter=2000, **SET)
    for kw in (dict(alpha=2.5), dict(alpha=-1.0), dict(eps_abs=-1.0), dict(eps_rel=-1.0), dict(max_iter=-1), dict(check_every=-3)):
        with pytest.raises(RuntimeError, match=adjoint + "bad argument"):
            bs.solve_constrained_adjoint(G, **kw)
    # the constraint gradients and the read-outs before the adjoint
    for name, call in (("ndlqr_hip_constraint_gradients", bs.constraint_gradients),
                       ("ndlqr_hip_download_constraint_adjoint_multipliers", bs.constraint_adjoint_multipliers),
                       ("ndlqr_hip_download_constraint_adjoint_residuals", bs.constraint_adjoint_residuals),
                       ("ndlqr_hip_download_constraint_codes", bs.constraint_codes)):
        with pytest.raises(RuntimeError, match=name + ": no constrained adjoint of the resident solution"):
            call()
    iters, status = bs.solve_constrained_adjoint(G, max_iter=2000, **adj_set())
    assert (status == 1).all()
    bs.constraint_gradients()
    # ... and after a later solve
    bs.solve_constrained(max_iter=2000, **SET)
    with pytest.raises(RuntimeError, match=grads + "no constrained adjoint of the resident solution"):
        bs.constraint_gradients()
    with pytest.raises(RuntimeError, match="ndlqr_hip_download_adjoint: no adjoint of the resident solution"):
        bs.adjoint()
    # a new right-hand side, new bounds
    bs.solve_constrained_adjoint(G, max_iter=2000, **adj_set())
    _, _, _, _, _, q, r, d, x0 = cs.flat([c["p"] for c in cases])
    bs.set_rhs_flat(q, r, d, x0)
    with pytest.raises(RuntimeError, match=grads + "no constrained adjoint of the resident solution"):
        bs.constraint_gradients()
    with pytest.raises(RuntimeError, match=not_latest):
        bs.solve_constrained_adjoint(G)
    bs.solve_constrained(max_iter=2000, **SET)
    bs.solve_constrained_adjoint(G, max_iter=2000, **adj_set())
    bs.set_constraint_bounds(lo, hi)
    with pytest.raises(RuntimeError, match=grads + "no constrained adjoint of the resident solution"):
        bs.constraint_gradients()
    with pytest.raises(RuntimeError, match=not_latest):
        bs.solve_constrained_adjoint(G)
    # the C-level parameter gradients stay refused in dense-cost mode
    bs.solve_constrained(max_iter=2000, **SET)
    bs.solve_constrained_adjoint(G, max_iter=2000, **adj_set())
    with pytest.raises(RuntimeError, match="ndlqr_hip_gradients"):
        bs.gradients()
    # memory of another device: needs a second GPU. On a box with one MI355X, where the suite usually runs, these refusals
    # are NOT exercised (unverified there); the CallerArrays path they take is the one test_gpu_lin.py's refusals share.
    if ndlqr.device_count() > 1:
        import torch

        class Foreign:
            def __init__(self, a):
                self.t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:1")
                self.ptr, self.size = self.t.data_ptr(), self.t.numel()
        with pytest.raises(RuntimeError, match=adjoint + "g lies in the memory of another device"):
            bs.solve_constrained_adjoint(Foreign(G))
        bs.solve_constrained_adjoint(G, max_iter=2000, **adj_set())
        with pytest.raises(RuntimeError, match=grads + "an output lies in the memory of another device"):
            bs.constraint_gradients(out=dict(C=Foreign(np.zeros((cs.BATCH, N, (m + 2) * n)))))
    bs.close()


# ---------------------------------------------------------------------------- 6: lqr_solve_constrained
# The torch cases run in a child process, as those of test_gpu_box_gradients.py do: torch's HIP runtime has to be the
# first in its process.
def _run_case(name, *args):
    import json
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys, json; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import torch; torch.zeros(1, device='cuda')\n"
            "import rslqr_amd, test_gpu_lin_gradients as T\n"
            "T.%s(rslqr_amd, *json.loads(%r))\n"
            "print('case ok')\n" % (os.path.dirname(here), here, name, json.dumps(args)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "case ok" in r.stdout, (name, args, r.returncode, r.stdout[-2000:], r.stderr[-4000:])


@pytest.mark.parametrize("rows", ["per_problem", "shared"])
def test_torch_against_dense_active_set_reference(rows):
    _run_case("_case_dense_reference", rows)


def test_torch_backwards_in_reverse_order():
    _run_case("_case_backwards_in_reverse_order")


def test_torch_gradcheck():
    _run_case("_case_gradcheck")


def test_torch_raises_on_non_convergence():
    _run_case("_case_non_convergence")


NAMES13 = cs.NAMES + ("C", "D", "lo", "hi")
KW = dict(rho=ls.RHO, alpha=ls.ALPHA, eps_abs=1e-11, eps_rel=1e-11, max_iter=20000)


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _torch_case(n, m, N, rows, scale=1.0):
    """the thirteen leaves of lin_support.case(n, m, N) as torch tensors (math convention). rows == "shared": C, D of the
    first problem for all of them and bounds at 0.6 of the largest |C x + D u| any problem's unconstrained solution has, per
    row -- all four without a batch dimension. scale: a factor on q (another problem of the same shape)."""
    import torch
    cases = ls.case(n, m, N)
    arr = {k: np.stack([c["p"][k] for c in cases]) for k in cs.NAMES}
    if rows == "shared":
        C, D = cases[0]["C"], cases[0]["D"]
        fam = cs.family(n, m, N, "moderate")
        w = np.stack([np.abs(ls.rows_of(c["p"], C, D, np.asarray(fam["z"][i]))).max(axis=0) for i, c in enumerate(cases)])
        hi = np.broadcast_to(0.6 * w.max(axis=0), (N, m + 2)).copy()
        arr.update(C=C, D=D, lo=-hi, hi=hi)
    else:
        arr.update({k: np.stack([c[k] for c in cases]) for k in ("C", "D", "lo", "hi")})
    arr["q"] = arr["q"] * scale
    return {k: torch.tensor(np.ascontiguousarray(arr[k]), dtype=torch.float64, device="cuda", requires_grad=True) for k in NAMES13}


def _dense_active_solve(t, z_fwd, n, m, N, batch, tol=1e-7):
    """z* [batch, nvars] of the equality-constrained KKT system on the active set of z_fwd (the rows within tol of a bound),
    assembled in torch and solved by torch.linalg.solve: differentiable in the thirteen tensors"""
    import torch
    zb = 2 * n + m
    nv = zb * N - m
    per = dict(A=3, B=3, Q=3, H=3, R=3, q=2, r=2, d=2, x0=1, C=3, D=3, lo=2, hi=2)
    eye = torch.eye(n, dtype=torch.float64, device="cuda")
    zs, active = [], 0
    for b in range(batch):
        A, B, Q, H, R, q, r, d, x0, C, D, lo, hi = [t[k] if t[k].dim() == per[k] else t[k][b] for k in NAMES13]
        K = torch.zeros((nv, nv), dtype=torch.float64, device="cuda")
        rhs = torch.zeros(nv, dtype=torch.float64, device="cuda")
        K[0:n, n:2 * n] = -eye
        K[n:2 * n, 0:n] = -eye
        rhs[0:n] = -x0
        for k in range(N):
            xo, uo = k * zb + n, k * zb + 2 * n
            K[xo:xo + n, xo:xo + n] = 0.5 * (Q[k] + Q[k].T)
            rhs[xo:xo + n] = -q[k]
            if k == N - 1:
                break
            l1, x1 = (k + 1) * zb, (k + 1) * zb + n
            K[uo:uo + m, uo:uo + m] = 0.5 * (R[k] + R[k].T)
            K[xo:xo + n, uo:uo + m] = H[k]
            K[uo:uo + m, xo:xo + n] = H[k].T
            rhs[uo:uo + m] = -r[k]
            K[l1:l1 + n, xo:xo + n] = A[k]
            K[xo:xo + n, l1:l1 + n] = A[k].T
            K[l1:l1 + n, uo:uo + m] = B[k]
            K[uo:uo + m, l1:l1 + n] = B[k].T
            K[l1:l1 + n, x1:x1 + n] = -eye
            K[x1:x1 + n, l1:l1 + n] = -eye
            rhs[l1:l1 + n] = -d[k]
        Z = torch.nn.functional.pad(z_fwd[b], (0, m)).reshape(N, zb)
        rows, vals = [], []
        for k in range(N):
            w = C[k].detach() @ Z[k, n:2 * n] + (D[k].detach() @ Z[k, 2 * n:] if k < N - 1 else 0)
            for j in range(C.shape[1]):
                for side in (hi, lo):
                    if abs(float(w[j]) - float(side[k, j])) <= tol:
                        row = torch.zeros(nv, dtype=torch.float64, device="cuda")
                        row[k * zb + n:k * zb + 2 * n] = C[k, j]
                        if k < N - 1:
                            row[k * zb + 2 * n:k * zb + 2 * n + m] = D[k, j]
                        rows.append(row)
                        vals.append(side[k, j])
                        break
        na = len(rows)
        active += na
        KK = torch.zeros((nv + na, nv + na), dtype=torch.float64, device="cuda")
        KK[:nv, :nv] = K
        if na:
            Gm = torch.stack(rows)
            KK[nv:, :nv] = Gm
            KK[:nv, nv:] = Gm.T
            rhs = torch.cat([rhs, torch.stack(vals)])
        zs.append(torch.linalg.solve(KK, rhs)[:nv])
    assert active > 0
    return torch.stack(zs)


def _grads13(fn, leaves, gz):
    for v in leaves.values():
        v.grad = None
    z = fn()
    (z * gz).sum().backward()
    return z.detach(), {k: (None if v.grad is None else v.grad.detach().clone()) for k, v in leaves.items()}


def _case_dense_reference(ndlqr, rows):
    import torch
    from rslqr_amd.autograd import lqr_solve_constrained
    n, m, N, batch = 6, 3, 5, 3
    t = _torch_case(n, m, N, rows)
    gz = torch.tensor(np.stack([lg.seeded_g(n, m, N, i) for i in range(batch)]), dtype=torch.float64, device="cuda")
    args = [t[k] for k in NAMES13]
    z, got = _grads13(lambda: lqr_solve_constrained(*args, **KW), t, gz)
    zr, ref = _grads13(lambda: _dense_active_solve(t, z, n, m, N, batch), t, gz)
    assert rel(z.cpu().numpy(), zr.cpu().numpy()) <= 1e-8
    for k in NAMES13:
        assert got[k] is not None and got[k].shape == t[k].shape, k
        gr = ref[k] if ref[k] is not None else torch.zeros_like(got[k])
        err = rel(got[k].cpu().numpy(), gr.cpu().numpy())
        print(rows, k, "relative error %.3e" % err)
        assert err <= 1e-6, (k, err)


def _case_backwards_in_reverse_order(ndlqr):
    import torch
    from rslqr_amd.autograd import lqr_solve_constrained, lqr_solve_dense
    n, m, N, batch = 6, 3, 5, 3
    gz = torch.tensor(np.stack([lg.seeded_g(n, m, N, i) for i in range(batch)]), dtype=torch.float64, device="cuda")
    cases = []
    for scale in (1.0, 0.9):
        t = _torch_case(n, m, N, "per_problem", scale)
        args = [t[k] for k in NAMES13]
        _, ref = _grads13(lambda: lqr_solve_constrained(*args, **KW), t, gz)
        cases.append((t, args, ref))
    for t, _, _ in cases:
        for v in t.values():
            v.grad = None
    z1 = lqr_solve_constrained(*cases[0][1], **KW)
    z2 = lqr_solve_constrained(*cases[1][1], **KW)  # (same shape: the same cached solver)
    z3 = lqr_solve_dense(*cases[0][1][:9])           # (a solver of its own: lqr_solve_dense's cache)
    (z2 * gz).sum().backward()
    (z1 * gz).sum().backward()
    (z3 * 0).sum().backward()
    for t, _, ref in cases:
        for k in NAMES13:
            assert rel(t[k].grad.cpu().numpy(), ref[k].cpu().numpy()) <= 1e-9, k


def _case_gradcheck(ndlqr):
    import torch
    from rslqr_amd.autograd import lqr_solve_constrained
    n, m, N = 6, 3, 5
    t = _torch_case(n, m, N, "per_problem")
    sym = lambda M: 0.5 * (M + M.transpose(-1, -2))

    def fn(A, B, Q, H, R, *rest):
        # (Q and R are symmetric matrices, read through their lower triangles: the entries move in pairs)
        return lqr_solve_constrained(A, B, sym(Q), H, sym(R), *rest, rho=ls.RHO, alpha=ls.ALPHA, eps_abs=1e-12, eps_rel=1e-12,
                                     max_iter=50000)
    assert torch.autograd.gradcheck(fn, tuple(t[k] for k in NAMES13), eps=1e-6, atol=1e-5, rtol=1e-4, fast_mode=True)


def _case_non_convergence(ndlqr):
    import torch
    from rslqr_amd.autograd import lqr_solve_constrained
    n, m, N = 6, 3, 5
    t = _torch_case(n, m, N, "per_problem")
    args = [t[k] for k in NAMES13]
    with pytest.raises(RuntimeError, match="lqr_solve_constrained: 3 of 3 problems did not converge"):
        lqr_solve_constrained(*args, rho=ls.RHO, alpha=ls.ALPHA, eps_abs=1e-11, eps_rel=1e-11, max_iter=5)
    with pytest.raises(TypeError, match="must be float64"):
        lqr_solve_constrained(*[a.float() if i == 0 else a for i, a in enumerate(args)])
    with pytest.raises(ValueError, match="C must be"):
        lqr_solve_constrained(*args[:9], args[9][:, :, :, :2], *args[10:])

"""Infeasibility detection of the box-constrained batch solve (ndlqr_BatchSetInfeasibilityDetection,
ndlqr_CopyBatchInfeasibilityCertificate) on the device, against box_infeas_support.py: the
numpy restatement of the iteration with the certificate test, driven by the oracle, and the long-double evaluation of
the certificate the device returns.

Every batch: problem 1 infeasible -- |u| <= ubar on every knot and xhi[N-1][0] placed `gap` below the smallest value that
state reaches inside the input box, so the contradiction travels the whole horizon --, the others barely feasible (the
same bound `gap` above it). ubar = UFRAC x the mean |u| of the problem's unconstrained solution, gap = GFRAC x the width
||G[0, :]||_1 ubar of the reachable interval's half, seeds SEED0 + p, rho = the mean of diag Q over the batch (state
bounds: DESIGN.md section 3.9), alpha 1.6, eps_abs = eps_rel = 1e-6, detection every 10 iterations with eps 1e-4.

The reference alone (admm_infeas_reference on the CPU; measured before anything ran on a device) certifies problem 1 of
every case within 2000 iterations and ends no barely feasible problem as 4:

    case             shape       rho     problem 1 certified at    barely feasible problems converge at
    compact          (12,4,16)   1.255   320                       191, 197
    tree             (6,3,8)     1.320   160                       95, 604
    runtime-sized-a  (5,2,2)     1.166   40                        422, 548
    runtime-sized-b  (16,4,8)    1.242   640                       604
    padded           (7,9,16)    1.253   680                       177
    knot-lean        (2,1,16)    1.174   80                        130, 202
    strict-knot      (12,4,16)   1.234   330                       195
    strict-generic   (20,6,16)   1.279   360                       194
    one-sided (f)    (6,3,8)     1.320   160                       139, 142

(every test recomputes the reference's run of problem 1 once per case and asserts that it
certifies). The device solve gets max_iter = 2 x (the reference's certification iteration) + EVERY and has to certify
within one check interval of the reference: in fast mode its re-solve differs from the oracle's in the last bits, which
can move a threshold crossing by one check. In strict mode the device iterates are the restatement's bit for bit, so
strict-knot and strict-generic certify at the reference's iteration exactly, with the reference's differences bit for
bit and its four numbers (ndlqr_CopyBatchInfeasibilityMeasures) within the bounds of box_infeas_measures_support.py --
wherever the reference's own margins are not within 1e-6 of 1 at that check and the one before, which the test asserts.
"""
import functools

import numpy as np
import pytest

from box_infeas_measures_support import measures_reference
from box_infeas_support import admm_infeas_reference, barely_feasible_bounds, farkas_check, infeasible_bounds
from box_support import condensed, split
from support import Problem

pytestmark = pytest.mark.gpu

ARGS = ("A", "B", "Q", "R", "q", "r", "d", "x0")
UFRAC, GFRAC, SEED0 = 0.5, 0.2, 2100
EVERY, EPS = 10, 1e-4
ALPHA, EPS_ADMM = 1.6, 1e-6

# name -> (n, m, N, batch, flags, NDLQR_TREE): the small rows of test_gpu_box.SCHEDULE_CASES, one per re-solve family
CASES = {"compact": (12, 4, 16, 3, "records", "0"),
         "tree": (6, 3, 8, 3, "records", None),
         "runtime-sized-a": (5, 2, 2, 3, "records", None),
         "runtime-sized-b": (16, 4, 8, 2, "records", None),
         "padded": (7, 9, 16, 2, "records", "0"),
         "knot-lean": (2, 1, 16, 3, "records", None),
         "strict-knot": (12, 4, 16, 2, "strict", None),
         "strict-generic": (20, 6, 16, 2, "strict", None)}


def synth(ndlqr, n, m, N, seed):
    g = ndlqr.generate_synthetic(n, m, N, seed)
    return Problem(n, m, N, *[g[k] for k in ARGS])


def stack(probs, keys=ARGS):
    return [np.stack([getattr(p, k) for p in probs]) for k in keys]


class Case:
    """problems, bounds [batch, N, ..] (problem 1 infeasible), rho and the reference's run of problem 1"""

    def __init__(self, ndlqr, oracle, name, one_sided=False):
        n, m, N, batch, self.flags, self.tree = CASES[name]
        self.n, self.m, self.N, self.batch = n, m, N, batch
        self.probs = [synth(ndlqr, n, m, N, SEED0 + p) for p in range(batch)]
        self.solve = lambda pr: oracle.solve(pr, 1)[0][: pr.nvars]
        self.rho = float(np.mean([p.Q.mean() for p in self.probs]))
        self.knot = N - 1
        rows, self.feasible1 = [], None
        for p, prob in enumerate(self.probs):
            ubar = UFRAC * float(np.abs(split(self.solve(prob), n, m, N)[2]).mean())
            G = condensed(prob)[0][self.knot][0]
            gap = GFRAC * float(np.abs(G).sum()) * ubar
            make = lambda f: self.sided(f(prob, ubar, self.knot, gap), G) if one_sided else f(prob, ubar, self.knot, gap)
            rows.append(make(infeasible_bounds if p == 1 else barely_feasible_bounds))
            if p == 1:
                self.feasible1 = make(barely_feasible_bounds)  # the same problem after relaxing the bound: gap -> -gap
        self.bounds = [np.stack([r[i] for r in rows]) for i in range(4)]
        self.trace = []
        self.ref = admm_infeas_reference(self.probs[1], self.solve, *rows[1], self.rho, ALPHA, EPS_ADMM, EPS_ADMM, 2000, EVERY, EPS,
                                         trace=self.trace)
        print("reference: problem 1 status %d at iteration %d" % self.ref[:2])
        assert self.ref[0] == 4, self.ref[:2]
        self.max_iter = 2 * self.ref[1] + EVERY

    def sided(self, b, G):
        """of every input bound only the side that the smallest reachable value leans on (lower where G > 0, upper where
        G < 0): every input entry keeps one finite bound, and the problem stays infeasible / feasible"""
        xlo, xhi, ulo, uhi = b
        g = np.concatenate([G, np.zeros(self.m)]).reshape(self.N, self.m)
        return xlo, xhi, np.where(g >= 0, ulo, -np.inf), np.where(g < 0, uhi, np.inf)

    def solver(self, ndlqr, monkeypatch, probs=None):
        if self.tree is not None:
            monkeypatch.setenv("NDLQR_TREE", self.tree)
        probs = self.probs if probs is None else probs
        fl = {"records": ndlqr.FLAG_KEEP_RECORDS, "strict": ndlqr.FLAG_STRICT_FP | ndlqr.FLAG_KEEP_FACT}[self.flags]
        bs = ndlqr.BatchSolver(self.n, self.m, self.N, len(probs), flags=fl)
        bs.initialize_flat(*stack(probs))
        return bs

    def solve_box(self, bs, **kw):
        args = dict(rho=self.rho, alpha=ALPHA, eps_abs=EPS_ADMM, eps_rel=EPS_ADMM, max_iter=self.max_iter, check_every=EVERY)
        args.update(kw)
        return bs.solve_box(**args)

    def decisive_margins(self):
        """The reference's margins E / (eps D), I / (eps D) and S / (-eps D) at its certifying check and at the one before,
        none of them within 1e-6 of 1: there the fp64 evaluation of the kernel decides as the reference does (its errors,
        box_infeas_measures_support, are many orders below 1e-6 of these numbers). Returns the certifying check's
        reference numbers."""
        b = [a[1] for a in self.bounds]
        refs = []
        for it, dlam, dmu_x, dmu_u in self.trace[-2:]:
            r = measures_reference(self.probs[1], b, dlam, dmu_x, dmu_u)
            assert r["D"] > 0, (it, r)
            margins = [r["E"] / (EPS * r["D"]), r["I"] / (EPS * r["D"]), r["S"] / (-EPS * r["D"])]
            print("reference check at %d: E / (eps D) %.6g, I / (eps D) %.6g, S / (-eps D) %.6g" % (it, *margins))
            assert all(abs(v - 1.0) > 1e-6 for v in margins), (it, margins)
            assert max(r["tol_E"] / (EPS * r["D"]), r["tol_S"] / (EPS * r["D"])) < 1e-7, (it, r)
            refs.append(r)
        assert self.trace[-1][0] == self.ref[1] and (len(self.trace) < 2 or self.trace[-2][0] == self.ref[1] - EVERY)
        return refs[-1]

    def check_certificate(self, bs, st, eps=EPS):
        """status-4 rows pass the long-double test at 2 eps (the factor covers the kernel's fp64 evaluation of e against
        the long-double one), the others are exactly zero"""
        dlam, dmu_x, dmu_u = bs.infeasibility_certificate()
        for p in range(self.batch):
            if st[p] == 4:
                b = [a[p] for a in self.bounds]
                c = farkas_check(self.probs[p], b, dlam[p], dmu_x[p], dmu_u[p], 2 * eps)
                print("problem %d: e_inf %.3g dmu_inf %.3g S %.3g" % (p, c["e_inf"], c["dmu_inf"], c["S"]))
                assert c["ok"], (p, c)
            else:
                assert not dlam[p].any() and not dmu_x[p].any() and not dmu_u[p].any(), p


@functools.lru_cache(maxsize=None)
def _case(ndlqr, oracle, name, one_sided=False):
    return Case(ndlqr, oracle, name, one_sided)


def others(case):
    return [p for p in range(case.batch) if p != 1]


# ------------------------------------------------------------------------------------------------ a. statuses, certificate

@pytest.mark.parametrize("name", list(CASES))
def test_infeasible_member_is_certified_in_every_family(ndlqr, oracle, monkeypatch, name):
    case = _case(ndlqr, oracle, name)
    bs = case.solver(ndlqr, monkeypatch)
    bs.set_bounds(*case.bounds)
    bs.set_box_infeasibility(EVERY, EPS)
    it, st = case.solve_box(bs)
    print("schedule %s, iterations %s, status %s, reference %d" % (bs.schedule(), it.tolist(), st.tolist(), case.ref[1]))
    assert st[1] == 4, (it, st)
    assert abs(int(it[1]) - case.ref[1]) <= EVERY, (it, case.ref[1])
    assert all(st[p] in (1, 2) for p in others(case)), st
    case.check_certificate(bs, st)
    if case.flags == "strict":
        # the device iterates are the restatement's bit for bit: the same check certifies, with the same differences, and
        # the numbers it decided on are the reference's within the bounds of test_gpu_box_infeas_measures.py
        ref = case.decisive_margins()
        assert it[1] == case.ref[1], (it, case.ref[1])
        dlam, dmu_x, dmu_u = bs.infeasibility_certificate()
        assert np.array_equal(dlam[1], case.ref[2]) and np.array_equal(dmu_x[1], case.ref[3]) and np.array_equal(dmu_u[1], case.ref[4])
        measures, at = bs.infeasibility_measures()
        E, D, I, S = measures[1]
        print("read-out at %d: E %.17g (ref %.17g) D %.17g I %.17g S %.17g (ref %.17g)" % (at[1], E, ref["E"], D, I, S, ref["S"]))
        assert at[1] == case.ref[1]
        assert D == ref["D"] and I == ref["I"], (D, ref["D"], I, ref["I"])
        assert abs(E - ref["E"]) <= ref["tol_E"] and abs(S - ref["S"]) <= ref["tol_S"], (E, S, ref)
    bs.close()


# ------------------------------------------------------------------------------------------------ b. off is off

def test_detection_off_is_the_previous_behaviour(ndlqr, oracle, monkeypatch):
    case = _case(ndlqr, oracle, "compact")
    bs = case.solver(ndlqr, monkeypatch)
    bs.set_bounds(*case.bounds)
    it, st = case.solve_box(bs)  # (the initial state: off)
    assert st[1] == 2 and it[1] == case.max_iter, (it, st)
    with pytest.raises(RuntimeError):
        bs.infeasibility_certificate()
    bs.set_box_infeasibility(EVERY)
    it, st = case.solve_box(bs)
    assert st[1] == 4, (it, st)
    bs.set_box_infeasibility(0)
    it, st = case.solve_box(bs)
    assert st[1] == 2 and it[1] == case.max_iter, (it, st)
    with pytest.raises(RuntimeError):
        bs.infeasibility_certificate()
    bs.close()


# ------------------------------------------------------------------------------------------------ c. the others are undisturbed

@pytest.mark.parametrize("name", ["compact", "strict-knot"])
def test_detection_does_not_disturb_the_other_problems(ndlqr, oracle, monkeypatch, name):
    case = _case(ndlqr, oracle, name)
    bs = case.solver(ndlqr, monkeypatch)
    bs.set_bounds(*case.bounds)
    got = []
    for every in (0, EVERY):
        bs.set_box_infeasibility(every)
        it, st = case.solve_box(bs)
        got.append((it, st, bs.solutions().copy(), bs.bound_multipliers()))
    (it0, st0, z0, mu0), (it1, st1, z1, mu1) = got
    assert st0[1] == 2 and st1[1] == 4
    for p in others(case):
        assert it0[p] == it1[p] and st0[p] == st1[p], (p, it0, it1, st0, st1)
        assert np.array_equal(z0[p], z1[p]), p
        assert np.array_equal(mu0[0][p], mu1[0][p]) and np.array_equal(mu0[1][p], mu1[1][p]), p
    bs.close()


# ------------------------------------------------------------------------------------------------ d. the batch stops early

def test_the_batch_stops_early(ndlqr, oracle, monkeypatch):
    case = _case(ndlqr, oracle, "compact")  # (its barely feasible members converge well below max_iter)
    bs = case.solver(ndlqr, monkeypatch)
    bs.set_bounds(*case.bounds)
    bs.set_box_infeasibility(EVERY)
    it, st = case.solve_box(bs)
    assert st[1] == 4 and all(st[p] == 1 for p in others(case)), (it, st)
    assert it.max() < case.max_iter, it
    bs.set_box_infeasibility(0)
    it, st = case.solve_box(bs)
    assert all(st[p] == 1 for p in others(case)) and it.max() == case.max_iter, (it, st)
    bs.close()


# ------------------------------------------------------------------------------------------------ e. adaptive penalty

def test_certificate_across_changes_of_the_adaptive_penalty(ndlqr, oracle, monkeypatch):
    case = _case(ndlqr, oracle, "compact")
    bs = case.solver(ndlqr, monkeypatch)
    bs.set_bounds(*case.bounds)
    bs.set_box_infeasibility(EVERY)
    # (from a tenth of the penalty the other tests use, so that the rule has to move it; checks and adaptions coincide at
    # every 50th iteration)
    it, st = case.solve_box(bs, rho=0.1 * case.rho, adapt_every=25, max_iter=2000)
    rho = bs.box_penalties()
    print("iterations %s, status %s, penalties %s" % (it.tolist(), st.tolist(), rho.tolist()))
    assert st[1] == 4, (it, st)
    assert rho[1] != 0.1 * case.rho  # the penalty did change on the way
    assert all(st[p] in (1, 2) for p in others(case)), st
    case.check_certificate(bs, st)
    bs.close()


# ------------------------------------------------------------------------------------------------ f. infinite bounds

def test_one_sided_bounds(ndlqr, oracle, monkeypatch):
    """Every input entry with one finite bound only -- the side the contradiction leans on; the other is infinite -- plus
    the contradicting upper state bound: still certified, and dmu points to no infinite bound. The barely feasible
    members, whose bounds are one-sided and compatible, never end as 4."""
    case = _case(ndlqr, oracle, "tree", True)
    assert all(np.isinf(a).any() for a in case.bounds[2:])
    bs = case.solver(ndlqr, monkeypatch)
    bs.set_bounds(*case.bounds)
    bs.set_box_infeasibility(EVERY)
    it, st = case.solve_box(bs)
    print("iterations %s, status %s, reference %d" % (it.tolist(), st.tolist(), case.ref[1]))
    assert st[1] == 4 and abs(int(it[1]) - case.ref[1]) <= EVERY, (it, st)
    assert all(st[p] in (1, 2) for p in others(case)), st
    case.check_certificate(bs, st)
    # the feasible members alone, run to max_iter with a convergence test that never holds: never 4
    it, st = case.solve_box(bs, eps_abs=1e-300, eps_rel=1e-300)
    assert st[1] == 4 and all(st[p] == 2 for p in others(case)), (it, st)
    bs.close()


# ------------------------------------------------------------------------------------------------ g. state rules

def test_state_rules(ndlqr, oracle, monkeypatch):
    case = _case(ndlqr, oracle, "compact")
    bs = case.solver(ndlqr, monkeypatch)
    bs.set_bounds(*case.bounds)
    # the setter's refusals leave the previous setting
    bs.set_box_infeasibility(EVERY, EPS)
    for every, eps in ((-1, 0.0), (EVERY, float("nan")), (EVERY, -1e-4), (EVERY, float("inf"))):
        with pytest.raises(RuntimeError):
            bs.set_box_infeasibility(every, eps)
    it, st = case.solve_box(bs)
    assert st[1] == 4, (it, st)
    case.check_certificate(bs, st)
    z = bs.solutions().copy()
    mu = [a.copy() for a in bs.bound_multipliers()]
    # the box adjoint does not iterate the certified problem: status 4, w = 0
    ait, ast = bs.solve_box_adjoint(np.ones((case.batch, bs.nvars)), alpha=ALPHA, eps_abs=EPS_ADMM, eps_rel=EPS_ADMM, max_iter=4000)
    assert ast[1] == 4 and ait[1] == 0 and all(ast[p] in (1, 2) for p in others(case)), (ait, ast)
    w = bs.adjoint()
    assert not w[1].any() and all(w[p].any() for p in others(case))
    bg = bs.bound_gradients()
    assert all(not g[1].any() for g in bg.values())
    case.check_certificate(bs, st)  # (the adjoint leaves the forward as it is)
    # the polish reports 2 for it and leaves it bit for bit
    steps, pst = bs.polish_box()
    assert pst[1] == 2 and steps[1] == 0, (steps, pst)
    assert np.array_equal(bs.solutions()[1], z[1])
    mu2 = bs.bound_multipliers()
    assert np.array_equal(mu2[0][1], mu[0][1]) and np.array_equal(mu2[1][1], mu[1][1])
    # the bound relaxed (gap -> -gap), warm start: the member starts cold and takes the iterations of a cold solve of it alone
    relaxed = [a.copy() for a in case.bounds]
    for a, f in zip(relaxed, case.feasible1):
        a[1] = f
    bs.set_bounds(*relaxed)
    it, st = case.solve_box(bs, warm_start=True, max_iter=2000)
    assert st[1] == 1, (it, st)
    alone = case.solver(ndlqr, monkeypatch, [case.probs[1]])
    alone.set_bounds(*[f[None] for f in case.feasible1])
    it1, st1 = case.solve_box(alone, max_iter=2000)
    assert st1[0] == 1 and it[1] == it1[0], (it, it1)
    alone.close()
    # the getter refuses when the resident solution is not a constrained solve's
    bs.set_bounds(*case.bounds)
    it, st = case.solve_box(bs)
    assert st[1] == 4
    bs.infeasibility_certificate()
    assert bs.solve() == 0
    with pytest.raises(RuntimeError):
        bs.infeasibility_certificate()
    bs.close()


# ------------------------------------------------------------------------------------------------ h. NaN data

def test_nan_data_ends_as_3_not_4(ndlqr, oracle, monkeypatch):
    case = _case(ndlqr, oracle, "compact")
    bs = case.solver(ndlqr, monkeypatch)
    bs.set_bounds(*case.bounds)
    bs.set_box_infeasibility(1)  # (a check at every iteration from the second on)
    x0 = np.stack([p.x0 for p in case.probs])
    x0[2, 3] = np.nan
    bs.set_rhs_flat(*stack(case.probs, ("q", "r", "d")), x0)
    it, st = case.solve_box(bs, check_every=1)
    assert st[2] == 3 and it[2] == 1 and st[1] == 4 and st[0] in (1, 2), (it, st)
    case.check_certificate(bs, st)
    bs.close()


# ------------------------------------------------------------------------------------------------ i. torch

def _case_torch(ndlqr):
    """lqr_solve_box(..., infeas_every=k): the certified member does not raise and gets zero gradients in every tensor"""
    import torch
    from rslqr_amd.autograd import lqr_solve_box
    from support import Oracle
    case = Case(ndlqr, Oracle(), "compact")
    n, m, N, batch = case.n, case.m, case.N, case.batch
    t = []
    for k, a in zip(ARGS, stack(case.probs)):
        if k in ("A", "B"):
            a = a.reshape(batch, N, n if k == "A" else m, n).transpose(0, 1, 3, 2)  # column-major flat -> row-major matrices
        t.append(torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda", requires_grad=True))
    b = [torch.tensor(a, dtype=torch.float64, device="cuda", requires_grad=True) for a in case.bounds[1:]]
    kw = dict(rho=case.rho, alpha=ALPHA, eps_abs=EPS_ADMM, eps_rel=EPS_ADMM, max_iter=2000)
    with pytest.raises(RuntimeError):  # (without detection the infeasible member runs to max_iter: status 2)
        lqr_solve_box(*t, None, *b, **kw)
    z = lqr_solve_box(*t, None, *b, infeas_every=EVERY, **kw)
    (z * z).sum().backward()
    for name, x in zip(ARGS + ("xhi", "ulo", "uhi"), t + b):
        g = x.grad.cpu().numpy()
        assert np.isfinite(g).all() and not g[1].any(), name
    assert all(t[ARGS.index(k)].grad[p].abs().max() > 0 for k in ("q", "r", "x0") for p in others(case))


def test_torch_infeasible_member_gets_zero_gradients():
    """in a fresh process that initialises torch's device first (as test_gpu_box_gradients._run_case)"""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import torch; torch.zeros(1, device='cuda')\n"
            "import rslqr_amd, test_gpu_box_infeas as T\n"
            "T._case_torch(rslqr_amd)\n"
            "print('case ok')\n" % (os.path.dirname(here), here))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "case ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])

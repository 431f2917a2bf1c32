"""CPU checks of tests/sde_step_ref.py, the reference and yardstick of test_gpu_sde_steps.py. Without them the GPU
tests could be vacuous (a tolerance no wrong update exceeds) or unreachable (one that correct float32 arithmetic
misses). At every (potential, d) of the GPU matrix, with 64 rows:

  * reachable: each fp32 variant's own e_rel is within FACTOR / 2 of the largest e_rel of the others (leave one out),
    and a float32 run carried forward through a variant that is not the one the yardstick's rows come from passes
    the checker the GPU tests use;
  * not vacuous: each wrong update of sde_step_ref.MUTATIONS that applies to the case exceeds FACTOR x e_rel x S in
    an entry it touches: the last update with h = dt, friction taken on the new p, q' from the old p, the noise of
    update s + 1, noise scaled by h instead of sqrt(h), the centre dropped, 1 / sigma^2 dropped (sigma = 0.7), a
    padded GMM slot counted as a centre at 0, the mean-field xbar of row s + 1, two neighbouring rows swapped in one
    step, and one entry off by 64 x 2^-24 x S;
  * tau_rows is oracle.numpy_ref.sde_scan's float32 tau bit for bit.
"""
import numpy as np
import pytest

import sde_step_ref as R
from oracle import numpy_ref as nr

F32 = np.float32
N_CPU = 64
CASES = [c._replace(N=N_CPU) for c in R.explicit_cases()]


def _tau0(c, inp):
    """Explicit shift_u for the uncoupled potentials; one shared clock for the mean-field ensemble."""
    if c.pot == "meanfield":
        return np.full(c.N, F32(0.37) * F32(R.DT), F32)
    return R.tau0_of(inp["u"])


def _carried(c, inp, tau0, variant):
    """A float32 run [n+1, N, 2d] carried forward through one variant (a stand-in for a correct kernel)."""
    hs = R.step_sizes(tau0, c.n_steps)
    z, rows = inp["z0"], []
    for s in range(c.n_steps + 1):
        z = R.variants32(c, inp, z, hs[s], inp["xi"][s], s)[variant]
        rows.append(z)
    return np.stack(rows)


def test_case_matrix_covers_every_instantiation():
    cases = R.explicit_cases()
    for d in R.DIMS:
        pots = {(c.pot, c.centre) for c in cases if c.d == d}
        assert pots == {("quadratic", False), ("quadratic", True), ("none", False), ("gmm", False),
                        ("meanfield", False)}
        assert {R.gmm_km(c.K) for c in cases if c.d == d and c.pot == "gmm"} == {4, 8, 16}
        assert any(c.sigma == 0.7 for c in cases if c.d == d)
    assert {c.pot for c in cases if c.ns == 0.9} == {"quadratic", "none", "gmm", "meanfield"}
    assert {c.K for c in cases if c.d in (3, 4) and c.pot == "gmm"} == {1, 3, 4, 5, 8, 9, 16}
    assert all(km * c.d <= 64 for c, km in R.res_cases()) and {c.d for c, _ in R.res_cases()} == set(range(1, 9))
    # every mutation is exercised somewhere, and the special shifts are in every explicit shift_u
    assert {m for c in cases for m in R.mutations_of(c)} == set(R.MUTATIONS)
    u = R.inputs(cases[0])["u"]
    assert u[0] == 0 and u[1] == F32(2.0 ** -24) and u[2] == F32(1 - 2.0 ** -24) and u[-1] == 0


@pytest.mark.parametrize("c", CASES, ids=R.case_id)
def test_tolerance_reachable_and_not_vacuous(c):
    inp = R.inputs(c)
    tau0 = _tau0(c, inp)
    errs = R.variant_errors(c, inp, tau0)
    erel = float(errs.max())
    assert 2.0 ** -25 < erel < 2.0 ** -21, erel  # a few ulp of S: the scales are the right size
    # reachable: leave one out
    loo = max(errs[v] / np.delete(errs, v).max() for v in range(len(errs)))
    print(f"{R.case_id(c)}: e_rel {erel:.3g}, leave-one-out {loo:.3g}")
    assert loo <= R.FACTOR / 2, (loo, errs)
    # ... and a run carried through the last variant (the yardstick's rows come from the first) passes the checker
    run = _carried(c, inp, tau0, len(errs) - 1)
    worst = R.check_trajectory(c, inp, tau0, inp["xi"], run[:-1], run[-1], erel, R.case_id(c))
    assert worst <= R.FACTOR / 2
    # not vacuous: every wrong update moves an entry past the tolerance, judged from the same rows
    hs = R.step_sizes(tau0, c.n_steps)
    n = c.n_steps
    for m in R.mutations_of(c):
        caught = 0.0
        for s in range(n + 1):
            z_prev = inp["z0"] if s == 0 else run[s - 1]
            ref = R.update64(c, inp, z_prev, hs[s], inp["xi"][s], s)
            S = R.scale(c, inp, z_prev, hs[s], inp["xi"][s], s)
            if m == "one_entry":
                mut = ref.copy()
                if s == min(1, n):
                    for i, k in ((c.N // 2, 0), (c.N - 1, 2 * c.d - 1)):
                        mut[i, k] += 64 * 2.0 ** -24 * S[i, k]
            else:
                mut = R.update64(c, inp, z_prev, hs[s], inp["xi"][s], s, mutate=m, xi_next=inp["xi"][(s + 1) % (n + 1)])
            touched = mut != ref
            if not touched.any():
                continue
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.where(touched, np.abs(mut - ref) / (erel * S), 0.0)
            caught = max(caught, float(ratio.max()))
            if m == "one_entry":  # both entries, through the checker itself
                assert (ratio[touched] > R.FACTOR).all(), ratio[touched]
                with pytest.raises(AssertionError, match="off by"):
                    R.check_update(mut, ref, S, erel, m)
        print(f"  {m}: {caught:.3g} x e_rel S")
        assert caught > R.FACTOR, (m, caught)


@pytest.mark.parametrize("n_steps", [1, 2, 6])
def test_tau_rows_are_the_restatement_bit_for_bit(n_steps):
    c = R.case("none", 2, n_steps=n_steps)
    inp = R.inputs(c)
    _, _, tau32 = nr.sde_scan(inp["z0"], n_steps, R.DT, R.GAMMA, lambda q: np.zeros_like(q), inp["xi"], inp["u"],
                              dtype=np.float32)
    assert tau32.dtype == F32 and np.array_equal(R.tau_rows(R.tau0_of(inp["u"]), n_steps), tau32)
    h = R.step_sizes(R.tau0_of(inp["u"]), n_steps)
    assert h.shape == (n_steps + 1, c.N) and h[0, 0] == 0 and h[-1, 0] == F32(R.DT)

"""CPU checks of tests/kmv_sums_ref.py, the reference and yardstick of test_gpu_kmv_sums.py. Without them the GPU
tests could be vacuous: a tolerance that no wrong kernel exceeds, or a reference that restates the kernels' own
coefficient table.

  * dlogrho_coefficients (the host table behind every weight) reproduces the closed form oracle.numpy_ref
    .partial_s_log_density / partial_s2_log_density at every compiled dimension, with the product's centred initial law
    and with a shifted one (m1 and beta are identically 0 in the centred problem);
  * for every (d, N, chain lengths) the GPU tests use, states 0.8 randn + 0.25 and tau in {0.02, 0.37, 1.9}:
    a fresh row order evaluated in fp32 stays within half the tolerance FACTOR x E; every single dropped row moves an
    entry other than the (exact) count past it; three wrong formulas (Gamma unsymmetrised over the upper triangle,
    x for r, no gamma ds) each exceed it;
  * residual_ref (the finalize from sums, any counts) equals oracle.numpy_ref.kmv_from_moments on equal counts.
"""
import numpy as np
import pytest

import kmv_sums_ref as R
from oracle import numpy_ref as nr

GAMMA = 1.0


@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("d", R.WEIGHT_DIMS)
def test_coefficients_reproduce_closed_form(d, shifted):
    """a + beta . r + r^T Gamma r in fp64 from the table == the closed form: 1e-10 of 1 + |ref|, 500 rows, 3 stamps."""
    cfg = R.problem_cfg(d, shifted)
    coef = R.coefficients(R.TAUS, cfg, d)
    assert coef.shape == (3, 3 * d + 2 + 2 * d * d)
    x = R.states(500, d, 40 + d).astype(np.float64)
    for t, tau in enumerate(R.TAUS):
        m1, a1, b1, G1, a2, b2, G2 = R.unpack_coef(coef[t], d)
        r = m1[None] - x
        for a, b, G, fn in ((a1, b1, G1, nr.partial_s_log_density), (a2, b2, G2, nr.partial_s2_log_density)):
            got = a + r @ b + np.einsum("ni,ij,nj->n", r, G, r)
            ref = fn(tau, x, cfg)
            assert np.max(np.abs(got - ref) / (1 + np.abs(ref))) < 1e-10, (d, tau, fn.__name__)
    if shifted:  # the shifted problem exercises what the centred one cannot
        assert np.abs(coef[:, :d]).min() > 1e-4 and np.abs(coef[:, d + 1:2 * d + 1]).max() > 1e-3


def _weighted_cases():
    """(d, N, chains) of every weighted-sum comparison of test_gpu_kmv_sums.py."""
    cases = [(d, n, R.SIM_CHAINS) for d, n in R.SIM_CASES]                              # a: sde_mf_kmv_kernel
    cases += [(d, n, R.mw_chains(3, n)) for d in range(1, 9) for n in R.MW_ROWS]        # b: kmv_moments_weights
    cases += [(d, R.MW_CAPPED["n_rows"], R.mw_chains(R.MW_CAPPED["n_sets"], R.MW_CAPPED["n_rows"]))
              for d in R.MW_CAPPED["dims"]]
    cases += [(d, n, R.sep_chains(3, n)) for d in R.WEIGHT_DIMS for n in R.SEP_ROWS]    # c: kmv_weights
    return sorted(set(cases))


def _caught_share(terms, tol):
    """Share of rows whose removal moves some entry other than the count past the tolerance."""
    return float((np.abs(terms[:, 1:]) > tol[None, 1:]).any(1).mean())


@pytest.mark.parametrize("d,n,chains", _weighted_cases())
def test_yardstick_conditions(d, n, chains):
    assert R.MW_CAPPED["n_rows"] > 4099 and R.mw_chains(512, 6100) == (192, 4)
    cfg = R.problem_cfg(d)
    coef32 = R.coefficients(R.TAUS, cfg, d).astype(np.float32)
    z = R.states(n, 2 * d, 100 * d + n)
    lz = R.moment_len(2 * d)
    for t, tau in enumerate(R.TAUS):
        mom_t, wst_t = R.stamp_terms(z, tau, cfg, d, GAMMA)
        terms = np.concatenate([mom_t, wst_t], 1)
        ref = terms.sum(0)
        E = R.fp32_yardstick(z, coef32[t], d, GAMMA, chains, ref)
        tol = R.FACTOR * E
        t32 = R.terms32(z, coef32[t], d, GAMMA, "sym")
        fresh = R.row_orders(n, first=R.N_ORDERS, count=1)[0]  # an order the yardstick has not seen
        err = np.abs(R.chain_sum(t32[fresh], chains) - ref)
        assert np.all(err <= 0.5 * tol), (tau, np.max(err[tol > 0] / tol[tol > 0]))
        # dropping one row (the count, which alone would catch every row, is left out of the condition)
        share = _caught_share(terms, tol)
        assert share == 1.0 if n <= 4099 else share >= 0.999, (tau, share)
        # wst alone cannot catch every row (a row with w ~ 0 adds nothing to it), but it must catch nearly all
        assert _caught_share(terms[:, lz - 1:], tol[lz - 1:]) >= 0.95, tau
        for mutate in R.MUTATIONS:
            if mutate == "upper_only" and d == 1:
                continue  # no off-diagonal entry at d = 1: the two forms coincide
            bad = R.chain_sum(R.terms32(z, coef32[t], d, GAMMA, "sym", mutate), chains)
            assert np.any(np.abs(bad - ref)[lz:] > tol[lz:]), (tau, mutate)
            assert np.array_equal(bad[:lz], R.chain_sum(t32, chains)[:lz])  # mom has no weight in it


@pytest.mark.parametrize("m", range(1, 17))
@pytest.mark.parametrize("n", R.SEP_ROWS)
def test_moments_yardstick_conditions(m, n):
    """The plain moments of moments_batched_kernel<M>: fresh order within half the tolerance, every dropped row caught."""
    z = R.states(n, m, 300 + 17 * m + n)
    chains = R.sep_chains(3, n)
    terms = R.moment_terms(z.astype(np.float64))
    ref = terms.sum(0)
    tol = R.FACTOR * R.moments_yardstick(z, chains, ref)
    fresh = R.row_orders(n, first=R.N_ORDERS, count=1)[0]
    err = np.abs(R.chain_sum(R.moment_terms(z)[fresh], chains) - ref)
    assert np.all(err <= 0.5 * tol)
    assert tol[0] == 0.0 and _caught_share(terms, tol) == 1.0


def test_stamp_terms_layout_and_chain_sum():
    """Entry order = include/pdeinv.h's (nr.moments); chain_sum in one fp64 chain = the plain sum."""
    d, n = 3, 50
    cfg = R.problem_cfg(d)
    z = R.states(n, 2 * d, 5)
    mom_t, wst_t = R.stamp_terms(z, 0.37, cfg, d, 0.5)
    assert mom_t.shape == (n, R.moment_len(2 * d)) and wst_t.shape == (n, R.moment_len(d))
    assert np.allclose(mom_t.sum(0), nr.moments(z.astype(np.float64)), rtol=1e-13)
    x = z[:, :d].astype(np.float64)
    w = (nr.partial_s2_log_density(0.37, x, cfg) + nr.partial_s_log_density(0.37, x, cfg) ** 2
         + 0.5 * nr.partial_s_log_density(0.37, x, cfg))
    ref = np.concatenate([[w.sum()], w @ x, ((x * w[:, None]).T @ x)[np.triu_indices(d)]])
    assert np.allclose(wst_t.sum(0), ref, rtol=1e-12)
    t32 = R.terms32(z, R.coefficients(0.37, cfg, d)[0].astype(np.float32), d, 0.5)
    a = R.chain_sum(t32, (7, 3))
    assert np.allclose(a, t32.astype(np.float64).sum(0), rtol=1e-5)
    assert np.array_equal(R.chain_sum(t32[:1], (64, 4)), t32[0].astype(np.float64))  # one row: exact


def test_batched_grid_restated():
    """The chain lengths follow csrc/kmv.hip's batched_bx: one trip at the small cases, three at the capped one."""
    assert R.batched_bx(3, 257) == 2 and R.batched_trips(3, 257) == 1
    assert R.batched_bx(512, 6100) == 8 and R.batched_trips(512, 6100) == 3
    assert R.batched_bx(7, 50_001) == 196 and R.batched_trips(7, 50_001) == 1
    # every wave of the capped case makes 3 trips, and the last wave's third block is partial
    stride, last_wave = 8 * 256, 8 * 256 - 64
    assert last_wave + 2 * stride < 6100 < last_wave + 2 * stride + 64 and 3 * stride > 6100


@pytest.mark.parametrize("d", range(1, 9))
def test_residual_ref_equals_kmv_from_moments(d):
    """residual_ref on host sums == nr.kmv_from_moments on the samples (equal counts), to fp64 cancellation."""
    rng = np.random.default_rng(60 + d)
    n, n_t = 300, 3
    x, v = rng.standard_normal((n, n_t, d)) * 0.8 + 0.25, rng.standard_normal((n, n_t, d))
    F = nr.problem_constants(d).astype(np.float32).astype(np.float64)
    cfg = nr.ou_configuration(F)
    K = rng.standard_normal((d, d)).astype(np.float32).astype(np.float64)
    b = rng.standard_normal(d).astype(np.float32).astype(np.float64)
    tau = np.array(R.TAUS)
    mom, wst = R.host_sums(x, v, tau, cfg, 1.0)
    got, mag = R.residual_ref(K, b, F, mom, wst), R.residual_ref(K, b, F, mom, wst, magnitude=True)
    loss, gt, gK, gb = nr.kmv_from_moments(K, b, x, v, tau, cfg)
    assert abs(got["loss"] - loss) <= 1e-12 * mag["loss"] and abs(got["loss_gt"] - gt) <= 1e-12 * mag["loss_gt"]
    assert np.all(np.abs(got["grad"] - np.concatenate([gK.ravel(), gb])) <= 1e-12 * mag["grad"])
    assert abs(got["loss"] - (got["nabla"] - 2 * got["hess"] + 2 * got["value"] + got["true"])) <= 1e-12 * mag["loss"]
    for k in ("loss", "loss_gt", "nabla", "hess", "value", "true", "grad_norm"):
        assert mag[k] >= abs(got[k])
    assert np.all(mag["grad"] >= np.abs(got["grad"]))

"""sde_simulate_kernel and mf_step_kernel (csrc/sde.hip) against fp64, one update at a time and entry by entry, at
every compiled dimension and potential.

The aggregate simulator tests (test_gpu_kernels.py, test_gpu_meanfield.py, the golden files) compare 100-step
trajectories under a tolerance that must hide 100 steps of accumulated rounding, at d in {1, 2, 3, 4, 8} only. Here
update s of particle i is taken from the GPU's own previous row and compared with the fp64 update of
tests/sde_step_ref.py: every entry within FACTOR x e_rel x S of its rounding scale S (that module's docstring; e_rel
from NumPy float32 restatements of the same update, no kernel output in it). test_sde_step_ref.py shows on the CPU
that this tolerance is reachable and that eleven wrong updates exceed it at every (potential, d) used here.
Asserted bit for bit: tau, update 0 at h = 0, and that a particle's numbers depend on its global id and its row
only (call splits, output subsets, the stride of z0).

Each case prints `FAMILY <kernel family> <max |err| / (e_rel S)>` (pytest -s); the maxima of the MI355X run are in
sde_step_ref.MEASURED.
"""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import kmv_sums_ref as KR
import sde_step_ref as R
from oracle import numpy_ref as nr

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
SEED, CTR = 0x5EED_0007_1234, 13


def _t(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _np(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def _family(name, worst):
    print(f"FAMILY {name} {worst:.4g}")


def _pot(native, c, inp):
    if c.pot == "none":
        return dict(kind=native.POT_NONE)
    if c.pot == "quadratic":
        params = inp["A"].ravel() if inp["c"] is None else np.concatenate([inp["A"].ravel(), inp["c"]])
        return dict(kind=native.POT_QUADRATIC, params=params, has_center=inp["c"] is not None)
    assert c.pot == "gmm"
    return dict(kind=native.POT_GMM, params=inp["mus"], n_centers=c.K, sigma=c.sigma)


def _simulate(native, c, inp, **kw):
    """pdeinv_sde_simulate in the explicit-noise mode on the case's inputs."""
    args = dict(seed=SEED, noise_scale=c.ns, noise=_t(inp["xi"]), shift_u=_t(inp["u"]))
    args.update(kw)
    return _np(native.sde_simulate(_t(inp["z0"]), c.n_steps, R.DT, R.GAMMA, _pot(native, c, inp), **args))


def _check_run(c, inp, res, tau0, what, xi=None, philox=False):
    """tau bit for bit, h = 0 rows unchanged, then every update of the run under the rule."""
    xi = inp["xi"] if xi is None else xi
    if "tau" in res:
        assert np.array_equal(res["tau"], R.tau_rows(tau0, c.n_steps)), f"{what}: tau"
    still = tau0 == 0
    if still.any() and "traj" in res:  # update 0 with h = 0 leaves the row as it was, bit for bit
        assert np.array_equal(res["traj"][0][still], inp["z0"][still]), f"{what}: update 0 at h = 0"
    erel = R.e_rel(c, inp, tau0, xi)
    return R.check_trajectory(c, inp, tau0, xi, res.get("traj"), res.get("last"), erel, what, philox=philox)


# ---- a. explicit noise, every compiled d, every potential, with and without the fused moments ------------------
_UNCOUPLED = [c for c in R.explicit_cases() if c.pot != "meanfield"]
_EXPLICIT = [(c, False) for c in _UNCOUPLED] + [(c, True) for c in _UNCOUPLED if c.d <= 8]


@pytest.mark.parametrize("c,moments", _EXPLICIT, ids=lambda v: R.case_id(v) if isinstance(v, tuple) else f"mom{int(v)}")
def test_explicit_noise_updates_vs_fp64(native, c, moments):
    """sde_simulate_kernel<d, POT, MOM, staged, KM, explicit noise>: explicit shift_u holding 0, 2^-24 and 1 - 2^-24;
    without the fused moments also random_shift = False (h = 0 on update 0 of every row)."""
    inp = R.inputs(c)
    what = R.case_id(c) + (" moments" if moments else "")
    res = _simulate(native, c, inp, moments=moments)
    worst = _check_run(c, inp, res, R.tau0_of(inp["u"]), what)
    if not moments:
        res0 = _simulate(native, c, inp, shift_u=None, random_shift=False)
        assert np.array_equal(res0["traj"][0], inp["z0"])
        worst = max(worst, _check_run(c, inp, res0, np.zeros(c.N, F32), what + " unshifted"))
    fam = {"quadratic": "quadratic", "none": "quadratic", "gmm": f"GMM KM={R.gmm_km(c.K)}"}[c.pot]
    _family(f"sde_simulate_kernel {fam}" + (", fused moments" if moments else ""), worst)


def _mf_run(native, oracle_lib, c, inp, random_shift=True):
    """pdeinv_sde_simulate, MEANFIELD_QUADRATIC, on a given d_meanfield path; returns (res, tau0 [N])."""
    noise = _t(inp["xi"])  # the descriptor holds its address only: bound to a name until the call is done
    desc, keep = native.mf_desc(c.N, c.d, c.n_steps, R.DT, R.GAMMA, inp["A"], seed=SEED, counter_offset=CTR,
                                noise_scale=c.ns, random_shift=random_shift, noise=noise)
    xbar = _t(inp["xbar"])
    desc.d_meanfield = ctypes.c_void_p(xbar.data_ptr())
    out = dict(traj=torch.empty((c.n_steps, c.N, 2 * c.d), device=DEV), tau=torch.empty((c.n_steps, c.N), device=DEV),
               last=torch.empty((c.N, 2 * c.d), device=DEV))
    native.sde_simulate_desc(desc, _t(inp["z0"]), out["traj"], out["tau"], out["last"])
    res = _np(out)
    del keep, noise
    # the shared clock: the stream's shift of global id 2^64 - 1 (include/pdeinv.h), read back as tau[0]
    u = F32(oracle_lib.lib().oracle_shift_u(SEED, (1 << 64) - 1, CTR)) if random_shift else F32(0)
    tau0 = np.full(c.N, u * F32(R.DT), F32)
    assert np.array_equal(res["tau"][0], tau0)
    return res, tau0


@pytest.mark.parametrize("c", [c for c in R.explicit_cases() if c.pot == "meanfield"], ids=R.case_id)
def test_meanfield_updates_vs_fp64(native, oracle_lib, c):
    """sde_simulate_kernel<d, MEANFIELD_QUADRATIC>: grad_meanfield on a path of random rows, explicit noise."""
    inp = R.inputs(c)
    res, tau0 = _mf_run(native, oracle_lib, c, inp)
    worst = _check_run(c, inp, res, tau0, R.case_id(c))
    res0, zero = _mf_run(native, oracle_lib, c, inp, random_shift=False)
    assert np.array_equal(res0["traj"][0], inp["z0"])
    worst = max(worst, _check_run(c, inp, res0, zero, R.case_id(c) + " unshifted"))
    _family("sde_simulate_kernel mean-field", worst)


# ---- b. the GMM simulator with the fused KFP residual (RES: centres in LDS) ------------------------------------
@pytest.mark.parametrize("c,k_model", R.res_cases(), ids=lambda v: R.case_id(v) if isinstance(v, tuple) else f"Km{v}")
def test_fused_gmm_residual_trajectory_vs_fp64(native, c, k_model):
    inp = R.inputs(c)
    mus = np.random.default_rng(c.d + k_model).standard_normal((k_model, c.d)).astype(F32)
    T = c.n_steps * R.DT
    desc = native.kfp_gmm_desc(c.d, k_model, inp["mus"], R.GAMMA, T, c.N, c.N, c.N * c.n_steps)
    res = native.sde_simulate_kfp_gmm(_t(inp["z0"]), c.n_steps, R.DT, R.GAMMA, _pot(native, c, inp), desc, _t(mus),
                                      seed=SEED, noise=_t(inp["xi"]), shift_u=_t(inp["u"]))
    assert torch.isfinite(res.pop("acc")).all()
    worst = _check_run(c, inp, _np(res), R.tau0_of(inp["u"]), f"{R.case_id(c)} RES Km={k_model}")
    _family("sde_simulate_kernel GMM, fused residual", worst)


# ---- c. sizes: partial waves, block boundaries, the xcd_block remap on 12 blocks, n_steps in {1, 2, 6} ----------
@pytest.mark.parametrize("c", R.size_cases(), ids=R.case_id)
def test_sizes_updates_vs_fp64(native, c):
    worst = 0.0
    for n in R.SIZE_STEPS:
        cn = c._replace(n_steps=n)
        inp = R.inputs(cn)
        res = _simulate(native, cn, inp)
        assert res["traj"].shape == (n, c.N, 2 * c.d)
        worst = max(worst, _check_run(cn, inp, res, R.tau0_of(inp["u"]), R.case_id(cn)))
    _family("sde_simulate_kernel sizes", worst)


# ---- d. Philox mode -------------------------------------------------------------------------------------------
def _stream_normals(oracle_lib, n_steps, N, d, poff):
    return np.stack([np.stack([oracle_lib.sim_normals(SEED, poff + i, CTR + s, d) for i in range(N)])
                     for s in range(n_steps + 1)])


@pytest.mark.parametrize("poff", R.PHILOX_OFFSETS)
@pytest.mark.parametrize("c", R.philox_cases(), ids=R.case_id)
def test_philox_updates_vs_fp64(native, oracle_lib, c, poff):
    """xi from the C oracle's stream at (seed, particle_offset + i, counter_offset + s); the kernel's hardware
    normals are allowed 2e-6 (1 + |xi|) (sde_step_ref.normals_extra). tau0 is the stream's shift, read back."""
    inp = R.inputs(c)
    res = _np(native.sde_simulate(_t(inp["z0"]), c.n_steps, R.DT, R.GAMMA, _pot(native, c, inp), seed=SEED,
                                  counter_offset=CTR, particle_offset=poff))
    xi = _stream_normals(oracle_lib, c.n_steps, c.N, c.d, poff)
    u = np.array([oracle_lib.lib().oracle_shift_u(SEED, poff + i, CTR) for i in range(c.N)], F32)
    tau0 = R.tau0_of(u)
    assert np.array_equal(res["tau"][0], tau0)
    worst = _check_run(c, inp, res, tau0, f"{R.case_id(c)} philox poff={poff}", xi=xi, philox=True)
    _family("sde_simulate_kernel Philox", worst)


# ---- e. a particle's numbers depend on its global id and its row only ------------------------------------------
@pytest.mark.parametrize("pot,K", [("quadratic", 0), ("gmm", 5)])
@pytest.mark.parametrize("d", [3, 4, 8, 16])
def test_same_bits_however_the_rows_are_presented(native, d, pot, K):
    c = R.case(pot, d, N=700, K=K)
    inp = R.inputs(c)
    z0 = _t(inp["z0"])
    poff = (1 << 32) - 100  # the ids cross a multiple of 2^32 inside the call
    kw = dict(seed=SEED, counter_offset=CTR)

    def run(z, off, **sel):
        return native.sde_simulate(z, c.n_steps, R.DT, R.GAMMA, _pot(native, c, inp), particle_offset=off, **kw, **sel)

    full = run(z0, poff)
    assert all(torch.isfinite(full[k]).all() for k in ("traj", "tau", "last"))
    for cut in (1, 64, 333):  # one call == two calls with particle_offset advanced
        a, b = run(z0[:cut], poff), run(z0[cut:], poff + cut)
        assert torch.equal(torch.cat([a["traj"], b["traj"]], 1), full["traj"]), cut
        assert torch.equal(torch.cat([a["tau"], b["tau"]], 1), full["tau"]), cut
        assert torch.equal(torch.cat([a["last"], b["last"]], 0), full["last"]), cut
    names = ("traj", "tau", "last")
    for sel in itertools.product([False, True], repeat=3):  # every subset of the nullable outputs
        got = run(z0, poff, **dict(zip(names, sel)))
        assert set(got) == {k for k, on in zip(names, sel) if on}
        for k in got:
            assert torch.equal(got[k], full[k]), (sel, k)
    for ld in (2 * d + 3, 2 * d + 4):  # z0 as a column view of a wider buffer
        wide = torch.full((c.N, ld), float("nan"), device=DEV)
        wide[:, :2 * d] = z0
        view = wide[:, :2 * d]
        assert view.stride(0) == ld
        got = run(view, poff)
        for k in names:
            assert torch.equal(got[k], full[k]), (ld, k)


# ---- f. fused moments, entry by entry ---------------------------------------------------------------------------
@pytest.mark.parametrize("N", [321, 2853])
@pytest.mark.parametrize("pot,K", [("quadratic", 0), ("gmm", 3)])
@pytest.mark.parametrize("d", R.MOM_DIMS)
def test_fused_moments_vs_fp64(native, d, pot, K, N):
    """The three moment sets of sde_simulate_kernel<d, POT, MOM = true> against the fp64 moments of z0 and of the
    GPU's own traj and last: kmv_sums_ref.moments_yardstick with the kernel's chain lengths, the counts exactly."""
    n = 5
    c = R.case(pot, d, N=N, n_steps=n, K=K)
    inp = R.inputs(c)
    res = _simulate(native, c, inp, moments=True)
    worst = _check_run(c, inp, res, R.tau0_of(inp["u"]), R.case_id(c) + " moments")
    _family("sde_simulate_kernel" + (" quadratic" if pot == "quadratic" else " GMM KM=4") + ", fused moments", worst)
    chains_0t, chains_row = R.mom_chains(n)
    sets = ((0, "initial", inp["z0"], chains_row, N),
            (1, "0T", res["traj"].transpose(1, 0, 2).reshape(N * n, 2 * d), chains_0t, N * n),  # a lane's rows adjacent
            (2, "terminal", res["last"], chains_row, N))
    mom = res["moments"]
    assert mom.shape == (3, KR.moment_len(2 * d)) and mom.dtype == np.float64
    worst_m = 0.0
    for k, name, rows, chains, count in sets:
        assert mom[k, 0] == count, (name, mom[k, 0])
        ref = nr.moments(rows)
        E = KR.moments_yardstick(rows, chains, ref)
        worst_m = max(worst_m, KR.check_entries(mom[k], ref, E, f"fused moments {name} d={d} {pot} N={N}"))
    _family("fused moments / E (kmv_sums_ref.FACTOR)", worst_m)


# ---- g. the per-update mean-field driver ------------------------------------------------------------------------
@pytest.mark.parametrize("d", R.DIMS)
def test_mf_step_vs_fp64(native, d):
    """mf_step_kernel<d>: the tau0 update, a dt update and the final update from given rows and a given xbar_sum;
    d_xsum = [count, sum x'] against the fp64 sums of the GPU's own output rows."""
    c = R.case("meanfield", d)
    inp = R.inputs(c)
    N, n = c.N, c.n_steps
    rng = np.random.default_rng(900 + d)
    xbar_sum = np.concatenate([[N], N * 0.4 * rng.standard_normal(d)])
    xb32 = (xbar_sum[1:] / xbar_sum[0]).astype(F32)  # the kernel's (float)(sum / count)
    inp["xbar"] = np.tile(xb32, (n + 1, 1))
    noise = _t(inp["xi"])  # held while the descriptor points at it
    desc, keep = native.mf_desc(N, d, n, R.DT, R.GAMMA, inp["A"], seed=SEED, counter_offset=CTR, noise_scale=c.ns,
                                noise=noise)
    ws = native.mf_workspace(desc, DEV)
    zin, xs = _t(inp["z0"]), _t(xbar_sum, torch.float64)
    outs = {}
    for s in (0, 1, n):
        zout, tau_row = torch.empty((N, 2 * d), device=DEV), torch.empty(N, device=DEV)
        xsum = torch.empty(1 + d, device=DEV, dtype=torch.float64)
        native.mf_step(desc, s, zin, zout, tau_row, xs, ws, xsum)
        outs[s] = (zout.cpu().numpy(), tau_row.cpu().numpy(), xsum.cpu().numpy())
    del keep, noise
    tau0 = outs[0][1]  # tau_value(tau0, 0, dt) = tau0: the ensemble's shared clock
    assert (tau0 == tau0[0]).all() and 0 <= tau0[0] < F32(R.DT)
    hs = R.step_sizes(tau0, n)
    erel = R.e_rel(c, inp, tau0)
    worst = worst_x = 0.0
    for s, (zout, tau_row, xsum) in outs.items():
        assert np.array_equal(tau_row, tau0 + F32(s) * F32(R.DT)), s
        ref = R.update64(c, inp, inp["z0"], hs[s], inp["xi"][s], s)
        S = R.scale(c, inp, inp["z0"], hs[s], inp["xi"][s], s)
        worst = max(worst, R.check_update(zout, ref, S, erel, f"mf_step d={d} update {s}"))
        assert xsum[0] == N
        terms = np.concatenate([np.ones((N, 1), F32), zout[:, :d]], 1)
        sums = terms.astype(np.float64).sum(0)
        E = R.sums_yardstick(terms, R.MF_STEP_CHAINS, sums)
        worst_x = max(worst_x, KR.check_entries(xsum, sums, E, f"mf_step d={d} update {s} xsum"))
    _family("mf_step_kernel", worst)
    _family("mf_step_kernel xsum / E (kmv_sums_ref.FACTOR)", worst_x)


@pytest.mark.parametrize("N", [321, 4500])  # 4500: 16 rows per lane and a second block of mf_sums_kernel
@pytest.mark.parametrize("d", [5, 6, 7, 10, 12, 16])
def test_mf_sums_and_mean_path_vs_fp64(native, d, N):
    """pdeinv_mf_sums with explicit noise against fp64 column sums, per entry; pdeinv_mf_mean_path against
    oracle.numpy_ref.mf_mean_path of the GPU's sums; then the simulate on that path under the update rule."""
    c = R.case("meanfield", d, N=N)
    inp = R.inputs(c)
    n = c.n_steps
    noise = _t(inp["xi"])  # held while the descriptor points at it
    desc, keep = native.mf_desc(N, d, n, R.DT, R.GAMMA, inp["A"], seed=SEED, counter_offset=CTR, noise=noise)
    z0 = _t(inp["z0"])
    sums_t = native.mf_sums(desc, z0)
    sums = sums_t.cpu().numpy()
    terms = np.concatenate([np.ones((N, 1), F32), inp["z0"]] + [inp["xi"][s] for s in range(n + 1)], 1)
    ref = terms.astype(np.float64).sum(0)
    assert sums.shape == ref.shape and sums[0] == N
    E = R.sums_yardstick(terms, R.MF_SUMS_CHAINS, ref)
    _family("mf_sums_kernel / E (kmv_sums_ref.FACTOR)", KR.check_entries(sums, ref, E, f"mf_sums d={d} N={N}"))
    xbar_t, xs_t = native.mf_mean_path(desc, sums_t)
    desc.d_meanfield = ctypes.c_void_p(xbar_t.data_ptr())
    out = dict(traj=torch.empty((n, N, 2 * d), device=DEV), tau=torch.empty((n, N), device=DEV),
               last=torch.empty((N, 2 * d), device=DEV))
    native.sde_simulate_desc(desc, z0, out["traj"], out["tau"], out["last"])
    res = _np(out)
    del keep, noise
    tau0 = res["tau"][0]
    assert (tau0 == tau0[0]).all()
    # the fp64 recursion rounded once to fp32: half an ulp of the reference, plus the two fp64 evaluations' difference
    path = nr.mf_mean_path(sums, d, n, R.DT, tau0[0], R.GAMMA)
    xbar, xs = xbar_t.cpu().numpy(), xs_t.cpu().numpy()
    assert np.all(np.abs(xbar - path[:n + 1]) <= 2.0 ** -24 * np.abs(path[:n + 1]) + 1e-12)
    assert np.array_equal(xs[:, 0], np.full(n + 2, float(N)))
    assert np.all(np.abs(xs[:, 1:] - N * path) <= 1e-12 * N * (1 + np.abs(path)))
    inp["xbar"] = xbar  # the path the kernel was given
    _family("sde_simulate_kernel mean-field", _check_run(c, inp, res, tau0, f"{R.case_id(c)} on its mean path"))


# ---- h. rejections -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [9, 11, 13, 14, 15])
def test_uncompiled_dims_are_rejected(native, d):
    c = R.case("quadratic", d, N=8)
    inp = R.inputs(c)
    inp["A"] = np.eye(d, dtype=F32)
    with pytest.raises(NotImplementedError):
        _simulate(native, c, inp)
    desc, keep = native.mf_desc(c.N, d, c.n_steps, R.DT, R.GAMMA, inp["A"], seed=SEED)
    z, xs = _t(inp["z0"]), _t(np.concatenate([[c.N], np.zeros(d)]), torch.float64)
    with pytest.raises(NotImplementedError):
        native.mf_step(desc, 1, z, torch.empty_like(z), None, xs, native.mf_workspace(desc, DEV),
                       torch.empty(1 + d, device=DEV, dtype=torch.float64))
    del keep


def test_fused_moments_are_rejected_at_d10(native):
    c = R.case("quadratic", 10, N=8)
    with pytest.raises(NotImplementedError):
        _simulate(native, c, R.inputs(c), moments=True)

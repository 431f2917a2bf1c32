"""GPU tests of the learned potential V_theta = V_hypothesis as a batch function (pdeinv_mlp_potential) and as the
simulator's potential (pdeinv_sde_simulate_mlp).

Parity rule (tests/mlp_sim_ref.py): the GPU's scaled error against the fp64 restatement is at most 16 x the fp32
restatement's own error against fp64 on the same inputs. Gradient rows and values are scaled by max |g| / max |V|
of the input set, trajectories as test_sde_gmm_explicit_noise scales them.

The potential tests evaluate one set of 1000 rows per shape. The rule is asserted on the n = 1000 call; the calls
with n in {1, 15, 16, 17} take the set's first n rows and must return the n = 1000 call's rows bit for bit (a row's
numbers depend on the row only: MFMA columns do not mix), which carries the rule to them. (The fp32 restatement's
error over one or fifteen rows is no measure of the format: a single correctly rounded number has error ~0 by
chance — 6e-9 for the first row's value of the d = 1 net — and 16 x that is below one ulp.)
"""
import numpy as np
import pytest
import torch

import mlp_sim_ref as R
from oracle import numpy_ref as nr

pytestmark = pytest.mark.gpu
DEV = "cuda"
DEFAULT = (4, 8, 20, 40)


def _t(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _np(t):
    return t.cpu().numpy()


def _check_rule(what, gpu, ref32, ref64, err):
    e_gpu, e_32 = err(gpu, ref64), err(ref32, ref64)
    print(f"{what}: gpu {e_gpu:.3e} fp32 {e_32:.3e} ratio {e_gpu / max(e_32, 1e-300):.2f}")
    assert e_gpu <= R.RULE * e_32, (what, e_gpu, e_32)


def _potential_case(native, shape, n_all=1000):
    d = shape[0]
    params, rng = R.make_net(*shape)
    x = R.positions(rng, n_all, d)
    dims, flat = R.dims_of(*shape), _t(R.flat32(params))
    V64, g64 = R.value_grad64(params, x)
    V32, g32 = R.value_grad32(params, x)
    v, g = native.mlp_potential(dims, flat, _t(x))
    _check_rule(f"{shape} grad", _np(g), g32, g64, R.row_err)
    _check_rule(f"{shape} value", _np(v), V32, V64, R.row_err)
    return dims, flat, x, v, g


@pytest.mark.parametrize("shape", R.TILE_SHAPES)
def test_potential_tile_path(native, shape):
    assert native.mlp_potential_path(R.dims_of(*shape)) == 2
    dims, flat, x, v, g = _potential_case(native, shape)
    v1, none = native.mlp_potential(dims, flat, _t(x), True, False)
    none2, g1 = native.mlp_potential(dims, flat, _t(x), False, True)
    assert none is None and none2 is None and torch.equal(v1, v) and torch.equal(g1, g)
    for n in (1, 15, 16, 17):
        vn, gn = native.mlp_potential(dims, flat, _t(x[:n]))
        assert torch.equal(vn, v[:n]) and torch.equal(gn, g[:n]), n
    v0, g0 = native.mlp_potential(dims, flat, _t(x[:0]))
    assert v0.shape == (0,) and g0.shape == (0, shape[0])


def test_potential_strided_rows(native):
    """ld > d: the rows are a strided view (the position half of [x | v] samples)."""
    shape = (3, 3, 13, 7)
    dims, flat, x, v, g = _potential_case(native, shape)
    big = torch.full((x.shape[0], 11), float("nan"), device=DEV)
    big[:, 2:5] = _t(x)
    vs, gs = native.mlp_potential(dims, flat, big[:, 2:5])
    assert torch.equal(vs, v) and torch.equal(gs, g)


@pytest.mark.parametrize("shape", [(4, 2, 32, 40), (4, 2, 64, 40)])
def test_potential_row_engine_path(native, shape):
    assert native.mlp_potential_path(R.dims_of(*shape)) == 1
    dims, flat, x, v, g = _potential_case(native, shape)
    v1, _ = native.mlp_potential(dims, flat, _t(x), True, False)
    _, g1 = native.mlp_potential(dims, flat, _t(x), False, True)
    assert torch.equal(v1, v) and torch.equal(g1, g)


def test_potential_path_table(native):
    assert native.mlp_potential_path(R.dims_of(*DEFAULT)) == 2
    assert native.mlp_potential_path(R.dims_of(4, 2, 32, 40)) == 1
    assert native.mlp_potential_path(R.dims_of(4, 2, 64, 40)) == 1
    assert native.mlp_potential_path(R.dims_of(4, 2, 2048, 40)) == 0
    with pytest.raises(NotImplementedError):
        dims = R.dims_of(4, 2, 2048, 40)
        P = native.lib().pdeinv_mlp_param_count(4, 2, 2048, 40)
        native.mlp_potential(dims, torch.zeros(P, device=DEV), torch.zeros((4, 4), device=DEV))


def _ensemble(shape, N, n, with_noise=True):
    d = shape[0]
    params, rng = R.make_net(*shape)
    z0 = np.concatenate([R.positions(rng, N, d), R.velocities(rng, N, d)], 1)
    xi = rng.standard_normal((n + 1, N, d)).astype(np.float32) if with_noise else None
    u = rng.random(N).astype(np.float32) if with_noise else None
    return params, z0, xi, u


@pytest.mark.parametrize("shape", R.TILE_SHAPES)
def test_simulator_explicit_noise(native, shape):
    N, n, dt, gamma = 257, 20, 0.02, 0.5
    params, z0, xi, u = _ensemble(shape, N, n)
    res = native.sde_simulate_mlp(_t(z0), n, dt, gamma, R.dims_of(*shape), _t(R.flat32(params)), seed=1,
                                  noise=_t(xi), shift_u=_t(u))
    l64, t64, _ = nr.sde_scan(z0, n, dt, gamma, R.grad_fn64(params), xi, u)
    l32, t32, tau32 = R.sde_scan32(z0, n, dt, gamma, params, xi, u)
    assert np.isfinite(t64).all()
    _check_rule(f"{shape} traj", _np(res["traj"]), t32, t64, R.traj_err)
    _check_rule(f"{shape} last", _np(res["last"]), l32, l64, R.traj_err)
    assert tau32.dtype == np.float32 and np.array_equal(_np(res["tau"]), tau32)


@pytest.mark.parametrize("poff", [0, 5_000_000_000])
def test_shift_stream(native, poff):
    """Philox mode: tau is the stream of pdeinv_sde_simulate bit for bit."""
    N, n, dt = 300, 7, 0.02
    params, z0, _, _ = _ensemble(DEFAULT, N, n, False)
    kw = dict(seed=0xDEADBEEF12345, counter_offset=77, particle_offset=poff)
    a = native.sde_simulate_mlp(_t(z0), n, dt, 0.5, R.dims_of(*DEFAULT), _t(R.flat32(params)), traj=False,
                                last=False, **kw)
    b = native.sde_simulate(_t(z0), n, dt, 0.5, dict(kind=native.POT_NONE), traj=False, last=False, **kw)
    assert torch.equal(a["tau"], b["tau"])


def test_philox_mode_vs_restatement(native, oracle_lib):
    """Philox noise: normals from the C oracle's stream per particle and update, tau0 from pdeinv_sde_tau0.
    Bound: 4 x the larger of (a) the fp32-vs-fp64 restatement deviation and (b) the restatement's deviation when
    its normals move by +-2e-6 (1 + |xi|), the documented GPU-vs-libm normal tolerance (test_gpu_kernels.py)."""
    N, n, dt, gamma = 130, 20, 0.02, 0.5
    d = DEFAULT[0]
    seed, off, poff = 0x1234567ABCDEF, 41, (1 << 32) - 100
    params, z0, _, _ = _ensemble(DEFAULT, N, n, False)
    res = native.sde_simulate_mlp(_t(z0), n, dt, gamma, R.dims_of(*DEFAULT), _t(R.flat32(params)), seed=seed,
                                  counter_offset=off, particle_offset=poff)
    xi = np.stack([np.stack([oracle_lib.sim_normals(seed, poff + i, off + s, d) for i in range(N)])
                   for s in range(n + 1)])
    tau0 = _np(native.sde_tau0(N, dt, seed=seed, counter_offset=off, particle_offset=poff)).astype(np.float64)
    u = tau0 / np.float64(np.float32(dt))
    g64 = R.grad_fn64(params)
    l64, t64, tau64 = nr.sde_scan(z0, n, np.float64(np.float32(dt)), gamma, g64, xi, u)
    l32, t32, _ = R.sde_scan32(z0, n, dt, gamma, params, xi, u.astype(np.float32))
    sgn = np.random.default_rng(5).choice([-1.0, 1.0], size=xi.shape)
    xp = xi.astype(np.float64) + sgn * 2e-6 * (1 + np.abs(xi))
    lp, tp, _ = nr.sde_scan(z0, n, np.float64(np.float32(dt)), gamma, g64, xp, u)
    for name, gpu, r64, r32, rp in (("traj", res["traj"], t64, t32, tp), ("last", res["last"], l64, l32, lp)):
        a, b, e = R.traj_err(r32, r64), R.traj_err(rp, r64), R.traj_err(_np(gpu), r64)
        print(f"philox {name}: gpu {e:.3e} (a) {a:.3e} (b) {b:.3e}")
        assert e <= 4 * max(a, b), (name, e, a, b)
    assert np.allclose(_np(res["tau"]), tau64, rtol=0, atol=1e-6)


def test_sharding_and_edges(native):
    N, n, dt, gamma, P0 = 300, 20, 0.02, 0.5, (1 << 32) - 70
    params, z0, _, _ = _ensemble(DEFAULT, N, n, False)
    z, dims, flat = _t(z0), R.dims_of(*DEFAULT), _t(R.flat32(params))

    def run(lo, hi, **kw):
        return native.sde_simulate_mlp(z[lo:hi], n, dt, gamma, dims, flat, seed=9, counter_offset=3,
                                       particle_offset=P0 + lo, **kw)

    full = run(0, N)
    assert torch.isfinite(full["traj"]).all()
    for cut in (150, 160):
        a, b = run(0, cut), run(cut, N)
        assert torch.equal(torch.cat([a["traj"], b["traj"]], 1), full["traj"]), cut
        assert torch.equal(torch.cat([a["tau"], b["tau"]], 1), full["tau"]), cut
        assert torch.equal(torch.cat([a["last"], b["last"]], 0), full["last"]), cut
    for traj, tau in ((False, True), (True, False), (False, False)):
        r = run(0, N, traj=traj, tau=tau)
        assert ("traj" in r) == traj and ("tau" in r) == tau
        assert torch.equal(r["last"], full["last"])
        assert not traj or torch.equal(r["traj"], full["traj"])
        assert not tau or torch.equal(r["tau"], full["tau"])
    r = run(0, N, last=False)
    assert "last" not in r and torch.equal(r["traj"], full["traj"])
    for m in (0, 1, 16, 65):
        r = run(0, m)
        assert r["traj"].shape == (n, m, 8) and r["tau"].shape == (n, m) and r["last"].shape == (m, 8)
        assert torch.equal(r["traj"], full["traj"][:, :m]) and torch.equal(r["tau"], full["tau"][:, :m])
        assert torch.equal(r["last"], full["last"][:m])


def test_envelope(native):
    def sim(d, L, W):
        dims = R.dims_of(d, L, W, 40)
        P = native.lib().pdeinv_mlp_param_count(d, L, W, 40)
        return native.sde_simulate_mlp(torch.zeros((32, 2 * d), device=DEV), 5, 0.02, 0.5, dims,
                                       torch.zeros(P, device=DEV), seed=1)

    for d, L, W in ((4, 2, 32), (4, 9, 20), (9, 2, 20)):
        with pytest.raises(NotImplementedError, match="dim <= 8, width <= 20"):
            sim(d, L, W)
    with pytest.raises(NotImplementedError, match="unknown potential kind"):
        native.sde_simulate(torch.zeros((32, 8), device=DEV), 5, 0.02, 0.5, dict(kind=native.POT_MLP), seed=1)


def _model_and_tree(shape):
    from core.model import V_hypothesis
    d, L, W, O = shape
    params, rng = R.make_net(*shape)
    model = V_hypothesis(1, [W] * L, out_features=O)
    return model, model.unflat(_t(R.flat32(params)), d), params, rng


def test_python_surface_scan_and_moments(native):
    from core.potential import MLPPotential
    from utils import prng
    from utils.sampling_utils import simulate, underdamped_langevin_dynamics_scan
    N, n, dt, gamma = 203, 11, 0.02, 0.5
    model, tree, params, rng = _model_and_tree(DEFAULT)
    z0 = _t(np.concatenate([R.positions(rng, N, 4), R.velocities(rng, N, 4)], 1))
    pot, key = MLPPotential(model, tree), prng.PRNGKey(3)
    last, traj, tau = underdamped_langevin_dynamics_scan(z0, n, dt, key, pot.gradient, gamma)
    ref = native.sde_simulate_mlp(z0, n, dt, gamma, R.dims_of(*DEFAULT), _t(R.flat32(params)), seed=key.seed)
    assert traj.shape == (N, n, 8) and tau.shape == (N, n) and last.shape == (N, 8)
    assert torch.equal(last, ref["last"]) and torch.equal(traj, ref["traj"].permute(1, 0, 2))
    assert torch.equal(tau, ref["tau"].permute(1, 0))
    r = simulate(z0, n, dt, key, pot, gamma, moments=True)
    mom = _np(r["moments"])
    refs = [nr.moments(_np(z0)), nr.moments(_np(r["traj"])), nr.moments(_np(r["last"]))]
    for k in range(3):
        assert np.allclose(mom[k], refs[k], rtol=2e-5, atol=1e-3 * max(1.0, refs[k][0] ** 0.5)), k
    with pytest.raises(ValueError):
        simulate(z0, n, dt, key, pot, gamma, moments=True, traj=False)
    x = z0[:, :4]
    v, g = native.mlp_potential(R.dims_of(*DEFAULT), _t(R.flat32(params)), x)
    assert torch.equal(pot.value(x), v) and torch.equal(pot.gradient(x), g)
    assert torch.equal(pot.gradient(x[0]), g[0])


def test_relative_gradient_error(native):
    """The metric equals the same ratio computed from the fp64 restatement on the samples it drew. The gradient
    obeys the rule of the potential tests (errors of a few 1e-7 of max |g|, x 16), hence <= 1e-4 on the ratio."""
    from example_problems.kinetic_fokker_planck_example_OU import KineticFokkerPlanck
    from methods.consistency_instances import kinetic_fokker_planck as kfp
    from utils import config, prng
    d, n = 4, 10000
    cfg = config.compose("config", ["pde_instance=kinetic_fokker_planck", f"pde_instance.domain_dim={d}"])
    pi = KineticFokkerPlanck(cfg, prng.PRNGKey(0))
    model, tree, params, _ = _model_and_tree(DEFAULT)
    rng = prng.PRNGKey(17)
    out = kfp.relative_gradient_error(model.apply, tree, pi, rng, n=n)
    assert kfp.test_fn(model.apply, pi, rng) == {}
    F = np.asarray(pi.initial_configuration["tilde_F"], np.float64)
    k_i, k_t = prng.split(rng, 2)
    for name, dist_, key in (("initial", pi.distribution_initial, k_i), ("terminal", pi.distribution_terminal, k_t)):
        x = _np(dist_.sample(n, key))[:, :d].astype(np.float64)
        g = R.value_grad64(params, x)[1]
        gt = x @ F.T
        ref = np.sqrt(np.mean(np.sum((g - gt) ** 2, -1)) / np.mean(np.sum(gt ** 2, -1)))
        got = float(out[f"relative error of gradient estimation {name}"])
        print(f"relative gradient error {name}: {got:.8e} ref {ref:.8e}")
        assert abs(got - ref) <= 1e-4 * ref

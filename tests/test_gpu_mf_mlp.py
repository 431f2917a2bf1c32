"""GPU tests of the learned interaction Phi_theta = V_hypothesis of the kinetic McKean–Vlasov system: the mean-field
force (pdeinv_mf_mlp_force), the per-update simulator (pdeinv_mf_mlp_step through utils.mean_field) and the Python
surface on top of them.

Yardstick (tests/mf_mlp_ref.py): the rule of tests/mlp_sim_ref.py — 16 x the fp32 restatement's error against fp64 —
applied per pair: max |F_gpu - F_64| <= 16 E_pair, and per update, teacher-forced from the GPU's own previous state,
max |z_gpu - z_64| <= 16 (h_s E_pair,s + E_upd,s). Every check prints its measured ratio to the yardstick.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mf_mlp_ref as M
import mlp_sim_ref as R
import mp_mf_mlp_worker as W

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = (4, 8, 20, 40)
FORCE_SHAPES = [(4, 8, 20, 40), (2, 8, 20, 40), (8, 8, 20, 40), (3, 3, 13, 7), (1, 2, 20, 40), (5, 2, 17, 40),
                (4, 1, 20, 40)]
C = M.CHUNK
REF_COUNTS = (1, 15, 16, 17, C - 1, C, C + 1, 2 * C + 44)
SIM_CASES = [((4, 8, 20, 40), 257), ((2, 8, 20, 40), 300), ((8, 8, 20, 40), 65), ((3, 3, 13, 7), 40),
             ((1, 2, 20, 40), 17), ((5, 2, 17, 40), 33)]


def _t(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _np(t):
    return t.cpu().numpy()


def _check_force(what, f_gpu, f64, e_pair):
    err = float(np.max(np.abs(_np(f_gpu).astype(np.float64) - f64)))
    print(f"{what}: |F_gpu - F_64| {err:.3e} E_pair {e_pair:.3e} ratio {err / e_pair:.2f}")
    assert e_pair > 0 and err <= M.RULE * e_pair, (what, err, e_pair)


def _model_and_tree(shape):
    from core.model import V_hypothesis
    d, L, Wd, O = shape
    params, rng = R.make_net(*shape)
    model = V_hypothesis(1, [Wd] * L, out_features=O)
    return model, model.unflat(_t(R.flat32(params)), d), params, rng


# ---- force ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", FORCE_SHAPES)
def test_force_parity(native, shape):
    """n = 40 items against m references (items != references), m around the tile and the chunk sizes."""
    d = shape[0]
    params, rng = R.make_net(*shape)
    dims, flat = R.dims_of(*shape), _t(R.flat32(params))
    x, r = R.positions(rng, 40, d), R.positions(rng, max(REF_COUNTS), d)
    g64, g32 = M.pair_grads(params, x, r)  # once per shape: the cases are prefixes of the reference set
    xd, rd = _t(x), _t(r)
    for m in REF_COUNTS:
        e_pair = float(np.max(np.abs(g32[:, :m].astype(np.float64) - g64[:, :m])))
        _check_force(f"{shape} m={m}", native.kmv_mlp_force(dims, flat, xd, rd[:m]), g64[:, :m].mean(1), e_pair)


def test_force_parity_self_pairs(native):
    """ref=None: the items are the references (n = m = 300), the self pair y = 0 included."""
    params, rng = R.make_net(*DEFAULT)
    x = R.positions(rng, 300, 4)
    f64, e_pair = M.force64(params, x, x)
    f = native.kmv_mlp_force(R.dims_of(*DEFAULT), _t(R.flat32(params)), _t(x))
    _check_force("self pairs n=m=300", f, f64, e_pair)
    assert torch.equal(f, native.kmv_mlp_force(R.dims_of(*DEFAULT), _t(R.flat32(params)), _t(x), _t(x)))


@pytest.mark.parametrize("shape", [(4, 8, 20, 40), (5, 2, 17, 40)])
def test_force_bit_exact_invariants(native, shape):
    d = shape[0]
    params, rng = R.make_net(*shape)
    dims, flat = R.dims_of(*shape), _t(R.flat32(params))
    n, m = 40, 2 * C + 44
    x, r = _t(R.positions(rng, n, d)), _t(R.positions(rng, m, d))
    full = native.kmv_mlp_force(dims, flat, x, r)
    assert torch.isfinite(full).all()
    for cut in (1, 16, 17):  # a row does not depend on the items that share its call
        a, b = native.kmv_mlp_force(dims, flat, x[:cut], r), native.kmv_mlp_force(dims, flat, x[cut:], r)
        assert torch.equal(torch.cat([a, b]), full), cut
    assert native.kmv_mlp_force(dims, flat, x[:0], r).shape == (0, d)
    assert torch.equal(native.kmv_mlp_force(dims, flat, x[:1], r), full[:1])
    # strided [x | v] views give the bits of contiguous copies
    zx = torch.full((n, 2 * d + 3), float("nan"), device=DEV)
    zr = torch.full((m, 2 * d), float("nan"), device=DEV)
    zx[:, 1:1 + d], zr[:, :d] = x, r
    assert torch.equal(native.kmv_mlp_force(dims, flat, zx[:, 1:1 + d], zr[:, :d]), full)
    with pytest.raises(ValueError, match="m < 1"):
        native.kmv_mlp_force(dims, flat, x, r[:0])


def test_envelope(native):
    from utils.mean_field import simulate_mean_field
    from utils.prng import PRNGKey
    for d, L, Wd in ((4, 2, 32), (9, 2, 20), (4, 9, 20)):
        dims = R.dims_of(d, L, Wd, 40)
        P = native.lib().pdeinv_mlp_param_count(d, L, Wd, 40)
        flat = torch.zeros(P, device=DEV)
        with pytest.raises(NotImplementedError, match="dim <= 8, width <= 20, 1 <= n_layers <= 8"):
            native.kmv_mlp_force(dims, flat, torch.zeros((8, d), device=DEV))
        with pytest.raises(NotImplementedError, match="dim <= 8, width <= 20, 1 <= n_layers <= 8"):
            native.mf_mlp_prepare(dims, flat, 8, 8)
        model, tree, _, _ = _model_and_tree((d, L, Wd, 40))
        from core.potential import MeanFieldMLPPotential
        with pytest.raises(NotImplementedError, match="dim <= 8, width <= 20, 1 <= n_layers <= 8"):
            simulate_mean_field(torch.zeros((8, 2 * d), device=DEV), 3, 0.02, PRNGKey(1),
                                MeanFieldMLPPotential(model, tree), 0.5)


# ---- simulator -----------------------------------------------------------------------------------
def _teacher_forced(what, params, z0, res, n, dt, gamma, xi, tau_row0, random_shift=True):
    """Every update from the GPU's own previous state; prints and returns the largest ratio to the yardstick."""
    d = z0.shape[1] // 2
    h = M.step_sizes(tau_row0, n, dt, random_shift)
    traj, last = _np(res["traj"]), _np(res["last"])
    worst = 0.0
    for s in range(n + 1):
        z_prev = z0 if s == 0 else traj[s - 1]
        z_gpu = last if s == n else traj[s]
        z64, yard = M.teacher_forced_update(params, z_prev, z_prev[:, :d], h[s], gamma, xi[s])
        err = float(np.max(np.abs(z_gpu.astype(np.float64) - z64)))
        assert err <= M.RULE * yard, (what, s, err, yard)
        worst = max(worst, err / yard if yard > 0 else 0.0)
    print(f"{what}: max over updates of |z_gpu - z_64| / (h E_pair + E_upd) = {worst:.2f}")
    return worst


@pytest.mark.parametrize("shape,N", SIM_CASES)
def test_simulator_teacher_forced(native, shape, N):
    from core.potential import MeanFieldMLPPotential
    from utils.mean_field import simulate_mean_field, stamp_times
    from utils.prng import PRNGKey
    n, dt, gamma, ctr = 20, 0.02, 0.5, 5
    d = shape[0]
    model, tree, params, rng = _model_and_tree(shape)
    z0 = np.concatenate([R.positions(rng, N, d), R.velocities(rng, N, d)], 1)
    xi = rng.standard_normal((n + 1, N, d)).astype(np.float32)
    key = PRNGKey(100 + d)
    res = simulate_mean_field(_t(z0), n, dt, key, MeanFieldMLPPotential(model, tree), gamma, counter_offset=ctr,
                              noise=_t(xi))
    assert set(res) == {"last", "traj", "tau"}  # no xsum / xbar: no closed-form mean
    tau = stamp_times(key.seed, ctr, n, dt)
    assert np.array_equal(_np(res["tau"]), np.broadcast_to(tau[:, None], (n, N)))
    _teacher_forced(f"{shape} N={N}", params, z0, res, n, dt, gamma, xi, tau[0])


def test_simulator_without_shift(native):
    """random_shift=False: tau0 = 0, update 0 has h = 0 and leaves z0 unchanged; the rest obey the yardstick."""
    from core.potential import MeanFieldMLPPotential
    from utils.mean_field import simulate_mean_field, stamp_times
    from utils.prng import PRNGKey
    shape, N, n, dt, gamma = (3, 3, 13, 7), 40, 20, 0.02, 0.5
    model, tree, params, rng = _model_and_tree(shape)
    z0 = np.concatenate([R.positions(rng, N, 3), R.velocities(rng, N, 3)], 1)
    xi = rng.standard_normal((n + 1, N, 3)).astype(np.float32)
    res = simulate_mean_field(_t(z0), n, dt, PRNGKey(2), MeanFieldMLPPotential(model, tree), gamma, noise=_t(xi),
                              random_shift=False)
    assert np.array_equal(_np(res["traj"][0]), z0)
    tau = stamp_times(2, 0, n, dt, random_shift=False)
    assert tau[0] == 0 and np.array_equal(_np(res["tau"]), np.broadcast_to(tau[:, None], (n, N)))
    _teacher_forced("no shift", params, z0, res, n, dt, gamma, xi, 0.0, random_shift=False)
    for traj, tau_ in ((False, True), (True, False), (False, False)):  # two-slot state ring without traj
        r = simulate_mean_field(_t(z0), n, dt, PRNGKey(2), MeanFieldMLPPotential(model, tree), gamma, noise=_t(xi),
                                random_shift=False, traj=traj, tau=tau_)
        assert ("traj" in r) == traj and ("tau" in r) == tau_ and torch.equal(r["last"], res["last"])


@pytest.mark.parametrize("poff", [0, (1 << 32) - 70])
def test_philox_stream_is_the_quadratic_drivers(native, poff):
    """Philox mode. With a zero output layer grad Phi_theta = 0 exactly, and with A = 0 so is the quadratic drift:
    both per-update drivers then apply the same noise and step sizes to the same rows, so tau, traj and last agree
    bit for bit exactly when key, counter offset and particle ids give the same stream (ids past 2^32 included)."""
    from core.potential import MeanFieldQuadraticPotential
    from utils.mean_field import simulate_mean_field
    from utils.prng import PRNGKey
    N, n, dt, gamma, ctr = 300, 7, 0.02, 0.5, 77
    params, rng = M.zero_force_net(*DEFAULT)
    z0 = _t(np.concatenate([R.positions(rng, N, 4), R.velocities(rng, N, 4)], 1))
    key = PRNGKey(0xDEADBEEF12345)
    quad = simulate_mean_field(z0, n, dt, key, MeanFieldQuadraticPotential(np.zeros((4, 4))), gamma,
                               particle_offset=poff, counter_offset=ctr, exchange="per_update")
    traj, tau, last = M.native_steps(native, R.dims_of(*DEFAULT), _t(R.flat32(params)), z0, n, dt, gamma,
                                     lambda s, zin: zin[:, :4], seed=key.seed, counter_offset=ctr,
                                     particle_offset=poff)
    assert torch.equal(tau, quad["tau"])
    assert torch.equal(traj, quad["traj"]) and torch.equal(last, quad["last"])
    assert not torch.equal(traj[1], traj[0])  # the noise moved the rows
    other = M.native_steps(native, R.dims_of(*DEFAULT), _t(R.flat32(params)), z0, n, dt, gamma,
                           lambda s, zin: zin[:, :4], seed=key.seed, counter_offset=ctr, particle_offset=poff + 1)
    assert not torch.equal(other[0], traj)  # and depends on the ids


def _worker_case():
    params, z0 = W.ensemble()
    return params, _t(z0), W.potential(params, DEV)


def test_sharding_through_the_step_binding(native):
    """[0, 150) and [150, 300) as two calls per update with particle_offset, both against the full reference set:
    the rows of the single call, bit for bit (Philox noise: the ids are the stream)."""
    params, rng = R.make_net(*DEFAULT)
    N, n, dt, gamma, P0 = 300, 20, 0.02, 0.5, 1000
    z0 = _t(np.concatenate([R.positions(rng, N, 4), R.velocities(rng, N, 4)], 1))
    dims, flat = R.dims_of(*DEFAULT), _t(R.flat32(params))
    kw = dict(seed=9, counter_offset=3)
    traj, tau, last = M.native_steps(native, dims, flat, z0, n, dt, gamma, lambda s, zin: zin[:, :4],
                                     particle_offset=P0, **kw)
    assert torch.isfinite(traj).all()
    full_pos = lambda s, zin: (z0 if s == 0 else traj[s - 1])[:, :4]  # noqa: E731
    parts = [M.native_steps(native, dims, flat, z0[lo:hi], n, dt, gamma, full_pos, particle_offset=P0 + lo, **kw)
             for lo, hi in ((0, 150), (150, 300))]
    assert torch.equal(torch.cat([p[0] for p in parts], 1), traj)
    assert torch.equal(torch.cat([p[1] for p in parts], 1), tau)
    assert torch.equal(torch.cat([p[2] for p in parts], 0), last)


def test_two_ranks_equal_one_process(native, tmp_path):
    """Two ranks on the one GPU over gloo through simulate_mean_field (shares of 151 and 150 particles, n_global
    from the all-reduced counts): traj / last bit-identical to the one-process run."""
    from utils.mean_field import simulate_mean_field
    from utils.prng import PRNGKey
    _, z0, pot = _worker_case()
    one = simulate_mean_field(z0, W.N_STEPS, W.DT, PRNGKey(W.SEED), pot, W.GAMMA, counter_offset=W.CTR)
    env = dict(os.environ, PDEINV_DIST_BACKEND="gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", "--master-port=29671", os.path.join(ROOT, "tests", "mp_mf_mlp_worker.py"),
           str(tmp_path)]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stderr[-3000:]
    parts = [dict(np.load(tmp_path / f"rank{k}.npz")) for k in range(2)]
    assert [int(p["world"]) for p in parts] == [2, 2] and [int(p["off"]) for p in parts] == [0, 151]
    assert np.array_equal(np.concatenate([p["traj"] for p in parts], 1), _np(one["traj"]))
    assert np.array_equal(np.concatenate([p["last"] for p in parts], 0), _np(one["last"]))
    assert np.array_equal(np.concatenate([p["tau"] for p in parts], 1), _np(one["tau"]))


# ---- Python surface ------------------------------------------------------------------------------
def test_python_surface(native):
    from core.potential import MeanFieldMLPPotential
    from utils import prng
    from utils.mean_field import simulate_mean_field
    from utils.sampling_utils import simulate, underdamped_langevin_dynamics_scan
    N, n, dt, gamma = 203, 6, 0.02, 0.5
    model, tree, params, rng = _model_and_tree(DEFAULT)
    z0 = _t(np.concatenate([R.positions(rng, N, 4), R.velocities(rng, N, 4)], 1))
    pot, key = MeanFieldMLPPotential(model, tree), prng.PRNGKey(3)
    dims, flat = R.dims_of(*DEFAULT), _t(R.flat32(params))
    x, r = z0[:, :4], z0[:50, 4:]
    assert torch.equal(pot.force(x), native.kmv_mlp_force(dims, flat, x))
    assert torch.equal(pot.force(x, r), native.kmv_mlp_force(dims, flat, x, r))
    assert torch.equal(pot.gradient(x), pot.force(x))
    ref = simulate_mean_field(z0, n, dt, key, pot, gamma)
    got = simulate(z0, n, dt, key, pot, gamma)
    assert set(got) == {"last", "traj", "tau"} and all(torch.equal(got[k], ref[k]) for k in ref)
    assert torch.equal(simulate_mean_field(z0, n, dt, key, pot, gamma, exchange="per_update", n_global=N)["last"],
                       ref["last"])
    last, traj, tau = underdamped_langevin_dynamics_scan(z0, n, dt, key, pot.gradient, gamma)
    assert traj.shape == (N, n, 8) and tau.shape == (N, n) and torch.equal(last, ref["last"])
    t, _, l = M.native_steps(native, dims, flat, z0, n, dt, gamma, lambda s, zin: zin[:, :4], seed=key.seed)
    assert torch.equal(t, ref["traj"]) and torch.equal(l, ref["last"])
    with pytest.raises(ValueError, match="n_global"):
        simulate_mean_field(z0, n, dt, key, pot, gamma, n_global=N - 1)


def _kmv_instance(d=4):
    from example_problems.kinetic_mckean_vlasov_example_quadratic import KineticMcKeanVlasov
    from utils import config, prng
    cfg = config.compose("config", ["pde_instance=kinetic_mckean_vlasov", f"pde_instance.domain_dim={d}"])
    return KineticMcKeanVlasov(cfg, prng.PRNGKey(0))


def test_simulate_interacting_with_a_learned_interaction(native):
    from core.potential import MeanFieldMLPPotential
    from utils import prng
    pi = _kmv_instance()
    model, tree, _, _ = _model_and_tree(DEFAULT)
    z0q, rq = pi.simulate_interacting(prng.PRNGKey(5), 64, n_steps=6)
    z0, r = pi.simulate_interacting(prng.PRNGKey(5), 64, n_steps=6, interaction=MeanFieldMLPPotential(model, tree))
    assert torch.equal(z0, z0q)
    for k in ("traj", "tau", "last"):
        assert r[k].shape == rq[k].shape and r[k].dtype == rq[k].dtype and torch.isfinite(r[k]).all(), k
    assert "xsum" not in r and "xbar" not in r
    assert torch.equal(r["tau"][:, :1].expand_as(r["tau"]), r["tau"])  # one clock for the ensemble
    with pytest.raises(ValueError, match="stamp_sums"):
        pi.simulate_interacting(prng.PRNGKey(5), 64, n_steps=6, stamp_sums=True,
                                interaction=MeanFieldMLPPotential(model, tree))


def _ratio(f_theta, x64, F):
    """The metric's formula in fp64: F* = mean_j tilde_F (x_i - x_j) = tilde_F (x_i - xbar)."""
    ft = (x64 - x64.mean(0, keepdims=True)) @ F.T
    return np.sqrt(np.mean(np.sum((f_theta - ft) ** 2, -1)) / np.mean(np.sum(ft ** 2, -1))), ft


def test_relative_force_error(native):
    """The metric equals its fp64 restatement on the samples it drew (n = 200). Each force component is within
    16 E_pair of fp64, so the root-mean-square numerator moves by at most sqrt(d) 16 E_pair and the ratio by that
    over the denominator's root. With the true force in place of Phi_theta's the restatement is ~0."""
    from methods.consistency_instances import kinetic_mckean_vlasov as kmv
    from utils import prng
    d, n = 4, 200
    pi = _kmv_instance(d)
    model, tree, params, _ = _model_and_tree(DEFAULT)
    rng = prng.PRNGKey(17)
    out = kmv.relative_force_error(model.apply, tree, pi, rng, n=n)
    assert kmv.test_fn(model.apply, pi, rng) == {}
    F = np.asarray(pi.initial_configuration["tilde_F"], np.float64)
    k_i, k_t = prng.split(rng, 2)
    for name, dist_, key in (("initial", pi.distribution_initial, k_i), ("terminal", pi.distribution_terminal, k_t)):
        x = _np(dist_.sample(n, key))[:, :d]
        f64, e_pair = M.force64(params, x, x)
        x64 = x.astype(np.float64)
        ref, ft = _ratio(f64, x64, F)
        got = out[f"relative error of force estimation {name}"]
        assert got.dtype == torch.float64 and got.dim() == 0 and got.is_cuda
        tol = np.sqrt(d) * M.RULE * e_pair / np.sqrt(np.mean(np.sum(ft ** 2, -1)))
        print(f"relative force error {name}: {float(got):.8e} ref {ref:.8e} |diff| / tol "
              f"{abs(float(got) - ref) / tol:.3f}")
        assert abs(float(got) - ref) <= tol
        pairwise_true = ((x64[:, None, :] - x64[None, :, :]) @ F.T).mean(1)  # mean_j tilde_F (x_i - x_j)
        assert _ratio(pairwise_true, x64, F)[0] < 1e-12
    with pytest.raises(NotImplementedError):
        from core.model import QuadraticModel
        q = QuadraticModel(d)
        kmv.relative_force_error(q.apply, q.init(prng.PRNGKey(1), np.zeros(d)), pi, rng, n=n)

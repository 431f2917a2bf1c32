"""GPU tests of the wide learned potential (width 21..256): pdeinv_mlp_potential_wide as a batch function and
pdeinv_sde_simulate_mlp_wide as the simulator's potential.

Parity rule (tests/mlp_sim_ref.py, RULE = 16): the GPU's scaled error against the fp64 restatement is at most
16 x the fp32 restatement's own error against fp64 on the same inputs; row_err for gradient rows and values,
traj_err for trajectories. The rule is asserted on the 1000-row call; the short calls must return its rows bit for
bit, which carries the rule to them (see test_gpu_sim_mlp.py).

Shapes (d, L, W, O), each for a way the kernel can go wrong:
  (4, 2, 32, 40)   one slice set, the image resident in LDS
  (3, 2, 21, 7)    odd d (8-byte stores), width padded 21 -> 32, O < 16
  (1, 2, 48, 3)    d = 1, width 48
  (5, 1, 100, 40)  one layer, two coordinate k-steps, width padded 100 -> 112
  (2, 2, 128, 40)  streamed image, seven waves per block
  (4, 3, 64, 40)   three layers, resident with four waves
  (8, 2, 256, 40)  the C5 net: image larger than LDS, 80 slices cycle
  (4, 8, 64, 40)   at the layer limit of its width (64 x 8 = 512), streamed
"""
import functools
import itertools

import numpy as np
import pytest
import torch

import mlp_sim_ref as R
from oracle import numpy_ref as nr

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(4, 2, 32, 40), (3, 2, 21, 7), (1, 2, 48, 3), (5, 1, 100, 40), (2, 2, 128, 40), (4, 3, 64, 40),
          (8, 2, 256, 40), (4, 8, 64, 40)]
NARROW = (4, 8, 20, 40)
SMALL = (4, 2, 32, 40)


def _t(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _np(t):
    return t.cpu().numpy()


def _check_rule(what, gpu, ref32, ref64, err):
    e_gpu, e_32 = err(gpu, ref64), err(ref32, ref64)
    print(f"{what}: gpu {e_gpu:.3e} fp32 {e_32:.3e} ratio {e_gpu / max(e_32, 1e-300):.2f}")
    assert e_gpu <= R.RULE * e_32, (what, e_gpu, e_32)


@functools.lru_cache(maxsize=None)
def _potential_refs(shape, n_all=1000):
    """The net, 1000 rows and their fp64 / fp32 restatements: computed once per shape, never modified."""
    params, rng = R.make_net(*shape)
    x = R.positions(rng, n_all, shape[0])
    return params, x, R.value_grad64(params, x), R.value_grad32(params, x)


@pytest.mark.parametrize("shape", SHAPES)
def test_potential_wide(native, shape):
    params, x, (V64, g64), (V32, g32) = _potential_refs(shape)
    dims, flat, xd = R.dims_of(*shape), _t(R.flat32(params)), _t(x)
    assert native.sde_simulate_mlp_wide_supported(dims)
    v, g = native.mlp_potential_wide(dims, flat, xd)
    _check_rule(f"{shape} grad", _np(g), g32, g64, R.row_err)
    _check_rule(f"{shape} value", _np(v), V32, V64, R.row_err)
    v1, none = native.mlp_potential_wide(dims, flat, xd, True, False)
    none2, g1 = native.mlp_potential_wide(dims, flat, xd, False, True)
    assert none is None and none2 is None and torch.equal(v1, v) and torch.equal(g1, g)
    for n in (1, 15, 16, 17):
        vn, gn = native.mlp_potential_wide(dims, flat, xd[:n])
        assert torch.equal(vn, v[:n]) and torch.equal(gn, g[:n]), n
    v0, g0 = native.mlp_potential_wide(dims, flat, xd[:0])
    assert v0.shape == (0,) and g0.shape == (0, shape[0])
    d = shape[0]
    big = torch.full((x.shape[0], d + 8), float("nan"), device=DEV)  # ld > d: a strided view
    big[:, 2:2 + d] = xd
    vs, gs = native.mlp_potential_wide(dims, flat, big[:, 2:2 + d])
    assert torch.equal(vs, v) and torch.equal(gs, g)


@pytest.mark.parametrize("shape", [(4, 2, 32, 40), (4, 2, 64, 40)])
def test_potential_wide_beside_row_engine(native, shape):
    """Two independent GPU implementations, each held to the rule against fp64 on the same rows."""
    params, x, (V64, g64), (V32, g32) = _potential_refs(shape)
    dims, flat, xd = R.dims_of(*shape), _t(R.flat32(params)), _t(x)
    assert native.mlp_potential_path(dims) == 1
    for name, fn in (("wide", native.mlp_potential_wide), ("rows", native.mlp_potential)):
        v, g = fn(dims, flat, xd)
        _check_rule(f"{shape} {name} grad", _np(g), g32, g64, R.row_err)
        _check_rule(f"{shape} {name} value", _np(v), V32, V64, R.row_err)


def _ensemble(shape, N, n, with_noise=True):
    d = shape[0]
    params, rng = R.make_net(*shape)
    z0 = np.concatenate([R.positions(rng, N, d), R.velocities(rng, N, d)], 1)
    xi = rng.standard_normal((n + 1, N, d)).astype(np.float32) if with_noise else None
    u = rng.random(N).astype(np.float32) if with_noise else None
    return params, z0, xi, u


@pytest.mark.parametrize("shape", SHAPES)
def test_simulator_wide_explicit_noise(native, shape):
    N, n, dt, gamma = 257, 20, 0.02, 0.5
    params, z0, xi, u = _ensemble(shape, N, n)
    res = native.sde_simulate_mlp_wide(_t(z0), n, dt, gamma, R.dims_of(*shape), _t(R.flat32(params)), seed=1,
                                       noise=_t(xi), shift_u=_t(u))
    l64, t64, _ = nr.sde_scan(z0, n, dt, gamma, R.grad_fn64(params), xi, u)
    l32, t32, tau32 = R.sde_scan32(z0, n, dt, gamma, params, xi, u)
    assert np.isfinite(t64).all()
    _check_rule(f"{shape} traj", _np(res["traj"]), t32, t64, R.traj_err)
    _check_rule(f"{shape} last", _np(res["last"]), l32, l64, R.traj_err)
    assert tau32.dtype == np.float32 and np.array_equal(_np(res["tau"]), tau32)


@pytest.mark.parametrize("poff", [0, 5_000_000_000])
def test_shift_stream_wide(native, poff):
    """Philox mode: tau is the stream of pdeinv_sde_simulate bit for bit."""
    N, n, dt = 300, 7, 0.02
    params, z0, _, _ = _ensemble(SMALL, N, n, False)
    kw = dict(seed=0xDEADBEEF12345, counter_offset=77, particle_offset=poff)
    a = native.sde_simulate_mlp_wide(_t(z0), n, dt, 0.5, R.dims_of(*SMALL), _t(R.flat32(params)), traj=False,
                                     last=False, **kw)
    b = native.sde_simulate(_t(z0), n, dt, 0.5, dict(kind=native.POT_NONE), traj=False, last=False, **kw)
    assert torch.equal(a["tau"], b["tau"])


def test_philox_mode_vs_restatement_wide(native, oracle_lib):
    """The bound of test_philox_mode_vs_restatement: 4 x the larger of (a) the fp32-vs-fp64 restatement deviation
    and (b) the restatement's deviation when its normals move by +-2e-6 (1 + |xi|). Normals from the C oracle's
    stream per particle and update, tau0 from pdeinv_sde_tau0."""
    N, n, dt, gamma = 130, 20, 0.02, 0.5
    d = SMALL[0]
    seed, off, poff = 0x1234567ABCDEF, 41, (1 << 32) - 100
    params, z0, _, _ = _ensemble(SMALL, N, n, False)
    res = native.sde_simulate_mlp_wide(_t(z0), n, dt, gamma, R.dims_of(*SMALL), _t(R.flat32(params)), seed=seed,
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


@pytest.mark.parametrize("shape", [SMALL, (8, 2, 256, 40)])
def test_sharding_and_edges_wide(native, shape):
    """Resident and streamed image: a particle's bits depend on its global id and its row only."""
    N, n, dt, gamma, P0 = 300, 20, 0.02, 0.5, (1 << 32) - 70
    m2 = 2 * shape[0]
    params, z0, _, _ = _ensemble(shape, N, n, False)
    z, dims, flat = _t(z0), R.dims_of(*shape), _t(R.flat32(params))

    def run(lo, hi, **kw):
        return native.sde_simulate_mlp_wide(z[lo:hi], n, dt, gamma, dims, flat, seed=9, counter_offset=3,
                                            particle_offset=P0 + lo, **kw)

    full = run(0, N)
    assert torch.isfinite(full["traj"]).all()
    for cut in (150, 160):
        a, b = run(0, cut), run(cut, N)
        assert torch.equal(torch.cat([a["traj"], b["traj"]], 1), full["traj"]), cut
        assert torch.equal(torch.cat([a["tau"], b["tau"]], 1), full["tau"]), cut
        assert torch.equal(torch.cat([a["last"], b["last"]], 0), full["last"]), cut
    for traj, tau, last in itertools.product((False, True), repeat=3):  # every output combination, all-off too
        r = run(0, N, traj=traj, tau=tau, last=last)
        want = {k for k, on in (("traj", traj), ("tau", tau), ("last", last)) if on}
        assert set(r) == want, (traj, tau, last, set(r))
        for k in want:
            assert torch.equal(r[k], full[k]), (traj, tau, last, k)
    for m in (0, 1, 16, 65):
        r = run(0, m)
        assert r["traj"].shape == (n, m, m2) and r["tau"].shape == (n, m) and r["last"].shape == (m, m2)
        assert torch.equal(r["traj"], full["traj"][:, :m]) and torch.equal(r["tau"], full["tau"][:, :m])
        assert torch.equal(r["last"], full["last"][:m])


def test_second_tile_per_wave(native):
    """The grid rule of sde_mlp_wide.hip: blocks = min(ceil(tiles / waves), CUs), a block of `waves` <= 8 waves,
    a wave tile of 16 particles. With N = 16 * 8 * CUs + 40 there are more than 8 * CUs >= waves * CUs tiles, so
    at least one block (hence each of its waves) takes a second block tile. A call of at most 16 * CUs particles
    has at most CUs tiles and therefore at most CUs block tiles: no wave takes a second one."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    N, chunk, n, dt, gamma = 16 * 8 * cus + 40, 16 * cus, 3, 0.02, 0.5
    params, z0, _, _ = _ensemble(SMALL, N, n, False)
    z, dims, flat = _t(z0), R.dims_of(*SMALL), _t(R.flat32(params))

    def run(lo, hi):
        return native.sde_simulate_mlp_wide(z[lo:hi], n, dt, gamma, dims, flat, seed=21, counter_offset=5,
                                            particle_offset=lo)

    full = run(0, N)
    parts = [run(lo, min(lo + chunk, N)) for lo in range(0, N, chunk)]
    assert torch.isfinite(full["traj"]).all()
    assert torch.equal(torch.cat([p["traj"] for p in parts], 1), full["traj"])
    assert torch.equal(torch.cat([p["tau"] for p in parts], 1), full["tau"])
    assert torch.equal(torch.cat([p["last"] for p in parts], 0), full["last"])


def test_envelope_wide(native):
    def sim(d, L, W, O):
        dims = R.dims_of(d, L, W, O)
        P = native.lib().pdeinv_mlp_param_count(d, L, W, O)
        return native.sde_simulate_mlp_wide(torch.zeros((32, 2 * d), device=DEV), 5, 0.02, 0.5, dims,
                                            torch.zeros(P, device=DEV), seed=1)

    for s in ((4, 8, 20, 40), (9, 2, 32, 40), (4, 3, 256, 40), (4, 2, 257, 40), (4, 2, 32, 65)):
        assert not native.sde_simulate_mlp_wide_supported(R.dims_of(*s))
        with pytest.raises(NotImplementedError, match="21 <= width <= 256"):
            sim(*s)
        with pytest.raises(NotImplementedError, match="21 <= width <= 256"):
            P = native.lib().pdeinv_mlp_param_count(*s)
            native.mlp_potential_wide(R.dims_of(*s), torch.zeros(P, device=DEV), torch.zeros((4, s[0]), device=DEV))


def _model_and_tree(shape):
    from core.model import V_hypothesis
    d, L, W, O = shape
    params, rng = R.make_net(*shape)
    model = V_hypothesis(1, [W] * L, out_features=O)
    return model, model.unflat(_t(R.flat32(params)), d), params, rng


def test_python_surface_wide(native):
    from core.potential import MLPPotential
    from utils import prng
    from utils.sampling_utils import simulate, underdamped_langevin_dynamics_scan
    N, n, dt, gamma = 203, 11, 0.02, 0.5
    model, tree, params, rng = _model_and_tree(SMALL)
    z0 = _t(np.concatenate([R.positions(rng, N, 4), R.velocities(rng, N, 4)], 1))
    pot, key = MLPPotential(model, tree), prng.PRNGKey(3)
    last, traj, tau = underdamped_langevin_dynamics_scan(z0, n, dt, key, pot.gradient, gamma)
    ref = native.sde_simulate_mlp_wide(z0, n, dt, gamma, R.dims_of(*SMALL), _t(R.flat32(params)), seed=key.seed)
    assert traj.shape == (N, n, 8) and tau.shape == (N, n) and last.shape == (N, 8)
    assert torch.equal(last, ref["last"]) and torch.equal(traj, ref["traj"].permute(1, 0, 2))
    assert torch.equal(tau, ref["tau"].permute(1, 0))
    r = simulate(z0, n, dt, key, pot, gamma, moments=True)
    assert torch.equal(r["traj"], ref["traj"]) and torch.equal(r["last"], ref["last"])
    mom = _np(r["moments"])
    refs = [nr.moments(_np(z0)), nr.moments(_np(r["traj"])), nr.moments(_np(r["last"]))]
    for k in range(3):
        assert np.allclose(mom[k], refs[k], rtol=2e-5, atol=1e-3 * max(1.0, refs[k][0] ** 0.5)), k
    with pytest.raises(ValueError):
        simulate(z0, n, dt, key, pot, gamma, moments=True, traj=False)


def test_narrow_net_keeps_the_narrow_kernel(native):
    from core.potential import MLPPotential
    from utils import prng
    from utils.sampling_utils import simulate
    N, n, dt, gamma = 203, 11, 0.02, 0.5
    model, tree, params, rng = _model_and_tree(NARROW)
    z0 = _t(np.concatenate([R.positions(rng, N, 4), R.velocities(rng, N, 4)], 1))
    key = prng.PRNGKey(3)
    assert not native.sde_simulate_mlp_wide_supported(R.dims_of(*NARROW))
    r = simulate(z0, n, dt, key, MLPPotential(model, tree), gamma)
    ref = native.sde_simulate_mlp(z0, n, dt, gamma, R.dims_of(*NARROW), _t(R.flat32(params)), seed=key.seed)
    assert all(torch.equal(r[k], ref[k]) for k in ("traj", "tau", "last"))

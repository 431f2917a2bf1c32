"""GPU-less checks of the learned-interaction entry points (pdeinv_mf_mlp_*): exports, the envelope table, argument
validation before the HIP runtime is touched, the ValueError cases of the Python drivers, and the test helpers
against the oracle's pair-tensor restatement."""
import ctypes

import numpy as np
import pytest
import torch

import mf_mlp_ref as M
import mlp_sim_ref as R
from oracle import numpy_ref as nr

NEW_SYMBOLS = ("pdeinv_mf_mlp_supported", "pdeinv_mf_mlp_workspace_bytes", "pdeinv_mf_mlp_prepare",
               "pdeinv_mf_mlp_force", "pdeinv_mf_mlp_step")


def _lib():
    from utils import native
    return native, native.lib()


def test_library_exports_the_new_symbols():
    native, L = _lib()
    for s in NEW_SYMBOLS:
        assert s in native.EXPORTED_SYMBOLS and hasattr(L, s), s
    assert native.POT_MEANFIELD_MLP == 5 and L.pdeinv_abi_version() == native.ABI_VERSION == 10


def test_supported_matches_the_envelope_table():
    native, L = _lib()
    sup = lambda *s: L.pdeinv_mf_mlp_supported(ctypes.byref(native.MlpShape(*s)))  # noqa: E731
    wsb = lambda s, n, m: L.pdeinv_mf_mlp_workspace_bytes(ctypes.byref(native.MlpShape(*s)), n, m)  # noqa: E731
    for s in R.TILE_SHAPES + [(8, 8, 20, 1), (1, 1, 1, 1), (8, 8, 20, 4096)]:
        assert sup(*s) == 1 and wsb(s, 40, 300) > 0, s
    for s in [(4, 2, 32, 40), (4, 8, 21, 40), (4, 9, 20, 40), (9, 8, 20, 40), (0, 2, 20, 40), (4, 0, 20, 40),
              (4, 2, 0, 40), (4, 2, 20, 0)]:
        assert sup(*s) == 0 and wsb(s, 40, 300) == 0, s
    assert L.pdeinv_mf_mlp_supported(None) == 0
    assert native.mf_mlp_supported(R.dims_of(4, 8, 20, 40)) and not native.mf_mlp_supported(R.dims_of(4, 2, 32, 40))
    s = (4, 8, 20, 40)
    assert wsb(s, 40, 0) == 0 and wsb(s, -1, 5) == 0
    # the partials are per (item, chunk of references): one more chunk, more bytes
    assert wsb(s, 40, 1) == wsb(s, 40, M.CHUNK) < wsb(s, 40, M.CHUNK + 1) == wsb(s, 40, 2 * M.CHUNK)
    assert wsb(s, 0, 1) > 0


def test_argument_validation_without_gpu():
    native, L = _lib()
    INV, UNS, OK = native.PDEINV_ERR_INVALID, native.PDEINV_ERR_UNSUPPORTED, native.PDEINV_OK
    A = ctypes.c_void_p(256)  # an aligned non-null stand-in: every call below returns before it is read

    def force(shape=(4, 8, 20, 40), n=8, m=8, ldx=0, ldr=0, params=A, x=A, r=A, f=A, ws=A):
        s = native.MlpShape(*shape)
        return L.pdeinv_mf_mlp_force(ctypes.byref(s), params, x, n, ldx, r, m, ldr, f, ws, None)

    assert L.pdeinv_mf_mlp_force(None, A, A, 8, 0, A, 8, 0, A, A, None) == INV
    assert b"null shape" in L.pdeinv_last_error()
    assert force((0, 8, 20, 40)) == INV and force((4, 8, 20, 0)) == INV
    for shape in ((4, 8, 32, 40), (9, 8, 20, 40), (4, 9, 20, 40)):
        assert force(shape) == UNS
        assert b"dim <= 8, width <= 20, 1 <= n_layers <= 8" in L.pdeinv_last_error()
    assert force(n=-1) == INV and force(m=0) == INV and b"m < 1" in L.pdeinv_last_error()
    assert force(ldx=3) == INV and force(ldr=3) == INV
    assert force(n=0, params=None, x=None, r=None, f=None, ws=None) == OK
    for k in ("params", "x", "r", "f"):
        assert force(**{k: None}) == INV and b"null" in L.pdeinv_last_error(), k
        assert force(**{k: ctypes.c_void_p(258)}) == INV and b"aligned" in L.pdeinv_last_error(), k
    assert force(ws=None) == INV and force(ws=ctypes.c_void_p(384)) == INV and b"256-byte" in L.pdeinv_last_error()

    s = native.MlpShape(4, 8, 20, 40)
    assert L.pdeinv_mf_mlp_prepare(ctypes.byref(s), None, A, None) == INV
    assert L.pdeinv_mf_mlp_prepare(ctypes.byref(s), A, None, None) == INV
    assert L.pdeinv_mf_mlp_prepare(ctypes.byref(native.MlpShape(4, 8, 32, 40)), A, A, None) == UNS

    def step(shape=(4, 8, 20, 40), s=0, m=8, ldr=0, z=A, zo=A, ref=A, ws=A, tau=None, **kw):
        d = native.SdeDesc()
        d.n_particles, d.dim, d.n_steps, d.dt, d.gamma, d.noise_scale = 16, shape[0], 10, 0.02, 0.5, 1.41
        d.potential.kind = native.POT_MEANFIELD_MLP
        for k, v in kw.items():
            if k == "kind":
                d.potential.kind = v
            else:
                setattr(d, k, v)
        sh = native.MlpShape(*shape)
        return L.pdeinv_mf_mlp_step(ctypes.byref(d), ctypes.byref(sh), s, z, zo, tau, ref, m, ldr, ws, None)

    assert L.pdeinv_mf_mlp_step(None, ctypes.byref(s), 0, A, A, None, A, 8, 0, A, None) == INV
    for kind in (native.POT_QUADRATIC, native.POT_MEANFIELD_QUADRATIC, native.POT_MLP):
        assert step(kind=kind) == INV and b"PDEINV_POT_MEANFIELD_MLP" in L.pdeinv_last_error()
    assert step((4, 8, 21, 40)) == UNS and step((9, 8, 20, 40)) == UNS
    assert step(dim=3) == INV and b"disagree" in L.pdeinv_last_error()
    assert step(s=-1) == INV and step(s=11) == INV and step(m=0) == INV and step(ldr=3) == INV
    assert step(n_steps=0) == INV and step(dt=float("nan")) == INV and step(ld_z0=5) == INV
    assert step(d_shift_u=A) == INV and b"shift_u" in L.pdeinv_last_error()
    assert step(z=None) == INV and step(zo=None) == INV and step(ref=None) == INV
    assert step(ref=ctypes.c_void_p(258)) == INV and step(tau=ctypes.c_void_p(258)) == INV
    assert step(ws=None) == INV and step(ws=ctypes.c_void_p(384)) == INV
    assert step(n_particles=0, z=None, zo=None, ws=None) == OK
    # the other simulator entry points do not know the new kind
    d = native.SdeDesc()
    d.n_particles, d.dim, d.n_steps, d.dt, d.gamma, d.noise_scale = 16, 4, 10, 0.02, 0.5, 1.41
    d.potential.kind = native.POT_MEANFIELD_MLP
    assert L.pdeinv_sde_simulate(ctypes.byref(d), A, None, None, A, None, None, None) == UNS
    assert b"unknown potential kind" in L.pdeinv_last_error()


def _potential(shape=(3, 3, 13, 7)):
    from core.model import V_hypothesis
    from core.potential import MeanFieldMLPPotential
    d, L, W, O = shape
    params, _ = R.make_net(*shape)
    model = V_hypothesis(1, [W] * L, out_features=O)
    flat = torch.as_tensor(R.flat32(params))
    tree = model.unflat(flat, d)
    return MeanFieldMLPPotential(model, tree), model, tree, flat


def test_potential_object_and_resolve():
    from core.potential import MeanFieldMLPPotential, QuadraticPotential, resolve
    from utils import native
    pot, model, tree, flat = _potential()
    nd = pot.native_desc()
    assert nd["kind"] == native.POT_MEANFIELD_MLP and nd["dims"] == [3, 13, 13, 13, 7] and pot.dim == 3
    assert torch.equal(nd["params"], flat)
    assert resolve(pot) is pot and resolve(pot.gradient) is pot
    tree["params"]["layers_0"]["bias"].add_(1.0)  # the tree is read live
    assert torch.equal(pot.native_desc()["params"], model.flat(tree))
    with pytest.raises(ValueError):
        MeanFieldMLPPotential(QuadraticPotential(A=np.eye(2)), tree)


def test_driver_value_errors():
    """Raised before any device work: the learned interaction has no fused exchange and no stamp sums."""
    from core.potential import MeanFieldQuadraticPotential
    from example_problems.kinetic_mckean_vlasov_example_quadratic import KineticMcKeanVlasov
    from utils import prng
    from utils.mean_field import simulate_mean_field
    pot, *_ = _potential()
    z0, key = torch.zeros((8, 6)), prng.PRNGKey(1)
    with pytest.raises(ValueError, match="fused"):
        simulate_mean_field(z0, 5, 0.02, key, pot, 0.5, exchange="fused")
    with pytest.raises(ValueError, match="exchange"):
        simulate_mean_field(z0, 5, 0.02, key, pot, 0.5, exchange="other")
    with pytest.raises(ValueError, match="kmv_coef"):
        simulate_mean_field(z0, 5, 0.02, key, pot, 0.5, kmv_coef=torch.zeros((5, 29)))
    with pytest.raises(ValueError, match="n_global"):
        simulate_mean_field(z0, 5, 0.02, key, MeanFieldQuadraticPotential(np.eye(3)), 0.5, n_global=8)
    pi = KineticMcKeanVlasov.__new__(KineticMcKeanVlasov)  # the checks come before any sampler / device state
    with pytest.raises(ValueError, match="stamp_sums"):
        pi.simulate_interacting(prng.PRNGKey(2), 8, stamp_sums=True, interaction=pot)
    with pytest.raises(TypeError):
        pi.simulate_interacting(prng.PRNGKey(2), 8, interaction=MeanFieldQuadraticPotential(np.eye(3)))


def test_helpers_agree_with_the_pair_tensor_restatement():
    """force64 over a time stamp's particles is gbar of oracle.numpy_ref.kmv_mlp_pairwise_loss: its |gbar|^2 term
    and its ground-truth error against tilde_F (x_i - xbar) are the oracle's `nabla` and `loss ground truth`."""
    shape = (3, 3, 13, 7)
    d = shape[0]
    params, rng = R.make_net(*shape)
    n, nt = 9, 2
    # positions on a 2^-10 grid: the fp32 pair differences of the helper are then exact, as the oracle's fp64 ones
    x = (np.round(R.positions(rng, n * nt, d) * 1024) / 1024).astype(np.float32).reshape(n, nt, d)
    v = R.velocities(rng, n * nt, d).reshape(n, nt, d)
    F = nr.problem_constants(d)
    cfg = {"tilde_F": F, "gamma_friction": 0.5}
    _, loss_gt, terms = nr.kmv_mlp_pairwise_loss(params, x, v, np.array([0.3, 0.9]), cfg, weights=np.zeros((n, nt)))
    Fs = np.stack([M.force64(params, x[:, t], x[:, t])[0] for t in range(nt)], 1)  # [n, nt, d]
    x64 = x.astype(np.float64)
    Ft = (x64 - x64.mean(0, keepdims=True)) @ F.T
    assert np.isclose(np.mean(np.sum(Fs ** 2, -1)), terms["nabla"], rtol=1e-12)
    assert np.isclose(np.mean(np.sum((Ft - Fs) ** 2, -1)), loss_gt, rtol=1e-9)
    # the fp32 restatement of the pairs sits at fp32 rounding of the gradient's scale
    g64, g32 = M.pair_grads(params, x[:, 0], x[:, 0])
    y = M.pair_diffs(x[:, 0], x[:, 0]).reshape(-1, d)
    assert np.array_equal(g64.reshape(-1, d), R.value_grad64(params, y)[1])
    assert np.array_equal(g32.reshape(-1, d), R.value_grad32(params, y)[1])
    for s in R.TILE_SHAPES:  # grad64 is value_grad64's gradient, bit for bit
        p_s, rng_s = R.make_net(*s)
        xs = R.positions(rng_s, 300, s[0])
        assert np.array_equal(M.grad64(p_s, xs), R.value_grad64(p_s, xs)[1]), s
    assert 0 < np.max(np.abs(g32 - g64)) < 5e-6 * np.max(np.abs(g64))


def test_teacher_forced_helper_reproduces_a_scan():
    """Chained over the updates, teacher_forced_update's fp64 states are an fp64 scan whose drift is the mean-field
    force; its yardstick is positive and small against the state."""
    shape = (2, 8, 20, 40)
    d = shape[0]
    params, rng = R.make_net(*shape)
    N, n, dt, gamma = 12, 3, 0.02, 0.5
    z = np.concatenate([R.positions(rng, N, d), R.velocities(rng, N, d)], 1)
    xi = rng.standard_normal((n + 1, N, d)).astype(np.float32)
    h = M.step_sizes(np.float32(0.013), n, dt)
    assert h.dtype == np.float32 and np.isclose(h.sum(), n * dt, rtol=1e-6) and len(h) == n + 1
    z64, bound = M.teacher_forced_update(params, z, z[:, :d], h[0], gamma, xi[0])
    F64, _ = M.force64(params, z[:, :d], z[:, :d])
    p = z[:, d:].astype(np.float64)
    hh = np.float64(h[0])
    p_new = p - hh * F64 + np.sqrt(hh) * nr.SQRT2 * xi[0] - gamma * p * hh
    assert np.allclose(z64[:, d:], p_new, rtol=0, atol=1e-14)
    assert np.allclose(z64[:, :d], z[:, :d] + hh * p_new, rtol=0, atol=1e-14)
    assert 0 < bound < 1e-5

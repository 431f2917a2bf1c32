"""GPU-less checks of the learned-potential entry points (pdeinv_mlp_potential, pdeinv_sde_simulate_mlp): argument
validation before the HIP runtime is touched, the path / envelope tables, and the Python surface that needs no
device (MLPPotential.native_desc, resolve)."""
import ctypes

import numpy as np
import torch

import mlp_sim_ref as R


def _lib():
    from utils import native
    return native, native.lib()


def test_fp32_restatement_close_to_fp64():
    """The fp32 copy of the forward / reverse chain is the chain of oracle.numpy_ref.mlp_forward_terms."""
    for shape in R.TILE_SHAPES:
        params, rng = R.make_net(*shape)
        x = R.positions(rng, 64, shape[0])
        V64, g64 = R.value_grad64(params, x)
        V32, g32 = R.value_grad32(params, x)
        assert 10 <= np.abs(R.value_grad64(params, R.positions(rng, 1000, shape[0]))[1]).max() <= 110
        assert R.row_err(g32, g64) < 5e-6 and R.row_err(V32, V64) < 5e-6


def test_simulate_mlp_argument_validation_without_gpu():
    native, L = _lib()
    INV, UNS = native.PDEINV_ERR_INVALID, native.PDEINV_ERR_UNSUPPORTED

    def sim(shape=(4, 8, 20, 40), null_shape=False, **kw):
        d = native.SdeDesc()
        d.n_particles, d.dim, d.n_steps, d.dt, d.gamma, d.noise_scale = 16, shape[0], 10, 0.02, 0.5, 1.41
        d.potential.kind = native.POT_MLP
        for k, v in kw.items():
            if k == "kind":
                d.potential.kind = v
            else:
                setattr(d, k, v)
        s = native.MlpShape(*shape)
        return L.pdeinv_sde_simulate_mlp(ctypes.byref(d), None if null_shape else ctypes.byref(s), None, None, None,
                                         None, None, None, None)

    s = native.MlpShape(4, 8, 20, 40)
    assert L.pdeinv_sde_simulate_mlp(None, ctypes.byref(s), None, None, None, None, None, None, None) == INV
    assert b"null descriptor" in L.pdeinv_last_error()
    assert sim(null_shape=True) == INV and b"null shape" in L.pdeinv_last_error()
    for kind in (native.POT_QUADRATIC, native.POT_GMM, native.POT_NONE):
        assert sim(kind=kind) == INV and b"PDEINV_POT_MLP" in L.pdeinv_last_error()
    assert sim((0, 8, 20, 40)) == INV and sim((4, 0, 20, 40)) == INV
    assert sim((4, 8, 0, 40)) == INV and sim((4, 8, 20, 0)) == INV
    assert sim((4, 8, 21, 40)) == UNS and b"width <= 20" in L.pdeinv_last_error()
    assert sim((4, 9, 20, 40)) == UNS and sim((9, 8, 20, 40)) == UNS
    assert sim(dim=3) == INV and b"disagree" in L.pdeinv_last_error()
    assert sim(n_steps=0) == INV and sim(dt=float("nan")) == INV and sim(ld_z0=5) == INV
    # a well-formed call reaches the pointer checks (still before any HIP call)
    assert sim() == INV and b"null" in L.pdeinv_last_error()
    assert sim(n_particles=0) == native.PDEINV_OK


def test_mlp_potential_argument_validation_without_gpu():
    native, L = _lib()
    INV, UNS = native.PDEINV_ERR_INVALID, native.PDEINV_ERR_UNSUPPORTED

    def pot(shape, n=8, ld=0):
        s = native.MlpShape(*shape)
        return L.pdeinv_mlp_potential(ctypes.byref(s), None, None, n, ld, ctypes.c_void_p(256), ctypes.c_void_p(256),
                                      None, None)

    assert L.pdeinv_mlp_potential(None, None, None, 8, 0, None, None, None, None) == INV
    assert b"null shape" in L.pdeinv_last_error()
    assert pot((0, 8, 20, 40)) == INV and pot((4, 0, 20, 40)) == INV
    assert pot((4, 2, 2048, 40)) == UNS and pot((17, 2, 20, 40)) == UNS
    assert pot((4, 8, 20, 40), ld=3) == INV and b"ld < dim" in L.pdeinv_last_error()
    assert pot((4, 2, 64, 40), ld=3) == INV
    assert pot((4, 8, 20, 40), n=-1) == INV
    assert pot((4, 8, 20, 40)) == INV and b"null" in L.pdeinv_last_error()  # params / x
    assert pot((4, 8, 20, 40), n=0) == native.PDEINV_OK


def test_path_and_envelope_tables():
    native, L = _lib()
    path = lambda *s: L.pdeinv_mlp_potential_path(ctypes.byref(native.MlpShape(*s)))  # noqa: E731
    sup = lambda *s: L.pdeinv_sde_simulate_mlp_supported(ctypes.byref(native.MlpShape(*s)))  # noqa: E731
    for s in R.TILE_SHAPES + [(8, 8, 20, 1), (1, 1, 1, 1), (8, 8, 20, 4096)]:
        assert path(*s) == 2 and sup(*s) == 1, s
    for s in [(4, 2, 32, 40), (4, 2, 64, 40), (4, 8, 21, 40), (4, 9, 20, 40), (9, 8, 20, 40), (16, 16, 1024, 40)]:
        assert path(*s) == 1 and sup(*s) == 0, s
    for s in [(4, 2, 2048, 40), (17, 2, 20, 40), (4, 17, 32, 40), (0, 2, 20, 40), (4, 0, 20, 40), (4, 2, 20, 0)]:
        assert path(*s) == 0 and sup(*s) == 0, s
    assert L.pdeinv_mlp_potential_path(None) == 0 and L.pdeinv_sde_simulate_mlp_supported(None) == 0
    assert native.mlp_potential_path([4] + [20] * 8 + [40]) == 2 and native.POT_MLP == 4
    d = native.SdeDesc()
    ok, bad = native.MlpShape(4, 8, 20, 40), native.MlpShape(4, 8, 32, 40)
    assert L.pdeinv_sde_simulate_mlp_workspace_bytes(ctypes.byref(d), ctypes.byref(ok)) > 0
    assert L.pdeinv_sde_simulate_mlp_workspace_bytes(ctypes.byref(d), ctypes.byref(bad)) == 0
    assert L.pdeinv_mlp_potential_workspace_bytes(ctypes.byref(ok), 1000) > 0
    assert L.pdeinv_mlp_potential_workspace_bytes(ctypes.byref(bad), 1000) > 0
    assert L.pdeinv_mlp_potential_workspace_bytes(ctypes.byref(native.MlpShape(4, 2, 2048, 40)), 1000) == 0


def test_mlp_potential_object_and_resolve():
    from core.model import V_hypothesis
    from core.potential import MLPPotential, QuadraticPotential, resolve
    from utils import native
    d, L, W, O = 3, 3, 13, 7
    params, _ = R.make_net(d, L, W, O)
    model = V_hypothesis(1, [W] * L, out_features=O)
    flat = torch.as_tensor(R.flat32(params))
    tree = model.unflat(flat, d)
    pot = MLPPotential(model, tree)
    nd = pot.native_desc()
    assert nd["kind"] == native.POT_MLP == 4 and nd["dims"] == [d] + [W] * L + [O]
    assert torch.equal(nd["params"], flat) and pot.dim == d
    assert resolve(pot) is pot and resolve(pot.gradient) is pot
    tree["params"]["layers_0"]["bias"].add_(1.0)  # the tree is read live
    assert torch.equal(pot.native_desc()["params"], model.flat(tree))
    try:
        MLPPotential(QuadraticPotential(A=np.eye(2)), tree)
    except ValueError:
        pass
    else:
        raise AssertionError("MLPPotential accepted a non-MLP model")

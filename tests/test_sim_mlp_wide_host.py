"""GPU-less checks of the wide learned-potential entry points (pdeinv_mlp_potential_wide,
pdeinv_sde_simulate_mlp_wide): argument validation before the HIP runtime is touched, the envelope table, the
workspace sizes and the ABI version."""
import ctypes

import mlp_sim_ref as R

SHAPES = [(4, 2, 32, 40), (3, 2, 21, 7), (1, 2, 48, 3), (5, 1, 100, 40), (2, 2, 128, 40), (4, 3, 64, 40),
          (8, 2, 256, 40), (4, 8, 64, 40)]
OUTSIDE = [(4, 8, 20, 40), (9, 2, 32, 40), (4, 3, 256, 40), (4, 2, 257, 40), (4, 2, 32, 65)]


def _lib():
    from utils import native
    return native, native.lib()


def test_simulate_mlp_wide_argument_validation_without_gpu():
    native, L = _lib()
    INV, UNS = native.PDEINV_ERR_INVALID, native.PDEINV_ERR_UNSUPPORTED

    def sim(shape=(4, 2, 32, 40), null_shape=False, **kw):
        d = native.SdeDesc()
        d.n_particles, d.dim, d.n_steps, d.dt, d.gamma, d.noise_scale = 16, shape[0], 10, 0.02, 0.5, 1.41
        d.potential.kind = native.POT_MLP
        for k, v in kw.items():
            if k == "kind":
                d.potential.kind = v
            else:
                setattr(d, k, v)
        s = native.MlpShape(*shape)
        return L.pdeinv_sde_simulate_mlp_wide(ctypes.byref(d), None if null_shape else ctypes.byref(s), None, None,
                                              None, None, None, None, None)

    s = native.MlpShape(4, 2, 32, 40)
    assert L.pdeinv_sde_simulate_mlp_wide(None, ctypes.byref(s), None, None, None, None, None, None, None) == INV
    assert b"null descriptor" in L.pdeinv_last_error()
    assert sim(null_shape=True) == INV and b"null shape" in L.pdeinv_last_error()
    for kind in (native.POT_QUADRATIC, native.POT_GMM, native.POT_NONE):
        assert sim(kind=kind) == INV and b"PDEINV_POT_MLP" in L.pdeinv_last_error()
    assert sim((0, 2, 32, 40)) == INV and sim((4, 0, 32, 40)) == INV
    assert sim((4, 2, 0, 40)) == INV and sim((4, 2, 32, 0)) == INV
    for shape in OUTSIDE:
        assert sim(shape) == UNS, shape
        msg = L.pdeinv_last_error()
        assert b"dim <= 8" in msg and b"21 <= width <= 256" in msg and b"<= 512" in msg, msg
        assert b"out_features <= 64" in msg and b"narrow" in msg, msg
    assert sim(dim=3) == INV and b"disagree" in L.pdeinv_last_error()
    assert sim(n_steps=0) == INV and sim(dt=float("nan")) == INV and sim(ld_z0=5) == INV
    # a well-formed call reaches the pointer checks (still before any HIP call)
    for shape in SHAPES:
        assert sim(shape) == INV and b"null" in L.pdeinv_last_error(), shape
    assert sim(n_particles=0) == native.PDEINV_OK


def test_mlp_potential_wide_argument_validation_without_gpu():
    native, L = _lib()
    INV, UNS = native.PDEINV_ERR_INVALID, native.PDEINV_ERR_UNSUPPORTED

    def pot(shape, n=8, ld=0):
        s = native.MlpShape(*shape)
        return L.pdeinv_mlp_potential_wide(ctypes.byref(s), None, None, n, ld, ctypes.c_void_p(256),
                                           ctypes.c_void_p(256), None, None)

    assert L.pdeinv_mlp_potential_wide(None, None, None, 8, 0, None, None, None, None) == INV
    assert b"null shape" in L.pdeinv_last_error()
    assert pot((0, 2, 32, 40)) == INV and pot((4, 0, 32, 40)) == INV
    for shape in OUTSIDE:
        assert pot(shape) == UNS and b"21 <= width <= 256" in L.pdeinv_last_error(), shape
    assert pot((4, 2, 32, 40), ld=3) == INV and b"ld < dim" in L.pdeinv_last_error()
    assert pot((4, 2, 32, 40), n=-1) == INV
    assert pot((4, 2, 32, 40)) == INV and b"null" in L.pdeinv_last_error()  # params / x
    assert pot((4, 2, 32, 40), n=0) == native.PDEINV_OK


def test_wide_envelope_table_and_workspaces():
    native, L = _lib()
    sup = lambda *s: L.pdeinv_sde_simulate_mlp_wide_supported(ctypes.byref(native.MlpShape(*s)))  # noqa: E731
    d = native.SdeDesc()
    inside = SHAPES + [(4, 2, 64, 40), (8, 4, 128, 64), (8, 8, 21, 1), (1, 1, 256, 64), (4, 6, 80, 40),
                       (4, 2, 255, 40)]
    for s in inside:
        sh = native.MlpShape(*s)
        assert sup(*s) == 1 and native.sde_simulate_mlp_wide_supported(R.dims_of(*s)), s
        assert L.pdeinv_sde_simulate_mlp_wide_workspace_bytes(ctypes.byref(d), ctypes.byref(sh)) > 0, s
        assert L.pdeinv_mlp_potential_wide_workspace_bytes(ctypes.byref(sh), 1000) > 0, s
    outside = OUTSIDE + [(4, 9, 64, 40), (4, 5, 128, 40), (4, 7, 80, 40), (0, 2, 32, 40), (4, 0, 32, 40),
                         (4, 2, 32, 0), (4, 2, 1024, 40)] + R.TILE_SHAPES
    for s in outside:
        sh = native.MlpShape(*s)
        assert sup(*s) == 0, s
        assert L.pdeinv_sde_simulate_mlp_wide_workspace_bytes(ctypes.byref(d), ctypes.byref(sh)) == 0, s
        assert L.pdeinv_mlp_potential_wide_workspace_bytes(ctypes.byref(sh), 1000) == 0, s
    assert L.pdeinv_sde_simulate_mlp_wide_supported(None) == 0
    ok = native.MlpShape(4, 2, 32, 40)
    assert L.pdeinv_sde_simulate_mlp_wide_workspace_bytes(None, ctypes.byref(ok)) == 0
    assert L.pdeinv_mlp_potential_wide_workspace_bytes(ctypes.byref(ok), -1) == 0
    # the narrow entry and the path table do not move
    assert L.pdeinv_sde_simulate_mlp_supported(ctypes.byref(ok)) == 0
    assert L.pdeinv_mlp_potential_path(ctypes.byref(ok)) == 1
    assert not native.sde_simulate_mlp_supported(R.dims_of(4, 2, 32, 40))
    assert native.sde_simulate_mlp_supported(R.dims_of(4, 8, 20, 40))
    assert L.pdeinv_abi_version() == 10  # the new entry points are additive

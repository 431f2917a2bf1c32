"""CPU checks of tests/flow_map_ref.py (the restatement the GPU tests of pdeinv_realnvp_map compare with) and of the
host side of the two entry points that needs no GPU: symbols, the path table, the argument checks."""
import ctypes
import os
import re

import numpy as np
import pytest

import flow_map_ref as fmr
from oracle import numpy_ref as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"pdeinv_realnvp_map", "pdeinv_realnvp_map_path"}
OK, INVALID, UNSUPPORTED = 0, -1, -2
AUTO, GENERAL, MATRIX = 0, 1, 2


@pytest.mark.parametrize("case", fmr.CASES, ids=fmr.case_id)
def test_restatement_vs_numpy_ref(case):
    """fp64: y and ldj equal nr.realnvp_apply in both directions (1e-12 of scale), logp of the likelihood direction
    equals nr.realnvp_logdensity, the generative logp is log p0(x0) - ldj; the round trip closes in fp64; the
    float32 run stays float32 and within 1e-4 of scale."""
    c = fmr.case_inputs(*case)
    flat, t, kw = c["flat"], c["t"].astype(np.float64), c["kw"]
    flow_kw = {k: v for k, v in kw.items() if k not in ("base_mean", "base_cov")}
    for reverse, x in ((True, c["z"][:, :case[0]].astype(np.float64)), (False, c["x0"].astype(np.float64))):
        y, ldj, logp = fmr.flow_map(flat, t, x, reverse, **kw)
        y_ref, ldj_ref = nr.realnvp_apply(flat, t, x, reverse=reverse, **flow_kw)
        assert np.abs(y - y_ref).max() <= 1e-12 * (1 + np.abs(y_ref).max())
        assert np.abs(ldj - ldj_ref).max() <= 1e-12 * (1 + np.abs(ldj_ref).max())
        if reverse:
            lp_ref = nr.realnvp_logdensity(flat, t, x, **kw)
        else:
            off = x - c["mean"]
            lp_ref = -0.5 * (np.log(np.linalg.det(c["cov"] * 2 * np.pi))
                             + np.einsum("ni,ij,nj->n", off, np.linalg.inv(c["cov"]), off)) - ldj_ref
        assert np.abs(logp - lp_ref).max() <= 1e-12 * (1 + np.abs(lp_ref).max())
        lo = fmr.flow_map(flat, t, x, reverse, dtype=np.float32, **kw)
        for a, b in zip(lo, (y, ldj, logp)):
            assert a.dtype == np.float32
            assert np.abs(a - b).max() <= 1e-4 * (1 + np.abs(b).max())
        if not reverse:   # x0 -> y -> x0, and the density of y is the likelihood direction's
            back, ldj_b, logp_b = fmr.flow_map(flat, t, y, True, **kw)
            assert np.abs(back - x).max() <= 1e-11 * (1 + np.abs(x).max())
            assert np.abs(ldj + ldj_b).max() <= 1e-11 * (1 + np.abs(ldj).max())
            assert np.abs(logp - logp_b).max() <= 1e-10 * (1 + np.abs(logp).max())


def test_header_binding_and_library_have_the_entry_points():
    from utils import native
    txt = open(os.path.join(ROOT, "include", "pdeinv.h")).read()
    declared = set(re.findall(r"^(?:int|int64_t|size_t|const char\*)\s+(pdeinv_\w+)\(", txt, flags=re.M))
    assert NEW_SYMBOLS <= declared and NEW_SYMBOLS <= set(native.EXPORTED_SYMBOLS)
    assert native.ABI_VERSION == 10
    lib = native.lib()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s)
    assert lib.pdeinv_abi_version() == 10
    for f in ("realnvp_map", "realnvp_map_path"):
        assert callable(getattr(native, f))


def nvp_desc(native, dim=2, E=10, act="celu", couple=2, ignore_time=False, soft_init=1.0):
    masks = nr.nvp_masks(dim, couple, "loop")
    acts = dict(native.ACTIVATIONS)
    acts.setdefault(act, 0)
    m = np.ascontiguousarray(masks, dtype=np.float32)
    mu, ic = np.zeros(dim, np.float32), np.ascontiguousarray(np.eye(dim), dtype=np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    desc = native.RealNvpDesc(dim, m.shape[0], E, int(ignore_time), soft_init, acts[act], p(m), p(mu), p(ic), 0.0)
    return desc, (m, mu, ic)


def _err(native):
    return native.lib().pdeinv_last_error().decode()


def test_map_path_table():
    from utils import native
    path = native.lib().pdeinv_realnvp_map_path
    for act in ("celu", "elu"):
        d, _k = nvp_desc(native, act=act)
        assert path(ctypes.byref(d), GENERAL) == 0
        assert path(ctypes.byref(d), MATRIX) == 1
        assert path(ctypes.byref(d), AUTO) in (0, 1)
        assert native.realnvp_map_path(d, "general") == "general" and native.realnvp_map_path(d, "matrix") == "matrix"
    d, _k = nvp_desc(native, act="tanh")
    assert path(ctypes.byref(d), MATRIX) == UNSUPPORTED and "realnvp_map_path" in _err(native)
    assert path(ctypes.byref(d), GENERAL) == 0 and path(ctypes.byref(d), AUTO) == 0
    with pytest.raises(NotImplementedError):
        native.realnvp_map_path(d, "matrix")
    d, _k = nvp_desc(native, dim=9)
    for impl in (AUTO, GENERAL, MATRIX):
        assert path(ctypes.byref(d), impl) == UNSUPPORTED
    d, _k = nvp_desc(native, E=2)
    assert path(ctypes.byref(d), AUTO) == UNSUPPORTED
    d, _k = nvp_desc(native)
    assert path(ctypes.byref(d), 7) == INVALID and "realnvp_map_path" in _err(native)
    assert path(ctypes.byref(d), -1) == INVALID
    assert path(None, AUTO) == INVALID
    with pytest.raises(ValueError):
        native.realnvp_map_path(d, "fast")


def test_map_argument_checks_need_no_gpu():
    """Every INVALID / UNSUPPORTED case of pdeinv_realnvp_map with null device pointers (nothing is launched: the
    checks run before any device call); n == 0 is a no-op; the messages name the entry point."""
    from utils import native
    fn = native.lib().pdeinv_realnvp_map
    d, _k = nvp_desc(native)

    def call(desc=d, t_stride=1, n=5, ld=2, reverse=1, impl=AUTO, y=None, ld_y=0, ldj=None, logp=None, params=None,
             t=None, x=None):
        return fn(ctypes.byref(desc) if desc is not None else None, params, t, t_stride, x, n, ld, reverse, impl, y,
                  ld_y, ldj, logp, None)

    assert call(n=0) == OK
    assert call(n=0, reverse=0, impl=MATRIX) == OK
    bad = [dict(reverse=2), dict(reverse=-1), dict(impl=7), dict(impl=-1), dict(ld=1), dict(ld_y=1), dict(t_stride=-1),
           dict(n=-1), dict(desc=None), dict(y=ctypes.c_void_p(0x1002)), dict(ldj=ctypes.c_void_p(0x1001)),
           dict(logp=ctypes.c_void_p(0x1003)), dict(x=ctypes.c_void_p(0x1002)), dict(t=ctypes.c_void_p(0x1001)),
           dict(params=ctypes.c_void_p(0x1002)),
           dict(),                                   # no output requested
           dict(y=ctypes.c_void_p(0x1000))]          # null inputs
    for kw in bad:
        assert call(**kw) == INVALID, kw
        assert "realnvp_map" in _err(native), kw
    # the size and alignment checks come before the n == 0 return
    assert call(n=0, ld=1) == INVALID and call(n=0, reverse=3) == INVALID
    assert call(n=0, y=ctypes.c_void_p(0x1002)) == INVALID
    dt, _kt = nvp_desc(native, act="tanh")
    assert call(desc=dt, impl=MATRIX) == UNSUPPORTED and "realnvp_map" in _err(native)
    assert call(desc=dt, impl=MATRIX, n=0) == UNSUPPORTED
    assert call(desc=dt, impl=GENERAL, n=0) == OK
    for kw in (dict(dim=9), dict(E=2), dict(E=18), dict(act="prelu?")):
        dd, _kk = nvp_desc(native, **kw) if "act" not in kw else nvp_desc(native)
        if "act" in kw:
            dd.activation = 99
        assert call(desc=dd, n=0) == UNSUPPORTED, kw
    # the descriptor's checks come first: a bad descriptor with a bad impl reports the descriptor
    d9, _k9 = nvp_desc(native, dim=9)
    assert call(desc=d9, impl=7) == UNSUPPORTED

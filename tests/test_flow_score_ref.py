"""CPU checks of tests/flow_score_ref.py (the restatement the GPU tests of pdeinv_realnvp_score compare with): against
torch autograd and finite differences, that the yardstick built on it convicts wrong rules and acquits a second
float32 evaluation; and of the host side that needs no GPU: symbols, the path table, the argument checks, the
closed-form X-marginal."""
import ctypes
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

import flow_map_ref as fmr
import flow_score_ref as fsr
from test_flow_map_ref import AUTO, GENERAL, INVALID, MATRIX, OK, UNSUPPORTED, _err, nvp_desc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"pdeinv_realnvp_score", "pdeinv_realnvp_score_path", "pdeinv_realnvp_score_workspace_bytes"}


def rel(got, ref):
    """The project's error measure: max|got - ref| / (1 + max|ref|)"""
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / (1 + np.abs(ref).max()))


@functools.lru_cache(maxsize=None)
def solved(case):
    """A case's inputs, its fp64 score / logp / margin and the float32 restatement's errors (kept inputs)."""
    c = fmr.case_inputs(*case)
    x = c["z"][:, :case[0]].astype(np.float64)
    t = c["t"].astype(np.float64)
    s64, lp64, margin = fsr.score(c["flat"], t, x, **c["kw"])
    s32, lp32, _ = fsr.score(c["flat"], t, x, dtype=np.float32, **c["kw"])
    return dict(c=c, x=x, t=t, score=s64, logp=lp64, margin=margin, s32=s32, lp32=lp32, err32=rel(s32, s64),
                err32_logp=rel(lp32, lp64))


def _torch_logp(flat, t, x, *, dim, masks, base_mean, base_cov, E, ignore_time, soft_init, act):
    """Torch fp64 restatement of flow_map_ref.flow_map(..., reverse=True)[2], differentiable in x."""
    from oracle import numpy_ref as nr
    T = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))
    c_gelu = math.sqrt(2 / math.pi)
    g = {"celu": lambda z: torch.where(z > 0, z, torch.expm1(torch.clamp(z, max=0.0))),
         "elu": lambda z: torch.where(z > 0, z, torch.expm1(torch.clamp(z, max=0.0))),
         "relu": lambda z: torch.clamp(z, min=0.0),
         "tanh": torch.tanh,
         "silu": lambda z: z * torch.sigmoid(z),
         "softplus": lambda z: torch.logaddexp(z, torch.zeros_like(z)),
         "gelu": lambda z: 0.5 * z * (1 + torch.tanh(c_gelu * (z + 0.044715 * z ** 3)))}[act]
    masks = np.asarray(masks, dtype=np.float64)
    temb, layers = nr.nvp_unflat(flat, dim, masks.shape[0], E, ignore_time)

    def mlp(net, h):
        for k, (W, b) in enumerate(net):
            h = h @ T(W) + T(b)
            if k < 3:
                h = g(h)
        return h

    xs, t = x, T(t)
    if ignore_time:
        tc = torch.zeros((xs.shape[0], 0), dtype=torch.float64)
    elif E > 0:
        half = E // 2
        w = T(np.exp(np.arange(half) * -(np.log(10000) / (half - 1))))
        e = t[:, None] * w
        se = torch.cat([torch.sin(e), torch.cos(e)], -1)
        (W1, b1), (W2, b2) = temb
        tc = g(se @ T(W1) + T(b1)) @ T(W2) + T(b2)
    else:
        tc = t[:, None]
    ldj = torch.zeros(xs.shape[0], dtype=torch.float64)
    for l in range(masks.shape[0] - 1, -1, -1):
        m = T(masks[l])
        sf, snet, tnet = layers[l]
        xt = torch.cat([xs * m, tc], -1)
        s, tr = mlp(snet, xt), mlp(tnet, xt)
        if not ignore_time and soft_init == 0.0:
            s, tr = t[:, None] * s, t[:, None] * tr
        f = torch.exp(T(sf))
        s = torch.tanh(s / f) * f * (1 - m)
        xs = (xs + tr * (1 - m)) * torch.exp(s)
        ldj = ldj + s.sum(-1)
    off = xs - T(base_mean)
    cov = np.asarray(base_cov, dtype=np.float64)
    quad = torch.einsum("ni,ij,nj->n", off, T(np.linalg.inv(cov)), off)
    return -0.5 * (float(np.log(np.linalg.det(cov * 2 * np.pi))) + quad) + ldj


@pytest.mark.parametrize("case", fmr.CASES, ids=fmr.case_id)
def test_restatement_vs_autograd(case):
    """fp64: logp is flow_map_ref's (1e-12 of scale) and the score is torch autograd's of a torch restatement of
    log p (1e-8 of scale), on every case; the margin is one finite non-negative number per sample."""
    r = solved(case)
    kw = r["c"]["kw"]
    lp_map = fmr.flow_map(r["c"]["flat"], r["t"], r["x"], True, **kw)[2]
    assert rel(r["logp"], lp_map) <= 1e-12
    x = torch.as_tensor(r["x"]).clone().requires_grad_(True)
    lp = _torch_logp(r["c"]["flat"], r["t"], x, **kw)
    assert rel(lp.detach().numpy(), lp_map) <= 1e-12
    (grad,) = torch.autograd.grad(lp.sum(), x)
    assert rel(r["score"], grad.numpy()) <= 1e-8
    mg = r["margin"]
    assert mg.shape == (case[6],) and (mg >= 0).all() and np.isfinite(mg).all()


@pytest.mark.parametrize("case", fmr.CASES, ids=fmr.case_id)
def test_restatement_vs_finite_differences(case):
    """fp64: the score equals central differences (h = 1e-5) of flow_map_ref's logp to 1e-6 of scale."""
    r = solved(case)
    d, h = case[0], 1e-5
    f = lambda xx: fmr.flow_map(r["c"]["flat"], r["t"], xx, True, **r["c"]["kw"])[2]
    fd = np.empty_like(r["score"])
    for k in range(d):
        e = np.zeros(d)
        e[k] = h
        fd[:, k] = (f(r["x"] + e) - f(r["x"] - e)) / (2 * h)
    assert rel(r["score"], fd) <= 1e-6


@pytest.mark.parametrize("case", fmr.CASES, ids=fmr.case_id)
def test_float32_mode(case):
    """The float32 run stays float32 in both modes and within 1e-3 of scale of the fp64 one."""
    r = solved(case)
    assert r["s32"].dtype == np.float32 and r["lp32"].dtype == np.float32
    assert r["err32"] <= 1e-3 and r["err32_logp"] <= 1e-4
    s_inv, lp_inv, _ = fsr.score(r["c"]["flat"], r["t"], r["x"], dtype=np.float32, keep_inputs=False, **r["c"]["kw"])
    assert s_inv.dtype == np.float32 and lp_inv.dtype == np.float32
    assert rel(s_inv, r["score"]) <= 1e-3
    assert np.array_equal(lp_inv, r["lp32"])
    # fp64: rebuilding the inputs by inversion is the same score
    s_inv64 = fsr.score(r["c"]["flat"], r["t"], r["x"], keep_inputs=False, **r["c"]["kw"])[0]
    assert rel(s_inv64, r["score"]) <= 1e-9


@pytest.mark.parametrize("case", fmr.CASES, ids=fmr.case_id)
def test_yardstick_convicts_wrong_rules(case):
    """bound = max(4 err32, 2e-5), the GPU tests' rule: each rule with one term left out, evaluated in fp64, lies
    outside it (the t factor: on the hard parameterisation, where there is one). At dim 1 every mask is 0: no net
    sees x, the rule reads g <- g e^s, and s^bar and tau^bar reach the score only through the m (...) term, which
    the mask removes. There only the dropped mask can show, and the three other terms must change nothing."""
    r = solved(case)
    bound = max(4 * r["err32"], 2e-5)
    hard = not case[4] and case[3] == 0.0
    for drop in fsr.DROPS:
        if drop == "hard_t" and not hard:
            continue
        wrong = fsr.score(r["c"]["flat"], r["t"], r["x"], drop=drop, **r["c"]["kw"])[0]
        if case[0] == 1 and drop != "mask":
            assert np.array_equal(wrong, r["score"]), drop
            continue
        assert rel(wrong, r["score"]) > bound, (drop, rel(wrong, r["score"]), bound)


@pytest.mark.parametrize("case", fmr.CASES, ids=fmr.case_id)
def test_yardstick_acquits_second_float32_evaluation(case):
    """The same algebra in float32 with the samples permuted and the nets' matrix products taken in the other
    association stays within 2 err32 of the fp64 score."""
    r = solved(case)
    perm = np.random.default_rng(7).permutation(case[6])
    s_b = fsr.score(r["c"]["flat"], r["t"][perm], r["x"][perm], dtype=np.float32, assoc="forward", **r["c"]["kw"])[0]
    assert s_b.dtype == np.float32
    err_b = rel(s_b, r["score"][perm])
    assert err_b <= 2 * r["err32"], (err_b, r["err32"])
    # fp64: the two associations are the same score
    s_f = fsr.score(r["c"]["flat"], r["t"], r["x"], assoc="forward", **r["c"]["kw"])[0]
    assert rel(s_f, r["score"]) <= 1e-10


def test_header_binding_and_library_have_the_entry_points():
    from utils import native
    txt = open(os.path.join(ROOT, "include", "pdeinv.h")).read()
    declared = set(re.findall(r"^(?:int|int64_t|size_t|const char\*)\s+(pdeinv_\w+)\(", txt, flags=re.M))
    assert NEW_SYMBOLS <= declared and NEW_SYMBOLS <= set(native.EXPORTED_SYMBOLS)
    assert native.ABI_VERSION == 10
    assert re.search(r"^#define PDEINV_ABI_VERSION 10\b", txt, flags=re.M)
    lib = native.lib()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s)
    assert lib.pdeinv_abi_version() == 10
    for f in ("realnvp_score", "realnvp_score_path"):
        assert callable(getattr(native, f))


def test_score_path_table():
    """pdeinv_realnvp_score_path without a GPU, the envelope table: the general path takes the whole descriptor
    envelope, the matrix-core path celu / elu flows (MATRIX on a tanh flow: NotImplementedError), AUTO names one of
    the two; a bad descriptor or impl is refused."""
    from utils import native
    path = native.lib().pdeinv_realnvp_score_path
    for act in native.ACTIVATIONS:
        for kw in (dict(), dict(dim=8, E=0), dict(dim=1, E=16, soft_init=0.0), dict(ignore_time=True)):
            d, _k = nvp_desc(native, act=act, **kw)
            assert path(ctypes.byref(d), GENERAL) == 0
            assert native.realnvp_score_path(d, "general") == "general"
            if act in ("celu", "elu"):
                assert path(ctypes.byref(d), MATRIX) == 1 and native.realnvp_score_path(d, "matrix") == "matrix"
                assert path(ctypes.byref(d), AUTO) in (0, 1)
            else:
                assert path(ctypes.byref(d), MATRIX) == UNSUPPORTED and "realnvp_score_path" in _err(native)
                assert path(ctypes.byref(d), AUTO) == 0 and native.realnvp_score_path(d) == "general"
    d, _k = nvp_desc(native, act="tanh")
    with pytest.raises(NotImplementedError):
        native.realnvp_score_path(d, "matrix")
    d, _k = nvp_desc(native, dim=9)
    for impl in (AUTO, GENERAL, MATRIX):
        assert path(ctypes.byref(d), impl) == UNSUPPORTED
    with pytest.raises(NotImplementedError):
        native.realnvp_score_path(d, "general")
    d, _k = nvp_desc(native, E=2)
    assert path(ctypes.byref(d), AUTO) == UNSUPPORTED
    d, _k = nvp_desc(native)
    d.masks = None
    assert path(ctypes.byref(d), AUTO) == INVALID
    with pytest.raises(ValueError):
        native.realnvp_score_path(d, "auto")
    d, _k = nvp_desc(native)
    assert path(ctypes.byref(d), 7) == INVALID and "realnvp_score_path" in _err(native)
    assert path(ctypes.byref(d), -1) == INVALID
    assert path(None, AUTO) == INVALID
    with pytest.raises(ValueError):
        native.realnvp_score_path(d, "fast")


def test_score_argument_checks_need_no_gpu():
    """Every INVALID / UNSUPPORTED case of pdeinv_realnvp_score with null device pointers (nothing is launched: the
    checks run before any device call); n == 0 is a no-op; the workspace size is n_layers * dim * n floats."""
    from utils import native
    lib = native.lib()
    fn, wsb = lib.pdeinv_realnvp_score, lib.pdeinv_realnvp_score_workspace_bytes
    d, _k = nvp_desc(native)   # dim 2, 4 layers

    def call(desc=d, t_stride=1, n=5, ld=2, impl=GENERAL, score=None, ld_s=0, logp=None, params=None, t=None, x=None,
             ws=None, ws_bytes=0):
        return fn(ctypes.byref(desc) if desc is not None else None, params, t, t_stride, x, n, ld, impl, score, ld_s,
                  logp, ws, ws_bytes, None)

    assert wsb(ctypes.byref(d), 5, GENERAL) == d.n_layers * 2 * 5 * 4 and wsb(ctypes.byref(d), 0, GENERAL) == 0
    assert wsb(ctypes.byref(d), 5, AUTO) in (d.n_layers * 2 * 5 * 4, d.n_layers * 64 * 4)
    assert wsb(ctypes.byref(d), 17, MATRIX) == d.n_layers * 2 * 64 * 4    # packed layout: one register, two tiles
    d8, _k8 = nvp_desc(native, dim=8)
    assert wsb(ctypes.byref(d8), 16, MATRIX) == d8.n_layers * 4 * 64 * 4  # identity layout: four registers
    dt, _kt = nvp_desc(native, act="tanh")
    assert wsb(ctypes.byref(dt), 5, MATRIX) == 0 and wsb(ctypes.byref(dt), 5, AUTO) == dt.n_layers * 2 * 5 * 4
    assert wsb(None, 5, AUTO) == 0 and wsb(ctypes.byref(d), -1, AUTO) == 0 and wsb(ctypes.byref(d), 5, 7) == 0
    assert call(n=0) == OK and call(n=0, impl=GENERAL) == OK
    p = ctypes.c_void_p
    full = dict(params=p(0x1000), t=p(0x1000), x=p(0x1000))
    bad = [dict(impl=7), dict(impl=-1), dict(ld=1), dict(ld_s=1), dict(t_stride=-1), dict(n=-1), dict(desc=None),
           dict(score=p(0x1002)), dict(logp=p(0x1003)), dict(x=p(0x1002)), dict(t=p(0x1001)), dict(params=p(0x1002)),
           dict(ws=p(0x1001)),
           dict(),                                                  # no output requested
           dict(logp=p(0x1000)),                                    # null inputs
           dict(score=p(0x1000), **full),                           # no workspace
           dict(score=p(0x1000), ws=p(0x1000), ws_bytes=d.n_layers * 2 * 5 * 4 - 1, **full)]   # one byte short
    for kw in bad:
        assert call(**kw) == INVALID, kw
        assert "realnvp_score" in _err(native), kw
    assert call(n=0, ld=1) == INVALID and call(n=0, score=p(0x1002)) == INVALID
    assert call(desc=dt, impl=MATRIX) == UNSUPPORTED and "realnvp_score" in _err(native)
    assert call(desc=dt, impl=MATRIX, n=0) == UNSUPPORTED and call(desc=dt, impl=GENERAL, n=0) == OK
    assert call(impl=MATRIX, n=0) == OK and call(impl=AUTO, n=0) == OK
    assert call(impl=MATRIX, score=p(0x1000), ws=p(0x1000), ws_bytes=d.n_layers * 64 * 4 - 1, **full) == INVALID
    d9, _k9 = nvp_desc(native, dim=9)
    assert call(desc=d9, impl=7) == UNSUPPORTED
    # the Python wrapper's own argument errors need a GPU only after them
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            native.realnvp_score(d, torch.zeros(1), torch.zeros(1), torch.zeros(1, 2))


def test_x_marginal_is_the_x_block_of_the_closed_form():
    from example_problems.kinetic_mckean_vlasov_example_quadratic import KineticMcKeanVlasov, _mean_cov_stamps
    from utils import config, prng
    for d in (2, 3):
        cfg = config.compose("config", ["pde_instance=kinetic_mckean_vlasov", f"pde_instance.domain_dim={d}"])
        pi = KineticMcKeanVlasov(cfg, prng.PRNGKey(0))
        taus = np.array([0.0, 0.3, 1.7])
        mean, cov = pi.x_marginal(taus)
        m_ref, c_ref = _mean_cov_stamps(taus, pi.initial_configuration)
        assert mean.dtype == cov.dtype == np.float64 and mean.shape == (3, d) and cov.shape == (3, d, d)
        assert np.array_equal(mean, m_ref[:, :d]) and np.array_equal(cov, c_ref[:, :d, :d])
        g = pi.distribution_initial_x
        assert np.allclose(mean[0], g.mu_host, atol=1e-13) and np.allclose(cov[0], g.cov_host, atol=1e-13)

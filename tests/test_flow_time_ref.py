"""CPU checks of tests/flow_time_ref.py (the fp64 Taylor-mode restatement the GPU tests of
pdeinv_realnvp_time_derivs compare with), and of the Python-side logic of the learned-density KMV branch
that needs no GPU."""
import os
import re

import numpy as np
import pytest
import torch

import flow_time_ref as ftr
from oracle import numpy_ref as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 4096
NEW_SYMBOLS = {"pdeinv_realnvp_time_derivs", "pdeinv_realnvp_time_derivs_sets", "pdeinv_realnvp_time_impl",
               "pdeinv_kmv_weights_from_ds_workspace_bytes", "pdeinv_kmv_weights_from_ds"}


def _setup(dim, mask_type, E, soft_init, ignore_time, n=N, seed=None):
    couple = 3 if mask_type == "random" else (2 if dim == 8 else 4)
    masks = nr.nvp_masks(dim, couple, mask_type)
    rng = np.random.default_rng(100 + dim if seed is None else seed)
    mean = rng.standard_normal(dim) * 0.3
    Lc = rng.standard_normal((dim, dim)) * 0.3
    cov = Lc @ Lc.T + np.eye(dim)
    flat = nr.nvp_init(dim, masks.shape[0], E, ignore_time, seed=dim + 1, scale=1.3, perturb=True)
    x = rng.standard_normal((n, dim)) * 1.5
    t = rng.uniform(0.05, 2.0, n)
    kw = dict(dim=dim, masks=masks, base_mean=mean, base_cov=cov, E=E, ignore_time=ignore_time, soft_init=soft_init)
    return flat, t, x, kw


CASES = [(2, "loop", 10, 1.0, False), (3, "random", 0, 0.0, False), (5, "random", 6, 0.0, False),
         (1, "loop", 4, 0.0, False), (4, "loop", 16, 1.0, False)]
ACTS = ["celu", "relu", "tanh", "elu", "silu", "softplus", "gelu"]
SMOOTH = ("tanh", "softplus", "silu", "gelu")


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("dim,mask_type,E,soft_init,ignore_time", CASES[:3])
def test_value_and_differences(dim, mask_type, E, soft_init, ignore_time, act):
    """Value vs nr.realnvp_logdensity at 1e-9; dt (every activation) vs its central difference at 2e-4 of
    scale; dt2 (smooth activations) vs its second difference at 1e-5 of scale, h = 1e-4, all fp64."""
    flat, t, x, kw = _setup(dim, mask_type, E, soft_init, ignore_time)
    logp, d1, d2, margin = ftr.time_derivs(flat, t, x, act=act, **kw)
    f = lambda tt: nr.realnvp_logdensity(flat, tt, x, act=act, **kw)
    h = 1e-4
    f0, fp, fm = f(t), f(t + h), f(t - h)
    assert np.abs(logp - f0).max() < 1e-9 * (1 + np.abs(f0).max())
    fd1 = (fp - fm) / (2 * h)
    err1 = np.abs(d1 - fd1)
    tol1 = 2e-4 * (1 + np.abs(d1).max())
    if act == "relu":
        # relu is only C0: log p has a slope jump wherever a pre-activation crosses 0, and on the ~1 % of
        # samples with such a crossing inside (t - h, t + h) the central difference averages the two slopes
        # (measured: off by up to 2e-2 of scale on 11-36 of the 4096 samples). Those samples are recognised
        # by the reference itself (its one-sided differences disagree beyond the tolerance) and are
        # compared with the second-order one-sided difference of their own side (same points plus t -+ h/2)
        # instead; every sample stays in, at the same tolerance. celu / elu (alpha = 1) are C1 and need
        # none of this.
        jump = np.abs((fp - f0) / h - (f0 - fm) / h) > tol1
        assert jump.mean() < 0.02
        fw = (-3 * f0 + 4 * f(t + h / 2) - fp) / h
        bw = (3 * f0 - 4 * f(t - h / 2) + fm) / h
        err1 = np.where(jump, np.minimum(np.abs(d1 - fw), np.abs(d1 - bw)), err1)
    assert err1.max() < tol1
    assert margin.shape == (x.shape[0],) and (margin >= 0).all() and np.isfinite(margin).all()
    if act in SMOOTH:
        # second difference of an O(10) value in fp64: rounding ~ 1e-15 * |f| / h^2 ~ 1e-6, truncation ~ h^2 f''''
        fd2 = (fp - 2 * f0 + fm) / (h * h)
        assert np.abs(d2 - fd2).max() < 1e-5 * (1 + np.abs(d2).max())


def _torch_logp(flat, t, x, *, dim, masks, base_mean, base_cov, E, ignore_time, soft_init, act):
    """Torch fp64 restatement of nr.realnvp_logdensity for celu / elu / relu, differentiable in t."""
    T = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))
    g = {"celu": lambda z: torch.where(z > 0, z, torch.expm1(torch.clamp(z, max=0.0))),
         "elu": lambda z: torch.where(z > 0, z, torch.expm1(torch.clamp(z, max=0.0))),
         "relu": lambda z: torch.clamp(z, min=0.0)}[act]
    temb, layers = nr.nvp_unflat(flat, dim, masks.shape[0], E, ignore_time)

    def mlp(net, h):
        for k, (W, b) in enumerate(net):
            h = h @ T(W) + T(b)
            if k < 3:
                h = g(h)
        return h

    xs = T(x)
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
    quad = torch.einsum("ni,ij,nj->n", off, T(np.linalg.inv(base_cov)), off)
    return -0.5 * (float(np.log(np.linalg.det(base_cov * 2 * np.pi))) + quad) + ldj


@pytest.mark.parametrize("act", ["celu", "elu", "relu"])
@pytest.mark.parametrize("dim,mask_type,E,soft_init,ignore_time", CASES + [(8, "loop", 10, 1.0, False),
                                                                            (3, "random", 6, 1.0, True)])
def test_kinked_activations_vs_double_autograd(dim, mask_type, E, soft_init, ignore_time, act):
    """celu / elu / relu: the second difference is wrong on samples that cross a kink inside +-h, so the
    helper is pinned by torch fp64 double autograd (the same kink conventions: the derivative of the
    branch taken) at 1e-8 of scale."""
    flat, t, x, kw = _setup(dim, mask_type, E, soft_init, ignore_time, n=512)
    logp, d1, d2, _ = ftr.time_derivs(flat, t, x, act=act, **kw)
    tt = torch.tensor(t, dtype=torch.float64, requires_grad=True)
    lp = _torch_logp(flat, tt, x, act=act, **kw)
    assert np.abs(lp.detach().numpy() - logp).max() < 1e-9 * (1 + np.abs(logp).max())
    if ignore_time:
        assert not lp.requires_grad and (d1 == 0).all() and (d2 == 0).all()
        return
    (g1,) = torch.autograd.grad(lp.sum(), tt, create_graph=True)
    (g2,) = torch.autograd.grad(g1.sum(), tt, allow_unused=True)
    g2 = torch.zeros_like(g1) if g2 is None else g2
    a1, a2 = g1.detach().numpy(), g2.detach().numpy()
    assert np.abs(d1 - a1).max() < 1e-8 * (1 + np.abs(a1).max())
    assert np.abs(d2 - a2).max() < 1e-8 * (1 + np.abs(a2).max())


def test_float32_mode_stays_float32_and_close():
    flat, t, x, kw = _setup(2, "loop", 10, 1.0, False, n=300)
    ref = ftr.time_derivs(flat, t, x, act="tanh", **kw)
    lo = ftr.time_derivs(flat, t, x, act="tanh", dtype=np.float32, **kw)
    assert all(a.dtype == np.float32 for a in lo[:3])
    for a, b in zip(lo[:3], ref[:3]):
        assert np.abs(a - b).max() < 1e-3 * (1 + np.abs(b).max())


def test_header_and_binding_have_the_new_entry_points():
    from utils import native
    txt = open(os.path.join(ROOT, "include", "pdeinv.h")).read()
    declared = set(re.findall(r"^(?:int|int64_t|size_t|const char\*)\s+(pdeinv_\w+)\(", txt, flags=re.M))
    assert NEW_SYMBOLS <= declared and NEW_SYMBOLS <= set(native.EXPORTED_SYMBOLS)
    assert native.ABI_VERSION == 10
    for f in ("realnvp_time_derivs", "realnvp_time_derivs_sets", "kmv_weights_from_ds"):
        assert callable(getattr(native, f))


def test_kmv_sums_with_learned_density_is_an_error():
    """data["kmv_sums"] are formed inside the simulator from the analytic coefficients: with a learned
    density attached the combination is refused, naming both (no GPU is touched before the check)."""
    from core.model import QuadraticModel
    from example_problems.kinetic_mckean_vlasov_example_quadratic import KineticMcKeanVlasov
    from methods.consistency_instances import kinetic_mckean_vlasov as kmv

    inst = KineticMcKeanVlasov.__new__(KineticMcKeanVlasov)  # no sampler / device state needed for the check
    inst.dim = 2
    inst.initial_configuration = {"gamma_friction": 1.0, "tilde_F": np.eye(2)}
    assert inst.learned_log_density is None
    with pytest.raises(TypeError):
        inst.use_learned_log_density(lambda t, x: x)  # no .partial_s / .model
    fn = lambda t, x: x
    fn.model, fn.params, fn.partial_s = object(), {}, lambda t, x: None
    inst.use_learned_log_density(fn)
    assert inst.learned_log_density is fn
    model = QuadraticModel(2, name="tilde_F")
    with pytest.raises(ValueError) as e:
        kmv.value_and_grad_fn(model.apply, None, {"kmv_sums": (None, None)}, None, inst)
    assert "kmv_sums" in str(e.value) and "learned" in str(e.value)
    inst.use_learned_log_density(None)
    assert inst.learned_log_density is None

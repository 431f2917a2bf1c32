"""GPU tests of the RealNVP score (pdeinv_realnvp_score) and of what is built on it (RealNVP.score,
log_density_fn.score, flow_divergence_from_gaussian, flow_divergence), against the restatement tests/flow_score_ref.py
(pinned on the CPU by tests/test_flow_score_ref.py).

Accuracy rule (the project's own, tests/test_gpu_flow_time.py): per output (score, logp), err = max |got - fp64| /
(1 + max |fp64|) <= max(4 x err32, 2e-5), err32 the same error of the float32 restatement with kept inputs on the
same inputs. No sample is left out, except on the relu case: the score jumps where a pre-activation crosses 0, so
there the samples whose margin (the smallest |pre-activation| of the nets) is below 1e-4 may be dropped from the
score comparison, at most 10 % of them.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import flow_map_ref as fmr
import flow_score_ref as fsr

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = fmr.CASES
OUTS = ("score", "logp")


def _t(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _rel(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / (1 + np.abs(ref).max()))


@functools.lru_cache(maxsize=None)
def _case(*case):
    """Inputs and the fp64 / float32 restatements of a case (computed once, shared, left unchanged)."""
    from core.distribution import Gaussian
    from core.normalizing_flow import MNF, RealNVP
    dim, mask_type, E, soft_init, ignore_time, act, n = case
    c = fmr.case_inputs(*case)
    mnf = MNF(dim, c["couple"], mask_type, soft_init, ignore_time, act, E)
    assert np.array_equal(mnf.masks, c["kw"]["masks"])
    flow = RealNVP(mnf, Gaussian(c["mean"], c["cov"]).logdensity)
    t64, x64 = c["t"].astype(np.float64), c["z"][:, :dim].astype(np.float64)
    ref = {"rows": fsr.score(c["flat"], t64, x64, **c["kw"]), "one_t": fsr.score(c["flat"], t64[:1], x64, **c["kw"])}
    lo = {"rows": fsr.score(c["flat"], t64, x64, dtype=np.float32, **c["kw"]),
          "one_t": fsr.score(c["flat"], t64[:1], x64, dtype=np.float32, **c["kw"])}
    z = _t(c["z"])
    return dict(flow=flow, desc=flow._desc, flat=_t(c["flat"]), z=z, x=z[:, :dim], t=_t(c["t"]), ref=ref, lo=lo, dim=dim,
                n=n, act=act, kw=c["kw"], flat64=c["flat"])


def _impls(native, c):
    out = ["general"]
    if c["act"] in ("celu", "elu"):
        assert native.realnvp_score_path(c["desc"], "matrix") == "matrix"
        out.append("matrix")
    else:
        with pytest.raises(NotImplementedError):
            native.realnvp_score_path(c["desc"], "matrix")
    return out + ["auto"]


def _compare(c, which, got, label):
    (s64, lp64, margin), (s32, lp32, _) = c["ref"][which], c["lo"][which]
    keep = np.ones(c["n"], bool)
    if c["act"] == "relu":
        keep = margin >= 1e-4
        print(f"{label}: relu samples with margin < 1e-4 left out of the score comparison: {(~keep).mean():.3f}")
        assert (~keep).mean() <= 0.10
    missed = []
    for name, ref, lo, rows in (("score", s64, s32, keep), ("logp", lp64, lp32, np.ones(c["n"], bool))):
        scale = 1.0 + np.abs(ref).max()
        err32 = np.abs(lo.astype(np.float64) - ref)[rows].max() / scale
        err = np.abs(got[name].double().cpu().numpy() - ref)[rows].max() / scale
        tol = max(4.0 * err32, 2e-5)
        print(f"{label} {name}: kernel err {err:.3e}, float32 restatement err {err32:.3e}, tol {tol:.3e}, "
              f"max|ref| {scale - 1:.3e}")
        if not err <= tol:
            missed.append((label, name, err, tol))
    assert not missed, missed


def _same(a, b):
    return list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("case", CASES, ids=fmr.case_id)
def test_parity_and_structure_every_path(native, case):
    c = _case(*case)
    desc, flat, t, x, dim, n = c["desc"], c["flat"], c["t"], c["x"], c["dim"], c["n"]
    for impl in _impls(native, c):
        got = native.realnvp_score(desc, flat, t, x, impl=impl)      # x: rows of the [n, 2 dim] view
        assert got["score"].shape == (n, dim) and got["logp"].shape == (n,)
        _compare(c, "rows", got, impl)
        _compare(c, "one_t", native.realnvp_score(desc, flat, t[:1], x, impl=impl), impl + " t_stride 0")
        assert _same(got, native.realnvp_score(desc, flat, t, x, impl=impl))                  # deterministic
        assert _same(got, native.realnvp_score(desc, flat, t, x.contiguous(), impl=impl))     # ld_x = dim
        for name in OUTS:                                                                     # one output at a time
            one = native.realnvp_score(desc, flat, t, x, impl=impl, want=(name,))
            assert list(one) == [name] and torch.equal(one[name], got[name])
        buf = torch.full((n, dim + 3), float("nan"), device=DEV)                               # ld_s = dim + 3
        res = native.realnvp_score(desc, flat, t, x, impl=impl, out=buf[:, :dim])
        assert torch.equal(buf[:, :dim], got["score"]) and torch.isnan(buf[:, dim:]).all()
        assert torch.equal(res["logp"], got["logp"])
        if impl == "auto":   # as dispatched: the path realnvp_score_path names, bit for bit
            assert _same(got, native.realnvp_score(desc, flat, t, x, impl=native.realnvp_score_path(desc, "auto")))
        # logp against the map's on the same path
        lp_map = native.realnvp_map(desc, flat, t, x, 1, impl=native.realnvp_score_path(desc, impl), want=("logp",))["logp"]
        err = float((got["logp"] - lp_map).abs().max()) / (1 + float(lp_map.abs().max()))
        print(f"{impl} logp vs realnvp_map(reverse=1): {err:.3e}")
        assert err <= 2e-5


@pytest.mark.parametrize("case", [CASES[0], CASES[1], CASES[12]], ids=fmr.case_id)
def test_outputs_do_not_depend_on_position_or_n(native, case):
    c = _case(*case)
    desc, flat, t, x = c["desc"], c["flat"], c["t"], c["x"]
    for impl in ("general", "matrix"):
        full = native.realnvp_score(desc, flat, t, x, impl=impl)
        for k in (1, 15, 16, 17, 127, 129):
            part = native.realnvp_score(desc, flat, t[:k], x[:k], impl=impl)
            assert all(torch.equal(part[o], full[o][:k]) for o in OUTS), (impl, k)


@pytest.mark.parametrize("case", [CASES[1], CASES[5], CASES[12]], ids=fmr.case_id)
def test_workspace_of_exactly_the_stated_size(native, case):
    """The C entry point with a NaN-filled workspace of exactly workspace_bytes followed by a NaN guard region: the
    guard stays untouched and the outputs are the wrapper's bits."""
    c = _case(*case)
    desc, flat, t, x, dim, n = c["desc"], c["flat"], c["t"], c["x"], c["dim"], c["n"]
    lib = native.lib()
    p = lambda a: ctypes.c_void_p(a.data_ptr())
    for impl, code in (("general", 1), ("matrix", 2)):
        if impl == "matrix" and c["act"] not in ("celu", "elu"):
            assert lib.pdeinv_realnvp_score_workspace_bytes(ctypes.byref(desc), n, code) == 0
            continue
        nbytes = int(lib.pdeinv_realnvp_score_workspace_bytes(ctypes.byref(desc), n, code))
        assert nbytes % 4 == 0 and nbytes >= desc.n_layers * 4 * n    # at least the changed coordinate per layer
        guard = 4096
        buf = torch.full((nbytes // 4 + guard,), float("nan"), device=DEV)
        score = torch.empty((n, dim), device=DEV)
        logp = torch.empty(n, device=DEV)
        rc = lib.pdeinv_realnvp_score(ctypes.byref(desc), p(flat), p(t), 1, p(x), n, x.stride(0), code, p(score), dim,
                                      p(logp), p(buf), nbytes, native.stream_handle())
        assert rc == 0, lib.pdeinv_last_error()
        torch.cuda.synchronize()
        assert torch.isnan(buf[nbytes // 4:]).all(), impl
        got = native.realnvp_score(desc, flat, t, x, impl=impl)
        assert torch.equal(score, got["score"]) and torch.equal(logp, got["logp"]), impl
    # n == 0 is a no-op; an empty batch through the wrapper gives empty outputs
    assert lib.pdeinv_realnvp_score(ctypes.byref(desc), None, None, 1, None, 0, dim, 0, None, 0, None, None, 0,
                                    native.stream_handle()) == 0
    empty = native.realnvp_score(desc, flat, t[:0], x[:0])
    assert empty["score"].shape == (0, dim) and empty["logp"].shape == (0,)
    with pytest.raises(ValueError):
        native.realnvp_score(desc, flat, t[:3], x)
    with pytest.raises(ValueError):
        native.realnvp_score(desc, flat, t, x, want=("y",))
    with pytest.raises(ValueError):
        native.realnvp_score(desc, flat, t, x, out=torch.empty((n + 1, dim), device=DEV))
    with pytest.raises(ValueError):
        native.realnvp_score(desc, flat, t, x, impl="fast")
    if c["act"] not in ("celu", "elu"):
        with pytest.raises(NotImplementedError):
            native.realnvp_score(desc, flat, t, x, impl="matrix")


def test_model_and_log_density_fn_score(native):
    from core.log_density_estimation import make_log_density_fn
    c = _case(*CASES[0])
    flow, flat, t, x, dim = c["flow"], c["flat"], c["t"], c["x"], c["dim"]
    ref = native.realnvp_score(c["desc"], flat, t, x, want=("score",))["score"]
    assert torch.equal(flow.score({"params": flat}, t, x), ref) and torch.equal(flow.score(flat, t, x), ref)
    one = flow.score(flat, float(t[0]), x[0])
    assert one.shape == (dim,) and torch.equal(one, ref[0])
    fn = make_log_density_fn(flow, {"params": flat})
    assert torch.equal(fn.score(t, x), ref) and torch.equal(fn.score(float(t[0]), x[0].cpu().numpy()), ref[0])
    same_t = fn.score(0.7, x[:10])
    assert torch.equal(same_t, native.realnvp_score(c["desc"], flat, _t([0.7]), x[:10])["score"])


def _redraw(native, key, mean, cov, n, **kw):
    """The rows flow_divergence_from_gaussian draws, as its docstring states them."""
    return native.gaussian_sample_grouped(n, _t(mean), _t(np.linalg.cholesky(cov)), seed=key.seed, **kw)


def test_divergence_of_the_identity_flow(native):
    """All-zero flow parameters: the flow is the identity and rho^ is its base N(mu, Sigma) at every t."""
    from core.distribution import Gaussian
    from core.log_density_estimation import flow_divergence_from_gaussian, make_log_density_fn
    from core.normalizing_flow import MNF, RealNVP
    from utils import prng
    d, n, taus = 3, 4096, np.array([0.2, 1.1])
    rng = np.random.default_rng(31)
    mu = rng.standard_normal(d) * 0.3
    Lc = rng.standard_normal((d, d)) * 0.3
    Sig = Lc @ Lc.T + np.eye(d)
    mnf = MNF(d, 4, "loop", 1.0, False, "celu", 10)
    flow = RealNVP(mnf, Gaussian(mu, Sig).logdensity)
    fn = make_log_density_fn(flow, {"params": torch.zeros(mnf.param_count(), device=DEV)})
    key = prng.PRNGKey(17)
    mean, cov = np.tile(mu, (2, 1)), np.tile(Sig, (2, 1, 1))
    kl, fi = flow_divergence_from_gaussian(fn, key, taus, mean, cov, n)
    assert kl.dtype == fi.dtype == torch.float64 and kl.shape == fi.shape == (2,) and kl.is_cuda
    print("identity flow, truth = base: kl", kl.cpu().numpy(), "fisher_rel", fi.cpu().numpy())
    assert float(kl.abs().max()) < 1e-5 and float(fi.abs().max()) < 1e-5
    delta = np.array([0.5, -0.3, 0.2])
    Pinv = np.linalg.inv(Sig)
    q = float(delta @ Pinv @ delta)
    kl, fi = flow_divergence_from_gaussian(fn, key, taus, mean + delta, cov, n)
    sigma = np.sqrt(q / n)
    print("identity flow, shifted truth: kl", kl.cpu().numpy(), "exact", 0.5 * q, "sigma", sigma)
    assert (np.abs(kl.cpu().numpy() - 0.5 * q) <= 5 * sigma).all()
    x = _redraw(native, key, mean + delta, cov, n).double().cpu().numpy().reshape(2, n, d)
    w = np.einsum("ij,knj->kni", Pinv, x - (mu + delta))
    ratio = float((Pinv @ delta) @ (Pinv @ delta)) / (w ** 2).sum(-1).mean(1)    # the numerator: the same on every sample
    print("fisher_rel", fi.cpu().numpy(), "fp64 on the redrawn rows", ratio)
    assert (np.abs(fi.cpu().numpy() - ratio) <= 1e-4 * ratio).all()
    # row_offset / counter_offset select the stream's rows
    kl_o, fi_o = flow_divergence_from_gaussian(fn, key, taus, mean + delta, cov, n, row_offset=5, counter_offset=3)
    assert not torch.equal(kl_o, kl)
    x_o = _redraw(native, key, mean + delta, cov, n, row_offset=5, counter_offset=3).double().cpu().numpy().reshape(2, n, d)
    w_o = np.einsum("ij,knj->kni", Pinv, x_o - (mu + delta))
    ratio_o = float((Pinv @ delta) @ (Pinv @ delta)) / (w_o ** 2).sum(-1).mean(1)
    assert (np.abs(fi_o.cpu().numpy() - ratio_o) <= 1e-4 * ratio_o).all()


@pytest.mark.parametrize("case", [CASES[0], CASES[1]], ids=fmr.case_id)
def test_divergence_of_a_flow_against_the_restatement(native, case):
    """3 stamps x 257 rows: the function's two means equal the same means formed in NumPy fp64 from flow_score_ref on
    the redrawn rows. Tolerance: the parity rule propagated. With eps_l = tol_logp (1 + max|logp|) and eps_s =
    tol_score (1 + max|score|) the per-sample bounds of the rule (tol = max(4 err32, 2e-5) on these rows), the truth's
    terms being fp64 on both sides: |d kl| <= eps_l, and with r = score + w, |r + e|^2 - |r|^2 <= 2 |r| sqrt(d) eps_s +
    d eps_s^2 per sample, so |d fisher_rel| <= (2 sqrt(d) eps_s mean|r| + d eps_s^2) / mean|w|^2."""
    from core.log_density_estimation import flow_divergence_from_gaussian, make_log_density_fn
    from utils import prng
    c = _case(*case)
    d, n, taus = c["dim"], 257, np.array([0.3, 0.9, 1.6])
    rng = np.random.default_rng(50 + d)
    mean = rng.standard_normal((3, d)) * 0.5
    Lc = rng.standard_normal((3, d, d)) * 0.4
    cov = Lc @ Lc.transpose(0, 2, 1) + 0.8 * np.eye(d)
    fn = make_log_density_fn(c["flow"], {"params": c["flat"]})
    key = prng.PRNGKey(23)
    kl, fi = flow_divergence_from_gaussian(fn, key, taus, mean, cov, n)
    x = _redraw(native, key, mean, cov, n).double().cpu().numpy()
    tt = np.repeat(taus.astype(np.float32).astype(np.float64), n)
    s64, lp64, _ = fsr.score(c["flat64"], tt, x, **c["kw"])
    s32, lp32, _ = fsr.score(c["flat64"], tt, x, dtype=np.float32, **c["kw"])
    eps_s = max(4 * _rel(s32, s64), 2e-5) * (1 + np.abs(s64).max())
    eps_l = max(4 * _rel(lp32, lp64), 2e-5) * (1 + np.abs(lp64).max())
    off = x.reshape(3, n, d) - mean[:, None, :]
    w = np.einsum("kij,knj->kni", np.linalg.inv(cov), off)
    lp_true = -0.5 * (np.linalg.slogdet(2 * np.pi * cov)[1][:, None] + (off * w).sum(-1))
    kl_ref = (lp_true - lp64.reshape(3, n)).mean(1)
    r = s64.reshape(3, n, d) + w
    den = (w ** 2).sum(-1).mean(1)
    fi_ref = (r ** 2).sum(-1).mean(1) / den
    tol_f = (2 * np.sqrt(d) * eps_s * np.sqrt((r ** 2).sum(-1)).mean(1) + d * eps_s ** 2) / den
    print("kl", kl.cpu().numpy(), "ref", kl_ref, "tol", eps_l)
    print("fisher_rel", fi.cpu().numpy(), "ref", fi_ref, "tol", tol_f)
    assert (np.abs(kl.cpu().numpy() - kl_ref) <= eps_l).all()
    assert (np.abs(fi.cpu().numpy() - fi_ref) <= tol_f).all()


def test_flow_divergence_uses_the_instance_marginal(native):
    from core.log_density_estimation import (create_normalizing_flow_fn, flow_divergence,
                                             flow_divergence_from_gaussian, make_log_density_fn)
    from example_problems.kinetic_mckean_vlasov_example_quadratic import KineticMcKeanVlasov
    from utils import config, prng
    d = 2
    cfg = config.compose("config", ["pde_instance=kinetic_mckean_vlasov", f"pde_instance.domain_dim={d}"])
    pi = KineticMcKeanVlasov(cfg, prng.PRNGKey(0))
    flow = create_normalizing_flow_fn(pi.distribution_initial_x.logdensity, d)
    fn = make_log_density_fn(flow, {"params": torch.zeros(flow.mnf.param_count(), device=DEV)})
    taus, key = np.array([0.0, 0.5]), prng.PRNGKey(4)
    kl, fi = flow_divergence(fn, key, pi, taus, 2048)
    mean, cov = pi.x_marginal(taus)
    kl2, fi2 = flow_divergence_from_gaussian(fn, key, taus, mean, cov, 2048)
    assert torch.equal(kl, kl2) and torch.equal(fi, fi2)
    # the identity flow is the initial marginal: exact at t = 0, not later
    print("kl", kl.cpu().numpy(), "fisher_rel", fi.cpu().numpy())
    assert abs(float(kl[0])) < 1e-5 and float(fi[0]) < 1e-5 and float(kl[1]) > 1e-3 and float(fi[1]) > 1e-3

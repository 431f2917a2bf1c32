"""GPU tests of the RealNVP flow as a map (pdeinv_realnvp_map: general and matrix-core path, both directions) and of
what is built on it (MNF.apply, RealNVP.inverse / forward / sample, flow_sample_moments, flow_moment_error), against
the restatement tests/flow_map_ref.py (pinned on the CPU by tests/test_flow_map_ref.py).

Accuracy rule (the project's own, tests/test_gpu_flow_time.py): per output (y, ldj, logp), err = max |got - fp64| /
(1 + max |fp64|) <= max(4 x err32, 2e-5), err32 the same error of the float32 restatement on the same inputs. No
sample is left out: the map and log p are continuous at the activations' kinks.
"""
import functools

import numpy as np
import pytest
import torch

import flow_map_ref as fmr

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = fmr.CASES
OUTS = ("y", "ldj", "logp")


def _t(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


@functools.lru_cache(maxsize=None)
def _case(*case):
    """Inputs and the fp64 / float32 restatements of a case (computed once, shared, left unchanged)."""
    from core.distribution import Gaussian
    from core.normalizing_flow import MNF, RealNVP
    dim, mask_type, E, soft_init, ignore_time, act, n = case
    c = fmr.case_inputs(*case)
    mnf = MNF(dim, c["couple"], mask_type, soft_init, ignore_time, act, E)
    assert np.array_equal(mnf.masks, c["kw"]["masks"])
    gauss = Gaussian(c["mean"], c["cov"])
    flow = RealNVP(mnf, gauss.logdensity)
    t64 = c["t"].astype(np.float64)
    xin = {1: c["z"][:, :dim].astype(np.float64), 0: c["x0"].astype(np.float64)}
    ref, lo = {}, {}
    for rev in (0, 1):
        ref[rev, "rows"] = fmr.flow_map(c["flat"], t64, xin[rev], bool(rev), **c["kw"])
        ref[rev, "one_t"] = fmr.flow_map(c["flat"], t64[:1], xin[rev], bool(rev), **c["kw"])
        lo[rev, "rows"] = fmr.flow_map(c["flat"], t64, xin[rev], bool(rev), dtype=np.float32, **c["kw"])
        lo[rev, "one_t"] = fmr.flow_map(c["flat"], t64[:1], xin[rev], bool(rev), dtype=np.float32, **c["kw"])
    # the float32 restatement's own round trip x0 -> y -> x0' (its figures size the round-trip bound)
    y32, ldj32, _ = lo[0, "rows"]
    b32, ldjb32, _ = fmr.flow_map(c["flat"], t64, y32.astype(np.float64), True, dtype=np.float32, **c["kw"])
    rt32 = np.abs(b32.astype(np.float64) - xin[0]).max() / (1 + np.abs(xin[0]).max())
    sg32 = np.abs(ldj32.astype(np.float64) + ldjb32).max() / (1 + np.abs(ref[0, "rows"][1]).max())
    z = _t(c["z"])
    return dict(flow=flow, mnf=mnf, gauss=gauss, desc=flow._desc, flat=_t(c["flat"]), z=z, x={1: z[:, :dim], 0: _t(c["x0"])},
                t=_t(c["t"]), ref=ref, lo=lo, rt32=rt32, sg32=sg32, dim=dim, n=n, act=act, kw=c["kw"])


def _impls(native, c):
    out = ["general"]
    if c["act"] in ("celu", "elu"):
        assert native.realnvp_map_path(c["desc"], "matrix") == "matrix"
        out.append("matrix")
    else:
        with pytest.raises(NotImplementedError):
            native.realnvp_map_path(c["desc"], "matrix")
    return out + ["auto"]


def _compare(c, rev, which, got, label):
    ref, lo = c["ref"][rev, which], c["lo"][rev, which]
    missed = []
    for k, name in enumerate(OUTS):
        scale = 1.0 + np.abs(ref[k]).max()
        err32 = np.abs(lo[k].astype(np.float64) - ref[k]).max() / scale
        err = np.abs(got[name].double().cpu().numpy() - ref[k]).max() / scale
        tol = max(4.0 * err32, 2e-5)
        print(f"{label} {name}: kernel err {err:.3e}, float32 restatement err {err32:.3e}, tol {tol:.3e}, "
              f"max|ref| {scale - 1:.3e}")
        if not err <= tol:
            missed.append((label, name, err, tol))
    assert not missed, missed


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("case", CASES, ids=fmr.case_id)
def test_parity_both_directions_every_path(native, case):
    c = _case(*case)
    desc, flat, t, dim, n = c["desc"], c["flat"], c["t"], c["dim"], c["n"]
    for rev in (1, 0):
        x = c["x"][rev]
        for impl in _impls(native, c):
            label = f"{'reverse' if rev else 'generate'} {impl}"
            got = native.realnvp_map(desc, flat, t, x, rev, impl=impl)
            assert got["y"].shape == (n, dim) and got["ldj"].shape == (n,) and got["logp"].shape == (n,)
            _compare(c, rev, "rows", got, label)
            _compare(c, rev, "one_t", native.realnvp_map(desc, flat, t[:1], x, rev, impl=impl), label + " t_stride 0")
            assert _same(got, native.realnvp_map(desc, flat, t, x, rev, impl=impl))          # deterministic
            for name in OUTS:                                                                 # one output at a time
                one = native.realnvp_map(desc, flat, t, x, rev, impl=impl, want=(name,))
                assert list(one) == [name] and torch.equal(one[name], got[name])
            buf = torch.full((n, dim + 3), float("nan"), device=DEV)                           # ld_y = dim + 3
            res = native.realnvp_map(desc, flat, t, x, rev, impl=impl, out=buf[:, :dim])
            assert torch.equal(buf[:, :dim], got["y"]) and torch.isnan(buf[:, dim:]).all()
            assert torch.equal(res["ldj"], got["ldj"]) and torch.equal(res["logp"], got["logp"])
            if impl == "auto":   # as dispatched: one of the two, bit for bit
                assert _same(got, native.realnvp_map(desc, flat, t, x, rev, impl=native.realnvp_map_path(desc, "auto")))


@pytest.mark.parametrize("case", [CASES[0], CASES[1], CASES[12]], ids=fmr.case_id)
def test_outputs_do_not_depend_on_position_or_n(native, case):
    c = _case(*case)
    desc, flat, t = c["desc"], c["flat"], c["t"]
    for rev in (1, 0):
        x = c["x"][rev]
        for impl in ("general", "matrix"):
            full = native.realnvp_map(desc, flat, t, x, rev, impl=impl)
            for k in (1, 15, 16, 17, 127, 129):
                part = native.realnvp_map(desc, flat, t[:k], x[:k], rev, impl=impl)
                assert all(torch.equal(part[o], full[o][:k]) for o in OUTS), (rev, impl, k)


@pytest.mark.parametrize("case", CASES, ids=fmr.case_id)
def test_log_density_tie(native, case):
    c = _case(*case)
    desc, flat, t, x = c["desc"], c["flat"], c["t"], c["x"][1]
    val = native.realnvp_logdensity(desc, flat, t, x)
    gen = native.realnvp_map(desc, flat, t, x, 1, impl="general", want=("logp",))["logp"]
    assert torch.equal(gen, val)
    if c["act"] in ("celu", "elu"):
        mat = native.realnvp_map(desc, flat, t, x, 1, impl="matrix", want=("logp",))["logp"]
        err = float((mat - val).abs().max()) / (1 + float(val.abs().max()))
        print(f"matrix-core logp vs pdeinv_realnvp_logdensity: {err:.3e}")
        assert err <= 2e-5


@pytest.mark.parametrize("case", CASES, ids=fmr.case_id)
def test_round_trip_and_sign(native, case):
    c = _case(*case)
    desc, flat, t, x0 = c["desc"], c["flat"], c["t"], c["x"][0]
    for impl in _impls(native, c)[:-1]:
        f = native.realnvp_map(desc, flat, t, x0, 0, impl=impl)
        r = native.realnvp_map(desc, flat, t, f["y"], 1, impl=impl)
        rt = float((r["y"] - x0).abs().max()) / (1 + float(x0.abs().max()))
        sg = float((f["ldj"] + r["ldj"]).abs().max()) / (1 + np.abs(c["ref"][0, "rows"][1]).max())
        print(f"{impl}: round trip {rt:.3e} (float32 restatement {c['rt32']:.3e}), sign {sg:.3e} ({c['sg32']:.3e})")
        assert rt <= max(4 * c["rt32"], 2e-5) and sg <= max(4 * c["sg32"], 2e-5)


@pytest.mark.parametrize("case", [CASES[0], CASES[1], CASES[2]], ids=fmr.case_id)
def test_in_place(native, case):
    c = _case(*case)
    desc, flat, t, dim = c["desc"], c["flat"], c["t"], c["dim"]
    for rev in (1, 0):
        for impl in ("general", "matrix"):
            z = c["z"].clone()
            ref = native.realnvp_map(desc, flat, t, z[:, :dim], rev, impl=impl)
            res = native.realnvp_map(desc, flat, t, z[:, :dim], rev, impl=impl, out=z[:, :dim])   # ld_y = ld_x = 2 dim
            assert torch.equal(z[:, :dim], ref["y"]) and torch.equal(z[:, dim:], c["z"][:, dim:])
            assert torch.equal(res["ldj"], ref["ldj"]) and torch.equal(res["logp"], ref["logp"])


@pytest.mark.parametrize("case", [CASES[0], CASES[1]], ids=fmr.case_id)
def test_sampler(native, case):
    from utils import prng
    c = _case(*case)
    flow, flat, dim = c["flow"], c["flat"], c["dim"]
    key, n = prng.PRNGKey(41), 1000
    t = _t(np.random.default_rng(3).uniform(0.05, 2.0, n))
    x, logp = flow.sample({"params": flat}, key, t, n)
    assert x.shape == (n, dim) and logp.shape == (n,)
    x0 = c["gauss"].sample(n, key)
    push = native.realnvp_map(c["desc"], flat, t, x0, 0)
    assert torch.equal(push["y"], x) and torch.equal(push["logp"], logp)
    xa, la = flow.sample(flat, key, t[:389], 389)
    xb, lb = flow.sample(flat, key, t[389:], 611, row_offset=389)
    assert torch.equal(torch.cat([xa, xb]), x) and torch.equal(torch.cat([la, lb]), logp)
    val = native.realnvp_logdensity(c["desc"], flat, t, x)
    assert float((logp - val).abs().max()) <= 2e-5 * (1 + float(val.abs().max()))
    xs, ls = flow.sample(flat, key, 0.7, n)
    xe, le = flow.sample(flat, key, torch.full((n,), 0.7, device=DEV), n)
    assert torch.equal(xs, xe) and torch.equal(ls, le)
    f = flow.forward(flat, t, x0)
    assert torch.equal(f[0], x) and torch.equal(f[1], logp)
    inv = flow.inverse(flat, t, x)
    back = native.realnvp_map(c["desc"], flat, t, x, 1)
    assert torch.equal(inv[0], back["y"]) and torch.equal(inv[1], back["ldj"])


def test_law_of_an_affine_flow(native):
    """d = 3, E = 0, every net kernel zero (biases and scaling factors perturbed): each layer is one affine map for
    all samples, so samples are Gaussian with a closed-form mean and covariance (composed here in fp64). Over 2^16
    samples: mean and covariance within 5.5 sigma, logp = that Gaussian's log-density under the accuracy rule."""
    from core.distribution import Gaussian
    from core.normalizing_flow import MNF, RealNVP
    from oracle import numpy_ref as nr
    from utils import prng
    d, n, tval = 3, 1 << 16, 0.8
    mnf = MNF(d, 4, "loop", 1.0, False, "celu", 0)
    flat = nr.nvp_init(d, mnf.n_layers, 0, False, seed=7, scale=1.0, perturb=True)
    _, layers = nr.nvp_unflat(flat, d, mnf.n_layers, 0, False)
    for sf, snet, tnet in layers:          # views into flat: zero the kernels in place
        for W, _b in snet + tnet:
            W[...] = 0.0
    flat = flat.astype(np.float32).astype(np.float64)
    rng = np.random.default_rng(12)
    mean = rng.standard_normal(d) * 0.3
    Lc = rng.standard_normal((d, d)) * 0.3
    cov = Lc @ Lc.T + np.eye(d)
    flow = RealNVP(mnf, Gaussian(mean, cov).logdensity)
    # x -> x e^{-s} - tr per layer, s and tr constants: compose mu, C
    _, layers = nr.nvp_unflat(flat, d, mnf.n_layers, 0, False)
    mu, C = mean.copy(), cov.copy()
    zero_in = np.zeros((1, d + 1))
    for l in range(mnf.n_layers):
        sf, snet, tnet = layers[l]
        keep = 1 - mnf.masks[l]
        s = np.tanh(nr._nvp_mlp(snet, zero_in, "celu")[0] / np.exp(sf)) * np.exp(sf) * keep
        tr = nr._nvp_mlp(tnet, zero_in, "celu")[0] * keep
        D = np.diag(np.exp(-s))
        mu, C = D @ mu - tr, D @ C @ D
    x, logp = flow.sample(_t(flat), prng.PRNGKey(5), tval, n)
    xs = x.double().cpu().numpy()
    m_hat, c_hat = xs.mean(0), np.cov(xs.T, bias=True)
    sig_m = np.sqrt(np.diag(C) / n)
    sig_c = np.sqrt((np.outer(np.diag(C), np.diag(C)) + C * C) / n)
    print("mean dev / sigma", np.abs(m_hat - mu) / sig_m, "cov dev / sigma", np.abs(c_hat - C) / sig_c)
    assert (np.abs(m_hat - mu) <= 5.5 * sig_m).all() and (np.abs(c_hat - C) <= 5.5 * sig_c).all()
    off = xs - mu
    exact = -0.5 * (np.log(np.linalg.det(2 * np.pi * C)) + np.einsum("ni,ij,nj->n", off, np.linalg.inv(C), off))
    kw = dict(dim=d, masks=mnf.masks, base_mean=mean, base_cov=cov, E=0, act="celu")
    x0 = flow.log_prob_0.__self__.sample(n, prng.PRNGKey(5)).double().cpu().numpy()
    lo = fmr.flow_map(flat, np.full(n, tval), x0, False, dtype=np.float32, **kw)[2]
    hi = fmr.flow_map(flat, np.full(n, tval), x0, False, **kw)[2]
    scale = 1 + np.abs(exact).max()
    tol = max(4 * np.abs(lo - hi).max() / scale, 2e-5)
    err = np.abs(logp.double().cpu().numpy() - exact).max() / scale
    print(f"affine flow logp vs the exact Gaussian: {err:.3e} (tol {tol:.3e})")
    assert err <= tol


def test_product_functions(native):
    from core.log_density_estimation import flow_moment_error, flow_sample_moments, make_log_density_fn
    from utils import prng
    c = _case(*CASES[0])
    flow, flat, dim = c["flow"], c["flat"], c["dim"]
    fn = make_log_density_fn(flow, {"params": flat})
    taus, n = np.array([0.3, 0.9, 1.6]), 4096
    key = prng.PRNGKey(8)
    mean, cov = flow_sample_moments(fn, key, taus, n)
    x, _ = fn.sample(key, _t(taus).repeat_interleave(n), 3 * n)
    xs = x.double().cpu().numpy().reshape(3, n, dim)
    assert mean.shape == (3, dim) and cov.shape == (3, dim, dim)
    np.testing.assert_allclose(mean.cpu().numpy(), xs.mean(1), rtol=1e-5, atol=1e-5 * np.abs(xs).max())
    ref_cov = np.stack([np.cov(xs[k].T, bias=True) for k in range(3)])
    np.testing.assert_allclose(cov.cpu().numpy(), ref_cov, rtol=1e-5, atol=1e-5 * np.abs(ref_cov).max())
    # a dataset made of the flow's own samples under another key: [n_time, n_traj, 2 dim] time-major, tau per stamp
    n_traj = 4096
    xd, _ = fn.sample(prng.PRNGKey(9), _t(taus).repeat_interleave(n_traj), 3 * n_traj)
    data = {"0T_tm": torch.cat([xd.reshape(3, n_traj, dim), torch.zeros((3, n_traj, dim), device=DEV)], -1),
            "tau_0T": _t(taus).repeat(n_traj, 1)}
    e_mean, e_cov = flow_moment_error(fn, key, data, [0, 1, 2], n)
    # sampling error of the difference of two independent estimates, relative to the Frobenius norms
    sig_m = np.sqrt(np.trace(ref_cov, axis1=1, axis2=2) * (1 / n + 1 / n_traj)) / np.linalg.norm(xs.mean(1), axis=1)
    x4 = ((xs - xs.mean(1, keepdims=True))[:, :, :, None] * (xs - xs.mean(1, keepdims=True))[:, :, None, :])
    var_c = x4.reshape(3, n, -1).var(1).sum(-1)
    sig_c = np.sqrt(var_c * (1 / n + 1 / n_traj)) / np.linalg.norm(ref_cov.reshape(3, -1), axis=1)
    print("flow_moment_error mean", e_mean.cpu().numpy(), "sigma", sig_m, "cov", e_cov.cpu().numpy(), "sigma", sig_c)
    assert ((e_mean.cpu().numpy() > 0) & (e_mean.cpu().numpy() < 6 * sig_m)).all()
    assert ((e_cov.cpu().numpy() > 0) & (e_cov.cpu().numpy() < 6 * sig_c)).all()
    inv = fn.inverse(0.9, x[:10])
    assert torch.equal(inv[0], flow.inverse(flat, 0.9, x[:10])[0])
    # MNF.apply: the reference's call, batched and unbatched
    x0, t = c["x"][0], c["t"]
    y, ldj = c["mnf"].apply({"params": flat}, t, x0, reverse=False)
    res = native.realnvp_map(c["desc"], flat, t, x0, 0)
    assert torch.equal(y, res["y"]) and torch.equal(ldj, res["ldj"])
    yr, ldjr = c["mnf"](flat, t, c["x"][1], reverse=True)
    res = native.realnvp_map(c["desc"], flat, t, c["x"][1], 1)
    assert torch.equal(yr, res["y"]) and torch.equal(ldjr, res["ldj"])
    y1, l1 = c["mnf"].apply(flat, float(t[0]), x0[0])
    assert y1.shape == (dim,) and l1.dim() == 0 and torch.equal(y1, y[0]) and torch.equal(l1, ldj[0])

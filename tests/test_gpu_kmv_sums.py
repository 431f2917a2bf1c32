"""The quadratic-Phi McKean-Vlasov residual's HIP stages against fp64, entry by entry, at every compiled dimension.

The product path of BASELINE config C4 runs through pdeinv_sde_simulate_mf_kmv (the stamp sums formed inside the
simulator), pdeinv_kmv_moments_weights and the split pair pdeinv_moments_batched + pdeinv_kmv_weights (the same sums
from a written trajectory) and pdeinv_residual_kmv (sums -> loss and gradient). test_gpu_meanfield.py compares these
kernels with each other; here each is compared with tests/kmv_sums_ref.py: the fp64 column sums of stamp_terms (ds
log rho from the closed form, not from the coefficient table), every entry within FACTOR x E[e] of the fp32 yardstick
built for the kernel's own chain lengths (the count exactly), and the finalize within one fp32 rounding of
oracle.numpy_ref.kmv_from_moments. test_kmv_sums_ref.py (CPU) shows that this tolerance rejects any single dropped
row and three wrong formulas at every (d, N) used here. The coefficient stamps come from a problem with a shifted
initial mean, so that m1 and beta are not identically zero as they are in the product's centred problem.

Each case prints its max |err| / E (pytest -s); the figures of the MI355X run are in kmv_sums_ref.MEASURED.
"""
import ctypes

import numpy as np
import pytest
import torch

import kmv_sums_ref as R
from oracle import numpy_ref as nr

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32


def _t(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _coef(tau, cfg, d):
    """(fp32 coefficient rows on the host, the same on the device)."""
    c32 = R.coefficients(tau, cfg, d).astype(F32)
    return c32, _t(c32)


def _check_stamp(got_mom, got_wst, z, tau, cfg, coef32, d, gamma, chains, what):
    """One stamp's [mom | wst] against the fp64 sums over the fp32 rows z, per entry; the count exactly."""
    ref = R.stamp_sums(z, tau, cfg, d, gamma)
    E = R.fp32_yardstick(z, coef32, d, gamma, chains, ref)
    got = np.concatenate([got_mom, got_wst])
    assert got[0] == len(z), (what, got[0])
    return R.check_entries(got, ref, E, what)


# ---- a. sde_mf_kmv_kernel<D> ---------------------------------------------------------------------------------
# D in {2, 4, 6, 8} are all the compiled dimensions: sde_mf_kmv_kernel<D, 4, false>. The <D, 4, true> instances (with
# the next simulate's sums) are held bit-equal to these in mom / wst at every D by test_gpu_meanfield.py's
# test_simulate_mf_kmv_equals_separate. N = 1, 63: one
# partial wave; 64: one full wave, three waves past N; 65: a full and a one-row wave; 255 / 257: the block boundary
# (257 = two blocks); 4099: 17 blocks, three rows in the last.
_SIM = [(d, n, 3, 1.0) for d, n in R.SIM_CASES] + [(8, 257, 1, 1.0),   # n_steps = 1: only red[0] carries data
                                                    (6, 257, 3, 0.5)]   # gamma = 0.5 in the weight


@pytest.mark.parametrize("d,N,n_steps,gamma", _SIM)
def test_simulate_mf_kmv_sums_vs_fp64(native, d, N, n_steps, gamma):
    """pdeinv_sde_simulate_mf_kmv: mom / wst against fp64 sums over the trajectory the same call wrote (bit-equal
    to the plain simulate, which test_mean_field_vs_c_oracle pins against the C oracle). n_steps = 3 puts data in
    both halves of the red[s & 1] double buffer."""
    cfg = R.problem_cfg(d)
    z0 = _t(R.states(N, 2 * d, 7 * d + N))
    desc, keep = native.mf_desc(N, d, n_steps, 0.02, 1.0, cfg["tilde_F"], seed=0x5EED_0004, counter_offset=777)
    xbar, _ = native.mf_mean_path(desc, native.mf_sums(desc, z0), xsum=False)
    desc.d_meanfield = ctypes.c_void_p(xbar.data_ptr())
    tau = np.linspace(0.2, 1.8, n_steps)
    coef32, coef = _coef(tau, cfg, d)
    traj, traj0 = (torch.empty((n_steps, N, 2 * d), device=DEV) for _ in range(2))
    last, last0 = (torch.empty((N, 2 * d), device=DEV) for _ in range(2))
    mom, wst = native.sde_simulate_mf_kmv(desc, z0, traj, None, last, gamma, coef)
    native.sde_simulate_desc(desc, z0, traj0, None, last0)
    assert torch.equal(traj, traj0) and torch.equal(last, last0)
    mom, wst, rows = mom.cpu().numpy(), wst.cpu().numpy(), traj.cpu().numpy()
    assert np.array_equal(mom[:, 0], np.full(n_steps, float(N)))
    for s in range(n_steps):
        _check_stamp(mom[s], wst[s], rows[s], tau[s], cfg, coef32[s], d, gamma, R.SIM_CHAINS,
                     f"sde_mf_kmv d={d} N={N} n_steps={n_steps} gamma={gamma} stamp={s}")
    del keep


# ---- b. kmv_moments_weights_kernel<D, PACKED> ----------------------------------------------------------------
def _layout(z_np, layout):
    """z_np [n_t, n, m] -> (device tensor, set_stride, ld) in one of the row layouts the dispatch distinguishes."""
    n_t, n, m = z_np.shape
    if layout == "time_major":    # ld == 2d, 16-byte aligned: PACKED for even d (one coalesced block load per wave)
        return _t(z_np), n * m, m
    if layout == "particle_major":  # the reference's (particle, stamp) row order: lane-private dwordx4 for even d
        return _t(z_np.transpose(1, 0, 2)), m, n_t * m
    buf = torch.zeros(n_t * n * m + 4, device=DEV)  # a view one float into its storage: scalar loads
    view = buf[1:1 + n_t * n * m].view(n_t, n, m)
    view.copy_(_t(z_np))
    assert view.data_ptr() % 16 == 4
    return view, n * m, m


@pytest.mark.parametrize("layout", ["time_major", "particle_major", "offset_one_float"])
@pytest.mark.parametrize("d", range(1, 9))  # kmv_moments_weights_kernel<d, PACKED = (d even and time_major)>
def test_kmv_moments_weights_vs_fp64(native, d, layout):
    """n_rows = 1, 63 (a partial wave), 65 (a one-row wave), 257 (two blocks), n_t = 3: one row block per wave."""
    cfg = R.problem_cfg(d)
    coef32, coef = _coef(R.TAUS, cfg, d)
    for n in R.MW_ROWS:
        z_np = np.stack([R.states(n, 2 * d, 1000 * t + 10 * d + n) for t in range(3)])
        z, set_stride, ld = _layout(z_np, layout)
        assert R.batched_trips(3, n) == 1
        mom, wst = native.kmv_moments_weights(d, 1.0, coef, z, 3, n, set_stride, ld)
        mom, wst = mom.cpu().numpy(), wst.cpu().numpy()
        for t, tau in enumerate(R.TAUS):
            _check_stamp(mom[t], wst[t], z_np[t], tau, cfg, coef32[t], d, 1.0, R.mw_chains(3, n),
                         f"kmv_moments_weights d={d} {layout} n={n} stamp={t}")


@pytest.mark.parametrize("d,aligned", [(8, True),    # kmv_moments_weights_kernel<8, true>: the prefetching loop
                                       (3, False)])  # <3, false>: the lane-private prefetching loop
def test_kmv_moments_weights_grid_capped(native, d, aligned):
    """n_sets = 512 caps the grid at batched_bx = 8 blocks of 256 rows: with n_rows = 6100 every wave makes exactly 3
    trips (rows r0, r0 + 2048, r0 + 4096) and the last wave's third block holds 20 rows; the accumulators carry over
    the trips (chains (192, 4)). The 512 sets read the same rows (set_stride = 0) at three stamps in turn, so three
    references serve them all; sets of the same stamp must agree bit for bit."""
    n_sets, n = R.MW_CAPPED["n_sets"], R.MW_CAPPED["n_rows"]
    assert R.batched_bx(n_sets, n) == 8 and R.batched_trips(n_sets, n) == 3
    cfg = R.problem_cfg(d)
    c3, _ = _coef(R.TAUS, cfg, d)
    coef = _t(c3[np.arange(n_sets) % 3])
    z_np = R.states(n, 2 * d, 99 + d)
    z = _t(z_np)
    assert d in R.MW_CAPPED["dims"] and (z.data_ptr() % 16 == 0) and aligned == (d % 2 == 0)
    mom, wst = native.kmv_moments_weights(d, 1.0, coef, z, n_sets, n, 0, 2 * d)
    mom, wst = mom.cpu().numpy(), wst.cpu().numpy()
    for t, tau in enumerate(R.TAUS):
        assert np.array_equal(mom[t::3], np.broadcast_to(mom[t], mom[t::3].shape))
        assert np.array_equal(wst[t::3], np.broadcast_to(wst[t], wst[t::3].shape))
        _check_stamp(mom[t], wst[t], z_np, tau, cfg, c3[t], d, 1.0, R.mw_chains(n_sets, n),
                     f"kmv_moments_weights capped d={d} stamp={t}")


# ---- c. kmv_weights_kernel<D> and moments_batched_kernel<M> ----------------------------------------------------
@pytest.mark.parametrize("d", R.WEIGHT_DIMS)  # kmv_weights_kernel<d>: every instance of the dispatch
def test_kmv_weights_vs_fp64(native, d):
    """The weighted sums per entry and the per-row (ds log rho, ds2 log rho) against the closed form; n = 65 (a
    one-row wave) and 257 (two blocks), rows of 2d floats."""
    cfg = R.problem_cfg(d)
    coef32, coef = _coef(R.TAUS, cfg, d)
    lz = R.moment_len(2 * d)
    outside = total = 0
    for n in R.SEP_ROWS:
        z_np = np.stack([R.states(n, 2 * d, 2000 * t + 10 * d + n) for t in range(3)])
        wst, ds = native.kmv_weights(d, 1.0, coef, _t(z_np), 3, n, n * 2 * d, 2 * d, want_ds=True)
        wst, ds = wst.cpu().numpy(), ds.double().cpu().numpy()
        for t, tau in enumerate(R.TAUS):
            ref = R.stamp_sums(z_np[t], tau, cfg, d, 1.0)
            E = R.fp32_yardstick(z_np[t], coef32[t], d, 1.0, R.sep_chains(3, n), ref)
            R.check_entries(wst[t], ref[lz:], E[lz:], f"kmv_weights d={d} n={n} stamp={t}")
            ref_ds, tol_ds, e_row = R.ds_rows_tolerance(z_np[t][:, :d], tau, cfg, coef32[t], d)
            err = np.abs(ds[t] - ref_ds)
            print(f"max|err|/tol kmv_weights ds rows d={d} n={n} stamp={t} = {np.max(err / tol_ds):.3g}")
            assert np.all(err <= tol_ds), (d, n, t, np.max(err / tol_ds))
            outside, total = outside + int((err > R.FACTOR * e_row).sum()), total + err.size
    print(f"kmv_weights ds rows d={d}: {outside} of {total} outside {R.FACTOR:g} E_row")
    assert outside <= 0.05 * total, (d, outside, total)  # the literal per-row rule as a share (kmv_sums_ref docstring)


def test_kmv_weights_d9_unsupported(native):
    """The dispatch has no kmv_weights_kernel<9>: UNSUPPORTED, not a silent other path."""
    d, n = 9, 65
    coef = torch.zeros((1, native.kmv_ncoef(d)), device=DEV)
    with pytest.raises(NotImplementedError):
        native.kmv_weights(d, 1.0, coef, _t(R.states(n, 2 * d, 9)), 1, n, n * 2 * d, 2 * d)


@pytest.mark.parametrize("m", range(1, 17))  # moments_batched_kernel<m>
def test_moments_batched_vs_fp64(native, m):
    for n in R.SEP_ROWS:
        z_np = np.stack([R.states(n, m, 3000 * t + 10 * m + n) for t in range(3)])
        out = native.moments_batched(_t(z_np), 3, n, m, n * m, m).cpu().numpy()
        for t in range(3):
            ref = R.moment_terms(z_np[t].astype(np.float64)).sum(0)
            E = R.moments_yardstick(z_np[t], R.sep_chains(3, n), ref)
            assert out[t, 0] == n
            R.check_entries(out[t], ref, E, f"moments_batched m={m} n={n} set={t}")


# ---- d. kmv_terms_kernel / kmv_combine_kernel ----------------------------------------------------------------
_OUT = dict(loss=0, loss_gt=1, grad_norm=2, nabla=3, hess=4, value=5, true=6)  # include/pdeinv.h PDEINV_KFP_*


def _residual_inputs(d, counts=(300, 300, 300), seed=0):
    """Random fp64 samples per stamp, theta and tilde_F rounded to fp32 first; host sums in fp64."""
    rng = np.random.default_rng(500 + 10 * d + seed)
    F = nr.problem_constants(d).astype(F32).astype(np.float64)
    cfg = nr.ou_configuration(F)
    cfg["m_0"] = R.problem_cfg(d)["m_0"]
    K = rng.standard_normal((d, d)).astype(F32).astype(np.float64)
    b = rng.standard_normal(d).astype(F32).astype(np.float64)
    xs = [0.8 * rng.standard_normal((n, d)) + 0.25 for n in counts]
    vs = [rng.standard_normal((n, d)) for n in counts]
    tau = np.array(R.TAUS)
    sums = [R.host_sums(x[:, None], v[:, None], tau[t:t + 1], cfg, 1.0) for t, (x, v) in enumerate(zip(xs, vs))]
    mom, wst = np.concatenate([s[0] for s in sums]), np.concatenate([s[1] for s in sums])
    return dict(F=F, cfg=cfg, K=K, b=b, xs=xs, vs=vs, tau=tau, mom=mom, wst=wst, theta=np.concatenate([K.ravel(), b]))


def _run_residual(native, p, mom=None, wst=None):
    out, grad = native.residual_kmv(_t(p["mom"] if mom is None else mom, torch.float64),
                                    _t(p["wst"] if wst is None else wst, torch.float64), _t(p["theta"]), p["F"], 1.0)
    return out, grad


def _check_residual(out, grad, ref, mag, what):
    tol = R.residual_tolerance(ref, mag)
    out, grad = out.double().cpu().numpy(), grad.double().cpu().numpy()
    for k, idx in _OUT.items():
        err = abs(out[idx] - ref[k])
        print(f"residual_kmv {what} {k}: err / tol = {err / tol[k]:.3g}")
        assert err <= tol[k], (what, k, out[idx], ref[k], err, tol[k])
    err = np.abs(grad - ref["grad"])
    print(f"residual_kmv {what} grad: max err / tol = {np.max(err / tol['grad']):.3g}")
    assert np.all(err <= tol["grad"]), (what, np.flatnonzero(err > tol["grad"]), np.max(err / tol["grad"]))


@pytest.mark.parametrize("d", range(1, 9))  # kmv_terms_kernel / kmv_combine_kernel take d at run time: 1..8
def test_residual_kmv_vs_fp64(native, d):
    """loss, loss ground truth, the reported parts, every gradient entry and the gradient norm against
    nr.kmv_from_moments on the same samples: 2^-22 |ref| + 1e-12 S (kmv_sums_ref.residual_tolerance)."""
    p = _residual_inputs(d)
    x, v = np.stack(p["xs"], 1), np.stack(p["vs"], 1)  # [n = 300, n_t = 3, d]
    loss, gt, gK, gb = nr.kmv_from_moments(p["K"], p["b"], x, v, p["tau"], p["cfg"])
    ref = R.residual_ref(p["K"], p["b"], p["F"], p["mom"], p["wst"])  # the parts and the norm (pinned on the CPU)
    mag = R.residual_ref(p["K"], p["b"], p["F"], p["mom"], p["wst"], magnitude=True)
    assert abs(ref["loss"] - loss) <= 1e-12 * mag["loss"] and abs(ref["loss_gt"] - gt) <= 1e-12 * mag["loss_gt"]
    ref.update(loss=loss, loss_gt=gt, grad=np.concatenate([gK.ravel(), gb]))
    out, grad = _run_residual(native, p)
    _check_residual(out, grad, ref, mag, f"d={d}")
    assert out[7].item() == 0.0 and out[8].item() == 0.0


@pytest.mark.parametrize("d", [3, 8])
def test_residual_kmv_empty_set_changes_nothing(native, d):
    """An appended set with count 0 and zero sums leaves every output bit-equal."""
    p = _residual_inputs(d)
    out, grad = _run_residual(native, p)
    mom = np.concatenate([p["mom"], np.zeros((1, p["mom"].shape[1]))])
    wst = np.concatenate([p["wst"], np.zeros((1, p["wst"].shape[1]))])
    out2, grad2 = _run_residual(native, p, mom, wst)
    assert torch.equal(out, out2) and torch.equal(grad, grad2)


@pytest.mark.parametrize("d", [2, 8])
def test_residual_kmv_unequal_counts(native, d):
    """Sets of 300, 120 and 57 samples: every term is a mean over all 477 samples, so the result is the
    count-weighted mean of the three single-set computations (nr.kmv_from_moments on each set alone, fp64)."""
    counts = (300, 120, 57)
    p = _residual_inputs(d, counts, seed=1)
    N = float(sum(counts))
    loss = gt = 0.0
    grad = np.zeros(d * d + d)
    for t, n in enumerate(counts):
        l, g, gK, gb = nr.kmv_from_moments(p["K"], p["b"], p["xs"][t][:, None], p["vs"][t][:, None],
                                           p["tau"][t:t + 1], p["cfg"])
        loss, gt, grad = loss + n / N * l, gt + n / N * g, grad + n / N * np.concatenate([gK.ravel(), gb])
    ref = R.residual_ref(p["K"], p["b"], p["F"], p["mom"], p["wst"])
    mag = R.residual_ref(p["K"], p["b"], p["F"], p["mom"], p["wst"], magnitude=True)
    ref.update(loss=loss, loss_gt=gt, grad=grad, grad_norm=float(np.sqrt(np.sum(grad ** 2))))
    out, grad_gpu = _run_residual(native, p)
    _check_residual(out, grad_gpu, ref, mag, f"unequal counts d={d}")


# ---- e. end to end against the C oracle ----------------------------------------------------------------------
@pytest.mark.parametrize("d,N,n", [(8, 4099, 30), (2, 999, 10)])
def test_kmv_end_to_end_vs_c_oracle(native, oracle_lib, d, N, n):
    """simulate_mf_kmv (no trajectory written) + residual_kmv against the interacting C oracle's trajectory summed
    in fp64 (nr.kmv_from_moments), on the same Philox stream and stamps. A consistency check across the
    transcendental difference of the normals (tolerances of test_gpu_meanfield.py: loss 1e-4, gradient 1e-3, tau
    bit-equal); the tight checks are the tests above."""
    cfg = R.problem_cfg(d)
    A = cfg["tilde_F"]
    rng = np.random.default_rng(31 * d + N)
    z0 = R.states(N, 2 * d, 5 * d + N)
    o = oracle_lib.sde_simulate(z0, n, 0.02, 1.0, "meanfield", A, seed=0x5EED_0004, counter_offset=5)
    tau = o["tau"][:, 0].astype(np.float64)
    K, b = rng.standard_normal((d, d)).astype(F32), rng.standard_normal(d).astype(F32)
    x = o["traj"][:, :, :d].transpose(1, 0, 2).astype(np.float64)
    v = o["traj"][:, :, d:].transpose(1, 0, 2).astype(np.float64)
    loss, gt, gK, gb = nr.kmv_from_moments(K, b, x, v, tau, cfg)
    g_ref = np.concatenate([gK.ravel(), gb])

    z0_d = _t(z0)
    desc, keep = native.mf_desc(N, d, n, 0.02, 1.0, A, seed=0x5EED_0004, counter_offset=5)
    xbar, _ = native.mf_mean_path(desc, native.mf_sums(desc, z0_d), xsum=False)
    desc.d_meanfield = ctypes.c_void_p(xbar.data_ptr())
    _, coef = _coef(tau, cfg, d)
    tau_d = torch.empty((n, N), device=DEV)
    last = torch.empty((N, 2 * d), device=DEV)
    mom, wst = native.sde_simulate_mf_kmv(desc, z0_d, None, tau_d, last, 1.0, coef)
    assert np.array_equal(tau_d.cpu().numpy(), o["tau"])
    out, grad = native.residual_kmv(mom, wst, _t(np.concatenate([K.ravel(), b])), A, 1.0)
    out, grad = out.cpu().numpy(), grad.cpu().numpy()
    print(f"end to end d={d}: loss {out[0]} vs {loss}, loss_gt {out[1]} vs {gt}, "
          f"max grad err {np.max(np.abs(grad - g_ref)):.3g} of {np.abs(g_ref).max():.3g}")
    assert abs(out[0] - loss) < 1e-4 * (1 + abs(loss)), (out[0], loss)
    assert abs(out[1] - gt) < 1e-4 * (1 + abs(gt)), (out[1], gt)
    assert np.max(np.abs(grad - g_ref)) < 1e-3 * (1 + np.abs(g_ref).max())
    del keep

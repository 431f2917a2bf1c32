"""Shared helpers of the simulator-update tests (test_sde_step_ref.py on the CPU, test_gpu_sde_steps.py on the GPU):
one Euler-Maruyama update of sde_simulate_kernel / mf_step_kernel (csrc/sde.hip) against fp64, entry by entry.

Rule (teacher-forced, the technique of tests/mf_mlp_ref.py made per entry). Update s of particle i starts from the
GPU's own previous row, z_prev = z0[i] (s = 0) or traj[s-1, i], and must land on traj[s, i] (s < n_steps) or last[i]
(s = n_steps). The fp64 reference applies oracle.numpy_ref.update_step to z_prev widened to fp64 with the kernel's
own fp32 inputs widened: h = tau0, dt, ..., dt, then the fp32 difference dt - tau0; noise_scale, gamma, A, c, mu,
sigma; the force nr.grad_quadratic(A, c), nr.grad_gmm(mus, sigma), zero (POT_NONE) or A (q - xbar_s) (mean-field).
Rounding does not accumulate over steps, so the tolerance of entry (s, i, k) is a few ulp of its rounding scale,
    S_p = |p| + h S_g + sqrt(h) ns |xi| + gamma h |p| ,     S_q = |q| + h S_p ,
    quadratic / mean-field:  S_g = |A| |q| + |A| |c|   (covers A (q - c) and the kernel's A q - b, b = A c),
    GMM:  S_g = [sum_k w_k |q - mu_k| + L sum_k w_k |mu_k - mubar| + |q| + |mubar|] / sigma^2 ,
          L = max_k (|q . mu_k| + |mu_k|^2 / 2) / sigma^2   (the kernel's dot-product logits, gmm_grad in common.h),
namely  tol = FACTOR x e_rel x S.  e_rel is the largest |z32 - z64| / S over the case's rows, updates and fp32
variants, the variants being NumPy float32 restatements of the same update run on the case's inputs alone (no kernel
output enters the yardstick): two forms of the force ((q - c) A^T and q A^T - b with b rounded once from fp64; for the
GMM the direct logits -|q - mu|^2 / (2 sigma^2) with exp, and the kernel's l2s (q . mu_k) + c_k with exp2 and
(q - mubar) / sigma^2) times three associations of the p' sum. A per-entry E from a handful of evaluations would be
too noisy (tests/kmv_sums_ref.py says why); e_rel pooled over a case is the ds_rows_tolerance precedent of that module.

Philox mode: xi comes from the C oracle's stream, whose normals the kernels reproduce to 2e-6 (1 + |xi|) (the
documented tolerance of tests/test_gpu_kernels.py); sqrt(h) ns times that is added to the p' tolerance and h times
that to the q' tolerance.

test_sde_step_ref.py shows on the CPU that the tolerance is reachable (each variant's e_rel within FACTOR / 2 of the
others') and not vacuous (eleven wrong updates each exceed it).

Measured on the MI355X: max |err| / (e_rel S) per kernel family over every case and entry of test_gpu_sde_steps.py,
in MEASURED below (tolerance: FACTOR = 4). The largest is 1.35; no kernel came near the factor and none was changed.
"""
from collections import namedtuple

import numpy as np

import kmv_sums_ref as KR
from oracle import numpy_ref as nr

F32 = np.float32
FACTOR = 4.0      # tolerance = FACTOR x e_rel x S; at least twice the worst leave-one-out ratio (test_sde_step_ref.py)
NORMAL_TOL = 2e-6  # |GPU normal - oracle normal| <= NORMAL_TOL (1 + |xi|), tests/test_gpu_kernels.py
DT, GAMMA, N_STEPS, N_ROWS = 0.02, 0.5, 6, 321  # 321 rows: one full block, a wave of 64 and a wave of 1
DIMS = (1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 16)     # the compiled dimensions of sde_simulate_kernel and mf_step_kernel
MOM_DIMS = tuple(range(1, 9))                   # fused moments and the fused GMM residual: d <= 8
LOG2E = 1.4426950408889634

# max |err| / (e_rel S) per kernel family on the MI355X (tolerance: FACTOR)
MEASURED = {
    "sde_simulate_kernel quadratic / none": 1.34,          # d = 10 with a centre, random_shift = False
    "sde_simulate_kernel quadratic, fused moments": 1.35,  # d = 6, n_steps = 5
    "sde_simulate_kernel GMM KM=4": 1.00,                  # the same with fused moments: 1.05 (d = 4, K = 3)
    "sde_simulate_kernel GMM KM=8": 1.00,
    "sde_simulate_kernel GMM KM=16": 1.00,
    "sde_simulate_kernel GMM, fused residual": 1.00,
    "sde_simulate_kernel mean-field": 1.06,                # d = 7, random_shift = False
    "sde_simulate_kernel sizes (N = 1 ... 2853, n_steps = 1, 2, 6)": 1.18,  # GMM d = 3, N = 1, n_steps = 2
    "sde_simulate_kernel Philox (with the normals' allowance)": 0.79,       # quadratic d = 12, particle_offset = 0
    "mf_step_kernel": 0.99,
    # against kmv_sums_ref.FACTOR = 8, max |err| / E:
    "fused moments": 1.79,                                 # the 0T set, d = 7 quadratic, N = 2853
    "mf_step_kernel xsum": 0.74,
    "mf_sums_kernel": 1.08,                                # d = 5, N = 321
}

Case = namedtuple("Case", "pot d N n_steps ns K sigma centre seed")


def case(pot, d, N=N_ROWS, n_steps=N_STEPS, ns=nr.SQRT2, K=0, sigma=1.0, centre=False, seed=0):
    return Case(pot, d, N, n_steps, ns, K, sigma, centre, seed)


def case_id(c):
    s = f"{c.pot}-d{c.d}"
    if c.pot == "gmm":
        s += f"-K{c.K}" + (f"-s{c.sigma}" if c.sigma != 1.0 else "")
    if c.centre:
        s += "-centre"
    if c.ns != nr.SQRT2:
        s += f"-ns{c.ns}"
    if c.N != N_ROWS:
        s += f"-N{c.N}"
    if c.n_steps != N_STEPS:
        s += f"-n{c.n_steps}"
    return s


def gmm_km(K_):
    """The centre-slot count of the instantiation that simulates K centres (launch_gmm_sim, csrc/sde.hip)."""
    return 4 if K_ <= 4 else (8 if K_ <= 8 else 16)


# ---- the case lists -------------------------------------------------------------------------------------------
def explicit_cases(dims=DIMS, mean_field=True):
    """The explicit-noise matrix: every potential at every compiled d."""
    out = []
    for d in dims:
        out += [case("quadratic", d), case("quadratic", d, centre=True), case("none", d)]
        out += [case("gmm", d, K=k) for k in (3, 8, 16)] + [case("gmm", d, K=8, sigma=0.7)]
        if d in (3, 4):  # a full KM tile, a half-filled pair, and the first K of each KM
            out += [case("gmm", d, K=k) for k in (1, 4, 5, 9)]
        if mean_field:
            out.append(case("meanfield", d))
        if d == 6:  # noise_scale != sqrt(2), once per potential
            out += [case("quadratic", d, ns=0.9, centre=True), case("none", d, ns=0.9), case("gmm", d, K=3, ns=0.9)]
            if mean_field:
                out.append(case("meanfield", d, ns=0.9))
    return out


RES_K = ((3, 3), (3, 8), (8, 16))  # (K of the simulated GMM, K of the model) of pdeinv_sde_simulate_kfp_gmm


def res_cases():
    """(case, K_model): the fused-residual (RES) instantiations, model K d <= 64."""
    return [(case("gmm", d, K=kt), km) for d in MOM_DIMS for kt, km in RES_K if km * d <= 64]


SIZE_N = (1, 63, 64, 65, 255, 256, 257, 2853)  # 2853: 12 blocks, so xcd_block has q = 1 and r = 4
SIZE_STEPS = (1, 2, 6)
SIZE_DIMS = (3, 4, 8)


def size_cases():
    return [case(pot, d, N=n, K=k) for d in SIZE_DIMS for pot, k in (("quadratic", 0), ("gmm", 3)) for n in SIZE_N]


def philox_cases():
    return [case("quadratic", d) for d in (3, 5, 8, 12, 16)] + [case("gmm", d, K=8) for d in (3, 8)]


PHILOX_OFFSETS = (0, 5_000_000_000, (1 << 32) - 100)


# ---- a case's inputs ------------------------------------------------------------------------------------------
def inputs(c):
    """The fp32 inputs the kernel is given: z0 [N, 2d], xi [n+1, N, d], u [N], and per potential A [d, d], c [d],
    mus [K, d], xbar [n+1, d]. Explicit shift_u starts with 0, 2^-24 and 1 - 2^-24 (as many as N allows)."""
    d, N, n = c.d, c.N, c.n_steps
    rng = np.random.default_rng([c.seed, d, N, n, c.K, int(c.centre), len(c.pot)])
    inp = dict(A=None, c=None, mus=None, xbar=None)
    q0 = rng.standard_normal((N, d))
    p0 = rng.standard_normal((N, d))
    if c.pot in ("quadratic", "meanfield"):
        inp["A"] = nr.problem_constants(d).astype(F32)
    if c.centre:
        cc = rng.standard_normal(d)
        inp["c"] = cc.astype(F32)
        near = np.arange(N) % 4 == 1  # a quarter of the rows close to the centre: A q - b cancels there
        q0[near] = cc + 1e-3 * q0[near]
    if c.pot == "meanfield":
        inp["xbar"] = (0.5 * rng.standard_normal((n + 1, d))).astype(F32)
    if c.pot == "gmm":
        mus = nr.gmm_centres(d, c.K)
        inp["mus"] = mus.astype(F32)
        k0, k1 = np.arange(N) % c.K, (np.arange(N) + 1) % c.K
        kind = (np.arange(N) // c.K) % 4  # at a centre, midway between two, beyond one, anywhere
        q0 = np.where((kind == 0)[:, None], mus[k0] + 0.3 * q0,
                      np.where((kind == 1)[:, None], 0.5 * (mus[k0] + mus[k1]) + 0.3 * q0,
                               np.where((kind == 2)[:, None], 1.5 * mus[k0] + 0.3 * q0, 2.0 * q0)))
        p0 = 0.3 * p0
    inp["z0"] = np.concatenate([q0, p0], 1).astype(F32)
    inp["xi"] = rng.standard_normal((n + 1, N, d)).astype(F32)
    u = rng.random(N).astype(F32)
    special = [0.0, 2.0 ** -24, 1.0 - 2.0 ** -24]
    u[:min(N, 3)] = special[:min(N, 3)]
    if N >= 5:
        u[N - 1] = 0.0  # a row with h = 0 in the last (partial) wave too
    inp["u"] = u
    return inp


def tau0_of(u, dt=DT):
    """The kernel's tau0 = u * dt in fp32."""
    t = np.asarray(u, F32) * F32(dt)
    assert t.dtype == F32
    return t


def step_sizes(tau0, n_steps, dt=DT):
    """h [n+1, N] in fp32: tau0, dt, ..., dt, and the fp32 difference dt - tau0."""
    tau0 = np.asarray(tau0, F32)
    h = np.empty((n_steps + 1,) + tau0.shape, F32)
    h[0] = tau0
    h[1:n_steps] = F32(dt)
    h[n_steps] = F32(dt) - tau0
    return h


def tau_rows(tau0, n_steps, dt=DT):
    """tau [n, N] = tau0 + (float) s * dt, two fp32 roundings (tau_value, csrc/sde_common.h)."""
    s_dt = np.arange(n_steps, dtype=F32) * F32(dt)
    t = np.asarray(tau0, F32)[None, :] + s_dt[:, None]
    assert t.dtype == F32
    return t


# ---- the fp64 update ------------------------------------------------------------------------------------------
MUTATIONS = ("last_h_dt", "friction_new_p", "q_from_old_p", "xi_next", "noise_h", "no_centre", "no_inv_s2",
             "pad_slot", "xbar_next", "rows_swapped", "one_entry")


def mutations_of(c):
    """The wrong updates that apply to a case."""
    out = ["last_h_dt", "friction_new_p", "q_from_old_p", "xi_next", "noise_h", "rows_swapped", "one_entry"]
    if c.centre:
        out.append("no_centre")
    if c.pot == "gmm" and c.sigma != 1.0:
        out.append("no_inv_s2")
    if c.pot == "gmm" and c.K < gmm_km(c.K):
        out.append("pad_slot")
    if c.pot == "meanfield":
        out.append("xbar_next")
    return out


def _w(a):
    return None if a is None else np.asarray(a, F32).astype(np.float64)


def grad_fn64(c, inp, s, mutate=None):
    """The fp64 force of update s from the fp32 parameters widened."""
    if c.pot == "none":
        return lambda q: np.zeros_like(q)
    if c.pot == "quadratic":
        return nr.grad_quadratic(_w(inp["A"]), None if mutate == "no_centre" else _w(inp["c"]))
    if c.pot == "meanfield":
        row = (s + 1) % (c.n_steps + 1) if mutate == "xbar_next" else s
        return nr.grad_quadratic(_w(inp["A"]), _w(inp["xbar"][row]))
    mus, sigma = _w(inp["mus"]), float(F32(c.sigma))
    if mutate == "pad_slot":
        mus = np.concatenate([mus, np.zeros((1, c.d))])
    g = nr.grad_gmm(mus, sigma)
    return (lambda q: g(q) * sigma * sigma) if mutate == "no_inv_s2" else g


def update64(c, inp, z_prev, h, xi, s, mutate=None, xi_next=None):
    """z64 [N, 2d]: oracle.numpy_ref.update_step on the fp32 row z_prev widened (mutate: a wrong update)."""
    z_prev, h = np.asarray(z_prev), np.asarray(h)
    assert z_prev.dtype == F32 and h.dtype == F32 and np.asarray(xi).dtype == F32
    d = c.d
    q, p = z_prev[:, :d].astype(np.float64), z_prev[:, d:].astype(np.float64)
    h64 = h.astype(np.float64)[:, None]
    gamma, ns = float(F32(GAMMA)), float(F32(c.ns))
    x = (xi_next if mutate == "xi_next" else xi).astype(np.float64)
    if mutate == "last_h_dt" and s == c.n_steps:
        h64 = np.full_like(h64, float(F32(DT)))
    fn = grad_fn64(c, inp, s, mutate)
    if mutate == "friction_new_p":
        pt = p - h64 * fn(q) + np.sqrt(h64) * ns * x
        pn = pt - gamma * pt * h64
        qn = q + h64 * pn
    elif mutate == "noise_h":
        pn = p - h64 * fn(q) + h64 * ns * x - gamma * p * h64
        qn = q + h64 * pn
    else:
        qn, pn = nr.update_step(q, p, h64, fn, gamma, x, ns)
        if mutate == "q_from_old_p":
            qn = q + h64 * p
    z = np.concatenate([qn, pn], 1)
    if mutate == "rows_swapped" and s == min(1, c.n_steps) and len(z) > 1:
        z[[0, 1]] = z[[1, 0]]
    return z


def scale(c, inp, z_prev, h, xi, s):
    """S [N, 2d] = [S_q | S_p], the per-entry rounding scale of update s (module docstring)."""
    d = c.d
    z = np.asarray(z_prev, F32).astype(np.float64)
    q, p = z[:, :d], z[:, d:]
    h64 = np.asarray(h, F32).astype(np.float64)[:, None]
    gamma, ns = float(F32(GAMMA)), float(F32(c.ns))
    if c.pot == "none":
        Sg = np.zeros_like(q)
    elif c.pot in ("quadratic", "meanfield"):
        A = np.abs(_w(inp["A"]))
        cc = _w(inp["xbar"][s]) if c.pot == "meanfield" else _w(inp["c"])
        Sg = np.abs(q) @ A.T + (0.0 if cc is None else (A @ np.abs(cc))[None, :])
    else:
        mus, s2 = _w(inp["mus"]), float(F32(c.sigma)) ** 2
        diff = q[:, None, :] - mus[None]
        a = -np.sum(diff * diff, -1) / (2 * s2)
        e = np.exp(a - a.max(1, keepdims=True))
        w = e / e.sum(1, keepdims=True)
        mbar = w @ mus
        L = np.max(np.abs(q @ mus.T) + 0.5 * np.sum(mus * mus, 1)[None, :], 1) / s2
        Sg = (np.einsum("nk,nkd->nd", w, np.abs(diff))
              + L[:, None] * np.einsum("nk,nkd->nd", w, np.abs(mus[None] - mbar[:, None, :]))
              + np.abs(q) + np.abs(mbar)) / s2
    Sp = np.abs(p) + h64 * Sg + np.sqrt(h64) * ns * np.abs(np.asarray(xi, np.float64)) + gamma * h64 * np.abs(p)
    Sq = np.abs(q) + h64 * Sp
    return np.concatenate([Sq, Sp], 1)


# ---- the fp32 variants ----------------------------------------------------------------------------------------
def _matvec32(A, y, init=None):
    """sum_c A[r, c] y[:, c] added sequentially in fp32 from init (zero, or the kernel's -b)."""
    shape = (y.shape[0], A.shape[0])
    acc = np.zeros(shape, F32) if init is None else np.broadcast_to(init, shape).astype(F32)
    for j in range(A.shape[1]):
        acc = acc + y[:, j:j + 1] * A[None, :, j]
    assert acc.dtype == F32
    return acc


def forces32(c, inp, q, s):
    """The fp32 forms of the force at the fp32 positions q [N, d] (one form for POT_NONE, else two)."""
    if c.pot == "none":
        return [np.zeros_like(q)]
    if c.pot in ("quadratic", "meanfield"):
        A = inp["A"]
        cc = inp["xbar"][s] if c.pot == "meanfield" else inp["c"]
        if cc is None:
            return [_matvec32(A, q), (q @ A.T).astype(F32)]
        b = (A.astype(np.float64) @ cc.astype(np.float64)).astype(F32)  # b = A c in fp64, rounded once (build_args)
        return [_matvec32(A, q - cc[None, :]), _matvec32(A, q, -b[None, :])]
    mus, sig = inp["mus"], F32(c.sigma)
    s2 = sig * sig
    diff = q[:, None, :] - mus[None]
    a = -np.sum(diff * diff, -1) / (F32(2) * s2)
    e = np.exp(a - a.max(1, keepdims=True))
    w = e / e.sum(1, keepdims=True)
    direct = np.sum(w[..., None] * diff, 1) / s2
    l2s = F32(LOG2E / (float(sig) * float(sig)))
    inv_s2 = F32(1) / s2
    ck = (-0.5 * np.sum(mus.astype(np.float64) ** 2, 1) * (LOG2E / (float(sig) * float(sig)))).astype(F32)
    t = _matvec32(mus, q)                      # q . mu_k, one d-term chain per centre
    lg = t * l2s + ck[None, :]
    e2 = np.exp2(lg - lg.max(1, keepdims=True))
    inv = F32(1) / e2.sum(1, keepdims=True)
    acc = _matvec32(mus.T.copy(), e2)          # sum_k E_k mu_k
    dots = inv_s2 * (q - acc * inv)
    assert direct.dtype == F32 and dots.dtype == F32
    return [direct, dots]


def variants32(c, inp, z_prev, h, xi, s):
    """The fp32 restatements of update s: every force form x three associations of the p' sum; each [N, 2d]."""
    z_prev = np.asarray(z_prev)
    assert z_prev.dtype == F32
    d = c.d
    q, p = z_prev[:, :d], z_prev[:, d:]
    h = np.asarray(h, F32)[:, None]
    gamma, ns, one = F32(GAMMA), F32(c.ns), F32(1)
    xi = np.asarray(xi, F32)
    out = []
    for g in forces32(c, inp, q, s):
        sh = np.sqrt(h) * ns
        gh = gamma * h
        for assoc in range(3):
            if assoc == 0:    # the kernel's order, unfused
                pn = ((p - h * g) + sh * xi) - gh * p
            elif assoc == 1:  # update_step's order
                pn = ((p - h * g) + np.sqrt(h) * (ns * xi)) - (gamma * p) * h
            else:
                pn = p * (one - gh) + (sh * xi - h * g)
            z = np.concatenate([q + h * pn, pn], 1)
            assert z.dtype == F32
            out.append(z)
    return out


def variant_errors(c, inp, tau0, xi=None):
    """max |z32 - z64| / S per fp32 variant, over every update and row of the case's own float32 trajectory (variant
    0 carried forward from z0): what float32 arithmetic of this shape gets wrong on this data. No kernel output."""
    xi = inp["xi"] if xi is None else xi
    hs = step_sizes(tau0, c.n_steps)
    z = inp["z0"]
    errs = None
    for s in range(c.n_steps + 1):
        z64 = update64(c, inp, z, hs[s], xi[s], s)
        S = scale(c, inp, z, hs[s], xi[s], s)
        vs = variants32(c, inp, z, hs[s], xi[s], s)
        with np.errstate(divide="ignore", invalid="ignore"):
            e = np.array([np.max(np.where(v != z64, np.abs(v - z64) / S, 0.0)) for v in vs])
        errs = e if errs is None else np.maximum(errs, e)
        z = vs[0]
    return errs


def e_rel(c, inp, tau0, xi=None):
    return float(variant_errors(c, inp, tau0, xi).max())


# ---- the checker ----------------------------------------------------------------------------------------------
def normals_extra(c, h, xi):
    """The Philox-mode addition to the tolerance [N, 2d]: sqrt(h) ns 2e-6 (1 + |xi|) on p', h times that on q'."""
    h64 = np.asarray(h, F32).astype(np.float64)[:, None]
    ep = np.sqrt(h64) * float(F32(c.ns)) * NORMAL_TOL * (1 + np.abs(np.asarray(xi, np.float64)))
    return np.concatenate([h64 * ep, ep], 1)


def check_update(got, ref, S, erel, what, extra=None, factor=None):
    """|got - ref| <= FACTOR x e_rel x S (+ extra) per entry; names the worst entry; returns max |err| / (tol / FACTOR)
    (entries of zero tolerance must be exact)."""
    factor = FACTOR if factor is None else factor
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    unit = erel * S + (0.0 if extra is None else extra / factor)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err > 0, err / unit, 0.0)
    ratio = np.where(np.isfinite(got), ratio, np.inf)
    worst = float(ratio.max()) if ratio.size else 0.0
    if not worst <= factor:
        idx = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        raise AssertionError(f"{what}: entry {tuple(int(v) for v in idx)} off by {err[idx]:.3g} = {ratio[idx]:.3g} x "
                             f"e_rel S (got {got[idx]!r}, ref {ref[idx]!r}, S {S[idx]:.3g}, e_rel {erel:.3g}); "
                             f"{int((ratio > factor).sum())} of {ratio.size} entries beyond {factor}")
    return worst


def check_trajectory(c, inp, tau0, xi, traj, last, erel, what, philox=False):
    """Every update of a run, each from the run's own previous row: traj [n, N, 2d], last [N, 2d] (either may be None).
    Returns the largest |err| / (e_rel S) and prints it (pytest -s)."""
    hs = step_sizes(tau0, c.n_steps)
    worst = 0.0
    for s in range(c.n_steps + 1):
        got = last if s == c.n_steps else (None if traj is None else traj[s])
        if got is None or (s > 0 and traj is None):
            continue
        z_prev = inp["z0"] if s == 0 else traj[s - 1]
        ref = update64(c, inp, z_prev, hs[s], xi[s], s)
        S = scale(c, inp, z_prev, hs[s], xi[s], s)
        extra = normals_extra(c, hs[s], xi[s]) if philox else None
        worst = max(worst, check_update(got, ref, S, erel, f"{what} update s={s}, entry (i, k)", extra))
    print(f"max|err|/(e_rel S) {what} = {worst:.3g} (e_rel {erel:.3g})")
    return worst


# ---- column sums against fp64 (fused moments, mf_step's and mf_sums' partial sums) -----------------------------
def sums_yardstick(terms, chains, ref):
    """kmv_sums_ref.moments_yardstick for any per-row terms [n, L] (fp32): E[e] = max |chain sum - ref[e]| over
    N_ORDERS row orders."""
    t = np.asarray(terms)
    assert t.dtype == F32
    E = np.zeros(len(ref))
    for order in KR.row_orders(len(t)):
        E = np.maximum(E, np.abs(KR.chain_sum(t[order], chains) - ref))
    return E


def mom_chains(n_steps):
    """Chain lengths of the fused moment sets, read from sde_simulate_kernel (csrc/sde.hip): the 0T set adds a
    particle's n_steps rows in the lane's PairGram (acc.add per step), then block_reduce_to_slab's 64-lane wave_sum
    and its sum of the 4 waves (csrc/common.h), blocks in fp64 (slab_reduce_kernel); the initial and terminal sets
    add one row per lane (MomentAcc::add from zero), then the same wave and block sums."""
    return (n_steps, 64, 4), (64, 4)


MF_STEP_CHAINS = (64, 4)     # mf_step_kernel: v = [1, x] per lane, block_reduce_to_slab, blocks in fp64
MF_SUMS_CHAINS = (16, 64, 4)  # mf_sums_kernel: kMfSumsPerThread = 16 rows per lane, then the wave and the 4 waves

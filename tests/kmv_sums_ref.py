"""Shared helpers of the KMV stamp-sum tests (test_kmv_sums_ref.py on the CPU, test_gpu_kmv_sums.py on the GPU): the
fp64 reference of the per-time-stamp sums the quadratic-Phi McKean-Vlasov residual reads, the fp32 yardstick that
sets the per-entry tolerance, and the fp64 reference of the residual finalize.

Reference. stamp_terms gives, per row z = [x, v] of one stamp, the terms of
    mom = [count, sum z, sum z_i z_j (i <= j)]                    (moment_len(2d) entries, include/pdeinv.h order)
    wst = [sum w, sum w x, sum w x_i x_j (i <= j)]                (moment_len(d) entries)
with w = ds2 + ds^2 + gamma ds (kinetic_mckean_vlasov.py:86-91) and ds = d_s log rho, ds2 = d_s^2 log rho taken from
the closed form oracle.numpy_ref.partial_s_log_density / partial_s2_log_density, NOT from the coefficient table
dlogrho_coefficients the kernels are fed (test_kmv_sums_ref.py pins that table against the same closed form). The
rows are the fp32 data widened to fp64; the sums are the column sums.

Yardstick. fp32_yardstick evaluates the same sums in NumPy float32 as a kernel would (fp32 coefficients, r = m1 - x,
the two quadratic forms, the weight, the per-row products), adds the rows in fp32 along chains of the kernel's real
chain lengths and in fp64 across chains, in two associations of the weight (the full Gamma of kmv_weights_kernel and
the symmetrised upper triangle of kmv_moments_weights_kernel / sde_mf_kmv_kernel) and N_ORDERS row orders each.
E[e] = the largest |fp32 sum - fp64 sum| of entry e over these 2 x N_ORDERS evaluations: what fp32 arithmetic of this
shape gets wrong on this very data, coefficient rounding included. The tolerance of entry e is FACTOR x E[e]; the
factor covers what NumPy cannot reproduce (the MFMA's internal order, FMA contraction, the packed-pair Horner order of
the weight). The count entry is exact. test_kmv_sums_ref.py checks that this tolerance is neither vacuous (every
single dropped row and three wrong formulas exceed it) nor unreachable (a fresh row order stays within half of it).

Chain lengths (`chains`: run lengths from the innermost level outwards; each level adds runs of that many partial
sums of the level below sequentially in fp32 — sequential is the pessimistic model of a butterfly or of the MFMA's
internal tree — and what is left is added in fp64), read from the kernels:
  * sde_mf_kmv_kernel: (64, 4). One v_mfma_f32_16x16x4 chain over the wave's 64 staged rows per update, from zero
    accumulators (csrc/sde_kmv.hip:236-245; sum w is a 64-lane wave_sum, :216); the block then adds its 4 waves' tiles
    in fp32 (:253-265); the blocks are added in fp64 (slab_reduce_kernel, csrc/moments.hip:31-50).
  * kmv_moments_weights_kernel: (64 * trips, 4). The Gram accumulator g4, the lane-private zs and acc run across
    every row block the wave visits (csrc/kmv.hip:188-193, :236-262, the loops :293-313), trips = ceil(n_rows /
    (256 * batched_bx)) row blocks per wave (:17-23, :233-234), then the wave (wave_sum) and the 4 waves of the block
    (:318-335, block_reduce_to_slab, csrc/common.h:102-122): 64 * trips rows per wave in fp32, then 4 waves.
  * kmv_weights_kernel and moments_batched_kernel: (trips, 64, 4). The lane's grid-stride trips (csrc/kmv.hip:33-39,
    :67-94), then block_reduce_to_slab's wave_sum over 64 lanes and its sum of the 4 waves.

Per-row (ds, ds2) of kmv_weights (want_ds): the tolerance of row r is FACTOR x e_rel x S_r, S_r = |a| + sum |b_i r_i|
+ sum |G_ij r_i r_j| the row's rounding scale and e_rel the largest |fp32 - fp64| / S_r over the case's rows and the
two associations. Taken row by row, E_r = the emulation's own error of that row, two evaluations are too few: with
independent errors of one size, P(both |e| < |e_kernel| / 8) is about (2 phi(0) / 8)^2 E[e^2] / sigma^2 = 0.01, so about
one row in a hundred of a correct kernel exceeds 8 E_r, and where both evaluations happen to round exactly E_r is 0.
Measured on the MI355X: 271 of 21 252 row values (1.3 %) outside 8 E_r, the worst at 3.8e4 E_r, while the same values
sit at 0.23 of the scaled tolerance. The literal rule is therefore kept as a share: at most 5 % of a dimension's row
values may lie outside 8 E_r (a kernel whose per-row error is systematically beyond 8 x the emulation's puts most of
its rows there).

Row orders. N_ORDERS = 32, not the 8 first planned. The mom entries do not depend on the association, so
they see only N_ORDERS evaluations, and at N ~ 64 the largest of 8 left single entries of E below one ulp of the sum:
over 32 further orders a fresh one then reached 8 E on the CPU. With 32 orders the worst fresh order of 64 tried
stays below 3.7 E, and every condition of test_kmv_sums_ref.py still holds.

Measured on the MI355X: max |err| / E over every case and entry of test_gpu_kmv_sums.py, per kernel, in MEASURED
below. The factor in force is FACTOR = 8; no kernel came near it and none was changed.
"""
import numpy as np

from oracle import numpy_ref as nr

F32 = np.float32
FACTOR = 8.0     # tolerance = FACTOR x E (a fresh fp32 row order stays below half of it, test_kmv_sums_ref.py)
N_ORDERS = 32    # row orders per association: the identity and N_ORDERS - 1 seeded permutations
TAUS = (0.02, 0.37, 1.9)

# max |err| / E per kernel on the MI355X, over every case and entry of test_gpu_kmv_sums.py (tolerance: FACTOR)
MEASURED = {
    "sde_mf_kmv_kernel": 2.05,                       # d = 8, N = 64
    "kmv_moments_weights_kernel": 2.89,              # d = 7, n = 1, the same in all three row layouts
    "kmv_moments_weights_kernel, grid-capped": 1.69,  # d = 3, 3 trips per wave
    "kmv_weights_kernel": 2.02,                      # d = 5, n = 65
    "kmv_weights_kernel, ds rows / row tolerance": 0.23,  # d = 10, n = 65
    "moments_batched_kernel": 1.22,                  # m = 11, n = 65
    "residual_kmv / its tolerance": 0.24,            # d = 7, a gradient entry
}

MUTATIONS = ("upper_only", "x_for_r", "no_gamma")


def moment_len(m):
    return 1 + m + m * (m + 1) // 2


def problem_cfg(d, shifted=True):
    """The OU configuration of problem_constants(d). shifted: with a non-zero initial mean m_0 (the product's is 0,
    which makes m1 = 0 and beta = 0 at every stamp: the kernels' m1 - x and beta . r would then go unchecked)."""
    cfg = nr.ou_configuration(nr.problem_constants(d))
    if shifted:
        cfg["m_0"] = 0.3 * np.random.default_rng(1000 + d).standard_normal(2 * d)
    return cfg


def states(n, width, seed):
    """The test states 0.8 randn + 0.25, fp32."""
    return (0.8 * np.random.default_rng(seed).standard_normal((n, width)) + 0.25).astype(F32)


def coefficients(tau, cfg, d):
    """dlogrho_coefficients rows [len(tau), 3d + 2 + 2d^2] in fp64 (the host table behind every weight)."""
    from example_problems.kinetic_mckean_vlasov_example_quadratic import dlogrho_coefficients
    return dlogrho_coefficients(np.atleast_1d(np.asarray(tau, np.float64)), cfg, d)


def unpack_coef(c, d):
    """One coefficient row -> (m1, a1, beta1, G1, a2, beta2, G2) (include/pdeinv.h)."""
    c = np.asarray(c)
    o = 2 * d + 1 + d * d
    return (c[:d], c[d], c[d + 1:2 * d + 1], c[2 * d + 1:o].reshape(d, d),
            c[o], c[o + 1:o + 1 + d], c[o + 1 + d:o + 1 + d + d * d].reshape(d, d))


def moment_terms(z):
    """Per-row terms [n, moment_len(m)] of [count, sum z, sum z_i z_j (i <= j)], in the dtype of z."""
    n, m = z.shape
    iu = np.triu_indices(m)
    return np.concatenate([np.ones((n, 1), z.dtype), z, z[:, iu[0]] * z[:, iu[1]]], 1)


def weighted_terms(w, x):
    """Per-row terms [n, moment_len(d)] of [sum w, sum w x, sum w x_i x_j (i <= j)]: (w x_i) x_j as the kernels."""
    iu = np.triu_indices(x.shape[1])
    wx = w[:, None] * x
    return np.concatenate([w[:, None], wx, wx[:, iu[0]] * x[:, iu[1]]], 1)


def stamp_terms(z, tau, cfg, d, gamma):
    """fp64 per-row terms (mom_t [n, moment_len(2d)], wst_t [n, moment_len(d)]) of the fp32 rows z [n, 2d] at stamp
    tau; the stamp sums are the column sums."""
    z = np.asarray(z)
    assert z.dtype == F32 and z.ndim == 2 and z.shape[1] == 2 * d
    z64 = z.astype(np.float64)
    x = z64[:, :d]
    ds = nr.partial_s_log_density(tau, x, cfg)
    ds2 = nr.partial_s2_log_density(tau, x, cfg)
    w = ds2 + ds ** 2 + gamma * ds
    return moment_terms(z64), weighted_terms(w, x)


def stamp_sums(z, tau, cfg, d, gamma):
    """[mom | wst] fp64 sums of one stamp."""
    mom_t, wst_t = stamp_terms(z, tau, cfg, d, gamma)
    return np.concatenate([mom_t.sum(0), wst_t.sum(0)])


def quad32(x, coef32, d, assoc="full", mutate=None):
    """(ds, ds2) per row in float32 from the fp32 coefficient row: q = a + sum_i r_i (b_i + sum_j G_ij r_j), r = m1 - x.
    assoc "full": every G_ij (kmv_weights_kernel); "sym": j >= i over G_ij + G_ji (the fused kernels).
    mutate: None or one of MUTATIONS (wrong formulas the tolerance must reject)."""
    c = np.asarray(coef32)
    assert c.dtype == F32
    m1, a1, b1, G1, a2, b2, G2 = unpack_coef(c, d)
    x = np.asarray(x, F32)
    r = x if mutate == "x_for_r" else m1[None, :] - x
    out = []
    for a, b, G in ((a1, b1, G1), (a2, b2, G2)):
        if assoc == "sym":
            G = np.triu(G) if mutate == "upper_only" else (np.triu(G) + np.tril(G, -1).T).astype(F32)
        q = np.full(x.shape[0], a, F32)
        for i in range(d):
            g = np.full(x.shape[0], b[i], F32)
            for j in range(i if assoc == "sym" else 0, d):
                g = g + G[i, j] * r[:, j]
            q = q + g * r[:, i]
        assert q.dtype == F32
        out.append(q)
    return out[0], out[1]


def terms32(z, coef32, d, gamma, assoc="sym", mutate=None):
    """float32 per-row terms [n, moment_len(2d) + moment_len(d)] of [mom | wst]."""
    z = np.asarray(z)
    assert z.dtype == F32
    x = z[:, :d]
    q1, q2 = quad32(x, coef32, d, assoc, mutate)
    w = q2 + q1 * q1
    if mutate != "no_gamma":
        w = w + F32(gamma) * q1
    t = np.concatenate([moment_terms(z), weighted_terms(w, x)], 1)
    assert t.dtype == F32
    return t


def chain_sum(t, chains):
    """Column sums of the fp32 terms t [n, L]: runs of chains[0] rows added sequentially in fp32, then runs of
    chains[1] of those partial sums, ...; the rest in fp64."""
    a = np.asarray(t)
    assert a.dtype == F32
    for run in chains:
        n, L = a.shape
        k = -(-n // run)
        a = np.concatenate([a, np.zeros((k * run - n, L), F32)]).reshape(k, run, L)  # + 0 is exact
        acc = np.zeros((k, L), F32)
        for p in range(run):
            acc = acc + a[:, p]
        a = acc
    return a.astype(np.float64).sum(0)


def row_orders(n, first=0, count=N_ORDERS):
    """Row orders first .. first + count - 1 of n rows: order 0 is the identity, order k > 0 a seeded permutation."""
    return [np.arange(n) if k == 0 else np.random.default_rng(77_000 + k).permutation(n)
            for k in range(first, first + count)]


def fp32_yardstick(z, coef32, d, gamma, chains, ref, terms=terms32):
    """E[e] = max |fp32 sum - ref[e]| over the two associations x N_ORDERS row orders. ref: the fp64 sums."""
    E = np.zeros(len(ref))
    for assoc in ("full", "sym"):
        t = terms(z, coef32, d, gamma, assoc)
        for order in row_orders(len(t)):
            E = np.maximum(E, np.abs(chain_sum(t[order], chains) - ref))
    return E


def moments_yardstick(z, chains, ref):
    """fp32_yardstick for the plain moments of rows of any width (moments_batched_kernel): no weight, so one
    association; N_ORDERS row orders."""
    t = moment_terms(np.asarray(z, F32))
    E = np.zeros(len(ref))
    for order in row_orders(len(t)):
        E = np.maximum(E, np.abs(chain_sum(t[order], chains) - ref))
    return E


def check_entries(got, ref, E, what=""):
    """|got - ref| <= FACTOR x E per entry; returns max |err| / E (entries with E = 0 must be exact)."""
    got, ref, E = (np.asarray(a, np.float64) for a in (got, ref, E))
    err = np.abs(got - ref)
    bad = np.flatnonzero(err > FACTOR * E)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err > 0, err / E, 0.0)
    worst = float(ratio.max()) if ratio.size else 0.0
    print(f"max|err|/E {what} = {worst:.3g}")  # the figure before the assertion (pytest -s)
    assert bad.size == 0, (f"{what}: entries {bad[:8].tolist()} of {len(ref)} off by {err[bad][:8].tolist()} "
                           f"(E {E[bad][:8].tolist()}, ref {ref[bad][:8].tolist()}), max err / E = {worst:.3g}")
    return worst


# ---- the kernels' grids: chain lengths per case --------------------------------------------------------------
SIM_CHAINS = (64, 4)
SIM_CASES = [(D, N) for D in (2, 4, 6, 8) for N in (1, 63, 64, 65, 255, 257)] + [(8, 4099), (4, 4099)]
MW_ROWS = (1, 63, 65, 257)
MW_CAPPED = dict(dims=(8, 3), n_sets=512, n_rows=6100)  # batched_bx = 8 blocks: 3 trips per wave, the last partial
SEP_ROWS = (65, 257)
WEIGHT_DIMS = (1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 16)


def batched_bx(n_sets, n_rows):
    """csrc/kmv.hip:15-23 (kBatchedGridTarget = 4096, 256 rows per block)."""
    bx = min(-(-4096 // n_sets), -(-n_rows // 256))
    return max(bx, 1)


def batched_trips(n_sets, n_rows):
    """Row blocks per wave (= grid-stride trips per lane) of the batched kernels: the most any wave makes."""
    return max(1, -(-n_rows // (256 * batched_bx(n_sets, n_rows))))


def mw_chains(n_sets, n_rows):
    return (64 * batched_trips(n_sets, n_rows), 4)


def sep_chains(n_sets, n_rows):
    return (batched_trips(n_sets, n_rows), 64, 4)


# ---- per-row ds, ds2 (kmv_weights want_ds) -------------------------------------------------------------------
def ds_rows_tolerance(x, tau, cfg, coef32, d):
    """((ds, ds2) fp64 closed form [n, 2], tolerance [n, 2], E_row [n, 2]) of the rows x [n, d] (fp32); E_row is the
    emulation's own error of that very row over the two associations. See the module docstring."""
    x = np.asarray(x)
    assert x.dtype == F32
    x64 = x.astype(np.float64)
    ref = np.stack([nr.partial_s_log_density(tau, x64, cfg), nr.partial_s2_log_density(tau, x64, cfg)], 1)
    m1, a1, b1, G1, a2, b2, G2 = (np.asarray(v, np.float64) for v in unpack_coef(coef32, d))
    r = np.abs(m1[None] - x64)
    scale = np.stack([abs(a) + r @ np.abs(b) + np.einsum("ni,ij,nj->n", r, np.abs(G), r)
                      for a, b, G in ((a1, b1, G1), (a2, b2, G2))], 1)
    e_rel, e_row = np.zeros(2), np.zeros_like(ref)
    for assoc in ("full", "sym"):
        q = np.stack(quad32(x, coef32, d, assoc), 1).astype(np.float64)
        e_row = np.maximum(e_row, np.abs(q - ref))
        e_rel = np.maximum(e_rel, (e_row / scale).max(0))
    return ref, FACTOR * e_rel[None, :] * scale, e_row


# ---- the residual finalize (kmv_terms_kernel / kmv_combine_kernel) ---------------------------------------------
def residual_ref(K, b, F, mom, wst, magnitude=False):
    """kmv.hip's finalize from the per-stamp sums mom [n_t, moment_len(2d)], wst [n_t, moment_len(d)] in fp64, any
    counts per stamp: dict(loss, loss_gt, nabla, hess, value, true, grad [d*d + d], grad_norm).
    magnitude=True: the same polynomial with every input replaced by its absolute value and every minus by a plus,
    i.e. per output the sum S of the absolute values of the terms that make it up (the cancellation scale)."""
    K, b, F, mom, wst = (np.asarray(a, np.float64) for a in (K, b, F, mom, wst))
    if magnitude:
        K, b, F, mom, wst = (np.abs(a) for a in (K, b, F, mom, wst))
    sg = 1.0 if magnitude else -1.0
    d = len(b)
    S = K + K.T
    D = F + sg * S
    cnt = mom[:, 0]
    N = cnt.sum()
    nabla = value = true = gt = 0.0
    G = np.zeros((d, d))
    gb = 2 * b.copy()
    Svv = np.zeros((d, d))
    iu = np.triu_indices(d)
    for t in range(len(cnt)):
        if cnt[t] == 0:
            continue
        _, mean, M2 = nr.unpack_moments(mom[t], 2 * d)
        xbar, M = mean[:d], M2[:d, :d]
        Svv += M2[d:, d:] * cnt[t]
        C = M + sg * np.outer(xbar, xbar)
        W, Wx = wst[t, 0], wst[t, 1:1 + d]
        Wxx = np.zeros((d, d))
        Wxx[iu] = wst[t, 1 + d:]
        Wxx = Wxx + Wxx.T - np.diag(np.diag(Wxx))
        w = cnt[t] / N
        nabla += w * np.trace(S @ C @ S)
        true += w * np.trace(F @ C @ F.T)
        gt += w * np.trace(D @ C @ D.T)
        value += (0.5 * np.trace(S @ Wxx) + sg * (xbar @ S @ Wx) + 0.5 * W * np.trace(S @ M)
                  + b @ (Wx + sg * W * xbar)) / N
        G += w * (S @ C + C @ S) + 2 * (0.5 * Wxx + sg * np.outer(xbar, Wx) + 0.5 * W * M) / N
        gb += 2 * (Wx + sg * W * xbar) / N
    Mvv = Svv / N
    nabla += b @ b
    gt += b @ b
    hess = np.trace(S @ Mvv)
    G = G + sg * 2 * Mvv
    grad = np.concatenate([(G + G.T).ravel(), gb])
    loss = nabla + sg * 2 * hess + 2 * value + true
    return dict(loss=loss, loss_gt=gt, nabla=nabla, hess=hess, value=value, true=true, grad=grad,
                grad_norm=float(np.sqrt(np.sum(grad ** 2))))


def host_sums(x, v, tau, cfg, gamma):
    """fp64 (mom [n_t, ...], wst [n_t, ...]) of fp64 samples x, v [n, n_t, d] from the closed form."""
    n, n_t, d = x.shape
    mom, wst = [], []
    for t in range(n_t):
        xt = x[:, t]
        ds = nr.partial_s_log_density(tau[t], xt, cfg)
        ds2 = nr.partial_s2_log_density(tau[t], xt, cfg)
        mom.append(nr.moments(np.concatenate([xt, v[:, t]], 1)))
        wst.append(weighted_terms(ds2 + ds ** 2 + gamma * ds, xt).sum(0))
    return np.stack(mom), np.stack(wst)


def residual_tolerance(ref, mag):
    """2^-22 |ref| + 1e-12 S per output: one fp32 rounding of an fp64 result (2^-24; a factor 4 is kept
    although theta and tilde_F are rounded to fp32 before the reference sees them) plus fp64 cancellation."""
    return {k: 2.0 ** -22 * np.abs(ref[k]) + 1e-12 * np.asarray(mag[k]) for k in ref}

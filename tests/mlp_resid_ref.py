"""Shared helpers of the V_hypothesis residual tests (test_mlp_resid_ref.py on the CPU, test_gpu_mlp_resid.py on the
GPU): the fp64 reference of pdeinv_residual_kfp_mlp's gradient and accumulator slots, the fp32 restatement that sets
the tolerance per parameter block and per slot, and the mutations that show the tolerance is not vacuous.

Reference. oracle.numpy_ref.mlp_grad_rows(params, Z, C) in fp64 on the stacked rows Z = [0T | initial | terminal]
with per-row weights C = [c1, c2, c3, c0] built from the very coefficients the call passes (rounded to fp32 as the
descriptor carries them, then widened); the per-row terms V, V', V'', g of the slots from
oracle.numpy_ref.mlp_forward_terms. Nothing comes from the library path or from any kernel.

fp32 restatement. grad_rows below restates mlp_grad_rows operation for operation (test_mlp_resid_ref.py pins it to
mlp_grad_rows: to fp64 rounding in fp64, bit for bit in fp32 with np.tanh) with the activation as a parameter, the
per-row terms as a second result and the mutations as switches. It is evaluated with every array in float32
  * with np.tanh and with the kernels' own formula 1 - 2 / (exp2(2.88539008 z) + 1) (mlp_fused.hip ftanh),
  * over n_orders orders (4; 2 in the wrapped-grid cases). Order 0 is the data as given; order k > 0 permutes the rows
    AND the units of every layer (columns of K_l, b_l, rows of K_l+1: the same function, the dot products of a row
    summed in another order), so that the per-row numbers of a set of one or fifteen rows get independent roundings
    too — a row permutation alone leaves them as they are.
E_block[K_l | b_l] = the largest |fp32 - fp64| over these evaluations and the block's entries; E_slot[s] the same per
accumulator slot (PDEINV_GMM_ACC_*), with the per-row slot terms added as mlp.hip's mlp_loss adds them: per set, a
thread's grid-stride rows, the wave's 64 lanes and the block's 4 waves in fp32 (kmv_sums_ref.chain_sum), blocks and
sets in fp64.

Rule. Every entry of a block: |gpu - fp64| <= RULE x E_block, every slot: |gpu - fp64| <= RULE x E_slot, RULE =
mlp_sim_ref.RULE = 16 — the project's margin for the hardware exp2 / rcp tanh and another summation order. No
entry is exempt; an entry whose E is 0 must be exact.

Measured on the MI355X over every case of test_gpu_mlp_resid.py: the fused kernels reach 1.62 E in the gradient and
5.56 E in a slot, the rocBLAS path 2.44 E and 2.56 E, the row engine's per-row V and grad V 1.87 and 1.67 (DESIGN.md
§3.1 lists them per kernel family). No chain had to be added to the restatement and no kernel was changed.
"""
import numpy as np

import kmv_sums_ref as KS
import mlp_sim_ref as MS
from oracle import numpy_ref as nr

RULE = MS.RULE
F32 = np.float32
N_ORDERS = 4
SLOTS = ("loss", "loss_gt", "nabla", "hessian", "friction", "nabla_true", "initial", "terminal")
COEF_KEYS = ("c_nabla", "c_hess", "c_fric", "c_true", "c_init", "c_term")
MUTATIONS = ("s2_sign", "no_s3", "no_abar_zeta", "bias_short")
LOSS_GRID, LOSS_BLOCK = 512, 256  # csrc/mlp_engine.h kLossGrid, csrc/common.h kBlock


def tanh_exp2(z):
    """mlp_fused.hip's ftanh in the dtype of z."""
    f = z.dtype.type
    with np.errstate(over="ignore"):
        e = np.exp2(f(2.8853900817779268) * z)
    return f(1) - f(2) / (e + f(1))


def make_params(dims, seed):
    """[(K, b), ...] fp64 holding fp32 values: kernels N(0, 1 / fan_in), biases 0.1 N(0, 1)."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(len(dims) - 1):
        K = rng.standard_normal((dims[i], dims[i + 1])) * np.sqrt(1.0 / dims[i])
        b = 0.1 * rng.standard_normal(dims[i + 1])
        out.append((K.astype(F32).astype(np.float64), b.astype(F32).astype(np.float64)))
    return out


def make_rows(d, n, seed):
    return np.random.default_rng(seed).standard_normal((n, 2 * d)).astype(F32)


def block_slices(dims):
    """[(name, slice into the flat flax vector)] : K1, b1, ..., Ko, bo."""
    out, o = [], 0
    L = len(dims) - 2
    for i in range(len(dims) - 1):
        tag = "o" if i == L else str(i + 1)
        nK, nb = dims[i] * dims[i + 1], dims[i + 1]
        out.append(("K" + tag, slice(o, o + nK)))
        out.append(("b" + tag, slice(o + nK, o + nK + nb)))
        o += nK + nb
    return out


def coefficients(n0, ni, nt, gamma, total_time, **override):
    """The reference's loss weights (kinetic_fokker_planck.py:33-50) or the overrides, rounded to fp32 as the
    descriptor carries them. Pass the result as native.residual_kfp_mlp(coefficients=...)."""
    c = dict(c_nabla=1.0 / n0, c_hess=-2.0 / n0, c_fric=2.0 * gamma / n0, c_true=1.0 / n0,
             c_init=(-2.0 / (total_time * ni)) if ni else 0.0, c_term=(2.0 / (total_time * nt)) if nt else 0.0)
    assert set(override) <= set(COEF_KEYS)
    c.update(override)
    return {k: float(F32(v)) for k, v in c.items()}


def only(name, n0, ni, nt, gamma, total_time):
    """coefficients() with every weight but `name` zero."""
    c = coefficients(n0, ni, nt, gamma, total_time)
    return {k: (v if k == name else 0.0) for k, v in c.items()}


def row_weights(coef, n0, ni, nt, boundary_value=False, swap_boundary=False):
    """C [n0 + ni + nt, 4] = [c1, c2, c3, c0] per row of [0T | initial | terminal].
    swap_boundary: c_init on the terminal rows and c_term on the initial ones (a mutation)."""
    ci, ct = (coef["c_term"], coef["c_init"]) if swap_boundary else (coef["c_init"], coef["c_term"])
    col = 3 if boundary_value else 2
    C = np.zeros((n0 + ni + nt, 4))
    C[:n0, :3] = coef["c_nabla"], coef["c_hess"], coef["c_fric"]
    C[n0:n0 + ni, col] = ci
    C[n0 + ni:, col] = ct
    return C


def grad_rows(params, Z, C, tanh=np.tanh, mutate=None):
    """oracle.numpy_ref.mlp_grad_rows (U = None) in the dtype of its arguments, operation for operation, with the
    activation as a parameter. Returns (grads [(gK, gb), ...], terms dict(V, Vd, Vdd, g) per row).
    mutate: None or one of MUTATIONS — s2 with the wrong sign, the s3 zd^2 term left out, the abar^T zeta pair left
    out of every kernel gradient, the bias gradients short of the last row."""
    assert mutate is None or mutate in MUTATIONS
    d = params[0][0].shape[0]
    L = len(params) - 1
    c1, c2, c3, c0 = C[:, :1], C[:, 1:2], C[:, 2:3], C[:, 3:4]
    x, v = Z[:, :d], Z[:, d:]
    A = [(x, v, np.zeros_like(x))]
    Zs, S = [], []
    for K, b in params[:-1]:
        h, hd, hdd = A[-1]
        z, zd, zdd = h @ K + b, hd @ K, hdd @ K
        hn = tanh(z)
        s1 = 1 - hn * hn
        s2 = -2 * hn * s1
        s3 = -2 * s1 * s1 - 2 * hn * s2
        if mutate == "s2_sign":
            s2 = -s2
        if mutate == "no_s3":
            s3 = np.zeros_like(s3)
        A.append((hn, s1 * zd, s1 * zdd + s2 * zd * zd))
        Zs.append((zd, zdd))
        S.append((s1, s2, s3))
    Ko, bo = params[-1]
    hL, hdL, hddL = A[-1]
    y, yd, ydd = hL @ Ko + bo, hdL @ Ko, hddL @ Ko
    u = 2 * y
    a_l = [None] * (L + 1)
    zeta = [None] * (L + 1)
    a = u @ Ko.T
    for l in range(L, 0, -1):
        a_l[l] = a
        zeta[l] = S[l - 1][0] * a
        a = zeta[l] @ params[l - 1][0].T
    g = a
    abar = [None] * (L + 1)
    zetabar = [None] * (L + 1)
    abar[0] = 2 * c1 * g + 0.0
    for l in range(1, L + 1):
        zetabar[l] = abar[l - 1] @ params[l - 1][0]
        abar[l] = S[l - 1][0] * zetabar[l]
    ubar = abar[L] @ Ko
    ybar = 2 * c3 * yd + 2 * c2 * ydd + 2 * ubar + 2 * c0 * y
    ydbar = 2 * c3 * y + 4 * c2 * yd
    yddbar = 2 * c2 * y
    pair = mutate != "no_abar_zeta"
    cut = slice(None, -1) if mutate == "bias_short" else slice(None)
    grads = [None] * (L + 1)
    gKo = hL.T @ ybar + hdL.T @ ydbar + hddL.T @ yddbar + (abar[L].T @ u if pair else 0)
    grads[L] = (gKo, ybar[cut].sum(0))
    hb, hdb, hddb = ybar @ Ko.T, ydbar @ Ko.T, yddbar @ Ko.T
    for l in range(L, 0, -1):
        s1, s2, s3 = S[l - 1]
        zd, zdd = Zs[l - 1]
        zb = s1 * hb + s2 * zd * hdb + (s2 * zdd + s3 * zd * zd) * hddb + s2 * a_l[l] * zetabar[l]
        zdb = s1 * hdb + 2 * s2 * zd * hddb
        zddb = s1 * hddb
        hp, hdp, hddp = A[l - 1]
        K = params[l - 1][0]
        gK = hp.T @ zb + hdp.T @ zdb + hddp.T @ zddb + (abar[l - 1].T @ zeta[l] if pair else 0)
        grads[l - 1] = (gK, zb[cut].sum(0))
        hb, hdb, hddb = zb @ K.T, zdb @ K.T, zddb @ K.T
    dt = Z.dtype
    V = np.sum(y * y, -1, dtype=dt)
    Vd = 2 * np.sum(y * yd, -1, dtype=dt)
    Vdd = 2 * np.sum(yd * yd + y * ydd, -1, dtype=dt)
    return grads, dict(V=V, Vd=Vd, Vdd=Vdd, g=g)


def unit_orders(dims, k):
    """Order k of the units of every layer past the input: identity for k = 0, else seeded permutations."""
    if k == 0:
        return [np.arange(n) for n in dims[1:]]
    rng = np.random.default_rng(88_000 + k)
    return [rng.permutation(n) for n in dims[1:]]


def permute_units(params, perms):
    """The same function with the units of layer l renumbered by perms[l] (layer 0 = the first hidden layer)."""
    out, prev = [], None
    for (K, b), p in zip(params, perms):
        K = K if prev is None else K[prev]
        out.append((np.ascontiguousarray(K[:, p]), np.ascontiguousarray(b[p])))
        prev = p
    return out


def unpermute_grads(grads, perms):
    out, prev = [], None
    for (gK, gb), p in zip(grads, perms):
        K = np.empty_like(gK)
        rows = np.arange(gK.shape[0]) if prev is None else prev
        K[np.ix_(rows, p)] = gK
        b = np.empty_like(gb)
        b[p] = gb
        out.append((K, b))
        prev = p
    return out


def true_grad(true, x):
    """grad V*(x) in the dtype of x. true = ("quad", F) or ("gmm", mus)."""
    kind, tp = true
    tp = np.asarray(tp).astype(x.dtype)
    if kind == "quad":
        return x @ tp.T
    return nr.gmm_value_grad(x, tp, 1.0)[1].astype(x.dtype)


def slot_terms(set_id, terms, x, coef, true, n_set, boundary_value):
    """Per-row contributions [n, 8] to the PDEINV_GMM_ACC_* slots (csrc/mlp.hip mlp_loss), in the dtype of x."""
    dt = x.dtype
    f = dt.type
    T1 = np.sum(terms["g"] * terms["g"], -1, dtype=dt)
    T2, T3, T0 = terms["Vdd"], terms["Vd"], terms["V"]
    out = np.zeros((len(x), 8), dt)
    if set_id == 0:
        gt = true_grad(true, x)
        Tt = np.sum(gt * gt, -1, dtype=dt)
        dg = gt - terms["g"]
        Tgt = np.sum(dg * dg, -1, dtype=dt)
        ct = f(coef["c_true"])
        out[:, 0] = f(coef["c_nabla"]) * T1 + f(coef["c_hess"]) * T2 + f(coef["c_fric"]) * T3 + ct * Tt
        out[:, 1], out[:, 2], out[:, 3], out[:, 4], out[:, 5] = ct * Tgt, ct * T1, ct * T2, ct * T3, ct * Tt
    else:
        b = T0 if boundary_value else T3
        out[:, 0] = f(coef["c_init" if set_id == 1 else "c_term"]) * b
        inv_n = 1.0 / n_set if dt == np.float64 else f(1) / f(n_set)
        out[:, 5 + set_id] = inv_n * b
    assert out.dtype == dt
    return out


def _cast(params, dt):
    return [(K.astype(dt), b.astype(dt)) for K, b in params]


class Case:
    """One residual call: its fp64 reference and its tolerances.
    sets = (z_0T, z_init, z_term) fp32 rows [n, 2d]; coef from coefficients() / only(); true = ("quad", F) |
    ("gmm", mus) with fp32-representable entries."""

    def __init__(self, dims, params, sets, coef, true, boundary_value=False, n_orders=N_ORDERS):
        self.dims, self.params, self.coef, self.true, self.bval = list(dims), params, coef, true, boundary_value
        self.sets = [np.asarray(z) for z in sets]
        assert all(z.dtype == F32 and z.ndim == 2 and z.shape[1] == 2 * dims[0] for z in self.sets)
        self.n = [len(z) for z in self.sets]
        assert self.n[0] >= 1
        self.blocks = block_slices(self.dims)
        self.Z = np.concatenate(self.sets).astype(np.float64)
        self.C = row_weights(coef, *self.n, boundary_value)
        self.ref_grad = nr.mlp_flat(nr.mlp_grad_rows(params, self.Z, self.C))
        self.ref_acc = self._slots64()
        self.E_flat = np.zeros_like(self.ref_grad)
        self.E_slot = np.zeros(8)
        for k in range(n_orders):
            for tanh in (np.tanh, tanh_exp2):
                g32, a32 = self.eval32(k, tanh)
                self.E_flat = np.maximum(self.E_flat, np.abs(g32 - self.ref_grad))
                self.E_slot = np.maximum(self.E_slot, np.abs(a32 - self.ref_acc))
        self.E_block = {name: float(self.E_flat[s].max()) for name, s in self.blocks}

    def _bounds(self):
        o = np.cumsum([0] + self.n)
        return [(int(o[i]), int(o[i + 1])) for i in range(3)]

    def _slots64(self):
        d = self.dims[0]
        acc = np.zeros(8)
        for sid, z in enumerate(self.sets):
            if len(z):
                z64 = z.astype(np.float64)
                V, g, Vd, Vdd = nr.mlp_forward_terms(self.params, z64[:, :d], z64[:, d:])
                t = slot_terms(sid, dict(V=V, g=g, Vd=Vd, Vdd=Vdd), z64[:, :d], self.coef, self.true, len(z), self.bval)
                acc += t.sum(0)
        return acc

    def eval32(self, k, tanh, mutate=None):
        """(flat gradient, slots) of evaluation k of the fp32 restatement, as fp64 arrays."""
        d = self.dims[0]
        perms = unit_orders(self.dims, k)
        p32 = _cast(permute_units(self.params, perms), F32)
        rows = KS.row_orders(len(self.Z), first=k, count=1)[0]
        inv = np.empty_like(rows)
        inv[rows] = np.arange(len(rows))
        Z32, C32 = self.Z.astype(F32)[rows], self.C.astype(F32)[rows]
        grads, terms = grad_rows(p32, Z32, C32, tanh, mutate)
        assert all(gK.dtype == F32 and gb.dtype == F32 for gK, gb in grads)
        flat = nr.mlp_flat(unpermute_grads(grads, perms)).astype(np.float64)
        terms = {key: v[inv] for key, v in terms.items()}  # back to the sets' own order: the kernel sums set by set
        acc = np.zeros(8)
        for sid, (lo, hi) in enumerate(self._bounds()):
            if hi > lo:
                order = KS.row_orders(hi - lo, first=k, count=1)[0]
                t = slot_terms(sid, {key: v[lo:hi] for key, v in terms.items()}, self.sets[sid][:, :d], self.coef,
                               self.true, hi - lo, self.bval)
                trips = -(-(hi - lo) // (LOSS_GRID * LOSS_BLOCK))
                acc += KS.chain_sum(t[order], (trips, 64, 4))
        return flat, acc

    def mutated64(self, mutate):
        """The fp64 gradient of a wrong formula (MUTATIONS), of a dropped last row ("drop0" / "drop1" / "drop2": the
        0T / initial / terminal set; the weights keep the full counts, as a kernel that masks one row too many
        would) or of c_init and c_term swapped ("swap_boundary")."""
        if mutate in MUTATIONS:
            return nr.mlp_flat(grad_rows(self.params, self.Z, self.C, np.tanh, mutate)[0])
        if mutate == "swap_boundary":
            return nr.mlp_flat(nr.mlp_grad_rows(self.params, self.Z, row_weights(self.coef, *self.n, self.bval, True)))
        assert mutate in ("drop0", "drop1", "drop2")
        lo, hi = self._bounds()[int(mutate[-1])]
        assert hi > lo
        keep = np.delete(np.arange(len(self.Z)), hi - 1)
        return nr.mlp_flat(nr.mlp_grad_rows(self.params, self.Z[keep], self.C[keep]))

    def block_ratios(self, flat):
        """{block: max |flat - fp64| / E_block}; inf where an entry differs and E_block is 0."""
        out = {}
        for name, s in self.blocks:
            err = float(np.max(np.abs(np.asarray(flat, np.float64)[s] - self.ref_grad[s])))
            E = self.E_block[name]
            out[name] = 0.0 if err == 0 else (err / E if E > 0 else np.inf)
        return out

    def slot_ratios(self, acc):
        err = np.abs(np.asarray(acc, np.float64) - self.ref_acc)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(err > 0, err / self.E_slot, 0.0)

    def check(self, what, grad, acc):
        """The rule on every entry of every block and on every slot; prints the figures first (pytest -s).
        Returns (max block ratio, max slot ratio)."""
        grad = np.asarray(grad, np.float64)
        assert grad.shape == self.ref_grad.shape and np.all(np.isfinite(grad)), what
        rb = self.block_ratios(grad)
        rs = self.slot_ratios(acc)
        wb, ws = max(rb.values()), float(rs.max())
        print(f"max|err|/E {what} n={self.n}: grad {wb:.3g} ({max(rb, key=rb.get)}) slots {ws:.3g} "
              f"({SLOTS[int(rs.argmax())]})")
        for name, s in self.blocks:  # entry by entry
            bad = np.flatnonzero(np.abs(grad[s] - self.ref_grad[s]) > RULE * self.E_block[name])
            assert bad.size == 0, (f"{what} n={self.n}: block {name}, {bad.size} of {s.stop - s.start} entries past "
                                   f"{RULE:g} E (E = {self.E_block[name]:.3g}), ratio {rb[name]:.3g}, "
                                   f"first at {bad[:4].tolist()}")
        bad = np.flatnonzero(rs > RULE)
        assert bad.size == 0, (f"{what} n={self.n}: slots {[SLOTS[i] for i in bad]} at {rs[bad].tolist()} E "
                               f"(E = {self.E_slot[bad].tolist()}, ref {self.ref_acc[bad].tolist()})")
        return wb, ws


# ---- per-row value and gradient (pdeinv_mlp_potential through the row engine) ------------------------------------
def potential_rows(params, x, n_orders=N_ORDERS):
    """(V64 [n], g64 [n, d], eV [n], eg [n]): the fp64 value / gradient of the fp32 rows x and, per row, the largest
    scaled error of the fp32 restatement over n_orders unit orders x the two activations, scaled row-wise:
    |V32 - V64| / |V64| and max_i |g32 - g64| / max_i |g64|."""
    x = np.asarray(x)
    assert x.dtype == F32
    dims = [params[0][0].shape[0]] + [K.shape[1] for K, _ in params]
    x64 = x.astype(np.float64)
    V64, g64, _, _ = nr.mlp_forward_terms(params, x64, np.zeros_like(x64))
    C = np.zeros((len(x), 4), F32)
    Z = np.concatenate([x, np.zeros_like(x)], 1)
    eV, eg = np.zeros(len(x)), np.zeros(len(x))
    for k in range(n_orders):
        p32 = _cast(permute_units(params, unit_orders(dims, k)), F32)
        for tanh in (np.tanh, tanh_exp2):
            t = grad_rows(p32, Z, C, tanh)[1]
            eV = np.maximum(eV, value_err(t["V"], V64))
            eg = np.maximum(eg, grad_err(t["g"], g64))
    return V64, g64, eV, eg


def value_err(V, V64):
    return np.abs(np.asarray(V, np.float64) - V64) / np.abs(V64)


def grad_err(g, g64):
    return np.abs(np.asarray(g, np.float64) - g64).max(1) / np.abs(g64).max(1)

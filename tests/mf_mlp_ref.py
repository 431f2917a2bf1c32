"""Shared helpers of the learned-interaction tests (test_gpu_mf_mlp.py, test_mf_mlp_host.py): the fp64 / fp32
restatements of the mean-field force F_i = mean_j grad Phi_theta(x_i - r_j) (kinetic_mckean_vlasov.py:20-23) and the
teacher-forced check of one simulator update.

Yardstick (the rule of tests/mlp_sim_ref.py, applied per pair): E_pair = max over a case's pairs of |grad Phi_32 -
grad Phi_64| (the gradients of value_grad32 / value_grad64 on the pair differences, which are formed in fp32 as the
kernel forms them). A mean of numbers each wrong by at most E is wrong by at most E, so the force must satisfy
    max |F_gpu - F_64| <= RULE x E_pair,
and one update from the GPU's own previous state must satisfy
    max |z_gpu - z_64| <= RULE x (h_s E_pair,s + E_upd,s),
E_upd,s the error of oracle.numpy_ref.update_step in fp32, fed the fp64 force rounded to fp32, against the fp64
update. The factor covers the hardware exp2 / rcp tanh, the folded output layer and the fp32 in-chunk sums.
"""
import numpy as np

import mlp_sim_ref as R
from oracle import numpy_ref as nr

RULE = R.RULE
CHUNK = 256  # references per work unit of the force kernel (csrc/sde_mf_mlp.hip kChunk)
F32 = np.float32


def pair_diffs(x, r):
    """y[i, j] = x_i - r_j formed in fp32, [n, m, d]."""
    x, r = np.asarray(x, F32), np.asarray(r, F32)
    y = x[:, None, :] - r[None, :, :]
    assert y.dtype == F32
    return y


def grad64(params, x):
    """The input gradient of mlp_sim_ref.value_grad64, bit for bit (test_mf_mlp_host.py checks it): the value and
    reverse chain of oracle.numpy_ref.mlp_forward_terms without its two Taylor streams, a third of the work. The
    simulator tests evaluate 21 x N^2 pairs per case."""
    h = np.asarray(x, np.float64)
    cache = []
    for K, b in params[:-1]:
        h = np.tanh(h @ K + b)
        cache.append(1 - h * h)
    Ko, bo = params[-1]
    a = (2 * (h @ Ko + bo)) @ Ko.T
    for (K, _), s1 in zip(reversed(params[:-1]), reversed(cache)):
        a = (s1 * a) @ K.T
    return a


def pair_grads(params, x, r):
    """(grad Phi_64, grad Phi_32) [n, m, d] of every pair: grad64 and mlp_sim_ref.value_grad32."""
    y = pair_diffs(x, r)
    n, m, d = y.shape
    g64 = grad64(params, y.reshape(-1, d)).reshape(n, m, d)
    g32 = R.value_grad32(params, y.reshape(-1, d))[1].reshape(n, m, d)
    assert g64.dtype == np.float64 and g32.dtype == F32
    return g64, g32


def force64(params, x, r):
    """(F_64 [n, d], E_pair) of items x against references r."""
    g64, g32 = pair_grads(params, x, r)
    return g64.mean(1), float(np.max(np.abs(g32.astype(np.float64) - g64)))


def step_sizes(tau_row0, n_steps, dt, random_shift=True):
    """The fp32 h of every update, from the shared tau0 = stamp_times(...)[0]: tau0, dt, ..., dt, dt - tau0."""
    dt32 = F32(dt)
    tau0 = F32(tau_row0) if random_shift else F32(0)
    return np.array([tau0] + [dt32] * (n_steps - 1) + [F32(dt32 - tau0)], dtype=F32)


def teacher_forced_update(params, z_prev, ref_pos, h, gamma, xi):
    """One update in fp64 from the fp32 state z_prev [N, 2d] (forces against ref_pos [m, d]) and the yardstick:
    returns (z_64 [N, 2d], bound / RULE = h E_pair + E_upd)."""
    z_prev = np.asarray(z_prev, F32)
    d = z_prev.shape[1] // 2
    F64, e_pair = force64(params, z_prev[:, :d], ref_pos)
    q, p = z_prev[:, :d].astype(np.float64), z_prev[:, d:].astype(np.float64)
    h64 = np.float64(h)
    q64, p64 = nr.update_step(q, p, h64, lambda _: F64, np.float64(gamma), np.asarray(xi, np.float64))
    q32, p32 = nr.update_step(z_prev[:, :d], z_prev[:, d:], F32(h), lambda _: F64.astype(F32), F32(gamma),
                              np.asarray(xi, F32), F32(nr.SQRT2))
    assert q32.dtype == F32 and p32.dtype == F32
    z64 = np.concatenate([q64, p64], 1)
    e_upd = float(np.max(np.abs(np.concatenate([q32, p32], 1).astype(np.float64) - z64)))
    return z64, float(h64) * e_pair + e_upd


def zero_force_net(d, L, W, O):
    """A net whose output layer is zero: Phi = 0 and grad Phi = 0 exactly (the noise-stream tests)."""
    params, rng = R.make_net(d, L, W, O)
    K, b = params[-1]
    params[-1] = (np.zeros_like(K), np.zeros_like(b))
    return params, rng


def native_steps(native, dims, flat, z0, n_steps, dt, gamma, ref_of, **kw):
    """The per-update loop through the native step binding for the rows z0 (a shard or the whole ensemble): before
    update s the references are ref_of(s, zin) [m, d], zin the rows' own state before it.
    Returns (traj [n, N, 2d], tau [n, N], last [N, 2d])."""
    import torch
    N, m2 = z0.shape
    desc = native.mf_mlp_desc(N, m2 // 2, n_steps, dt, gamma, **kw)
    ws = native.mf_mlp_prepare(dims, flat, N, ref_of(0, z0).shape[0])
    traj = torch.empty((n_steps, N, m2), device=z0.device)
    tau = torch.empty((n_steps, N), device=z0.device)
    last = torch.empty((N, m2), device=z0.device)
    for s in range(n_steps + 1):
        zin = z0 if s == 0 else traj[s - 1]
        native.mf_mlp_step(desc, dims, s, zin, last if s == n_steps else traj[s], tau[s] if s < n_steps else None,
                           ref_of(s, zin), ws)
    return traj, tau, last

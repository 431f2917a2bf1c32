"""Shared helpers of the learned-potential tests (test_gpu_sim_mlp.py, test_sim_mlp_host.py): the test nets, and the
restatement of V_hypothesis' value / input gradient (core/model.py:32-62) with every array and operation in fp32.

The fp64 restatement is oracle.numpy_ref.mlp_forward_terms; it casts to fp64, so the fp32 copy of the same forward /
reverse chain lives here. The parity rule of the tests: the GPU's scaled error against fp64 must be at most
RULE x the fp32 restatement's own error against fp64 on the same inputs. The factor covers what the fp32
restatement does not do: the hardware exp2 / rcp tanh, the folded output layer 2 (M (h - h0) + c0), and a different
summation order.
"""
import numpy as np

from oracle import numpy_ref as nr

RULE = 16.0
TILE_SHAPES = [(1, 2, 20, 40), (2, 8, 20, 40), (4, 8, 20, 40), (8, 8, 20, 40), (4, 1, 20, 40), (3, 3, 13, 7),
               (5, 2, 17, 40)]


def dims_of(d, L, W, O):
    return [d] + [W] * L + [O]


def make_net(d, L, W, O):
    """(params fp64 list [(K, b), ...], rng): kernels N(0, 2 / fan_in), biases 0.1 N(0, 1), rng = default_rng(100 d + L);
    the rng is returned so that the positions / velocities / noise of a test continue the same stream."""
    rng = np.random.default_rng(100 * d + L)
    dims = dims_of(d, L, W, O)
    params = []
    for i in range(len(dims) - 1):
        K = rng.standard_normal((dims[i], dims[i + 1])) * np.sqrt(2.0 / dims[i])
        b = 0.1 * rng.standard_normal(dims[i + 1])
        params.append((K.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64)))
    return params, rng


def positions(rng, n, d):
    return (1.5 * rng.standard_normal((n, d))).astype(np.float32)


def velocities(rng, n, d):
    return (0.3 * rng.standard_normal((n, d))).astype(np.float32)


def value_grad64(params, x):
    x = np.asarray(x, np.float64)
    V, g, _, _ = nr.mlp_forward_terms(params, x, np.zeros_like(x))
    return V, g


def value_grad32(params, x):
    """mlp_forward_terms' value and reverse chain with every array and operation in fp32."""
    f = np.float32
    p32 = [(K.astype(f), b.astype(f)) for K, b in params]
    h = np.asarray(x, f)
    cache = []
    for K, b in p32[:-1]:
        h = np.tanh(h @ K + b)
        cache.append(f(1) - h * h)
    Ko, bo = p32[-1]
    y = h @ Ko + bo
    V = np.sum(y * y, -1, dtype=f)
    a = (f(2) * y) @ Ko.T
    for (K, _), s1 in zip(reversed(p32[:-1]), reversed(cache)):
        a = (s1 * a) @ K.T
    assert V.dtype == f and a.dtype == f
    return V, a


def grad_fn64(params):
    return lambda q: value_grad64(params, q)[1]


def grad_fn32(params):
    return lambda q: value_grad32(params, q)[1]


def flat32(params):
    return nr.mlp_flat(params).astype(np.float32)


def row_err(a, ref):
    """max |a - ref| relative to max |ref| (gradient rows, values)."""
    ref = np.asarray(ref, np.float64)
    return float(np.max(np.abs(np.asarray(a, np.float64) - ref)) / np.max(np.abs(ref)))


def traj_err(a, ref):
    """the scaling of test_sde_gmm_explicit_noise: per particle, max |ref| over time and coordinates, + 1."""
    ref = np.asarray(ref, np.float64)
    if ref.ndim == 2:
        ref, a = ref[None], np.asarray(a)[None]
    scale = np.abs(ref).max(axis=(0, 2), keepdims=True) + 1.0
    return float(np.max(np.abs(np.asarray(a, np.float64) - ref) / scale))


def sde_scan32(z0, n, dt, gamma, params, xi, u, **kw):
    return nr.sde_scan(z0, n, dt, gamma, grad_fn32(params), xi, u, dtype=np.float32, **kw)

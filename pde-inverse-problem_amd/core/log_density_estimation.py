"""Log-density estimation driver (core/log_density_estimation.py of the reference).

`create_normalizing_flow_fn` builds the same model as the reference (:103-114): MNF(dim,
embed_time_dim=10, couple_mul=4, mask_type='loop', activation 'celu', soft_init=1,
ignore_time=False) inside RealNVP with the problem's initial x-marginal as base density.
`estimate_log_density` is the reference's maximum-likelihood training loop (:13-100): every epoch
takes one in five time stamps from a random phase and a random fifth of the offline trajectories
(the native gather kernel over the time-major dataset), evaluates loss = -mean log p and its
parameter gradient on the HIP kernel `pdeinv_realnvp_value_and_grad` (replacing
jax.value_and_grad) and takes an Adam step (b1 = 0.9, eps = 1e-4) on the fused native update,
with the reference's constant / cosine / constant learning-rate schedule (:116-145). Epoch losses
stay on the device and are fetched once per print interval. The closing density plot
(plot_trajectory_of_distributions, matplotlib + wandb) is out of scope; `flow_moment_error` is its numeric
stand-in (moments of flow samples against the data's, per time stamp); where the true marginal is a known Gaussian,
`flow_divergence` measures the fit itself: the KL and the relative Fisher divergence of the learned density from it.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from core.normalizing_flow import MNF, RealNVP
from utils import native, prng


def create_normalizing_flow_fn(log_prob_0, dim):
    param_dict = {
        "dim": dim,
        "embed_time_dim": 10,
        "couple_mul": 4,
        "mask_type": "loop",
        "activation_layer": "celu",
        "soft_init": 1.0,
        "ignore_time": False,
    }
    return RealNVP(MNF(**param_dict), log_prob_0)


def create_custom_schedule(lr, T0, T1):
    """optax.join_schedules([constant(lr), warmup_cosine_decay(lr, lr, 0, T1 - T0, lr * 1e-2),
    constant(lr * 1e-2)], [T0, T1]) (:116-145)."""
    def schedule(step):
        if step < T0:
            return lr
        if step < T1:
            s = min(step - T0, T1 - T0) / (T1 - T0)
            alpha = 1e-2
            return lr * ((1 - alpha) * 0.5 * (1 + math.cos(math.pi * s)) + alpha)
        return lr * 1e-2
    return schedule


def make_log_density_fn(model: RealNVP, params):
    """log_density_fn(t, x) of a flow and its parameters, as estimate_log_density returns it: .model, .params and
    .partial_s(t, x) -> (ds log p, ds2 log p) (pdeinv_realnvp_time_derivs), .sample(key, t, n) -> (x, log p) and
    .inverse(t, x) -> (x0, ldj) (pdeinv_realnvp_map), .score(t, x) -> grad_x log p (pdeinv_realnvp_score)."""
    def log_density_fn(t, x):
        return model.apply(params, t, x)

    def partial_s(t, x):
        _, d1, d2 = model.time_derivatives(params, t, x)
        return d1, d2

    log_density_fn.params = params
    log_density_fn.model = model
    log_density_fn.partial_s = partial_s
    log_density_fn.sample = lambda key, t, n, **kw: model.sample(params, key, t, n, **kw)
    log_density_fn.inverse = lambda t, x: model.inverse(params, t, x)
    log_density_fn.score = lambda t, x: model.score(params, t, x)
    return log_density_fn


def _moments_of_sets(rows, n_sets, n_rows, d):
    """(mean [n_sets, d], cov [n_sets, d, d]) fp64 of the row sets of a contiguous [n_sets * n_rows, >= d] tensor,
    from one native.moments_batched call ([count, sum x, sum x_i x_j (i <= j)] per set)."""
    ld = rows.stride(0)
    mom = native.moments_batched(rows, n_sets, n_rows, d, n_rows * ld, ld)
    cnt = mom[:, :1]
    mean = mom[:, 1:1 + d] / cnt
    iu = torch.triu_indices(d, d, device=mom.device)
    second = torch.zeros((n_sets, d, d), device=mom.device, dtype=mom.dtype)
    second[:, iu[0], iu[1]] = mom[:, 1 + d:]
    second[:, iu[1], iu[0]] = mom[:, 1 + d:]
    cov = second / cnt[:, :, None] - mean[:, :, None] * mean[:, None, :]
    return mean, cov


def flow_sample_moments(log_density_fn, key, taus, n_per_time):
    """(mean [n_t, d], cov [n_t, d, d]) (fp64, population covariance) of n_per_time flow samples per time stamp in
    `taus`: one `sample` call over all stamps with t repeated, one native.moments_batched call."""
    model = log_density_fn.model
    d = model.mnf.dim
    dev = log_density_fn.params["params"].device
    taus = torch.as_tensor(taus, dtype=torch.float32, device=dev).reshape(-1)
    n_t, n = taus.numel(), int(n_per_time)
    x, _ = log_density_fn.sample(key, taus.repeat_interleave(n), n_t * n)
    return _moments_of_sets(x, n_t, n, d)


def flow_moment_error(log_density_fn, key, dataset, time_index, n_per_time):
    """The numeric stand-in for the reference's closing density plot: per time stamp in `time_index` of
    dataset {"0T_tm": [n_time, n_traj, >= d] time-major, "tau_0T": [n_traj, n_time]}, the relative errors (Frobenius
    norm) of the mean and covariance of n_per_time flow samples against those of the dataset's x-rows at that stamp
    (the stamp's time: the mean of its tau column). Returns (err_mean [n_t], err_cov [n_t]) fp64."""
    model = log_density_fn.model
    d = model.mnf.dim
    traj = dataset["0T_tm"]
    ti = torch.as_tensor(np.asarray(time_index), device=traj.device, dtype=torch.long).reshape(-1)
    rows = traj[ti].contiguous()                                  # [n_t, n_traj, w]
    n_t, n_traj, w = rows.shape
    taus = dataset["tau_0T"].to(traj.device)[:, ti].double().mean(0)
    m_d, c_d = _moments_of_sets(rows.reshape(n_t * n_traj, w), n_t, n_traj, d)
    m_f, c_f = flow_sample_moments(log_density_fn, key, taus, n_per_time)
    err_mean = torch.linalg.vector_norm(m_f - m_d, dim=-1) / torch.linalg.vector_norm(m_d, dim=-1)
    err_cov = torch.linalg.matrix_norm(c_f - c_d) / torch.linalg.matrix_norm(c_d)
    return err_mean, err_cov


def flow_divergence_from_gaussian(log_density_fn, key, taus, mean, cov, n_per_time, row_offset=0, counter_offset=0):
    """Divergences of the learned density rho^_t from a known Gaussian truth rho_t = N(mean_k, cov_k) per time stamp
    taus[k] (what the reference's test_fn meant to report as "KL" and "Fisher Information"), estimated on n_per_time
    draws x of the truth per stamp:
      kl[k]         = mean[log rho(x) - log rho^(x)]                                   (KL(rho || rho^))
      fisher_rel[k] = mean|grad log rho^(x) + P^-1 (x - m)|^2 / mean|P^-1 (x - m)|^2   (relative Fisher divergence)
    The rows: native.gaussian_sample_grouped(n_per_time, mean as fp32, the lower Cholesky factors of cov as fp32,
    seed=key.seed, counter_offset=counter_offset, row_offset=row_offset), the seed taken from `key` as
    Gaussian.sample takes it, so a caller can redraw them; stamp k owns rows k * n_per_time .. (k + 1) * n_per_time.
    One native.realnvp_score call over all stamps with t repeated gives log rho^ and its score; the truth's terms
    and the means are formed in fp64 on the device. mean [n_t, d] and cov [n_t, d, d]: host fp64. Returns
    (kl [n_t], fisher_rel [n_t]) as fp64 device tensors."""
    model = log_density_fn.model
    d = model.mnf.dim
    flat = log_density_fn.params["params"]
    dev = flat.device
    taus = torch.as_tensor(taus, dtype=torch.float32, device=dev).reshape(-1)
    n_t, n = taus.numel(), int(n_per_time)
    mean = np.asarray(mean, dtype=np.float64).reshape(n_t, d)
    cov = np.asarray(cov, dtype=np.float64).reshape(n_t, d, d)
    half = np.linalg.cholesky(cov)
    x = native.gaussian_sample_grouped(n, torch.as_tensor(mean, dtype=torch.float32, device=dev),
                                       torch.as_tensor(half, dtype=torch.float32, device=dev), seed=key.seed,
                                       counter_offset=counter_offset, row_offset=row_offset)
    res = native.realnvp_score(model._desc, flat, taus.repeat_interleave(n), x)
    P_inv = torch.as_tensor(np.linalg.inv(cov), device=dev)                               # [n_t, d, d] fp64
    log_norm = torch.as_tensor(np.linalg.slogdet(2 * np.pi * cov)[1], device=dev)         # [n_t]
    off = x.double().reshape(n_t, n, d) - torch.as_tensor(mean, device=dev)[:, None, :]
    w = torch.einsum("kij,knj->kni", P_inv, off)                                          # -grad log rho
    logp_true = -0.5 * (log_norm[:, None] + (off * w).sum(-1))
    kl = (logp_true - res["logp"].double().reshape(n_t, n)).mean(1)
    num = ((res["score"].double().reshape(n_t, n, d) + w) ** 2).sum(-1).mean(1)
    return kl, num / (w ** 2).sum(-1).mean(1)


def flow_divergence(log_density_fn, key, pde_instance, taus, n_per_time):
    """flow_divergence_from_gaussian against the instance's closed-form X-marginal (pde_instance.x_marginal, the
    OU / McKean-Vlasov problems): (kl [n_t], fisher_rel [n_t]) of the learned density per time stamp."""
    mean, cov = pde_instance.x_marginal(np.asarray(torch.as_tensor(taus).detach().cpu(), dtype=np.float64).reshape(-1))
    return flow_divergence_from_gaussian(log_density_fn, key, taus, mean, cov, n_per_time)


def estimate_log_density(cfg, pde_instance, rng, num_epochs: int = 20000, frequency: int = 100, verbose=True,
                         dataset=None):
    """Train the flow on pde_instance.dataset (offline "0T" trajectories and their tau) and return
    log_density_fn(t, x) (:13-100) with .history (mean loss per interval), .params, .model (the RealNVP) and
    .partial_s(t, x) -> (ds log p, ds2 log p) (the time derivatives the KMV residual weights Phi with,
    kinetic_mckean_vlasov.py:57-72). `dataset` (optional): {"0T_tm": time-major trajectories [n_time, n_traj,
    >= dim], "tau_0T": [n_traj, n_time]} to train on instead of pde_instance.dataset, e.g. a KMV instance's own."""
    rngs = dict(zip(["model_init", "train"], prng.split(rng, 2)))
    dim = int(cfg.pde_instance.domain_dim)
    model = create_normalizing_flow_fn(pde_instance.distribution_initial_x.logdensity, dim)
    if dataset is None:
        dataset = pde_instance.dataset
    traj_tm = dataset["0T_tm"]                       # [n_time, n_traj, 2d] (time-major)
    dev = traj_tm.device
    params = model.init(rngs["model_init"], 0.0, np.zeros(dim), device=dev)
    flat = params["params"]
    tau_tm = dataset["tau_0T"].permute(1, 0).contiguous().unsqueeze(-1)  # [n_time, n_traj, 1]
    n_time, n_traj = traj_tm.shape[0], traj_tm.shape[1]
    schedule = create_custom_schedule(1e-3, 5000, 15000)
    mu, nu = torch.zeros_like(flat), torch.zeros_like(flat)
    interval_time, interval_sample = 5, 5
    time_base = np.arange(n_time // interval_time) * interval_time
    rng_epoch = prng.split(rngs["train"], num_epochs)
    acc = torch.zeros((), device=dev, dtype=torch.float32)
    history = []
    for epoch in range(num_epochs):
        rng_time, rng_sample = prng.split(rng_epoch[epoch])
        time_index = time_base + int(prng.randint(rng_time, (), 0, interval_time))
        sample_index = prng.permutation(rng_sample, n_traj)[: n_traj // interval_sample]
        si = torch.as_tensor(sample_index, device=dev)
        ti = torch.as_tensor(time_index, device=dev)
        rows = native.gather_subsample(traj_tm, si, ti)        # [n_sel * n_t, 2d]
        times = native.gather_subsample(tau_tm, si, ti)[:, 0]  # the matching tau
        loss, grad = native.realnvp_value_and_grad(model._desc, flat, times, rows[:, :dim])
        native.adam_update(flat, grad, mu, nu, lr=schedule(epoch), b1=0.9, b2=0.999, eps=1e-4, weight_decay=0.0,
                           count=epoch + 1)
        acc += loss
        if (epoch + 1) % frequency == 0:
            mean = float(acc) / frequency
            history.append(mean)
            acc.zero_()
            if verbose:
                print(f"Epoch {epoch + 1}, Loss: {mean}")

    log_density_fn = make_log_density_fn(model, params)
    log_density_fn.history = history
    return log_density_fn

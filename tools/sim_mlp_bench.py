#!/usr/bin/env python3
"""Time of the learned-potential simulator (pdeinv_sde_simulate_mlp) at the reference's default net
(d = 4 -> 20 x 8 -> 40), N = 2^20 particles, n = 100 steps, with the trajectory written and without, beside the
only way the package could do the same before the kernel existed: a torch loop of V_hypothesis.apply +
torch.autograd.grad + the element-wise update (torch.randn noise), on the same inputs.

The variants are timed alternately (one round = each variant once, between two device events after a
synchronise), after a warm-up of each; reported: the median over the rounds and the spread (min, max). The torch
loop takes `--torch-rounds` rounds (it is ~two orders slower). Also reported: the issue-cycle model of DESIGN.md
(MFMAs per 16 particle-steps x 32 cycles over the SIMDs' clock) and the measured time's ratio to it.

    python tools/sim_mlp_bench.py [--rounds 9] [--log2n 20] [--steps 100]   -> profiles/sim_mlp_bench.json

`--shape d,L,W,O` times another net. A net of the wide simulator (pdeinv_sde_simulate_mlp_wide, width 21..256)
gets a third baseline, "composed": per update one native.mlp_potential call (the fused row engine in gradient-only
mode) and the element-wise torch update with torch.randn noise — what the package offered for such a net before the
wide kernel. The result then goes to profiles/sim_mlp_wide_bench.json, with the wide tile's MFMA count.

    python tools/sim_mlp_bench.py --shape 8,2,256,40                        -> profiles/sim_mlp_wide_bench.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pde-inverse-problem_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def mfma_per_tile_step(d: int, L: int) -> int:
    """16x16x4 MFMAs of one tile_grad call (mlp_tile.h): layer 0 forward 2 KD, hidden forward 10 each, the folded
    output layer 10, hidden backward 10 each, layer 0 backward 5."""
    kd = 1 if d <= 4 else 2
    return 2 * kd + 10 * (L - 1) + 10 + 10 * (L - 1) + 5


def mfma_per_tile_step_wide(d: int, L: int, W: int, O: int) -> int:
    """16x16x4 MFMAs of one wide_grad call (mlp_tile_wide.h): four per quad-unit, two for a layer-0 forward one."""
    mb, ob = (W + 15) // 16, (O + 15) // 16
    units = 2 * (mb + (L - 1) * mb * mb + ob * mb)
    return 4 * units - 2 * mb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default=None, help="d,L,W,O (default: the reference's 4,8,20,40)")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--torch-rounds", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--clock-mhz", type=float, default=2400.0, help="engine clock of the issue model (MI355X peak)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sim_mlp_bench: needs the GPU (a CPU run gives no time)")
    from core.model import V_hypothesis
    from utils import native, prng
    dev = "cuda"
    d, L, W, O = (int(v) for v in a.shape.split(",")) if a.shape else (4, 8, 20, 40)
    N, n, dt, gamma = 1 << a.log2n, a.steps, 0.02, 0.5
    model = V_hypothesis(1, [W] * L, out_features=O)
    tree = model.init(prng.PRNGKey(11), np.zeros(d), device=dev)
    g = torch.Generator(device=dev).manual_seed(1)
    for p in tree["params"].values():  # off the zero-bias initialisation
        p["bias"].add_(0.1 * torch.randn(p["bias"].shape, device=dev, generator=g))
    flat = model.flat(tree)
    dims = model.dims(d)
    wide = not native.sde_simulate_mlp_supported(dims)
    if wide and not native.sde_simulate_mlp_wide_supported(dims):
        raise SystemExit(f"sim_mlp_bench: no simulator takes the net {dims}")
    sim = native.sde_simulate_mlp_wide if wide else native.sde_simulate_mlp
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "sim_mlp_wide_bench.json" if wide else "sim_mlp_bench.json")
    z0 = torch.cat([1.5 * torch.randn((N, d), device=dev, generator=g),
                    0.3 * torch.randn((N, d), device=dev, generator=g)], 1)
    bufs = {"traj": torch.empty((n, N, 2 * d), device=dev), "tau": torch.empty((n, N), device=dev),
            "last": torch.empty((N, 2 * d), device=dev)}

    def hip(traj):
        sim(z0, n, dt, gamma, dims, flat, seed=7, traj=traj, tau=traj, last=True, out=bufs)

    def step(q, p, gr, h):
        xi = torch.randn((N, d), device=dev, generator=g)
        sh = torch.sqrt(h) if torch.is_tensor(h) else h ** 0.5
        p = p - h * gr + sh * native.SQRT2 * xi - gamma * p * h
        return q + h * p, p

    def composed():
        q, p = z0[:, :d].clone(), z0[:, d:].clone()
        tau0 = torch.rand((N, 1), device=dev, generator=g) * dt
        for s in range(n + 1):
            h = tau0 if s == 0 else ((dt - tau0) if s == n else dt)
            _, gr = native.mlp_potential(dims, flat, q, False, True)
            q, p = step(q, p, gr, h)
            if s < n:
                bufs["traj"][s, :, :d] = q
                bufs["traj"][s, :, d:] = p
        bufs["last"][:, :d] = q
        bufs["last"][:, d:] = p

    def torch_loop():
        q, p = z0[:, :d].clone(), z0[:, d:].clone()
        tau0 = torch.rand((N, 1), device=dev, generator=g) * dt
        for s in range(n + 1):
            h = tau0 if s == 0 else ((dt - tau0) if s == n else dt)
            x = q.detach().requires_grad_(True)
            gr, = torch.autograd.grad(model.apply(tree, x).sum(), x)
            xi = torch.randn((N, d), device=dev, generator=g)
            sh = torch.sqrt(h) if torch.is_tensor(h) else h ** 0.5
            p = p - h * gr + sh * native.SQRT2 * xi - gamma * p * h
            q = q + h * p
            if s < n:
                bufs["traj"][s, :, :d] = q
                bufs["traj"][s, :, d:] = p
        bufs["last"][:, :d] = q
        bufs["last"][:, d:] = p

    variants = {"hip_traj": lambda: hip(True), "hip_no_traj": lambda: hip(False), "torch_loop_traj": torch_loop}
    rounds = {"hip_traj": a.rounds, "hip_no_traj": a.rounds, "torch_loop_traj": a.torch_rounds}
    if wide:
        variants["composed_traj"] = composed
        rounds["composed_traj"] = a.rounds
    for name, fn in variants.items():
        for _ in range(a.warmup if name != "torch_loop_traj" else 1):
            fn()
    torch.cuda.synchronize()
    assert torch.isfinite(bufs["last"]).all()
    times = {k: [] for k in variants}
    for r in range(max(rounds.values())):
        for name, fn in variants.items():
            if r >= rounds[name]:
                continue
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1))
    props = torch.cuda.get_device_properties(0)
    cus, clock_hz = props.multi_processor_count, a.clock_mhz * 1e6
    mf = mfma_per_tile_step_wide(d, L, W, O) if wide else mfma_per_tile_step(d, L)
    model_ms = (N / 16) * (n + 1) * mf * 32 / (cus * 4 * clock_hz) * 1e3
    res = {"device": props.name, "cus": cus, "clock_mhz": a.clock_mhz, "d": d, "layers": L, "width": W,
           "out_features": O, "N": N, "n_steps": n, "mfma_per_tile_step": mf, "issue_model_ms": model_ms,
           "trajectory_bytes": n * N * 2 * d * 4}
    for name, ts in times.items():
        res[name] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "rounds": len(ts)}
    res["hip_no_traj_over_model"] = res["hip_no_traj"]["median_ms"] / model_ms
    res["hip_traj_over_model"] = res["hip_traj"]["median_ms"] / model_ms
    res["torch_over_hip_traj"] = res["torch_loop_traj"]["median_ms"] / res["hip_traj"]["median_ms"]
    if wide:
        res["composed_over_hip_traj"] = res["composed_traj"]["median_ms"] / res["hip_traj"]["median_ms"]
        res["hip_slowest_over_composed_fastest"] = (max(res["hip_traj"]["max_ms"], res["hip_no_traj"]["max_ms"])
                                                    / res["composed_traj"]["min_ms"])
    res["particle_steps_per_s_no_traj"] = N * (n + 1) / (res["hip_no_traj"]["median_ms"] * 1e-3)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

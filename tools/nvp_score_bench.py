#!/usr/bin/env python3
"""Cost of the RealNVP score grad_x log p (pdeinv_realnvp_score) against what a caller did before it existed: 2 d
log-density passes for a central difference.

Batches: the reference's per-epoch batch (320 000 samples, d = 4, 16 loop-mask coupling layers, E = 10, celu), the
KMV recipe's stamp (5 000 samples, d = 2, 8 layers) and d = 8, 16 layers, 320 000 samples. Per batch the variants are
timed alternately (one round = each variant once, `--inner` back-to-back calls between two device events), after a
warm-up of every variant; reported: the median over the rounds of the per-call time and its spread (min, max). Rows
are [x | v] (ld = 2d), as the trajectory dataset has them.

    (a)  fd_logdensity   2 d calls of pdeinv_realnvp_logdensity (the kernel passes of a central difference; forming
                         the shifted rows and the difference itself are not counted)
    (a') fd_map_logp     2 d dispatched pdeinv_realnvp_map(reverse = 1, logp only) calls
    (b)  general         pdeinv_realnvp_score, the per-thread path (score and logp; the wrapper allocates the
                         workspace from torch's caching allocator)
         general_logp    the same call asked for logp only (no workspace, no backward sweep)
    (c)  matrix          pdeinv_realnvp_score, the matrix-core path (score and logp)

    python tools/nvp_score_bench.py [--rounds 15] [--inner 5] [--out profiles/nvp_score_bench.jsonl]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pde-inverse-problem_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", default="4:4:320000,2:4:5000,8:2:320000", help="dim:couple_mul:samples,...")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nvp_score_bench.jsonl"))
    a = ap.parse_args()
    from core.distribution import Gaussian
    from core.normalizing_flow import MNF, RealNVP
    from utils import native, prng
    if not torch.cuda.is_available():
        raise SystemExit("nvp_score_bench: needs the GPU (a CPU run gives no time)")
    dev = "cuda"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    lines = []
    for spec in a.batches.split(","):
        dim, couple, n = (int(v) for v in spec.split(":"))
        gauss = Gaussian(np.zeros(dim), 4 * np.eye(dim))
        flow = RealNVP(MNF(dim, couple, "loop", 1.0, False, "celu", 10), gauss.logdensity)
        flat = flow.init(prng.PRNGKey(0), 0.0, np.zeros(dim))["params"]
        g = torch.Generator(device=dev).manual_seed(1)
        flat = flat + 0.05 * torch.randn(flat.shape, device=dev, generator=g)   # off the identity map
        z = torch.randn((n, 2 * dim), device=dev, generator=g) * 1.5
        x = z[:, :dim]
        t = 0.05 + 1.95 * torch.rand(n, device=dev, generator=g)
        desc = flow._desc
        out = torch.empty((n, dim), device=dev)

        def fd_logdensity():
            for _ in range(2 * dim):
                native.realnvp_logdensity(desc, flat, t, x)

        def fd_map_logp():
            for _ in range(2 * dim):
                native.realnvp_map(desc, flat, t, x, 1, impl="auto", want=("logp",))

        variants = {"fd_logdensity": fd_logdensity, "fd_map_logp": fd_map_logp,
                    "general": lambda: native.realnvp_score(desc, flat, t, x, impl="general", out=out),
                    "matrix": lambda: native.realnvp_score(desc, flat, t, x, impl="matrix", out=out),
                    "general_logp": lambda: native.realnvp_score(desc, flat, t, x, impl="general", want=("logp",))}
        for fn in variants.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(a.rounds):
            for k, fn in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.inner):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1) / a.inner)
        rec = {"workload": f"RealNVP d={dim}, {flow.mnf.n_layers} coupling layers, E=10, celu", "samples": n,
               "rounds": a.rounds, "inner": a.inner, "auto_path": native.realnvp_score_path(desc, "auto"),
               "workspace_bytes": {k: int(native.lib().pdeinv_realnvp_score_workspace_bytes(ctypes.byref(desc), n, v))
                                   for k, v in (("general", 1), ("matrix", 2))}}
        for k, v in times.items():
            rec[k] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}
        gs, ms = (native.realnvp_score(desc, flat, t, x, impl=k) for k in ("general", "matrix"))
        rec["paths_max_rel_diff"] = {k: float((gs[k] - ms[k]).abs().max() / (1 + gs[k].abs().max())) for k in gs}
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time MCF dictionary synthesis (mfx_mcf_pgse / mfx_mcf_dde) on HCP's 552-row protocol x n_atoms
(radius, diffusivity) atoms; one JSON line per sequence type with items/s and the kernel time that
mfx_last_kernel_ms reports (both kernels of a call: closed-form rows and matrix exponentials).
   python tools/dev_time_mcf.py [n_atoms] [reps]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from microstructure_fingerprinting_amd import _lib as L  # noqa: E402
from microstructure_fingerprinting_amd import mcf  # noqa: E402

n_atoms = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 2
sch = np.load(os.path.join(ROOT, "tests", "golden", "real_hcp.npz"))["sch_mat"]
rng = np.random.default_rng(0)
rad = rng.uniform(0.5e-6, 8e-6, n_atoms)
dif = rng.uniform(1e-9, 3e-9, n_atoms)
# DDE rows from the same directions: second block orthogonal to the first, 10 ms mixing, the PGSE timing split in two
g1 = sch[:, :3]
g2 = np.cross(g1, np.array([0.0, 0.0, 1.0]) + 0.3 * g1[:, [1, 2, 0]])
n2 = np.linalg.norm(g2, axis=1, keepdims=True)
g2 = np.where(n2 > 0, g2 / np.where(n2 > 0, n2, 1.0), 0.0)
Dl, dl = sch[:, 4] / 2, sch[:, 5] / 2
dde = np.column_stack([g1, sch[:, 3], Dl, dl, np.full(len(sch), 0.01), g2, sch[:, 3], Dl, dl,
                       2 * (Dl + dl) + 0.011])
lam, B = mcf.mcf_tables('c', 60)
lib = L.lib()
lam, B, rad, dif = L.f64c(lam), L.f64c(B), L.f64c(rad), L.f64c(dif)
env = L.f64c([0.0, 0.0, 1.0])
gamma = 2 * np.pi * 42.577480e6
for name, fn, seq in (("pgse", lib.mfx_mcf_pgse, L.f64c(sch)), ("dde", lib.mfx_mcf_dde, L.f64c(dde))):
    E = np.empty((seq.shape[0], n_atoms))

    def run():
        L.check(fn(L.dptr(lam), L.dptr(B), 60, L.dptr(seq), seq.shape[0], L.dptr(rad), L.dptr(dif), n_atoms,
                   L.dptr(env), gamma, L.dptr(E)))

    run()
    lib.mfx_set_profiling(1)
    ks, ws = [], []
    for _ in range(reps):
        t0 = time.perf_counter(); run(); ws.append(time.perf_counter() - t0); ks.append(lib.mfx_last_kernel_ms())
    lib.mfx_set_profiling(0)
    n_items = int(np.sum(sch[:, 3] != 0)) * n_atoms
    kms = float(np.min(ks))
    print(json.dumps({"tool": "dev_time_mcf", "seq": name, "n_seq": int(seq.shape[0]), "n_atoms": n_atoms,
                      "matrix_items": n_items, "kernel_ms": round(kms, 3), "wall_ms": round(1e3 * min(ws), 3),
                      "items_per_s_kernel": round(n_items / (kms * 1e-3)), "finite": bool(np.all(np.isfinite(E))),
                      "range": [float(E.min()), float(E.max())]}), flush=True)

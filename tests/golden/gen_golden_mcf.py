#!/usr/bin/env python3
"""Generate tests/golden/mcf_cases.npz by RUNNING THE REFERENCE's mcf module (MCF_PGSE, MCF_DDE).

Runs only in the build container, next to gen_golden.py (whose import_reference() it uses).
Stored: the reference's MCF_data tables as arrays, the protocols, the reference's signals for a
grid of (radius, diffusivity, axis, M) cases, and the exception type and message of each invalid
input in ERROR_CASES (replayed by tests/test_mcf_host.py from the JSON stored beside them).

Usage:  OPENBLAS_NUM_THREADS=1 python tests/golden/gen_golden_mcf.py
"""
import json
import os
import sys

os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
os.environ.setdefault("OMP_NUM_THREADS", "1")

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden  # noqa: E402

GAMMA = 2 * np.pi * 42.577480e6


def dde_scheme():
    """Synthetic 14-column DDE protocol: parallel and orthogonal block pairs, several mixing times,
    a row without gradient and rows with one block switched off."""
    rows = []
    x, y, z = np.eye(3)
    o = np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0)
    for tmix in (0.0, 5e-3, 20e-3):
        for g1, g2 in ((x, x), (x, y), (x, -x), (o, x), (y, z)):
            for G in (0.04, 0.08):
                Del, dl = 20e-3, 8e-3
                TE = 2 * (Del + dl) + tmix + 5e-3
                rows.append(np.r_[g1, G, Del, dl, tmix, g2, G, Del, dl, TE])
    rows.append(np.r_[x, 0.0, 20e-3, 8e-3, 5e-3, y, 0.0, 20e-3, 8e-3, 70e-3])
    rows.append(np.r_[x, 0.0, 20e-3, 8e-3, 5e-3, y, 0.06, 25e-3, 6e-3, 70e-3])
    rows.append(np.r_[x, 0.06, 15e-3, 10e-3, 10e-3, z, 0.0, 20e-3, 8e-3, 70e-3])
    rows.append(np.r_[z, 0.07, 15e-3, 10e-3, 10e-3, z, 0.05, 20e-3, 8e-3, 70e-3])   # along the default axis
    return np.array(rows)


# (function, kwargs) of invalid calls; arrays as nested lists, "sch_ukbb_2" = the first two UKBB rows
ERROR_CASES = [
    ("MCF_PGSE", {"domain": "c", "L": 2e-6, "diff": 2e-9}),
    ("MCF_PGSE", {"domain": "c", "L": 2e-6, "diff": 2e-9, "G": 0.05}),
    ("MCF_PGSE", {"domain": "c", "L": 2e-6, "diff": 2e-9, "G": [0.05, 0.06], "Delta": [0.03], "delta": [0.01, 0.01]}),
    ("MCF_PGSE", {"domain": "c", "L": 2e-6, "diff": 2e-9, "G": [0.05, 0.06], "Delta": [0.03, 0.005], "delta": [0.01, 0.01]}),
    ("MCF_PGSE", {"domain": "c", "L": 2e-6, "diff": 2e-9, "scheme": "sch_ukbb_2", "envdir": [0.0, 0.0, 0.0]}),
    ("MCF_PGSE", {"domain": "cyl", "L": 2e-6, "diff": 2e-9, "scheme": "sch_ukbb_2"}),
    ("MCF_PGSE", {"domain": "c", "L": 40e-6, "diff": 0.5e-9, "scheme": "sch_ukbb_2"}),
    ("MCF_PGSE", {"domain": "c", "L": 20e-6, "diff": 0.5e-9, "scheme": "sch_ukbb_2", "M": 20}),
    ("MCF_PGSE", {"domain": "c", "L": 40e-6, "diff": 0.5e-9, "G": [0.0, 0.05, 0.08], "Delta": [0.03, 0.03, 0.03],
                  "delta": [0.01, 0.01, 0.01]}),
    ("MCF_PGSE", {"domain": "s", "L": 2e-6, "diff": 2e-9, "scheme": "sch_ukbb_2"}),
    ("MCF_PGSE", {"domain": "sphere", "L": 2e-6, "diff": 2e-9, "G": [0.05], "Delta": [0.03], "delta": [0.01]}),
    ("MCF_PGSE", {"domain": "p", "L": 2e-6, "diff": 2e-9, "scheme": "sch_ukbb_2"}),
    ("MCF_PGSE", {"domain": "planes", "L": 2e-6, "diff": 2e-9, "scheme": "sch_ukbb_2", "M": 80}),
    ("MCF_PGSE", {"domain": "c", "L": 2e-6, "diff": 2e-9, "scheme": [[1.0, 0.0, 0.0, 0.05, 0.03, 0.01]]}),
    ("MCF_PGSE", {"domain": "c", "L": 2e-6, "diff": 2e-9, "scheme": [[1.0, 0.5, 0.0, 0.05, 0.03, 0.01, 0.05]]}),
    ("MCF_DDE", {"domain": "c", "L": 2e-6, "diff": 2e-9, "scheme": [[1, 0, 0, .05, .02, .008, .005, 0, 1, 0, .05, .02, .008]]}),
    ("MCF_DDE", {"domain": "c", "L": 2e-6, "diff": 2e-9, "scheme": [[1, 1, 0, .05, .02, .008, .005, 0, 1, 0, .05, .02, .008, .07]]}),
    ("MCF_DDE", {"domain": "c", "L": 2e-6, "diff": 2e-9, "scheme": [[1, 0, 0, .05, .02, .008, .005, 0, 1, 1, .05, .02, .008, .07]]}),
    ("MCF_DDE", {"domain": "c", "L": 2e-6, "diff": 2e-9, "scheme": [[1, 0, 0, .05, .005, .008, .005, 0, 1, 0, .05, .02, .008, .07]]}),
    ("MCF_DDE", {"domain": "c", "L": 2e-6, "diff": 2e-9, "scheme": [[1, 0, 0, .05, .02, .008, .005, 0, 1, 0, .05, .005, .008, .07]]}),
    ("MCF_DDE", {"domain": "c", "L": 2e-6, "diff": 2e-9, "scheme": [[1, 0, 0, .05, .02, .008, .005, 0, 1, 0, .05, .02, .008, .05]]}),
    ("MCF_DDE", {"domain": "c", "L": 2e-6, "diff": 2e-9, "scheme": "dde_2", "envdir": [0.0, 0.0, 0.0]}),
    ("MCF_DDE", {"domain": "x", "L": 2e-6, "diff": 2e-9, "scheme": "dde_2"}),
    ("MCF_DDE", {"domain": "c", "L": 40e-6, "diff": 0.5e-9, "scheme": "dde_2"}),
    ("MCF_DDE", {"domain": "s", "L": 2e-6, "diff": 2e-9, "scheme": "dde_2"}),
    ("MCF_DDE", {"domain": "p", "L": 2e-6, "diff": 2e-9, "scheme": "dde_2"}),
    ("MCF_DDE", {"domain": "c", "L": 2e-6, "diff": 2e-9, "scheme": [1, 0, 0, .05, .02, .008, .005, 0, 1, 0, .05, .02, .008, .07]}),
    ("MCF_DDE", {"domain": "c", "L": 2e-6, "diff": 2e-9, "scheme": "a_list"}),
]


def resolve(kw, named):
    """kwargs of an ERROR_CASES entry -> call arguments (names of stored inputs are looked up, lists become arrays)."""
    out = dict(kw)
    for k, v in kw.items():
        if isinstance(v, str) and v in named:
            out[k] = named[v]
        elif isinstance(v, list):
            out[k] = np.array(v, dtype=float)
    return out


def main():
    mfu, _ = gen_golden.import_reference()
    from microstructure_fingerprinting import mcf as rmcf
    ref_dir = os.path.join(gen_golden.REF, "microstructure_fingerprinting", "MCF_data")
    out = {}
    for dom in ("cl", "sl", "pl"):
        out["B" + dom] = np.asarray(mfu.loadmat(os.path.join(ref_dir, "MCF_B%s.mat" % dom))["B"], dtype=np.float64)
        out["L" + dom] = np.asarray(mfu.loadmat(os.path.join(ref_dir, "MCF_L%s.mat" % dom))["L"], dtype=np.float64).ravel()
    ukbb = np.load(os.path.join(HERE, "real_ukbb.npz"))["sch_subj"]
    hcp = np.load(os.path.join(HERE, "real_hcp.npz"))["sch_mat"]
    hcp_slice = hcp[::8]                 # 69 rows covering every shell
    dde = dde_scheme()
    out["sch_ukbb"], out["sch_hcp_slice"], out["sch_dde"] = ukbb, hcp_slice, dde
    oblique = np.array([0.3, -0.5, 0.81])
    envs = {"z": np.array([0.0, 0.0, 1.0]), "x": np.array([1.0, 0.0, 0.0]), "o": oblique}
    out["envdirs"] = np.stack([envs["z"], envs["x"], envs["o"]])
    # PGSE cases: (scheme id, L, D, envdir id, M)
    pg = []
    for L in (0.4e-6, 1e-6, 2e-6, 4e-6, 8e-6, 10e-6):
        for D in (0.5e-9, 1.7e-9, 3e-9):
            pg.append((0, L, D, 0, 60))
    for L, D in ((1e-6, 2e-9), (5e-6, 1e-9)):
        pg += [(0, L, D, 1, 60), (0, L, D, 2, 60), (1, L, D, 0, 60), (1, L, D, 2, 60), (0, L, D, 0, 20)]
    scheds = [ukbb, hcp_slice]
    cases, sigs, offs = [], [], [0]
    for si, L, D, ei, M in pg:
        try:
            E = rmcf.MCF_PGSE('cylinder', L, D, scheme=scheds[si], envdir=envs["zxo"[ei]], gamma=GAMMA, M=M)
        except ValueError:
            continue                     # fails the q/p accuracy check: not a signal case
        cases.append((si, L, D, ei, M))
        sigs.append(E)
        offs.append(offs[-1] + E.size)
        print("PGSE", si, L, D, ei, M, "ok", flush=True)
    out["pgse_cases"] = np.array(cases, dtype=np.float64)
    out["pgse_sig"] = np.concatenate(sigs)
    out["pgse_off"] = np.array(offs, dtype=np.int64)
    # non-scheme mode
    Gn = np.array([0.0, 0.02, 0.05, 0.08, 0.03])
    Dn = np.array([0.03, 0.03, 0.04, 0.02, 0.05])
    dn = np.array([0.01, 0.005, 0.02, 0.02, 0.001])
    out["ns_G"], out["ns_Delta"], out["ns_delta"] = Gn, Dn, dn
    out["ns_sig"] = rmcf.MCF_PGSE('c', 3e-6, 2e-9, G=Gn, Delta=Dn, delta=dn, gamma=GAMMA)
    # DDE cases: (L, D, envdir id, M)
    dc, dsig = [], []
    for L, D, ei, M in ((1e-6, 2e-9, 0, 60), (3e-6, 1.7e-9, 0, 60), (5e-6, 1e-9, 2, 60), (2e-6, 3e-9, 1, 60),
                        (3e-6, 1.7e-9, 0, 20)):
        dsig.append(rmcf.MCF_DDE('cylinder', L, D, dde, envdir=envs["zxo"[ei]], gamma=GAMMA, M=M))
        dc.append((L, D, ei, M))
        print("DDE", L, D, ei, M, "ok", flush=True)
    out["dde_cases"] = np.array(dc, dtype=np.float64)
    out["dde_sig"] = np.stack(dsig)
    # sphere / planes with no gradient at all: ones, no NotImplementedError
    out["sphere_nograd"] = rmcf.MCF_PGSE('sphere', 2e-6, 2e-9, G=[0.0, 0.0], Delta=[0.03, 0.03], delta=[0.01, 0.01])
    # invalid inputs
    named = {"sch_ukbb_2": ukbb[:2], "dde_2": dde[:2], "a_list": [1.0, 2.0]}
    errs = []
    for fn, kw in ERROR_CASES:
        try:
            getattr(rmcf, fn)(**resolve(kw, named))
            errs.append([fn, kw, None, None])
        except Exception as e:  # noqa: BLE001  (recording what the reference raises)
            errs.append([fn, kw, type(e).__name__, str(e)])
        print(fn, errs[-1][2], (errs[-1][3] or "")[:60], flush=True)
    out["errors_json"] = np.array(json.dumps(errs))
    np.savez_compressed(os.path.join(HERE, "mcf_cases.npz"), **out)
    print("wrote", os.path.join(HERE, "mcf_cases.npz"), os.path.getsize(os.path.join(HERE, "mcf_cases.npz")), "bytes")


if __name__ == "__main__":
    main()

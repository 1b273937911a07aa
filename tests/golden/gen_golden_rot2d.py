#!/usr/bin/env python3
"""Generate tests/golden/rot2d_cases.npz by RUNNING THE REFERENCE's rotate_atom_2Dprotocol and its helpers
(rotate_scheme_mat, vrrotvec2mat, rotate_vector, get_perp_vector, project_PGSE_scheme_xy_plane).

Runs only in the build container, next to gen_golden.py (whose import_reference() it uses).
Stored:
  - the reference's 2-D fixture scheme (1776 rows, 9 (Delta, delta) pairs, two lines at about +-45 deg) and two
    synthetic axis-aligned 2-D protocols (lines exactly along x and y; two b0 rows per pair, or one);
  - analytic atoms on them that vary along each line (signs included), 3 on the fixture to keep this file
    under 1 MB;
  - value groups: (scheme, signals, refdir, DIFF) with a batch of new directions and the reference's outputs;
  - error cases: inputs and the reference's exception type and message (replayed by tests/test_rot2d_*.py);
  - the helpers' outputs on a few inputs.
The reference normalises sch_mat's first two columns in place when refdir is along z, so every call gets copies.

Usage:  OPENBLAS_NUM_THREADS=1 python tests/golden/gen_golden_rot2d.py
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

GAM = 2 * np.pi * 42.577480e6
FIXTURE = os.path.join(gen_golden.REF, "tests", "integration", "fixtures", "2D_qspace_clean_rot_xy.scheme")


def atoms(sch, N, seed):
    """N smooth atoms for a fascicle along z: free-diffusion decay times a term odd along every line."""
    rng = np.random.default_rng(seed)
    G, Dl, dl = sch[:, 3], sch[:, 4], sch[:, 5]
    b = (GAM * G * dl) ** 2 * (Dl - dl / 3)
    D = rng.uniform(0.3e-9, 2.5e-9, N)
    a = rng.uniform(-0.2, 0.2, (2, N))
    return np.exp(-np.outer(b, D)) * (1 + np.outer(G * sch[:, 0], a[0]) / 0.1 + np.outer(G * sch[:, 1], a[1]) / 0.1)


def axis_protocol(nb0, pairs=((20e-3, 5e-3), (30e-3, 8e-3), (45e-3, 10e-3)), Gs=(0.01, 0.02, 0.035, 0.05, 0.065)):
    """Lines exactly along x and y, both polarities, nb0 b0 rows per (Delta, delta) pair."""
    rows = []
    for Del, dl in pairs:
        TE = Del + dl + 10e-3
        rows += [[0, 0, 0, 0, Del, dl, TE]] * nb0
        for G in Gs:
            for g in ((1, 0), (-1, 0), (0, 1), (0, -1)):
                rows.append([g[0], g[1], 0, G, Del, dl, TE])
    return np.array(rows, dtype=np.float64)


def unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.sqrt(np.sum(v ** 2))


def random_dirs(rng, n, zmin):
    out = []
    while len(out) < n:
        d = unit(rng.standard_normal(3))
        if abs(d[2]) >= zmin:
            out.append(d)
    return np.array(out)


def call(mfu, sch, sig, refdir, newdir, DIFF):
    try:
        return mfu.rotate_atom_2Dprotocol(sig.copy(), sch.copy(), np.array(refdir, dtype=np.float64),
                                          np.array(newdir, dtype=np.float64), DIFF), None
    except Exception as e:  # noqa: BLE001  (recording what the reference raises)
        return None, [type(e).__name__, str(e)]


def main():
    mfu, _ = gen_golden.import_reference()
    rng = np.random.default_rng(20261016)
    out = {}
    fix = np.loadtxt(FIXTURE, skiprows=1)
    syn2, syn1 = axis_protocol(2), axis_protocol(1)
    arrays = {"fix_sch": fix, "syn2_sch": syn2, "syn1_sch": syn1,
              "fix_sig": atoms(fix, 3, 1), "syn2_sig": atoms(syn2, 6, 2), "syn1_sig": atoms(syn1, 6, 3)}
    arrays["syn2_sig1"] = arrays["syn2_sig"][:, 0].copy()
    z, x, y = np.eye(3)[2], np.eye(3)[0], np.eye(3)[1]
    o1, o2 = unit([0.3, -0.2, 0.93]), unit([-0.5, 0.4, 0.77])
    DIFF = 2.2e-9
    groups = [
        ("fix", "fix_sig", z, np.vstack([z, -z, x, y, random_dirs(rng, 8, 0.05)])),
        ("fix", "fix_sig", o1, random_dirs(rng, 4, 0.05)),
        ("fix", "fix_sig", o2, random_dirs(rng, 4, 0.05)),
        ("syn2", "syn2_sig", z, np.vstack([z, -z, x, y, -x, unit([1, 0, 1]), random_dirs(rng, 6, 0.05)])),
        ("syn2", "syn2_sig", o1, np.vstack([x, y, random_dirs(rng, 4, 0.05)])),
        ("syn1", "syn1_sig", z, np.vstack([x, y, -y, random_dirs(rng, 4, 0.05)])),
        ("syn2", "syn2_sig1", z, np.vstack([x, random_dirs(rng, 3, 0.05)])),
    ]
    vals, errs = [], []
    for gi, (sk, gk, refdir, dirs) in enumerate(groups):
        ok_dirs, outs = [], []
        for d in dirs:
            r, e = call(mfu, arrays[sk + "_sch"], arrays[gk], refdir, d, DIFF)
            if e is None:
                ok_dirs.append(d)
                outs.append(r)
            else:
                errs.append({"sch": sk + "_sch", "sig": gk, "refdir": list(refdir), "newdir": list(d), "DIFF": DIFF,
                             "type": e[0], "msg": e[1], "host": False, "why": "group %d direction" % gi})
            print("group", gi, np.round(d, 3), "ok" if e is None else e[1][:70], flush=True)
        out["val%d_dirs" % gi] = np.array(ok_dirs)
        out["val%d_out" % gi] = np.array(outs)
        vals.append({"sch": sk + "_sch", "sig": gk, "refdir": list(refdir), "DIFF": DIFF, "n": len(ok_dirs)})
    # error cases with inputs of their own
    bad = {}
    gz = syn2.copy()
    gz[7, 2] = 0.1
    bad["gz_sch"] = gz
    bad["rows_sig"] = arrays["syn2_sig"][:-1]
    nob0 = np.array([r for r in syn2 if not (r[3] == 0 and r[4] == 30e-3)])   # pair 2 without b0 rows
    bad["nob0_sch"], bad["nob0_sig"] = nob0, atoms(nob0, 3, 4)
    three = syn2.copy()
    sel = (three[:, 4] == 45e-3) & (three[:, 0] == 0) & (three[:, 3] > 0.03)
    three[np.where(sel)[0][:2], 0:2] = [[0.6, 0.8], [-0.6, -0.8]]             # pair 3: a third line
    bad["three_sch"], bad["three_sig"] = three, atoms(three, 3, 5)
    order = syn2.copy()
    order[1, 0] = 1.0                                                             # pair 1: a b0 row on the x line
    order = np.array([r for r in order if not (r[3] == 0 and r[4] == 30e-3)])     # pair 2: no b0 row
    bad["order_sch"], bad["order_sig"] = order, atoms(order, 3, 6)
    cases = [
        ("gz_sch", "syn2_sig", z, o1, True, "gz != 0"),
        ("syn2_sch", "rows_sig", z, o1, True, "row count"),
        ("syn2_sch", "syn2_sig", z, [0.0, 0.6, 0.6], True, "non-unit newdir"),
        ("syn2_sch", "syn2_sig", [0.0, 0.6, 0.6], o1, True, "non-unit refdir"),
        ("syn2_sch", "syn2_sig", z, [0.0, 1.0], True, "newdir with 2 entries"),
        ("nob0_sch", "nob0_sig", z, o1, False, "pair without b0 rows: 4 unique"),
        ("three_sch", "three_sig", z, o1, False, "three lines: 7 unique"),
        ("fix_sch", "fix_sig", z, unit([1, 1, 0]), False, "in-plane new fascicle: 4 pairs"),
        ("order_sch", "order_sig", z, z, False, "new-side failure in pair 1 before reference-side one in pair 2"),
    ]
    allarr = dict(arrays, **bad)
    for sk, gk, refdir, d, host, why in cases:
        r, e = call(mfu, allarr[sk], allarr[gk], refdir, d, DIFF)
        assert e is not None, why
        errs.append({"sch": sk, "sig": gk, "refdir": list(map(float, refdir)), "newdir": list(map(float, d)),
                     "DIFF": DIFF, "type": e[0], "msg": e[1], "host": host, "why": why})
        print("error", why, "->", e[0], e[1][:90], flush=True)
    # helpers
    hel = {}
    hel["rsm_in"] = fix[::37].copy()
    hel["rsm_dirs"] = np.vstack([z, -z, x, o1, o2, unit([1, 1, 0])])
    hel["rsm_out"] = np.array([mfu.rotate_scheme_mat(hel["rsm_in"].copy(), z, d) for d in hel["rsm_dirs"]])
    hel["rsm_pair_out"] = mfu.rotate_scheme_mat(hel["rsm_in"].copy(), o1, o2)
    hel["vrm_axes"] = np.vstack([x, unit([1, 2, 3]), unit([-1, 0.5, 0])])
    hel["vrm_theta"] = np.array([0.3, -1.2, 2.5])
    hel["vrm_out"] = np.array([mfu.vrrotvec2mat(a, t) for a, t in zip(hel["vrm_axes"], hel["vrm_theta"])])
    hel["rv_v"] = np.array([[1.0, 2.0, 3.0], [0.0, 0.0, 1.0], [-0.3, 0.2, 0.9]])
    hel["rv_out"] = np.array([mfu.rotate_vector(v, a, t) for v, a, t in zip(hel["rv_v"], hel["vrm_axes"], hel["vrm_theta"])])
    hel["gpv_in"] = np.array([[1.0, 0.0, 2.0, -1.0], [2.0, 0.0, 0.0, 3.0], [3.0, 1.0, 1.0, 0.5]])
    hel["gpv_out"] = mfu.get_perp_vector(hel["gpv_in"].copy())
    sch3 = gen_golden.synth_scheme(np.random.default_rng(7), 3, [1000, 2500], [12, 12])
    hel["proj_in"] = sch3
    hel["proj_out"] = mfu.project_PGSE_scheme_xy_plane(sch3.copy())
    helper_errs = []
    for fn, args in (("vrrotvec2mat", ([1.0, 0.0], 0.1)), ("vrrotvec2mat", ([1.0, 1.0, 0.0], 0.1)),
                     ("rotate_vector", ([1.0, 0.0, 0.0], [1.0, 1.0, 0.0], 0.1)),
                     ("rotate_scheme_mat", ("rsm_in", [0.0, 0.0, 1.0], [0.0, 1.0])),
                     ("rotate_scheme_mat", ("rsm_in", [0.0, 0.0, 1.0], [0.0, 1.0, 1.0]))):
        a = [hel[v].copy() if isinstance(v, str) else (np.array(v) if isinstance(v, list) else v) for v in args]
        try:
            getattr(mfu, fn)(*a)
            raise SystemExit("%s%r did not raise" % (fn, args))
        except Exception as e:  # noqa: BLE001
            helper_errs.append([fn, list(args), type(e).__name__, str(e)])
    # a scheme file for project_PGSE_scheme_xy_plane's path argument is written by the test itself
    out.update(arrays)
    out.update(bad)
    out.update(hel)
    out["values_json"] = np.array(json.dumps(vals))
    out["errors_json"] = np.array(json.dumps(errs))
    out["helper_errors_json"] = np.array(json.dumps(helper_errs))
    path = os.path.join(HERE, "rot2d_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

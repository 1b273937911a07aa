#!/usr/bin/env python3
"""Generate tests/golden/rot2d_wide.npz by RUNNING THE REFERENCE's rotate_atom_2Dprotocol on whole populations of
new fascicle directions: per (protocol, reference direction) 256 directions uniform on the sphere (no zmin) and a
list of edge directions, each with its outcome (success, or exception type and message).

Runs only in the build container, next to gen_golden.py (whose import_reference() it uses) and
gen_golden_rot2d.py (whose atoms() and protocols it reuses; the fixture, syn2 and syn1 are read from
rot2d_cases.npz, not stored again).  Only data is written.

Protocols:  fix, syn2, syn1 (rot2d_cases.npz) and
  A  "long and interleaved": lines at 30 and 100 degrees, both polarities; pair (20 ms, 5 ms) with 70 strengths from
     0.005 to 0.08 T/m, pair (35 ms, 8 ms) with 15; three b0 rows per pair; six DW rows repeated (interior
     strengths, so that no zero-width interval is an end interval); all rows permuted: 352 rows, pairs of 287 and 65.
     Its atoms are atoms() times 1 + 1e-3 N(0, 1) per entry, so that repeated rows carry different signals.
  B  "minimal": one pair, one b0 row, two lines, five strengths: 21 rows.
  C  "at the limit": 4000 rows in four pairs of 1000 (4 b0 rows + 249 strengths on two lines, both polarities),
     rows permuted, N = 2.

Values.  The reference's outputs are stored for every successful edge direction and the first 24 successful random
ones (A, B, syn1, syn2; 4 atoms) or for 8 directions (fix, C).  Whole [M, N] outputs of all of them would be 5 MB;
the file has to stay under 1 MB, so each stored direction keeps the outputs of a seeded random subset of rows of
its own (<key>_vrows), all rows for B.  The referee of tests/_rot2d_ref.py covers the rows in between.

Usage:  OPENBLAS_NUM_THREADS=1 python tests/golden/gen_golden_rot2d_wide.py
"""
import json
import os
import sys

os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
os.environ.setdefault("OMP_NUM_THREADS", "1")

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_golden  # noqa: E402
import gen_golden_rot2d as g2  # noqa: E402
import _rot2d_ref as ref2d  # noqa: E402

DIFF = 2.2e-9
NRAND = 256
VAL_ROWS = {"fix": 96, "syn2": 24, "syn1": 24, "A": 48, "B": 21, "C": 128}
VAL_ATOMS = {"fix": 3, "syn2": 4, "syn1": 4, "A": 4, "B": 4, "C": 2}
EDGE_NAMES = ["+z", "-z", "line1", "line1 tilted 1e-9", "line2", "line2 tilted 1e-9", "in-plane perpendicular of line1",
              "|z| = 0.004", "|z| = 1e-4", "unit(6e-10, 8e-10, 1)", "(0.6, 0, 0.8) (1 + 2e-6)", "(0.6, 0, 0.8) (1 - 2e-6)",
              "(0.6, 0, 0.8) (1 + 6e-6)", "in-plane at 0.4 rad"]


def line_protocol(angles_deg, pairs, nb0, repeats=()):
    """pairs: ((Delta, delta, strengths), ...); repeats: (pair index, line index, polarity, strength index)"""
    lines = [(np.cos(np.deg2rad(a)), np.sin(np.deg2rad(a))) for a in angles_deg]
    rows = []
    for pi, (Del, dl, Gs) in enumerate(pairs):
        TE = Del + dl + 10e-3
        rows += [[0, 0, 0, 0, Del, dl, TE]] * nb0
        for G in Gs:
            for lx, ly in lines:
                rows.append([lx, ly, 0, G, Del, dl, TE])
                rows.append([-lx, -ly, 0, G, Del, dl, TE])
        for rp, li, pol, gi in repeats:
            if rp == pi:
                rows.append([pol * lines[li][0], pol * lines[li][1], 0, Gs[gi], Del, dl, TE])
    return np.array(rows, dtype=np.float64)


def protocols():
    rng = np.random.default_rng(20261019)
    A = line_protocol((30, 100), ((20e-3, 5e-3, np.linspace(0.005, 0.08, 70)), (35e-3, 8e-3, np.linspace(0.01, 0.07, 15))),
                      3, repeats=((0, 0, 1, 10), (0, 0, -1, 33), (0, 1, 1, 0), (0, 1, -1, 51), (1, 0, 1, 7), (1, 1, -1, 3)))
    A = A[rng.permutation(A.shape[0])]
    B = line_protocol((10, 75), ((25e-3, 6e-3, np.array([0.01, 0.02, 0.035, 0.05, 0.065])),), 1)
    C = line_protocol((20, 110), tuple((Del, dl, np.linspace(0.004, 0.075, 249)) for Del, dl in
                                       ((18e-3, 4e-3), (25e-3, 6e-3), (32e-3, 8e-3), (40e-3, 10e-3))), 4)
    C = C[rng.permutation(C.shape[0])]
    assert A.shape[0] == 352 and B.shape[0] == 21 and C.shape[0] == 4000
    assert sorted(np.unique(A[:, 4], return_counts=True)[1].tolist()) == [65, 287]
    sigA = g2.atoms(A, 4, 11) * (1 + 1e-3 * rng.standard_normal((A.shape[0], 4)))
    return {"A_sch": A, "A_sig": sigA, "B_sch": B, "B_sig": g2.atoms(B, 4, 12), "C_sch": C, "C_sig": g2.atoms(C, 2, 13)}


def lines_of(sch):
    """the protocol's two in-plane line directions (unit 3-vectors)"""
    g = sch[sch[:, 3] > 0, 0:2]
    g = g / np.sqrt(np.sum(g ** 2, axis=1, keepdims=True))
    l1 = g[0]
    l2 = next(v for v in g if abs(v[0] * l1[1] - v[1] * l1[0]) > 1e-3)
    return np.array([l1[0], l1[1], 0.0]), np.array([l2[0], l2[1], 0.0])


def edge_dirs(sch):
    z = np.array([0.0, 0.0, 1.0])
    l1, l2 = lines_of(sch)

    def low(zc, phi=0.7):
        s = np.sqrt(1 - zc * zc)
        return np.array([s * np.cos(phi), s * np.sin(phi), zc])
    base = np.array([0.6, 0.0, 0.8])
    out = [z, -z, l1, g2.unit(l1 + 1e-9 * z), l2, g2.unit(l2 + 1e-9 * z), np.array([-l1[1], l1[0], 0.0]), low(0.004),
           low(-1e-4, 2.1), g2.unit([6e-10, 8e-10, 1.0]), base * (1 + 2e-6), base * (1 - 2e-6), base * (1 + 6e-6),
           np.array([np.cos(0.4), np.sin(0.4), 0.0])]
    assert len(out) == len(EDGE_NAMES)
    return np.array(out)


def main():
    mfu, _ = gen_golden.import_reference()
    cases = np.load(os.path.join(HERE, "rot2d_cases.npz"))
    arrays = protocols()
    full = dict(arrays)
    for k in ("fix", "syn2", "syn1"):
        full[k + "_sch"], full[k + "_sig"] = cases[k + "_sch"], cases[k + "_sig"][:, :VAL_ATOMS[k]]
    z = np.array([0.0, 0.0, 1.0])
    o1 = g2.unit([0.3, -0.2, 0.93])
    out = dict(arrays)
    combos, outcomes, shares = [], {}, {}
    for pi, proto in enumerate(("fix", "syn2", "syn1", "A", "B", "C")):
        sch, sig = full[proto + "_sch"], full[proto + "_sig"]
        refs = [("z", z), ("mz", -z), ("o1", o1)]
        if proto == "A":
            refs.append(("line1", lines_of(sch)[0]))
        for ri, (rname, refdir) in enumerate(refs):
            key = "%s_%s" % (proto, rname)
            rng = np.random.default_rng([20261019, pi, ri])
            rand = rng.standard_normal((NRAND, 3))
            rand /= np.sqrt(np.sum(rand ** 2, axis=1, keepdims=True))
            edge = edge_dirs(sch)
            dirs = np.vstack([edge, rand])
            R = ref2d.Referee(sig, sch, refdir, DIFF)
            results, errs, unclear, disagree = [], {}, [], []
            for k, d in enumerate(dirs):
                r, e = g2.call(mfu, sch, sig, refdir, d, DIFF)
                results.append(r)
                if e is not None:
                    errs[str(k)] = e
                q = R.rotate(d)
                if not q.clear:
                    unclear.append((k, q.unclear))
                elif (q.error is None) != (e is None) or (e is not None and list(q.error) != e):
                    disagree.append((k, q.error, e))
            ok = np.array([r is not None for r in results])
            n_edge = edge.shape[0]
            okE = [k for k in range(n_edge) if ok[k]]
            okR = [k for k in range(n_edge, dirs.shape[0]) if ok[k]]
            vidx = (okE + okR[:24]) if proto in ("A", "B", "syn1", "syn2") else \
                ([k for k in (2, 3, 7, 9, 0, 1, 4, 5) if ok[k]][:4] + okR[:4])
            nr = VAL_ROWS[proto]
            vrows = np.array([np.sort(rng.choice(sch.shape[0], nr, replace=False)) for _ in vidx]).reshape(len(vidx), nr)
            val = np.array([results[k][vrows[i]] for i, k in enumerate(vidx)])
            out[key + "_dirs"] = dirs
            out[key + "_ok"] = ok
            out[key + "_vidx"] = np.array(vidx, dtype=np.int32)
            out[key + "_vrows"] = vrows.astype(np.int32)
            out[key + "_val"] = val
            outcomes[key] = errs
            combos.append({"key": key, "proto": proto, "refdir": list(map(float, refdir)), "n_edge": n_edge,
                           "atoms": VAL_ATOMS[proto]})
            un_rand = sum(1 for k, _ in unclear if k >= n_edge)
            shares[key] = un_rand / NRAND
            print(key, "fail %d/%d" % (int((~ok).sum()), ok.size), "unclear random %d (%.2f %%)" % (un_rand, 100 * shares[key]),
                  "unclear edge", [(EDGE_NAMES[k], w) for k, w in unclear if k < n_edge],
                  "referee disagrees", disagree, flush=True)
            assert un_rand <= 0.02 * NRAND, "the clearance bands are too wide"
    out["combos_json"] = np.array(json.dumps(combos))
    out["outcomes_json"] = np.array(json.dumps(outcomes))
    out["edge_names_json"] = np.array(json.dumps(EDGE_NAMES))
    out["DIFF"] = np.array(DIFF)
    path = os.path.join(HERE, "rot2d_wide.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    main()

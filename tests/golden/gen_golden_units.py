#!/usr/bin/env python3
"""Generate tests/golden/units_cases.npz by RUNNING THE REFERENCE's solve_exhaustive_posweights on dictionaries and
signals stored in other units:  solve_exhaustive_posweights(A * c, y * cy, sizes).

The reference never normalises a dictionary or a signal, and its Cramer tests compare determinants against an ABSOLUTE
tolerance (mf_utils.py:480-481, 562: D >= -100 eps) although they scale as |y| |d|^5.  With q = log2(cy) + 5 log2(c):
around q = 0 the tolerance is inert and the reference is equivariant (w -> w cy / c, min_obj -> min_obj cy^2); once q
falls to about -40 the tolerance accepts unconstrained solutions and the reference returns NEGATIVE weights.  This
fixture pins the reference on both sides, so that the CPU oracle - which referees the GPU at these units - is itself
refereed there (tests/test_units_host.py: bit for bit, negative weights included).

Problems: sub-dictionary sizes [24, 24], [24, 24, 1], [16, 16, 16], [12, 12, 1, 3] on a 62-row protocol (2 b0 + 3 shells
of 20 directions), atoms with S0 ~ 1 rotated to random directions, a CSF-like column and three EAR-like columns, six
signals each near 500 at SNR 30 (the second with one weight zero).  Stored: the BASELINE A and y of every problem, the
unit pairs, and per (problem, signal, unit pair) the reference's w, sub-indices, min_obj and y_recons.

Runs only in the build container, next to gen_golden.py (whose import_reference() it uses).  The archive is written
with fixed time stamps: it regenerates byte for byte.

Usage:  OPENBLAS_NUM_THREADS=1 python tests/golden/gen_golden_units.py
"""
import io
import os
import sys
import zipfile

os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
os.environ.setdefault("OMP_NUM_THREADS", "1")

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden  # noqa: E402

# (c, cy): dictionary and signal units.  q = log2(cy) + 5 log2(c)
UNITS = [(1.0, 1.0),                      # q = 0     baseline
         (2.0 ** 16, 1.0),                # q = 80    inert
         (2.0 ** -10, 2.0 ** 34),         # q = -16   inert
         (1e4, 1.0),                      # q = 66.4  inert, not a power of two
         (1e-3, 1e10),                    # q = -16.6 inert, not a power of two
         (2.0 ** -10, 1.0),               # q = -50   tolerance regime
         (2.0 ** -14, 1.0),               # q = -70   tolerance regime
         (2.0 ** -20, 1.0)]               # q = -100  tolerance regime
PROBLEMS = [("k2", [24, 24]), ("k2c", [24, 24, 1]), ("k3", [16, 16, 16]), ("k4", [12, 12, 1, 3])]
NSIG = 6
M0, SNR = 500.0, 30.0


def save_npz(path, arrays):
    """np.savez_compressed with fixed time stamps and a fixed member order"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            zi = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            z.writestr(zi, buf.getvalue())


def main():
    mfu, _ = gen_golden.import_reference()
    rng = np.random.default_rng(20261019)
    sch = gen_golden.synth_scheme(rng, 2, [1000, 2000, 3000], [20, 20, 20])
    M = sch.shape[0]
    b = (gen_golden.GAM * sch[:, 3] * sch[:, 5]) ** 2 * (sch[:, 4] - sch[:, 5] / 3)
    csf = np.exp(-sch[:, 6] / 2.0) * np.exp(-b * 3e-9)
    ear = np.stack([np.exp(-sch[:, 6] / 0.08) * np.exp(-b * x) for x in (0.3e-9, 0.7e-9, 1.1e-9)], axis=1)
    out = {"units": np.array(UNITS), "names": np.array([p[0] for p in PROBLEMS]), "nsig": np.array(NSIG)}
    nneg = np.zeros(len(UNITS), dtype=int)
    for name, sizes in PROBLEMS:
        cols = []
        for k, sz in enumerate(sizes):
            if sz == 1:
                cols.append(csf[:, None])
            elif sz == 3:
                cols.append(ear)
            else:   # the same atoms for every fascicle, rotated to the fascicle's direction
                d = gen_golden.unit(rng, 1)[0]
                s = sch.copy()
                s[:, 2] = s[:, :3] @ d
                cols.append(gen_golden.synth_dictionary(np.random.default_rng(7), s, sz))
        A = np.ascontiguousarray(np.concatenate(cols, axis=1))
        ds = np.array(sizes)
        st = np.concatenate([[0], np.cumsum(sizes)[:-1]])
        Y = np.zeros((NSIG, M))
        for i in range(NSIG):
            gt = st + np.array([rng.integers(0, s) for s in sizes])
            nu = rng.dirichlet(np.ones(len(sizes)))
            if i == 1:
                nu[rng.integers(0, len(sizes))] = 0.0
            Y[i] = M0 * (A[:, gt] @ nu) + rng.normal(0, M0 / SNR, M)
        out[name + "_A"], out[name + "_Y"], out[name + "_sizes"] = A, Y, ds
        W = np.zeros((len(UNITS), NSIG, len(sizes)))
        SUB = np.zeros((len(UNITS), NSIG, len(sizes)), dtype=np.int64)
        OBJ = np.zeros((len(UNITS), NSIG))
        YREC = np.zeros((len(UNITS), NSIG, M))
        for u, (c, cy) in enumerate(UNITS):
            for i in range(NSIG):
                w, isub, _, mo, yr = mfu.solve_exhaustive_posweights(A * c, Y[i] * cy, ds)
                W[u, i], SUB[u, i], OBJ[u, i], YREC[u, i] = w, isub, mo, yr
                nneg[u] += bool(np.any(np.asarray(w) < 0))
        out[name + "_w"], out[name + "_sub"], out[name + "_obj"], out[name + "_yrec"] = W, SUB, OBJ, YREC
    path = os.path.join(HERE, "units_cases.npz")
    save_npz(path, out)
    for u, (c, cy) in enumerate(UNITS):
        print("c = %-12g cy = %-12g q = %6.1f: %d of %d results carry a negative weight"
              % (c, cy, np.log2(cy) + 5 * np.log2(c), nneg[u], NSIG * len(PROBLEMS)))
    print("units_cases.npz: %d bytes" % os.path.getsize(path))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generate tests/golden/mc_hp_cases.npz: 50-digit values of the Monte-Carlo phase average

    S = (1/n) sum_l cos(arg_l),     arg_l = fl(Ds * fl(fl(fl(g0 p0) + fl(g1 p1)) + fl(g2 p2)))

for the cases of tests/_mc_cases.py.  The argument is the float64 number the operation defines (computed by
_mc_cases.argument, one NumPy ufunc call per rounding); cos of that exact double, the sum and the division are
done with mpmath at 50 digits and rounded once to float64.  A sequence whose argument is not finite (an inf or
nan gradient scaling) has S = nan.

Stored, per case and in the order of _mc_cases.TABLE: S, A = (1/n) sum_l |cos(arg_l)| (the unit of the error bar),
and the SHA-256 of the case's input bytes, so that a NumPy whose generator stream differs fails loudly instead
of comparing other inputs.  No inputs are stored: the file stays a few kilobytes.

Usage:  python tests/golden/gen_golden_mc_hp.py          (about 5 s on 8 CPUs; at most 16 processes)
The module is also imported by tests/test_mc_referee_host.py, which recomputes part of the fixture.
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _mc_cases as mc  # noqa: E402

OUT = os.path.join(HERE, "mc_hp_cases.npz")
DPS = 50


def hp_mean(arg, dps=DPS):
    """(S, A) of one sequence as floats: the mean of cos(arg_l) and of |cos(arg_l)| at `dps` digits."""
    import mpmath as mp
    if not np.all(np.isfinite(arg)):
        return float("nan"), float("nan")
    with mp.workdps(dps):
        s, a = mp.mpf(0), mp.mpf(0)
        for x in arg.tolist():
            c = mp.cos(mp.mpf(x))
            s += c
            a += abs(c)
        return float(s / len(arg)), float(a / len(arg))


def _job(t):
    name, i = t
    c = mc.BY_NAME[name]
    return hp_mean(mc.argument(*mc.inputs(c))[i])


def check_coverage(d):
    """The coverage the fixture promises, counted from the case table and the stored arrays (d: load_golden's dict)."""
    T = mc.TABLE
    assert [c["name"] for c in T] == list(d), "the fixture's cases are not the table's"
    fam = lambda f: [c for c in T if c["family"] == f]  # noqa: E731
    for c in T:                                          # every case: acquisitions scaled apart, the last one used, one unused
        S, A, _ = d[c["name"]]
        _, dm, gs, _, n = mc.inputs(c)
        assert S.shape == A.shape == (len(dm),) and gs.shape == (len(dm), mc.case_dim(c))
        assert c["n_ref"] - 1 in set(dm.tolist())
        assert c["n_ref"] == 1 or len(set(dm.tolist())) < c["n_ref"], c["name"]
        assert c["n_ref"] > 1 or c["n_spin"] > 64 * mc.CHUNK
    lad = fam("ladder")
    assert {(c["scale"], c["Ds"]) for c in lad} == {(s, D) for s in mc.LADDER_SCALES for D in mc.LADDER_DS}
    assert mc.LADDER_SCALES == (1.0, 1e2, 1e4, 1e6, 1e12) and mc.LADDER_DS == (1.0, float(np.sqrt(2.0 / 3.0)))
    assert all(c["n_spin"] == 4099 and c["n_ref"] == 3 and c["dm"].size == 11 and c["dim"] == 3 for c in lad)
    for f, nbig in (("spin", 2), ("zero-g", 3)):
        assert [c["n_spin"] for c in fam(f)] == [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8193, 64 * 4096 + 1]
        assert all(c["scale"] == 1e4 and c["dim"] == 3 for c in fam(f))
        assert all((c["n_ref"], c["dm"].size) == ((2, 3) if c["n_spin"] < 10000 else (1, nbig))
                   for c in fam(f))
    assert -(-fam("spin")[-1]["n_spin"] // mc.CHUNK) == mc.WAVE + 1          # the finalize wave wraps once
    assert fam("spin")[-1]["n_spin"] * 3 * 8 <= 6.3e6                         # the largest upload
    for c in fam("zero-g"):
        assert np.all(d[c["name"]][0][[0, 2]] == 1.0) and d[c["name"]][0][1] != 1.0
    tile = fam("tile")
    assert all(c["n_spin"] == 257 for c in tile)
    count = lambda c: sorted(np.bincount(c["dm"])[np.bincount(c["dm"]) > 0].tolist())  # noqa: E731
    assert [count(c) for c in tile[:6]] == [[k] for k in (1, 7, 8, 9, 16, 17)]
    assert count(tile[6]) == count(tile[7]) == [1, 7, 8, 9, 16, 17]
    assert np.all(np.diff(tile[6]["dm"]) >= 0)
    dmi = tile[7]["dm"]
    order = np.argsort(dmi, kind="stable")
    assert np.all(np.diff(dmi) != 0) and np.mean(order == np.arange(order.size)) < 0.1, "the interleaved mapping is too tame"
    assert [c["dim"] for c in fam("dim")] == [1, 2, 3] and all(c["n_spin"] == 4097 and c["scale"] == 1e4 for c in fam("dim"))
    sp = {c["name"]: c for c in fam("special")}
    assert np.all(d["special:Ds0"][0] == 1.0) and sp["special:Ds0"]["Ds"] == 0.0
    ph = mc.raw_phases(sp["special:phase-zeros"])
    assert np.sum((ph == 0) & ~np.signbit(ph)) > 1000 and np.sum((ph == 0) & np.signbit(ph)) > 1000
    S = d["special:g-inf-nan"][0]
    gs = mc.inputs(sp["special:g-inf-nan"])[2]
    assert S.size == mc.TS and np.isnan(S[[3, 4]]).all() and np.isfinite(np.delete(S, [3, 4])).all()
    assert np.isinf(gs[3]).sum() == 1 and np.isnan(gs[4]).sum() == 1 and np.isfinite(np.delete(gs, [3, 4], axis=0)).all()
    pg = fam("pgse")
    assert [c["pgse"]["ext"] for c in pg[:4]] == ["bfloat", "lsingle", "ldouble", "bsingle"]
    assert all(c["n_spin"] == 4097 and c["pgse"]["sch_sim"].shape == (3, 7) and c["pgse"]["sch_new"].shape == (10, 7) for c in pg)
    dup = mc.BY_NAME["pgse:dup"]["pgse"]
    assert np.array_equal(dup["sch_sim"][0, 4:6], dup["sch_sim"][2, 4:6]) and not np.array_equal(dup["sch_sim"][0, :4], dup["sch_sim"][2, :4])
    assert set(mc.inputs(mc.BY_NAME["pgse:dup"])[1].tolist()) == {1, 2}
    d2 = mc.BY_NAME["pgse:dim2"]["pgse"]
    assert d2["kwargs"] == dict(dim=2, D_sim=3.0e-9, D=2.0e-9) and np.all(d2["sch_new"][:, 2] != 0)


def main():
    import multiprocessing as mpr
    t0 = time.time()
    jobs = [(c["name"], i) for c in mc.TABLE for i in range(len(mc.inputs(c)[1]))]
    jobs.sort(key=lambda t: -mc.BY_NAME[t[0]]["n_spin"])
    with mpr.Pool(min(16, os.cpu_count() or 1)) as pool:
        res = dict(zip(jobs, pool.map(_job, jobs, chunksize=1)))
    # an 80-digit repeat of one sequence per ladder rung: the 50 digits are enough
    for c in mc.TABLE:
        if c["family"] == "ladder" and c["Ds"] != 1.0:
            S80, _ = hp_mean(mc.argument(*mc.inputs(c))[0], 80)
            if S80 != res[(c["name"], 0)][0]:
                raise SystemExit("50-digit and 80-digit means differ for %s: fixture not written" % c["name"])
    names, off, S, A, sha = [], [0], [], [], []
    for c in mc.TABLE:
        n = len(mc.inputs(c)[1])
        names.append(c["name"])
        S += [res[(c["name"], i)][0] for i in range(n)]
        A += [res[(c["name"], i)][1] for i in range(n)]
        off.append(len(S))
        sha.append(mc.checksum(c))
    np.savez_compressed(OUT, names=np.array(names), offsets=np.array(off, dtype=np.int64), S=np.array(S), A=np.array(A),
                        sha256=np.array(sha))
    check_coverage(mc.load_golden(OUT))
    print("wrote %s: %d cases, %d sequences, %d bytes, %.0f s" % (OUT, len(names), len(S), os.path.getsize(OUT), time.time() - t0))


if __name__ == "__main__":
    main()

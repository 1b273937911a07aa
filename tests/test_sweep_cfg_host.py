"""The cases of tests/_sweep_cfg_cases.py, checked on the host: no GPU and nothing of the library.

1. the input condition of every comparison (tests/_post_ref.py's clear_of_the_cut) on the referee's 1 - c^2, plain and
   CSF-projected, of every (protocol, weights) block: it covers every row, whose pairs are a leading sub-block;
2. the Python restatement of the kernels' LDS formula reproduces the limits DESIGN.md 4.12, 4.15 and 4.16 print and the
   table of 4.16b;
3. every row's N lies inside the interval of the configuration it is meant for, and the rows name all 78 K = 2 kernels
   and the 8 K = 1 kernels (the GPU test learns from the library's hook whether the library agrees);
4. the float64 NumPy restatement of the referee stays inside the derived bars on these inputs.
"""
import numpy as np
import pytest

import _post_ref as R
import _sweep_cfg_cases as S

LD, EPS = R.LD, R.EPS

# largest dictionary (atoms) per configuration; None: the configuration is not on the path
TABLE = {
    ("post", 0, 0): (1056, 2176, 2720, 1520), ("post", 0, 1): (768, 1616, 2016, 1072),
    ("post", 1, 0): (880, 2016, 2544, 1056), ("post", 1, 1): (None, 1488, 1888, 720),
    ("prof", 0, 0): (848, 1984, 2480, 1376), ("prof", 0, 1): (None, 1488, 1872, 976),
    ("prof", 1, 0): (None, 1840, 2320, 944), ("prof", 1, 1): (None, 1376, 1760, 656),
    ("land", 0, 0): (1712, 3312, 4112, 2320), ("land", 0, 1): (None, 2176, 2704, 1440),
    ("land", 1, 0): (None, 3056, 3856, 1616), ("land", 1, 1): (None, 2000, 2544, 976),
}


@pytest.mark.parametrize("wgt", [False, True])
@pytest.mark.parametrize("proto", S.PROTOS)
def test_no_pair_near_the_cut(proto, wgt):
    """A condition on the inputs, not something to relax: a seed that fails it is replaced."""
    c2s = S.block_c2(proto, wgt)
    n = S.n_block(proto)
    assert c2s[0].shape == (n, n)
    print("%s%s: %d atoms, M = %d: smallest 1 - c^2 = %.3g plain, %.3g with the CSF column projected out"
          % (proto, " weighted" if wgt else "", n, S.M_of(proto), float(c2s[0].min()), float(c2s[1].min())))
    assert R.clear_of_the_cut(c2s, S.CUT)
    assert min(float(c.min()) for c in c2s) > 4 * S.CUT
    if proto == "short":   # the K = 1 rows: an atom against the CSF column
        b = S.block(proto, wgt)
        c2 = 1 - b["X1"] ** 2 / (b["A11"] * b["xx"])
        print("%s%s, one fascicle: smallest 1 - c^2 of an atom and the CSF column = %.3g" % (proto, " weighted" if wgt else "", float(c2.min())))
        assert R.clear_of_the_cut([c2], S.CUT) and float(c2.min()) > 4 * S.CUT


def test_protocols_are_what_the_cases_need():
    assert S.M_of("short") == S.M_of("short_br") == 23 and 200 < S.M_of("long") == S.M_of("long_br") <= 210
    for b in ("short", "long"):
        ms, br = S.scheme(b), S.scheme(b + "_br")
        Gs = np.unique(ms[:, 3])
        assert Gs.size == 4 and Gs[0] == 0
        moved = np.flatnonzero(br[:, 3] != ms[:, 3])
        nz = np.flatnonzero(ms[:, 3] > 0)
        assert moved.size == (nz.size + 1) // 2 and np.array_equal(np.delete(br, 3, 1), np.delete(ms, 3, 1))
        # strictly between two table shells, never on one
        assert np.all((br[moved, 3] > Gs[1]) & (br[moved, 3] < Gs[3])) and not np.isin(br[moved, 3], Gs).any()
        assert S.pool(b).shape == (ms.shape[0], S.POOL)
    pk = [S.peaks(p) for p in S.PROTOS]
    for p in pk:
        assert abs(np.linalg.norm(p[:3]) - 1) < 1e-12 and abs(np.linalg.norm(p[3:]) - 1) < 1e-12 and abs(p[:3] @ p[3:]) < 0.99
    for p in S.PROTOS:
        W = S.weights(p)
        assert W.min() == 0.0 and 0 < np.count_nonzero(W == 0) < W.size / 2 and W.max() <= 4.0


def test_lds_formula_reproduces_the_printed_limits():
    for (kind, br, csf), want in TABLE.items():
        got = tuple(S.cfg_max(kind, c, bool(br), bool(csf), False) for c in range(4))
        for c in range(4):
            if want[c] is not None:
                assert got[c] == want[c], (kind, br, csf, c, got)
        # the weighted forms hold 16 to 160 atoms fewer
        for c in range(4):
            d = got[c] - S.cfg_max(kind, c, bool(br), bool(csf), True)
            assert 16 <= d <= 160, (kind, br, csf, c, d)
    # include/mfx_profile.h and DESIGN.md 4.12: exact-G profile 2480 atoms for M <= 200, 1872 with CSF; 1376 and 976 for M <= 560
    assert [S.max_atoms("prof", M, False, c, False) for M in (200, 560) for c in (False, True)] == [2480, 1872, 1376, 976]
    # the posterior at M = 200: 2720 and 2016; never below the profile's
    assert [S.max_atoms("post", 200, False, c, False) for c in (False, True)] == [2720, 2016]
    for M in (23, 200, 203, 560):
        for br in (False, True):
            for csf in (False, True):
                for wgt in (False, True):
                    assert S.max_atoms("post", M, br, csf, wgt) >= S.max_atoms("prof", M, br, csf, wgt)
                    assert S.max_atoms("land", M, br, csf, wgt) >= S.max_atoms("post", M, br, csf, wgt)
    # pick() walks the path: below, at and above every boundary
    for kind in S.KINDS:
        for M in (23, 203):
            for br in (False, True):
                for csf in (False, True):
                    p = S.path(M, br, csf)
                    for c in p:
                        lo, hi = S.interval(kind, M, br, csf, False, c)
                        assert lo <= hi and S.pick(kind, M, br, csf, False, lo) == c and S.pick(kind, M, br, csf, False, hi) == c
                    assert S.pick(kind, M, br, csf, False, S.max_atoms(kind, M, br, csf, False) + 16) == -1


def test_rows_reach_every_kernel():
    rows, k1 = S.rows(), S.k1_rows()
    names = {S.kernel_name(r) for r in rows}
    assert len(names) == 78 and len({S.kernel_name(r) for r in k1}) == 8 and len(names | {S.kernel_name(r) for r in k1}) == 86
    # 13 forms per family and weighting, 26 posterior and 52 profile kernels
    assert sum(n[1] == "post" for n in names) == 26 and sum(n[1] == "prof" for n in names) == 52
    assert len({r["id"] for r in rows}) == len(rows) and len({r["seed"] for r in rows}) == len(rows)
    nlimit = 0
    for r in rows:
        M, br = S.M_of(r["proto"]), S.is_br(r["proto"])
        NP = (r["N"] + 15) // 16 * 16
        lo, hi = S.interval(r["kind"], M, br, r["csf"], r["wgt"], r["cfg"])
        assert lo <= NP <= hi, r["id"]
        assert S.pick(r["kind"], M, br, r["csf"], r["wgt"], NP) == r["cfg"], r["id"]
        assert r["form"][:4] == S.SWEEP_CFG[r["cfg"]] and r["form"][4:] == (int(br), int(r["csf"]), int(r["kind"] == "land"), int(r["wgt"]))
        assert r["N"] <= S.n_block(r["proto"]) <= S.POOL
        if r["limit"]:
            nlimit += 1
            assert r["N"] == hi == S.max_atoms(r["kind"], M, br, r["csf"], r["wgt"]) and S.SWEEP_CFG[r["cfg"]][3] == 1
        else:
            assert r["N"] % 16 != 0   # a padded last tile
    # every NBUF = 1 form has its limit row: the 24 of the table and their weighted twins
    assert nlimit == 48 and len(rows) == 78 + 48
    got = {(r["kind"], int(S.is_br(r["proto"])), int(r["csf"]), r["cfg"]): r["N"] for r in rows if r["limit"] and not r["wgt"]}
    for (kind, br, csf), want in TABLE.items():
        assert got[(kind, br, csf, 2)] == want[2] and got[(kind, br, csf, 3)] == want[3]
    for r in k1:
        assert r["N"] == S.POOL and r["proto"] == "short"


def _f64_rows():
    """one row per (family, protocol, CSF, weights): the form's own row with the fewest atoms"""
    best = {}
    for r in S.rows():
        key = (r["kind"], r["proto"], r["csf"], r["wgt"])
        if not r["limit"] and (key not in best or r["N"] < best[key]["N"]):
            best[key] = r
    return list(best.values())


@pytest.mark.parametrize("row", _f64_rows(), ids=lambda r: r["id"])
def test_float64_restatement_of_the_referee_stays_within_the_bar(row):
    """The referee's formulas in float64 NumPy against their long-double form: every bar the GPU test holds the kernels to
    has to hold for plain float64 arithmetic with a wide margin, or it is no bar for the kernels."""
    ref, f64 = S.referee(row), S.referee(row, dt=np.float64)
    assert not ref["below"].any() and np.array_equal(ref["below"], f64["below"])
    M, ysq, F = ref["M"], ref["ysq"], ref["F"]
    if row["kind"] == "land":
        ratio = float(np.max(np.abs(f64["F"].astype(LD) - F) / (16 * M * EPS * ysq / ref["c2bar"])))
    elif row["kind"] == "prof":
        bar = 16 * M * EPS * ysq / float(ref["c2bar"].min())
        ratio = max(float(np.max(np.abs(f64["F"].min(1 - k).astype(LD) - F.min(1 - k)))) / bar for k in range(2))
    else:
        T = 2.0 * S.SIGMA ** 2
        post = R.posterior(F, ref["c2bar"], ysq, M, T)
        p64 = R.posterior(f64["F"], f64["c2bar"], f64["ysq"], M, T, dt=np.float64)
        ratio = R.worst_ratio(p64["w"], p64["log_sum"], post)
        for k in range(2):
            assert abs(float(post["w"][k].sum()) - 1.0) < 1e-15
    print("%s: float64 against long double: %.3g of the bar (smallest 1 - c^2 = %.3g)" % (row["id"], ratio, float(ref["c2bar"].min())))
    assert ratio <= 1.0

"""csrc/mcf.hip against 50-digit values (tests/golden/mcf_hp_cases.npz, written by gen_golden_mcf_hp.py).

The fixture answers "what is the exact signal for these float64 inputs and these float64 tables" for
cases placed where the kernel can go wrong and the reference-recorded cases of test_mcf_gpu.py never
go: every matrix size around the 16-row tile edges and up to the unpadded M = 64, every squaring count
from 0 to 20 (radii from 0.04 um up to what the q/p check admits) and both sides of a change of s,
degenerate rows, DDE with a q = 0 block, and synthetic coupling tables for which the Pade solve swaps
rows.  Physical cylinder tables cannot do the last: of 381 admissible cases (M = 16 / 33 / 60,
L = 1..30 um, D = 0.5..3e-9, G = 0.04..0.3, three timings) none makes (V - U) need a row swap, and none
of this fixture's physical cases does either (the host test asserts it), so without the synthetic
tables the swap path of mcf_solve would be dead code under the whole suite.

The bar.  The errors of a squaring chain are absolute in units of the entries of X (at most 1 in
modulus) and double per squaring, so a case may miss its 50-digit value by

    K x 2^-52 x E_par x sum over blocks of 2^s_b,        K = 4 x K_scipy,

s_b the kernel's own squaring count (stored in the fixture).  K_scipy is measured, not chosen: the
largest error, in those units, of the reference's float64 formulation (scipy.linalg.expm) over all
fixture cases.  The factor 4 is what two correct float64 scaling-and-squaring codes may differ by
(degree 13 always and the kernel's own s here, lower degrees with less scaling there; Gauss-Jordan
against LU).  Neither figure depends on what the kernel returns.

This file reads the fixture and nothing else (no mpmath, no generator import)."""
import os

import numpy as np
import pytest

import microstructure_fingerprinting_amd as mf
from microstructure_fingerprinting_amd import _lib

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
S_GROUPS = ((0, 0), (1, 8), (9, 14), (15, 1000))


@pytest.fixture(scope="module")
def d():
    with np.load(os.path.join(G, "mcf_hp_cases.npz")) as z:
        return {k: z[k] for k in z.files}


def _scale(d):
    s = d["s"]
    return 2.0 ** -52 * d["E_par"] * np.sum(np.where(s >= 0, 2.0 ** np.maximum(s, 0), 0.0), axis=1)


def _abi(dde, lam, B, M, seq, L, D, env, gamma):
    """mfx_mcf_pgse / mfx_mcf_dde directly: what the public API cannot express (M > 60, tables or rows
    that its q/p check refuses).  Returns E [n_seq, n_atoms]."""
    lib = _lib.lib()
    lam, B = _lib.f64c(lam[:M]), _lib.f64c(B[:M, :M])
    seq, L, D, env = _lib.f64c(seq), _lib.f64c(np.atleast_1d(L)), _lib.f64c(np.atleast_1d(D)), _lib.f64c(env)
    E = np.full((seq.shape[0], L.size), -1.0)
    _lib.check(getattr(lib, "mfx_mcf_dde" if dde else "mfx_mcf_pgse")(
        _lib.dptr(lam), _lib.dptr(B), int(M), _lib.dptr(seq), seq.shape[0], _lib.dptr(L), _lib.dptr(D), L.size,
        _lib.dptr(env), float(gamma), _lib.dptr(E)))
    return E


def _one(d, i, default_tables=False):
    lam, B = d["tab_lam"][d["tab"][i]], d["tab_B"][d["tab"][i]]
    M, L, D, env, gamma = int(d["M"][i]), d["L"][i], d["D"][i], d["envdir"][i], d["gamma"][i]
    tables = None if default_tables else (lam, B)
    if d["dde"][i]:
        if d["api"][i]:
            return mf.mcf.MCF_DDE('cylinder', L, D, d["row"][i][None, :], envdir=env, gamma=gamma, M=M, tables=tables)[0]
        assert not default_tables
        return _abi(True, lam, B, M, d["row"][i][None, :], L, D, env, gamma)[0, 0]
    if d["api"][i]:
        return mf.mcf.MCF_PGSE('cylinder', L, D, scheme=d["row"][i][None, :7], envdir=env, gamma=gamma, M=M,
                               tables=tables)[0]
    assert not default_tables
    return _abi(False, lam, B, M, d["row"][i][None, :7], L, D, env, gamma)[0, 0]


@pytest.fixture(scope="module")
def single(d):
    """Every fixture case as a call of its own."""
    return np.array([_one(d, i) for i in range(d["M"].size)])


def _report(d, idx, ratio, what):
    """Largest ratio per group of s and its case, printed before anything is asserted."""
    smax = d["s"].max(axis=1)
    for lo, hi in S_GROUPS:
        m = [k for k, i in enumerate(idx) if lo <= smax[i] <= hi]
        if not m:
            continue
        k = m[int(np.argmax(ratio[m]))]
        i = idx[k]
        print("%s: s in %d..%s: %3d cases, largest |E - E50| / (2^-52 E_par sum 2^s) = %.3f  (case %d, %s, M = %d, "
              "L = %.4g, s = %s)" % (what, lo, hi if hi < 1000 else "", len(m), ratio[k], i, d["group"][i], d["M"][i],
                                     d["L"][i], d["s"][i].tolist()))


def test_every_case_meets_the_bar(d, single):
    n = d["M"].size
    K = 4.0 * float(d["K_scipy"])
    ratio = np.abs(single - d["E50"]) / _scale(d)
    print("K_scipy = %.4f, bar K = %.4f, %d cases" % (float(d["K_scipy"]), K, n))
    _report(d, np.arange(n), ratio, "kernel")
    sw = np.nonzero(d["n_swaps"] > 0)[0]
    print("cases whose Pade solve swaps rows: %d, largest ratio %.3f" % (sw.size, ratio[sw].max()))
    assert np.all(np.isfinite(single))
    bad = np.nonzero(~(ratio <= K))[0]
    assert bad.size == 0, "cases above the bar: %s" % [(int(i), str(d["group"][i]), int(d["M"][i]), d["s"][i].tolist(),
                                                        float(ratio[i])) for i in bad]


def test_default_tables_meet_the_same_bar(d):
    """MCF_PGSE / MCF_DDE without tables= on the physical cases the API admits: the generated tables are the
    closed-form ones to rounding (tests/test_mcf_hp_host.py), so the bar is the one above, not 5e-6."""
    idx = np.nonzero((d["tab"] == 0) & d["api"])[0]
    assert idx.size >= 100 and set(d["M"][idx].tolist()) >= {2, 3, 15, 16, 17, 31, 32, 33, 47, 48, 49, 59, 60}
    got = np.array([_one(d, i, default_tables=True) for i in idx])
    ratio = np.abs(got - d["E50"][idx]) / _scale(d)[idx]
    _report(d, idx, ratio, "default tables")
    bad = idx[~(ratio <= 4.0 * float(d["K_scipy"]))]
    assert bad.size == 0, "cases above the bar with the generated tables: %s" % bad.tolist()


def _batches(d):
    """PGSE cases that can share one call: same table set, M, envdir and gamma."""
    groups = {}
    for i in np.nonzero(~d["dde"])[0]:
        key = (int(d["tab"][i]), int(d["M"][i]), tuple(d["envdir"][i].tolist()), float(d["gamma"][i]))
        groups.setdefault(key, []).append(int(i))
    return groups


def test_batched_calls_equal_single_calls_bit_for_bit(d, single):
    """All PGSE cases of one table set and M as the columns of one call with the rows of all of them, plus a
    row without gradient and (axis along z) one along the axis: more items than compute units, each
    persistent workgroup walking through items whose s differs by up to 20 and whose pivots differ.  Small
    groups are tiled to at least 1200 items so that they, too, make workgroups take several items.  Whatever
    one item leaves in the workspace, in the LDS vectors or in the pivot word would show as a difference from
    the single-case call, or between the three orders."""
    ncase, nitems, napi = 0, 0, 0
    for (tab, M, env, gamma), idx in sorted(_batches(d).items()):
        idx = np.array(idx)
        lam, B = d["tab_lam"][tab], d["tab_B"][tab]
        env = np.array(env)
        n = idx.size
        rep = max(1, -(-1200 // (n * n)))
        on_axis = env[0] == 0.0 and env[1] == 0.0
        extra = [np.r_[1.0, 0.0, 0.0, 0.0, 0.03, 0.01, 0.05]]
        if on_axis:
            extra.append(np.r_[0.0, 0.0, -1.0, 0.07, 0.0431, 0.0106, 0.092])
        extra = np.array(extra)
        # the public API where it admits every (atom, row) pair of the batch, the C ABI otherwise
        qp = np.max((gamma * d["L"][idx]) * (d["L"][idx] ** 2 / d["D"][idx])) * max(np.max(d["row"][idx, 3]), extra[:, 3].max())
        use_api = M <= 60 and qp < lam[M - 1]
        first = None
        for order in range(3):
            perm = np.arange(n) if order == 0 else np.random.default_rng(100 * order + M).permutation(n)
            ii = idx[perm]
            rows = np.concatenate([d["row"][ii, :7], extra])
            if order == 2:   # the closed-form rows first: they shift every matrix item's place in the list
                rows = np.concatenate([extra, d["row"][ii, :7]])
            L, D = np.tile(d["L"][ii], rep), np.tile(d["D"][ii], rep)
            if use_api:
                E = mf.mcf.MCF_PGSE_atoms('cylinder', L, D, scheme=rows, envdir=env, gamma=gamma, M=M, tables=(lam, B))
            else:
                E = _abi(False, lam, B, M, rows, L, D, env, gamma)
            assert E.shape == (n + len(extra), n * rep)
            Ec, Ex = (E[len(extra):], E[:len(extra)]) if order == 2 else (E[:n], E[n:])
            for r in range(rep):
                blk = Ec[:, r * n:(r + 1) * n]
                assert np.array_equal(np.diag(blk), single[ii]), \
                    "table set %d, M = %d, order %d, copy %d: batched entries differ from the single-case calls" % (
                        tab, M, order, r)
                inv = np.argsort(perm)
                blk0 = blk[np.ix_(inv, inv)]          # back to fixture order
                if first is None:
                    first = blk0
                assert np.array_equal(blk0, first), "table set %d, M = %d: order %d, copy %d differs" % (tab, M, order, r)
            # rows of kind 0 and 1 inside the mixed batch
            assert np.all(Ex[0] == 1.0)
            if on_axis:
                b = (gamma * extra[1, 5] * extra[1, 3]) ** 2 * (extra[1, 4] - extra[1, 5] / 3)
                assert np.allclose(Ex[1], np.exp(-b * D), rtol=1e-15, atol=0)
                alone = _abi(False, lam, B, M, extra[1:2], L, D, env, gamma)
                assert np.array_equal(Ex[1], alone[0])
            nitems = max(nitems, n * n * rep)
        ncase += n
        napi += int(use_api)
    print("batched: %d PGSE cases in %d groups (%d through MCF_PGSE_atoms, the others through the C ABI), largest call "
          "%d matrix items" % (ncase, len(_batches(d)), napi, nitems))
    assert ncase == int(np.sum(~d["dde"])) and nitems > 4096 and napi >= 3


def test_dde_rows_batched_equal_single_calls(d, single):
    """The DDE cases of one (table set, M, L, D) as the rows of one call, in both orders: the vectors kept in
    LDS between the two blocks of one item must not leak into the next item."""
    groups = {}
    for i in np.nonzero(d["dde"])[0]:
        key = (int(d["tab"][i]), int(d["M"][i]), float(d["L"][i]), float(d["D"][i]))
        groups.setdefault(key, []).append(int(i))
    assert any(len(v) >= 8 for v in groups.values())
    for (tab, M, L, D), idx in groups.items():
        idx = np.array(idx)
        for ii in (idx, idx[::-1]):
            rows = np.tile(d["row"][ii], (40, 1))       # 40 copies: more items than compute units for the groups of 8
            E = _abi(True, d["tab_lam"][tab], d["tab_B"][tab], M, rows, L, D, d["envdir"][ii[0]], d["gamma"][ii[0]])
            assert np.array_equal(E[:, 0], np.tile(single[ii], 40)), "DDE batch, table set %d, M = %d, L = %g" % (tab, M, L)

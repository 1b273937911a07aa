"""The high-precision MCF fixture (tests/golden/mcf_hp_cases.npz) and the generated tables, checked on the host.

* the fixture covers what it promises (counted from the stored inputs: a regenerated fixture that lost a
  group fails here), some of its 50-digit values are recomputed with mpmath, and the float64 baseline that
  sets the GPU test's bar (K_scipy) is recomputed for every case;
* a NumPy restatement of the kernel's algorithm (float64 Pade 13, Gauss-Jordan with partial pivoting on the
  padded 64 x 64 matrix, s squarings) meets the GPU test's bar on every case, and misses it with one squaring
  too few or with the wrong row swapped: the bar is attainable by the algorithm and has teeth;
* mcf_tables against the exact closed form (and that against the defining integrals), to 1e-13 instead of the
  2e-6 that the reference's .mat allows.

Physical cylinder tables never make the Pade solve swap rows (0 of 381 admissible cases at M = 16 / 33 /
60, L = 1..30 um, D = 0.5..3e-9, G = 0.04..0.3 and three timings; 0 of this fixture's physical cases, asserted
below), which is why the fixture carries synthetic coupling tables.  No GPU needed."""
import os
import sys

import numpy as np
import pytest

from microstructure_fingerprinting_amd import mcf

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, G)
import gen_golden_mcf_hp as gen  # noqa: E402

# fifteen cases with M <= 20, fixed by index, spread over s (asserted below)
RECOMPUTED = (19, 59, 149, 132, 165, 64, 68, 21, 146, 72, 22, 76, 114, 177, 194)


@pytest.fixture(scope="module")
def d():
    with np.load(os.path.join(G, "mcf_hp_cases.npz")) as z:
        return {k: z[k] for k in z.files}


def _case(d, i):
    t = d["tab"][i]
    return (d["row"][i], d["L"][i], d["D"][i], d["envdir"][i], d["gamma"][i], d["tab_lam"][t], d["tab_B"][t],
            int(d["M"][i]), bool(d["dde"][i]))


def test_fixture_coverage(d):
    gen.check_coverage(d)
    n = d["M"].size
    assert 150 <= n <= 400
    assert set(d["M"].tolist()) >= set(gen.M_SET)
    smax = d["s"].max(axis=1)
    assert set(range(20)) <= set(smax.tolist())
    assert int(np.sum(d["n_swaps"] > 0)) >= 8
    assert np.all(d["api"][d["M"] > 60] == False)  # noqa: E712
    assert os.path.getsize(os.path.join(G, "mcf_hp_cases.npz")) < 1 << 20


def test_stored_analysis_matches_the_inputs(d):
    """s, the swaps, the API's admission and the table sets, recomputed from the stored inputs."""
    lam, B, _ = gen.exact_cylinder_tables(64)
    assert np.array_equal(lam, d["tab_lam"][0]) and np.array_equal(B, d["tab_B"][0])
    for i in range(d["M"].size):
        c = _case(d, i)
        blocks, kind = gen.kernel_blocks(*c)
        assert kind == 2
        assert [b[0] for b in blocks] == [s for s in d["s"][i].tolist() if s >= 0]
        swaps = [gen.solve_swaps(b[2]) for b in blocks]
        assert sum(len(x) for x in swaps) == d["n_swaps"][i]
        assert max((k for x in swaps for k, _ in x), default=-1) == d["swap_max"][i]
        assert gen.api_admits(c[0], c[1], c[2], c[4], c[5], c[7], c[8]) == d["api"][i]
        if d["tab"][i] == 0:
            assert not swaps[0] and not swaps[-1], "a physical case swaps rows"


def test_values_recomputed_with_mpmath(d):
    s = d["s"].max(axis=1)[list(RECOMPUTED)]
    assert len(set(RECOMPUTED)) == 15 and np.all(d["M"][list(RECOMPUTED)] <= 20)
    assert s.min() == 0 and s.max() >= 18 and len(set(s.tolist())) >= 10
    assert np.any(d["dde"][list(RECOMPUTED)]) and np.any(d["n_swaps"][list(RECOMPUTED)] > 0)
    for i in RECOMPUTED:
        E, Ep = gen.signal_mp(*_case(d, i))
        assert abs(float(E) - d["E50"][i]) <= 2 * np.spacing(d["E50"][i]), "case %d" % i
        assert abs(float(Ep) - d["E_par"][i]) <= 2 * np.spacing(d["E_par"][i]), "case %d" % i


def test_float64_baseline_sets_the_bar(d):
    """K_scipy is the largest error of the reference's float64 formulation in units of 2^-52 E_par sum 2^s:
    the stored figure is the maximum of the stored errors, and the recomputed baseline stays within it."""
    scale = gen.scale_of(d["E_par"], d["s"])
    K = float(d["K_scipy"])
    assert K == np.max(d["err_scipy"] / scale)
    assert 0.5 <= K <= 8.0, "the 2^s law does not describe the float64 baseline"
    ratio = np.array([abs(gen.signal_ref64(*_case(d, i)) - d["E50"][i]) for i in range(d["M"].size)]) / scale
    print("K_scipy stored %.4f, recomputed %.4f (case %d)" % (K, ratio.max(), int(np.argmax(ratio))))
    assert np.all(ratio <= K)


def test_algorithm_restated_in_numpy_meets_the_bar_and_breaks_miss_it(d):
    """float64 Pade-13 as the kernel does it is within 4 K_scipy everywhere; one squaring too few, or a wrong
    row in a swap, is not."""
    scale = gen.scale_of(d["E_par"], d["s"])
    K = 4.0 * float(d["K_scipy"])
    n = d["M"].size
    ratio = np.array([abs(gen.kernel_model(*_case(d, i)) - d["E50"][i]) for i in range(n)]) / scale
    smax = d["s"].max(axis=1)
    for lo, hi in gen.S_GROUPS:
        m = np.nonzero((smax >= lo) & (smax <= hi))[0]
        print("NumPy restatement, s in %d..%s: largest ratio %.3f (case %d)"
              % (lo, hi if hi < 1000 else "", ratio[m].max(), m[np.argmax(ratio[m])]))
    assert np.all(ratio <= K)
    short = np.nonzero(smax >= 1)[0][::3]
    r1 = np.array([abs(gen.kernel_model(*_case(d, i), s_shift=-1) - d["E50"][i]) for i in short]) / scale[short]
    assert np.mean(r1 > K) > 0.5, "s - 1 squarings go unnoticed in most cases"
    for lo, hi in gen.S_GROUPS[1:]:
        m = (smax[short] >= lo) & (smax[short] <= hi)
        assert np.any(r1[m] > 100 * K), "s - 1 squarings go unnoticed for s in %d..%d" % (lo, hi)
    sw = np.nonzero(d["n_swaps"] > 0)[0]
    r2 = np.array([abs(gen.kernel_model(*_case(d, i), bad_swap=True) - d["E50"][i]) for i in sw]) / scale[sw]
    assert np.all(r2 > 100 * K), "a wrong row swap goes unnoticed in cases %s" % sw[r2 <= 100 * K].tolist()


def test_cylinder_tables_against_the_closed_form():
    """mcf_tables evaluates Grebenkov's matrix elements in float64 from scipy's zeros; here the same elements
    come from mpmath zeros at 50 digits (scipy's are only the starting points of mp.findroot)."""
    lam, B = mcf.mcf_tables('c', 60)
    lam_x, B_x, order = gen.exact_cylinder_tables(60)
    assert order[0] == 0 and order[1] == 1 and order.max() >= 10
    assert np.all(np.abs(lam - lam_x) <= 4 * np.spacing(lam_x))
    print("generated B against the closed form: largest difference %.3g, B[0, 1] off by %.2f ulp"
          % (np.max(np.abs(B - B_x)), abs(B[0, 1] - B_x[0, 1]) / np.spacing(B_x[0, 1])))
    assert np.max(np.abs(B - B_x)) <= 1e-13
    assert np.array_equal(B != 0, B_x != 0)          # the mode order: couplings exactly where |n_i - n_j| = 1
    assert np.array_equal(B != 0, np.abs(order[:, None] - order[None, :]) == 1)
    # a factor 1 + 1e-8 on the entry that carries most of the signal is 4e4 times the bound
    Bp = B.copy()
    Bp[0, 1] *= 1 + 1e-8
    assert np.max(np.abs(Bp - B_x)) > 1e-13


def test_closed_form_against_the_defining_integrals():
    """The closed form itself, against B_ij = <u_i | x | u_j> by quadrature: modes J_n(alpha r) cos(n phi)
    normalised to a mean square of 1 over the disk, 200-node Gauss-Legendre in r (the integrands are entire),
    int cos(n_i phi) cos(phi) cos(n_j phi) dphi = pi/2 (1 + [n_i + n_j = 1])."""
    from scipy import special as sp
    lam_x, B_x, order = gen.exact_cylinder_tables(60)
    x, w = np.polynomial.legendre.leggauss(200)
    r, w = 0.5 * (x + 1.0), 0.5 * w
    R = np.array([sp.jv(k, a * r) for a, k in zip(np.sqrt(lam_x), order)])
    ang = np.where(order == 0, 2.0 * np.pi, np.pi)
    R = R / np.sqrt(ang * (R * R * r * w).sum(axis=1) / np.pi)[:, None]
    Bq = np.zeros((60, 60))
    for i in range(60):
        for j in range(60):
            if abs(order[i] - order[j]) == 1:
                angij = 0.5 * np.pi * (2.0 if order[i] + order[j] == 1 else 1.0)
                Bq[i, j] = abs(angij * np.sum(R[i] * R[j] * r * r * w) / np.pi)
    assert np.max(np.abs(Bq - B_x)) <= 1e-13


def test_cylinder_tables_truncate_bit_for_bit():
    lam, B = mcf.mcf_tables('c', 60)
    for M in range(1, 61):
        l, b = mcf.mcf_tables('c', M)
        assert np.array_equal(l, lam[:M]) and np.array_equal(b, B[:M, :M]), "M = %d" % M


def test_sphere_eigenvalues_are_zeros_of_the_derivative():
    import mpmath as mp
    from scipy import special as sp
    mp.mp.dps = 30
    lam, _ = mcf.mcf_tables('s', 60)
    assert lam[0] == 0.0 and np.all(np.diff(lam) > 0)

    def djl(l, x):   # j_l'(x) = j_{l-1}(x) - (l + 1) / x j_l(x)
        jl = lambda k: mp.sqrt(mp.pi / (2 * x)) * mp.besselj(k + mp.mpf(1) / 2, x)  # noqa: E731
        return (jl(l - 1) if l > 0 else -jl(1)) - (mp.mpf(l + 1) / x * jl(l) if l > 0 else 0)

    for a in np.sqrt(lam[1:]):
        l = int(np.argmin(np.abs(sp.spherical_jn(np.arange(0, 40), a, derivative=True))))
        assert abs(djl(l, mp.mpf(float(a)))) <= 1e-13, "alpha = %r is no zero of j_%d'" % (a, l)
    # no eigenvalue missed: sign changes of j_l' below alpha_60 on a grid twice as fine as the one mcf.py searches
    a60 = np.sqrt(lam[59])
    x = np.linspace(1e-3, np.pi * 62, 400 * 62)
    count = 1                                         # the constant mode
    for l in range(0, 62):
        f = sp.spherical_jn(l, x, derivative=True)
        lower = x[:-1][np.sign(f[:-1]) * np.sign(f[1:]) < 0]
        count += int(np.count_nonzero(lower < a60))   # brackets that start below alpha_60: every zero up to alpha_60
    assert count == 60

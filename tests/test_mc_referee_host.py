"""The 50-digit fixture of the Monte-Carlo phase average (tests/golden/mc_hp_cases.npz) and the bar that
tests/test_mc_referee_gpu.py holds the device to, checked on the host (cases and bar: tests/_mc_cases.py).

* the fixture covers what it promises, is small, belongs to the inputs that this NumPy builds, and a sample of it is
  recomputed with mpmath;
* a NumPy restatement of the kernel's sum order with np.cos meets the bar on every case: the bar is attainable;
* the same restatement misses it with the argument's inner product rounded once, with Ds folded into g, with one
  spin too few and with the neighbouring acquisition's phases: the bar has teeth;
* the CPU oracle stays within the project's 1e-13 of the 50-digit values.  No GPU needed."""
import os
import sys

import numpy as np
import pytest

import _mc_cases as mc

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, G)
import gen_golden_mc_hp as gen  # noqa: E402

NPZ = os.path.join(G, "mc_hp_cases.npz")
# at least one case per rung and per seam family, without the nchunks = 65 case; two sequences of each are recomputed
RECOMPUTED = ("ladder:1:Ds1", "ladder:100:Ds0", "ladder:10000:Ds1", "ladder:1e+06:Ds1", "ladder:1e+12:Ds0", "ladder:1e+12:Ds1",
              "spin:1", "spin:65", "spin:257", "spin:4097", "zero-g:256", "tile:single:9", "tile:together", "tile:interleaved",
              "dim:1", "dim:2", "special:Ds0", "special:phase-zeros", "special:g-inf-nan", "pgse:ext:bsingle", "pgse:dup",
              "pgse:dim2")


@pytest.fixture(scope="module")
def gold():
    return mc.load_golden(NPZ)


@pytest.fixture(scope="module")
def built():
    """{name: (inputs, argument [n_seq, n_spin])}, built once and left unchanged."""
    out = {}
    for c in mc.TABLE:
        inp = mc.inputs(c)
        out[c["name"]] = (inp, mc.argument(*inp))
    return out


def _misses(c, S, A, got):
    """Which finite sequences of a case miss the bar."""
    fin = np.isfinite(S)
    return fin & ~(np.abs(np.where(fin, got - S, 0.0)) <= mc.bar(c["n_spin"], np.where(fin, S, 0.0), np.where(fin, A, 0.0)))


def test_fixture_coverage_size_and_checksums(gold, built):
    gen.check_coverage(gold)
    assert os.path.getsize(NPZ) < 1 << 20
    assert mc.C_COS == int(np.ceil(mc.C_COS_MEASURED_MAX)) + 1
    for c in mc.TABLE:
        assert mc.checksum(c, built[c["name"]][0]) == gold[c["name"]][2], \
            "%s: this NumPy builds other inputs than the fixture was computed from" % c["name"]
        S, A, _ = gold[c["name"]]
        fin = np.isfinite(S)
        assert np.all(np.abs(S[fin]) <= A[fin]) and np.all(A[fin] <= 1.0)


def test_sample_recomputed_with_mpmath(gold, built):
    pytest.importorskip("mpmath")
    fams = {mc.BY_NAME[n]["family"] for n in RECOMPUTED}
    assert fams == {c["family"] for c in mc.TABLE}
    assert {mc.BY_NAME[n]["scale"] for n in RECOMPUTED if n.startswith("ladder")} == set(mc.LADDER_SCALES)
    assert all(mc.BY_NAME[n]["n_spin"] < 10000 for n in RECOMPUTED)
    for name in RECOMPUTED:
        S, A, _ = gold[name]
        arg = built[name][1]
        for i in (range(len(S)) if name == "special:g-inf-nan" else (0, len(S) - 1)):
            s, a = gen.hp_mean(arg[i])
            assert np.array_equal([s, a], [S[i], A[i]], equal_nan=True), "%s, sequence %d" % (name, i)


def test_the_bar_is_attainable(gold, built):
    """float64 arguments in the defined order, np.cos, the device's order of summation: within the bar everywhere."""
    worst = 0.0
    for c in mc.TABLE:
        S, A, _ = gold[c["name"]]
        inp, arg = built[c["name"]]
        with np.errstate(invalid="ignore"):
            got = mc.kernel_order_mean(np.cos(arg), c["n_spin"])
        assert np.array_equal(np.isnan(got), np.isnan(S)), c["name"]
        assert not np.any(_misses(c, S, A, got)), c["name"]
        fin = np.isfinite(S)
        worst = max(worst, float(np.max(np.abs(got[fin] - S[fin]) / mc.bar(c["n_spin"], S[fin], A[fin]))))
        for r in c["zero_rows"]:
            assert got[r] == 1.0 == S[r]
    print("NumPy restatement: largest error / bar = %.3f" % worst)
    assert worst < 1.0


def test_the_bar_rejects_a_contracted_argument_and_a_folded_ds(gold, built):
    """From the 1e6 rung upwards an inner product without intermediate rounding, or Ds multiplied into g first, moves at
    least one sequence of every case past the bar.  With Ds = 1.0 folding changes no bit (fl(1.0 g) = g), which is
    asserted instead: there is nothing to detect."""
    rungs = [c for c in mc.TABLE if c["family"] == "ladder" and c["scale"] >= 1e6]
    assert len(rungs) == 4
    for c in rungs:
        S, A, _ = gold[c["name"]]
        inp, arg = built[c["name"]]
        for variant in ("contracted", "folded"):
            bad = mc.argument(*inp, variant=variant)
            if variant == "folded" and c["Ds"] == 1.0:
                assert np.array_equal(bad, arg)
                continue
            miss = _misses(c, S, A, mc.kernel_order_mean(np.cos(bad), c["n_spin"]))
            print("%s %s: %d of %d sequences miss the bar" % (c["name"], variant, miss.sum(), miss.size))
            assert miss.any(), "%s: a %s argument goes unnoticed" % (c["name"], variant)
    # below the ladder's 1e6 rung a contracted argument is within the bar: why the small-phase tests could not notice
    c = mc.BY_NAME["ladder:1:Ds1"]
    inp, _ = built[c["name"]]
    S, A, _ = gold[c["name"]]
    assert not _misses(c, S, A, mc.kernel_order_mean(np.cos(mc.argument(*inp, variant="contracted")), c["n_spin"])).any()


def test_the_bar_rejects_a_missing_spin_and_a_neighbouring_acquisition(gold, built):
    seams = [c for c in mc.TABLE if c["family"] in ("spin", "zero-g", "tile")]
    assert len(seams) == 12 + 12 + 8
    for c in seams:
        S, A, _ = gold[c["name"]]
        inp, arg = built[c["name"]]
        short = mc.kernel_order_mean(np.cos(arg), c["n_spin"], n_sum=c["n_spin"] - 1)
        assert _misses(c, S, A, short).all(), "%s: a sum over one spin too few goes unnoticed" % c["name"]
        if c["n_ref"] == 1:
            continue                         # the nchunks = 65 case has one acquisition: no neighbour to read
        moving = np.any(inp[2] != 0.0, axis=1)
        assert moving.any()
        for shift in (-1, 1):
            other = mc.kernel_order_mean(np.cos(mc.argument(*inp, ref_shift=shift)), c["n_spin"])
            assert _misses(c, S, A, other)[moving].all(), "%s: phases of acquisition ref %+d go unnoticed" % (c["name"], shift)


def test_cpu_oracle_against_50_digits(gold, built):
    """The oracle's sequential float64 sum with libm's cosine, 1 and 3 threads, within the project's 1e-13 on every
    case.  Largest deviation seen: 2.44e-15 (ladder:1:Ds1)."""
    from oracle import oracle as orc
    worst, where = 0.0, None
    for c in mc.TABLE:
        S = gold[c["name"]][0]
        ph, dm, gs, Ds, n = built[c["name"]][0]
        for nt in (1, 3):
            got = orc.monte_carlo_average(ph, dm, gs, Ds, n, nthreads=nt)
            assert np.array_equal(np.isnan(got), np.isnan(S)), c["name"]
            fin = np.isfinite(S)
            dev = float(np.max(np.abs(got[fin] - S[fin])))
            if dev > worst:
                worst, where = dev, c["name"]
            assert dev <= 1e-13, "%s, %d threads: %.3g" % (c["name"], nt, dev)
    print("CPU oracle: largest deviation from the 50-digit means %.3g (%s)" % (worst, where))

"""The referee of tests/_rot2d_ref.py pinned on the wide recording of the reference (tests/golden/rot2d_wide.npz,
written by gen_golden_rot2d_wide.py).  No GPU: this is what lets tests/test_rot2d_referee_gpu.py hold the device
against the referee on directions, rows and atom counts the recording has no values for.

Bar: the project's rotation bar, rtol 1e-10, atol 1e-13 (tests/test_rot2d_gpu.py)."""
import numpy as np
import pytest

import _rot2d_ref as ref2d
import _rot2d_wide as W

CAP = 0.02      # largest share of a random population that may be unclear (the reference itself rejects up to 1.7 %)


@pytest.fixture(scope="module")
def wide():
    return W.Wide()


def test_recording_has_what_the_gpu_tests_rely_on(wide):
    assert len(wide.combos) == 19
    assert wide.w["A_sch"].shape == (352, 7) and wide.w["B_sch"].shape == (21, 7) and wide.w["C_sch"].shape == (4000, 7)
    assert sorted(np.unique(wide.w["A_sch"][:, 4], return_counts=True)[1].tolist()) == [65, 287]
    assert np.any(np.diff(wide.w["A_sch"][:, 4]) > 0) and np.any(np.diff(wide.w["A_sch"][:, 4]) < 0)   # interleaved
    A = wide.w["A_sch"]
    rows, counts = np.unique(A[A[:, 3] > 0][:, :6], axis=0, return_counts=True)
    assert (counts == 2).sum() == 6 and counts.max() == 2                                           # six repeated DW rows
    assert sorted(np.unique(wide.w["C_sch"][:, 4], return_counts=True)[1].tolist()) == [1000] * 4
    for c in wide.combos:
        dirs, ok = wide.w[c["key"] + "_dirs"], wide.w[c["key"] + "_ok"]
        assert dirs.shape == (c["n_edge"] + 256, 3) and c["n_edge"] == len(wide.edge_names)
        assert np.array_equal(~ok, np.array([str(k) in wide.outcomes[c["key"]] for k in range(ok.size)]))
        assert 0 < (~ok).sum() <= 0.03 * ok.size
        assert np.all(ok[wide.w[c["key"] + "_vidx"]])


@pytest.mark.parametrize("key", W.keys())
def test_referee_gives_the_reference_outcome_and_values(wide, key):
    c = wide.combo(key)
    res = wide.results(c)
    for k, r in enumerate(res):
        if r.clear:
            assert r.error == wide.recorded(c, k), (key, k)
            assert (r.out is not None) == (r.error is None)
    vidx, vrows, val = wide.w[key + "_vidx"], wide.w[key + "_vrows"], wide.w[key + "_val"]
    assert len(vidx) >= 8
    worst = max(W.worst_ratio(res[k].out[vrows[i]], val[i]) for i, k in enumerate(vidx) if res[k].clear)
    assert worst <= 1.0, worst


@pytest.mark.parametrize("key", W.keys())
def test_unclear_share_is_capped_and_edge_directions_are_named(wide, key):
    c = wide.combo(key)
    res = wide.results(c)
    n_edge = c["n_edge"]
    unclear_random = [k for k in range(n_edge, len(res)) if not res[k].clear]
    assert len(unclear_random) <= CAP * (len(res) - n_edge), unclear_random
    for k in range(n_edge):
        want = W.EDGE_UNCLEAR.get((key, wide.edge_names[k]))
        assert res[k].unclear == ([] if want is None else [want]), (key, wide.edge_names[k], res[k].unclear)


def test_edge_outcomes_are_the_intended_ones(wide):
    """what each edge direction is there for, on the recording itself"""
    for c in wide.combos:
        name = {n: k for k, n in enumerate(wide.edge_names)}
        rec = lambda n: wide.recorded(c, name[n])   # noqa: E731
        for n in ("+z", "-z", "line1", "line1 tilted 1e-9", "line2", "line2 tilted 1e-9", "|z| = 0.004",
                  "unit(6e-10, 8e-10, 1)", "(0.6, 0, 0.8) (1 + 2e-6)", "(0.6, 0, 0.8) (1 - 2e-6)"):
            assert rec(n) is None, (c["key"], n, rec(n))
        assert rec("(0.6, 0, 0.8) (1 + 6e-6)") == ("ValueError", ref2d.MSG_NORM)
        # a generic in-plane direction fails; the perpendicular of line 1 is generic unless it is line 2 itself
        # (the fixture's lines are only about perpendicular)
        generic = ["|z| = 1e-4", "in-plane at 0.4 rad"]
        if c["proto"] in ("A", "B", "fix"):
            generic.append("in-plane perpendicular of line1")
        else:
            assert rec("in-plane perpendicular of line1") is None
        for n in generic:
            assert rec(n)[0] == "AssertionError" and "found 4 instead of 2 pairs" in rec(n)[1], (c["key"], n)
    # the in-plane reference fascicle along line 1 of A leaves three reference directions, not five
    side = wide.referee(wide.combo("A_line1")).ref_side
    assert [s["un"].shape[0] for s in side] == [3, 3]
    assert [s["un"].shape[0] for s in wide.referee(wide.combo("A_o1")).ref_side] == [5, 5]


def test_edge_directions_take_the_paths_they_are_there_for(wide):
    c = wide.combo("A_o1")
    name = {n: k for k, n in enumerate(wide.edge_names)}
    res = wide.results(c)
    assert res[name["line1"]].margins["vanished"] > 0 and res[name["line1 tilted 1e-9"]].margins["vanished"] == 0
    assert res[name["+z"]].margins["extrapolated"] > 0

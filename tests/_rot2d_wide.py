"""Access to the wide recording of the reference's 2-D protocol rotation (tests/golden/rot2d_wide.npz, written by
tests/golden/gen_golden_rot2d_wide.py), shared by test_rot2d_ref_host.py and test_rot2d_referee_gpu.py: the
protocols, the recorded outcomes and one referee (tests/_rot2d_ref.py) per (protocol, reference direction)."""
import json
import os

import numpy as np

import _rot2d_ref as ref2d

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RTOL, ATOL = 1e-10, 1e-13          # the project's rotation bar (tests/test_rot2d_gpu.py)

# The edge directions that are not clear, with the decision that makes them so; every other recorded edge direction
# must be clear.  All are on protocol A, the one with repeated rows (a repeated knot is the only place where the
# interpolant jumps):
#   refdir +-z, new direction +-z or 5e-19 off it: the new side's abscissae are the knots themselves up to the last
#   bit of a norm taken once more (the reference normalises the scheme in place), repeated knots included;
#   refdir along line 1, new direction along a line: by symmetry the abscissae G sin(70 deg) fall on the knots;
#   refdir along line 1, new direction +-z: new line 1 is parallel to the reference fascicle, so its dot with every
#   reference direction is rounding noise and the arg-max is a tie.
EDGE_UNCLEAR = {
    ("A_z", "+z"): "knot", ("A_z", "-z"): "knot", ("A_z", "unit(6e-10, 8e-10, 1)"): "knot",
    ("A_mz", "+z"): "knot", ("A_mz", "-z"): "knot", ("A_mz", "unit(6e-10, 8e-10, 1)"): "knot",
    ("A_line1", "line1"): "knot", ("A_line1", "line1 tilted 1e-9"): "knot",
    ("A_line1", "line2"): "knot", ("A_line1", "line2 tilted 1e-9"): "knot",
    ("A_line1", "+z"): "argmax", ("A_line1", "-z"): "argmax", ("A_line1", "unit(6e-10, 8e-10, 1)"): "argmax",
}


def keys():
    w = np.load(os.path.join(G, "rot2d_wide.npz"))
    return [c["key"] for c in json.loads(str(w["combos_json"]))]


def worst_ratio(got, want):
    """largest |got - want| / (ATOL + RTOL |want|); at most 1 within the bar"""
    assert got.shape == want.shape
    return float(np.max(np.abs(got - want) / (ATOL + RTOL * np.abs(want))))


class Wide:
    def __init__(self):
        self.w = np.load(os.path.join(G, "rot2d_wide.npz"))
        self.cases = np.load(os.path.join(G, "rot2d_cases.npz"))
        self.combos = json.loads(str(self.w["combos_json"]))
        self.outcomes = json.loads(str(self.w["outcomes_json"]))
        self.edge_names = json.loads(str(self.w["edge_names_json"]))
        self.DIFF = float(self.w["DIFF"])
        self._ref, self._res = {}, {}

    def protocol(self, c):
        """(scheme [M, 7], signals [M, N]) of a combination, N the number of atoms the recording used"""
        src = self.w if c["proto"] in ("A", "B", "C") else self.cases
        return src[c["proto"] + "_sch"], np.ascontiguousarray(src[c["proto"] + "_sig"][:, :c["atoms"]])

    def combo(self, key):
        return next(c for c in self.combos if c["key"] == key)

    def referee(self, c):
        if c["key"] not in self._ref:
            sch, sig = self.protocol(c)
            self._ref[c["key"]] = ref2d.Referee(sig, sch, np.array(c["refdir"]), self.DIFF)
        return self._ref[c["key"]]

    def results(self, c):
        """the referee's Result for every recorded direction of the combination (computed once)"""
        if c["key"] not in self._res:
            R = self.referee(c)
            self._res[c["key"]] = [R.rotate(d) for d in self.w[c["key"] + "_dirs"]]
        return self._res[c["key"]]

    def recorded(self, c, k):
        """None for a success, else (type name, message)"""
        e = self.outcomes[c["key"]].get(str(k))
        return None if e is None else tuple(e)

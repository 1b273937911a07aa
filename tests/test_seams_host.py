"""The preconditions of tests/test_seams_gpu.py that need no GPU (cases: tests/_seam_cases.py): what
mfx_debug_seam answers is the table's expression at the shape used, every big call is longer than a piece, the voxels on
both sides of every piece boundary differ, no case builds a host array of 400 MB, and where a clamp is under test the byte
budget beside it would allow more."""
import numpy as np
import pytest

import _seam_cases as sc

# the table of DESIGN.md 4.28: name of the case -> items per piece, written out
TABLE = {
    "rotate": 32768,
    "k2sx-NN_1-M68": 32768,
    "k2x-NN_E-M62": 2048, "k2x-NN_1_E-M62": 2048, "k2x-NN_1-M68-screen-off": 2048,
    "dense-wfit-NN_1-M260": 2 ** 30 // (8 * 260 * (2 * 64 + 2)),
    "dense-wfit-NN-M260-explicit": 2 ** 30 // (8 * 260 * (2 * 64 + 1)),
    "dense-fit2d-NN_1-fix": 2 ** 30 // (8 * 1776 * (2 * 32 + 1)),
    "dense-w2d-NN_1-fix": 2 ** 30 // (8 * 1776 * (2 * 32 + 1)),
    "upload-wfit-M260": 2 ** 28 // (16 * 260),
    "upload-rfit-M260": 2 ** 28 // (32 * 260),
    "upload-rfit2d-fix": 2 ** 28 // (1776 * (6 * 8 + 2 * (28 + 32))),
    "solve-soft-8x8": 65535, "solve-soft-8x8x1": 65535,
    "boot2d-K1": 65535, "boot2d-K2": 65535, "wboot2d-K1": 65535, "wboot2d-K2": 65535,
}


def test_every_case_is_in_the_table():
    assert sorted(TABLE) == sorted(sc.CASES)
    assert TABLE["dense-wfit-NN_1-M260"] == 3970 and TABLE["upload-wfit-M260"] == 64527 and TABLE["upload-rfit-M260"] == 32263


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_hook_answers_the_table_and_the_case_crosses(name):
    c = sc.CASES[name]
    L, V, cuts = sc.sizes(name)
    assert L == TABLE[name], "mfx_debug_seam(%d, ..) = %d, DESIGN.md 4.28 says %d" % (c["which"], L, TABLE[name])
    assert V > L and 5 <= V - L <= 2048 + 70
    assert cuts and cuts[0] <= L and all(0 < s < V for s in cuts)
    if name == "k2sx-NN_1-M68":
        assert V == 32768 + 2048 + 5 and 32768 in cuts and 2048 in cuts and 34816 in cuts
    idx, seed = sc.indices(name)
    assert idx.shape == (V,) and idx.min() == 0 and idx.max() == c.get("D", sc.D) - 1       # every distinct voxel is used
    for s in cuts:
        assert idx[s - 1] != idx[s], "%s: the same voxel on both sides of the boundary at %d" % (name, s)
    assert seed - c["seed"] < 8
    assert sc.host_bytes(name) < sc.MAX_HOST_BYTES, "%s builds a host array of %.0f MB" % (name, sc.host_bytes(name) / 1e6)
    print("%s: L = %d, V = %d, %d pieces, %d boundaries checked, largest host array %.1f MB"
          % (name, L, V, -(-V // L), len(cuts), sc.host_bytes(name) / 1e6))


def test_hook_rejects_what_it_does_not_know():
    from microstructure_fingerprinting_amd import _lib as L
    lib = L.lib()
    for which, M, pv in ((0, 0, 0), (11, 0, 0), (-1, 0, 0), (sc.DENSE, 260, 0), (sc.WFIT_UPLOAD, 0, 0), (sc.RFIT_UPLOAD, -3, 0),
                         (sc.RFIT2D_UPLOAD, 0, 2), (sc.RFIT2D_UPLOAD, 66, 4)):
        assert lib.mfx_debug_seam(which, M, pv) == -1, (which, M, pv)
    # the byte-sized seams shrink with the protocol, and never below one voxel
    assert sc.seam(sc.WFIT_UPLOAD, 62) > sc.seam(sc.WFIT_UPLOAD, 260) > sc.seam(sc.RFIT_UPLOAD, 260) >= 1
    assert sc.seam(sc.WFIT_UPLOAD, 2 ** 30) == 1 and sc.seam(sc.RFIT_UPLOAD, 2 ** 30) == 1 and sc.seam(sc.RFIT2D_UPLOAD, 2 ** 30, 3) == 1
    assert sc.seam(sc.RFIT2D_UPLOAD, 66, 0) > sc.seam(sc.RFIT2D_UPLOAD, 66, 1) > sc.seam(sc.RFIT2D_UPLOAD, 66, 2)


@pytest.mark.parametrize("name", [n for n in sorted(sc.CASES) if "boot2d" in n])
def test_the_clamp_cuts_before_the_byte_budget(name):
    """seam 8: 65 535 voxels of the shared-fit route take less than the default budget (at the 66-row protocol the weighted
    two-fascicle case would not: 4 428 bytes a voxel)"""
    c = sc.CASES[name]
    L = sc.seam(c["which"])
    per_vox = sc.boot2d_shared_bytes(c["K"], c["N"], c["M"], c["B"], name.startswith("w"))
    assert sc.DEFAULT_BYTES // per_vox > L, (name, per_vox)
    assert sc.DEFAULT_BYTES // sc.boot2d_shared_bytes(2, 16, 66, 2, True) < L


def test_mixed_layout_scatters_the_classes():
    lab = sc.mixed_layout(500, 51)
    assert lab.size == 500 + 2 * sc.D and np.count_nonzero(lab == "NN") == 500
    for other in sc.MIXED_OTHERS:
        at = np.flatnonzero(lab == other)
        assert at.size == sc.D and at[0] < 100 and at[-1] > lab.size - 100

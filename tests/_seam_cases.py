"""Cases of tests/test_seams_host.py and tests/test_seams_gpu.py: every place where the host code cuts a batch into
pieces (a launch, an upload, a scratch block) crossed at the smallest shape that crosses it.

The method is that of test_fit_gpu.test_host_pipeline_chunks_rows_and_buffer_pool: D = 61 distinct voxels are fitted in one
small call `base`; the big call takes V = L + r voxels drawn from them, idx = rng.integers(0, D, V), and must return
base[idx] bit for bit - a voxel's result depends on nothing but the voxel.  L is not written down here: it is what
mfx_debug_seam (include/mfx.h) answers, by the expression the host code itself cuts with, so that a test goes on crossing
its seam when the threshold moves.  At every position s where the big call starts a new piece the voxels s - 1 and s
differ in content (idx[s - 1] != idx[s]): `draw` advances the seed until that holds.

Nothing here touches a device: the hook is host arithmetic."""
import numpy as np

D = 61
# `which` of mfx_debug_seam (csrc/mfx_host.h: MFX_SEAM_*)
ROTATE, K2SX_BIG, K2X_CHUNK, DENSE, WFIT_UPLOAD, RFIT_UPLOAD, SOLVE_SOFT, BOOT2D, RFIT2D_UPLOAD, WBOOT2D = range(1, 11)
MAX_HOST_BYTES = 400e6


def seam(which, M=0, per_vox=0):
    """items per piece of seam `which`, from the library"""
    from microstructure_fingerprinting_amd import _lib as L
    n = int(L.lib().mfx_debug_seam(int(which), int(M), int(per_vox)))
    assert n > 0, "mfx_debug_seam(%d, %d, %d) = %d" % (which, M, per_vox, n)
    return n


def positions(V, *Ls):
    """the first voxel of every piece but the first, for pieces of L voxels, over every L given"""
    return sorted(set(s for L in Ls for s in range(L, V, L)))


def draw(V, cuts, seed, D=D):
    """(idx [V] in 0..D-1, the seed used): the first seed from `seed` on whose draw has idx[s - 1] != idx[s] at every cut"""
    cuts = np.asarray(cuts, dtype=np.int64)
    assert cuts.size > 0 and cuts.min() >= 1 and cuts.max() < V, "no piece boundary inside 0..%d: %s" % (V, cuts)
    while True:
        idx = np.random.default_rng(seed).integers(0, D, V)
        if np.all(idx[cuts - 1] != idx[cuts]):
            return idx, seed
        seed += 1


# ---- the shapes.  M of uc.model(dirs, N) is 2 + 3 dirs.
def dense_per_vox(M, Ntot, signal=0):
    """bytes a voxel takes in the block of mfx_solve_dense_chunks: its dictionary [M x Ntot] (+ the scaled signal [M] of the
    weighted fit), csrc/fit_w.hip, fit2d.hip, w2d.hip"""
    return 8 * M * (Ntot + signal)


# name -> dict(which, M, per_vox (argument of the hook), r (voxels beyond L), also (further piece sizes the call cuts at),
#              row_bytes (of the largest host array, per voxel), seed, D (distinct voxels where not 61))
# PGSE fits: class, directions per shell and atoms of tests/_units_cases.py
CASES = {
    # 1  mfx_rotate / mfx_rotate_dev: B = L + 37 directions on a plan of M = 14 rows, N = 4 atoms; out is [B, M, N]
    "rotate": dict(which=ROTATE, dirs=4, N=4, r=37, row_bytes=8 * 14 * 4, seed=11),
    # 2  [N, N, 1] at M = 68, screen on: the pipeline; 32768 + 2048 + 5 voxels: its big launches and the hand-back pass
    "k2sx-NN_1-M68": dict(which=K2SX_BIG, cls="NN_1", dirs=22, N=64, r=2048 + 5, also=(K2X_CHUNK,), row_bytes=8 * 68, seed=21),
    # 3  the plain kernel: classes with EAR columns at M = 62, and [N, N, 1] at M = 68 with the screen off
    "k2x-NN_E-M62": dict(which=K2X_CHUNK, cls="NN_E", dirs=20, N=64, r=5, row_bytes=8 * 62, seed=31),
    "k2x-NN_1_E-M62": dict(which=K2X_CHUNK, cls="NN_1_E", dirs=20, N=64, r=5, row_bytes=8 * 62, seed=32),
    "k2x-NN_1-M68-screen-off": dict(which=K2X_CHUNK, cls="NN_1", dirs=22, N=64, r=5, row_bytes=8 * 68, seed=33),
    # 4  mfx_solve_dense_chunks behind engine.fit_weighted: M = 260, N = 64 (the hook's bound: 2^30 / per_vox)
    "dense-wfit-NN_1-M260": dict(which=DENSE, cls="NN_1", dirs=86, N=64, M=260, per_vox=dense_per_vox(260, 129, 1), r=5,
                                 row_bytes=8 * 260, seed=41),
    "dense-wfit-NN-M260-explicit": dict(which=DENSE, cls="NN", dirs=86, N=64, M=260, per_vox=dense_per_vox(260, 128, 1), r=5,
                                        row_bytes=8 * 260, seed=42),
    # ... and behind engine.fit2d / fit2d_weighted: two fascicles + CSF on the 1 776-row protocol of tests/golden, N = 32
    "dense-fit2d-NN_1-fix": dict(which=DENSE, sch="fix", N=32, M=1776, per_vox=dense_per_vox(1776, 65), r=5, row_bytes=8 * 1776,
                                 seed=43),
    "dense-w2d-NN_1-fix": dict(which=DENSE, sch="fix", N=32, M=1776, per_vox=dense_per_vox(1776, 65), r=5, row_bytes=8 * 1776,
                               seed=44),
    # 5, 6  upload chunks of the host entry points: a mixed batch (N, NN, NN_1), N = 16 atoms, M = 260; the NN bin crosses
    "upload-wfit-M260": dict(which=WFIT_UPLOAD, dirs=86, N=16, M=260, r=70, row_bytes=8 * 260, seed=51),
    "upload-rfit-M260": dict(which=RFIT_UPLOAD, dirs=86, N=16, M=260, r=70, row_bytes=8 * 260, seed=61),
    # 6  the 2-D formula (per_vox carries K = 2): the 1 776-row protocol gives the smallest chunk
    "upload-rfit2d-fix": dict(which=RFIT2D_UPLOAD, sch="fix", N=16, M=1776, per_vox=2, r=70, row_bytes=8 * 1776, seed=62),
    # 7  ss_chunk's clamp: solvers of sizes [8, 8] and [8, 8, 1], M = 20, on the 37 signals of tests/_solve_soft_cases.py (D = 37)
    "solve-soft-8x8": dict(which=SOLVE_SOFT, sizes=(8, 8), M=20, D=37, r=6, row_bytes=8 * 20, seed=71),
    "solve-soft-8x8x1": dict(which=SOLVE_SOFT, sizes=(8, 8, 1), M=20, D=37, r=6, row_bytes=8 * 20, seed=72),
    # 8  the clamp of the shared-fit bootstrap kernels: B = 2 replicates, N = 16 atoms, the first two (Delta, delta) series
    #    of the 66-row protocol (M = 44: at 66 rows the weighted K = 2 case is cut by its byte budget before the clamp)
    "boot2d-K1": dict(which=BOOT2D, sch="syn2-44", K=1, N=16, B=2, M=44, r=6, row_bytes=8 * 2 * 44, seed=81),
    "boot2d-K2": dict(which=BOOT2D, sch="syn2-44", K=2, N=16, B=2, M=44, r=6, row_bytes=8 * 2 * 44, seed=82),
    "wboot2d-K1": dict(which=WBOOT2D, sch="syn2-44", K=1, N=16, B=2, M=44, r=6, row_bytes=8 * 2 * 44, seed=83),
    "wboot2d-K2": dict(which=WBOOT2D, sch="syn2-44", K=2, N=16, B=2, M=44, r=6, row_bytes=8 * 2 * 44, seed=84),
}
# voxels of the classes that ride along in the mixed batches of seams 5 and 6 (one each of the distinct ones)
MIXED_OTHERS = ("N", "NN_1")


def sizes(name):
    """(L, V, cuts) of a case: the library's items per piece, the voxels of the big call (for the mixed batches: of the
    bin that crosses), and the positions where the call starts a new piece"""
    c = CASES[name]
    L = seam(c["which"], c.get("M", 0), c.get("per_vox", 0))
    V = L + c["r"]
    also = [seam(w) for w in c.get("also", ())]
    return L, V, positions(V, L, *also)


def indices(name):
    """(idx [V], the seed used) of a case"""
    L, V, cuts = sizes(name)
    return draw(V, cuts, CASES[name]["seed"], CASES[name].get("D", D))


def host_bytes(name):
    """bytes of the largest host array the case builds (for the mixed batches the other classes' voxels included)"""
    _, V, _ = sizes(name)
    if name.startswith("upload-rfit2d"):
        V += 2 * D
    elif name.startswith("upload-"):
        V += len(MIXED_OTHERS) * D
    return V * CASES[name]["row_bytes"]


# ---- byte budgets that must NOT be what cuts where a clamp is under test (restated from the sources; the GPU tests ask the
# library where it answers: mfx_solve_soft_bytes_per_signal)
DEFAULT_BYTES = 256 << 20      # SB_DEFAULT_BYTES, BOOT_DEFAULT_BYTES


def boot2d_shared_bytes(K, N, M, B, weighted):
    """b2_rows_bytes / wb2_rows_bytes of the shared-fit route (csrc/boot2d.hip, csrc/wboot2d.hip)"""
    NP = (N + 15) & ~15
    core = (NP * NP if K == 2 else 0) + K * NP * (B + 1) + B
    return 8 * (M + 1 + B * M + core) + 4 if weighted else 8 * core


def mixed_layout(V_nn, seed):
    """class label per voxel of a mixed batch: V_nn voxels "NN" with the D voxels of every class of MIXED_OTHERS
    scattered among them (a fixed permutation), so that every bin's index list is a true gather"""
    labels = np.array(["NN"] * V_nn + [c for c in MIXED_OTHERS for _ in range(D)])
    return labels[np.random.default_rng(1000 + seed).permutation(labels.size)]

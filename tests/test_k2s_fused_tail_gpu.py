"""The screening kernel's fused pass: for dictionaries with one row tile left after full rounds of eight, the shared last
row tile is swept FIRST and makes D2's column statistics on its way (no separate statistics pass).  Every case: at most
256 voxels, the screening kernel under both chunk-image schedules bit for bit equal to the FP64 kernel, the first 4 voxels
equal to the oracle, no guard hit and no audited pair beyond a quarter of the margin."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

Z = np.array([0.0, 0.0, 1.0])
RTOL_W = 1e-5


def _tables(ms):
    return {"S": ms.S, "N": ms.num_subs, "G_un": ms.Gms_un, "off": ms.off, "x": ms.x_flat, "Y": ms.Y_flat,
            "scheme_DeldelTE": ms["scheme_DeldelTE"]}


def _second_peak(rng, p1, deg):
    r = rng.standard_normal(p1.shape)
    r -= (r * p1).sum(1, keepdims=True) * p1
    r /= np.linalg.norm(r, axis=1, keepdims=True)
    a = np.deg2rad(deg)
    p2 = np.cos(a) * p1 + np.sin(a) * r
    return p2 / np.linalg.norm(p2, axis=1, keepdims=True)


def _model(N, dirs, seed, dup=False):
    from microstructure_fingerprinting_amd import synth
    from microstructure_fingerprinting_amd import mf_utils as mfu
    rng = np.random.default_rng(seed)
    sch = synth.make_scheme(rng, 2, [1000, 2000, 3000], dirs)
    dic = synth.make_dictionary(rng, sch, N)
    if dup:
        dic[:, N - 1] = dic[:, 3]      # the first-index rule must pick 3
    ms = mfu.init_PGSE_multishell_interp(dic, sch, Z)
    return rng, sch, ms


def _voxels(rng, plan, N, M):
    """64 voxels: 32 generic noisy mixtures, then single-fascicle voxels whose atom lies in the last tile (each dictionary in
    turn), voxels made of atom 3 alone (== column N - 1 where the dictionary has the duplicate), identical peaks, peaks
    0.2 degrees apart, noise-free voxels and an all-zero signal."""
    import torch
    from microstructure_fingerprinting_amd import engine, synth
    V = 64
    dev = torch.device("cuda", 0)
    p1, p2 = synth.unit_vectors(rng, V), synth.unit_vectors(rng, V)
    atoms = rng.integers(0, N, (V, 2)).astype(np.int32)
    nu = rng.dirichlet(np.ones(2), V)
    noise = rng.normal(0, 500 / 30.0, (V, M))
    last = 32 * ((N - 1) // 32)       # first atom of the last row / column tile
    nu[32:36] = [1.0, 0.0]; atoms[32:36, 0] = rng.integers(last, N, 4)
    nu[36:40] = [0.0, 1.0]; atoms[36:40, 1] = rng.integers(last, N, 4)
    nu[40:42] = [1.0, 0.0]; atoms[40:42, 0] = 3
    nu[42:44] = [0.0, 1.0]; atoms[42:44, 1] = 3
    noise[40:44] = 0.0
    p2[44:48] = p1[44:48]
    p2[48:52] = _second_peak(rng, p1[48:52], 0.2)
    noise[52:58] = 0.0
    atoms[52:55, 0] = rng.integers(last, N, 3)
    atoms[55:58, 1] = rng.integers(last, N, 3)
    peaks = np.concatenate([p1, p2], axis=1)
    d_pk = torch.from_numpy(peaks).to(dev)
    d_Y = torch.zeros((V, M), dtype=torch.float64, device=dev)
    for k in range(2):
        col = engine.rotate_columns_dev(plan, d_pk[:, 3 * k:3 * k + 3].contiguous(), torch.from_numpy(atoms[:, k].copy()).to(dev))
        d_Y += 500.0 * torch.from_numpy(nu[:, k:k + 1].copy()).to(dev) * col
    d_Y += torch.from_numpy(noise).to(dev)
    d_Y[58:60] = 0.0
    return peaks, d_pk, d_Y


def _compare(ms, sch, plan, peaks, d_pk, d_Y, cap=0):
    """Screening kernel (both schedules) against the FP64 kernel, bit for bit; counters; oracle on the first 4 voxels."""
    import torch
    from microstructure_fingerprinting_amd import _lib as L
    from microstructure_fingerprinting_amd import engine
    from oracle import oracle as orc
    lib = L.lib()
    res, cnt = [], []
    try:
        for screen, images in ((1, 0), (1, 2), (0, 0)):
            lib.mfx_debug_set_k2_screen(screen)
            lib.mfx_debug_set_k2s_images(images)
            lib.mfx_debug_set_k2s_cap(cap if screen else 0)
            out = engine.fit_batch_dev(plan, d_Y, d_pk, 2)
            torch.cuda.synchronize()
            cnt.append((lib.mfx_debug_last_fallback_count(), lib.mfx_debug_last_guard_count(), lib.mfx_debug_last_counter(8)))
            res.append(out.cpu().numpy())
    finally:
        lib.mfx_debug_set_k2_screen(1)
        lib.mfx_debug_set_k2s_images(0)
        lib.mfx_debug_set_k2s_cap(0)
    for r, c, what in ((res[0], cnt[0], "as many images as fit"), (res[1], cnt[1], "two chunk images")):
        print("%s: handed back %d, guard %d, audit beyond a quarter of the margin %d" % ((what,) + c))
        bad = np.where(np.any(r != res[2], axis=1))[0]
        assert bad.size == 0, "screening kernel (%s) differs from the FP64 kernel in voxels %s" % (what, bad[:10])
        assert c[1] == 0 and c[2] == 0, c
    ns = 4
    z = np.zeros(ns, bool)
    ref = orc.fit_batch(_tables(ms), sch, d_Y[:ns].cpu().numpy(), np.full(ns, 2), z, z, peaks[:ns], 2, False, False, None, None, 0,
                        nthreads=4)
    assert np.array_equal(res[0][:ns, 3:5], ref[:, 3:5]), "selected atom indices differ from the oracle's"
    assert np.allclose(res[0][:ns], ref, rtol=RTOL_W, atol=1e-10)
    return res, cnt


# nine tiles = one full round + the fused pass: 1, 14 and 32 atoms in the last tile; KS = 4 and once KS = 13;
# 256: no last tile (the statistics pass of phase 1, as before)
@pytest.mark.parametrize("N,dirs", [(257, [12, 12, 12]), (270, [12, 12, 12]), (288, [12, 12, 12]), (270, [66, 66, 66]),
                                    (256, [12, 12, 12])])
def test_fused_tail_tile_edges(N, dirs):
    rng, sch, ms = _model(N, dirs, 4000 + N + dirs[0], dup=True)
    plan = ms.plan_for(sch)
    peaks, d_pk, d_Y = _voxels(rng, plan, N, sch.shape[0])
    res, _ = _compare(ms, sch, plan, peaks, d_pk, d_Y)
    # first index on ties: the voxels made of atom 3 alone (column N - 1 is its copy) name atom 3, for D1 and for D2
    assert np.all(res[0][40:42, 3] == 3) and np.all(res[0][42:44, 4] == 3), res[0][40:44, 1:5]


def test_fused_tail_bracketed_rows():
    """G-bracketed protocol (BR = true), built as in test_k2_screening_kernel_bracketed_protocol, at N = 270."""
    rng, sch_ms, ms = _model(270, [12, 12, 12], 4600)
    Gs = ms["Gms_un"]
    sch = sch_ms.copy()
    nz = np.where(sch[:, 3] > 0)[0]
    between = [0.3 * Gs[1] + 0.7 * Gs[2], 0.55 * Gs[2] + 0.45 * Gs[3], 0.9 * Gs[2] + 0.1 * Gs[3], 0.5 * (Gs[1] + Gs[2])]
    sch[nz[::2], 3] = rng.choice(between, size=nz[::2].size)
    plan = ms.plan_for(sch)
    peaks, d_pk, d_Y = _voxels(rng, plan, 270, sch.shape[0])
    _compare(ms, sch, plan, peaks, d_pk, d_Y)


def test_fused_tail_ring_overflow_hands_back():
    """A ring of 16 entries at N = 270: voxels overflow it and take the hand-back path; results still identical."""
    rng, sch, ms = _model(270, [12, 12, 12], 4700)
    plan = ms.plan_for(sch)
    peaks, d_pk, d_Y = _voxels(rng, plan, 270, sch.shape[0])
    _, cnt = _compare(ms, sch, plan, peaks, d_pk, d_Y, cap=16)
    assert cnt[0][0] > 0 and cnt[1][0] > 0, cnt


def test_two_fascicles_plus_csf_keeps_old_route():
    """The [N, N, 1] class (XC) at N = 270: statistics before the sweep, shared tile last, as before - bit-identical to
    the FP64 kernel of the class."""
    from microstructure_fingerprinting_amd import _lib as L
    from microstructure_fingerprinting_amd import engine, synth
    from microstructure_fingerprinting_amd import mf_utils as mfu
    from oracle import oracle as orc
    N, V = 270, 64
    rng, sch, ms = _model(N, [30, 30, 30], 4800)
    plan = ms.plan_for(sch)
    M = sch.shape[0]
    gam = mfu.get_gyromagnetic_ratio('H')
    b = (gam * sch[:, 3] * sch[:, 5]) ** 2 * (sch[:, 4] - sch[:, 5] / 3)
    sig_csf = np.exp(-sch[:, 6] / 2.0) * np.exp(-b * 3.0e-9)
    peaks, d_pk, d_Y = _voxels(rng, plan, N, M)
    Y = d_Y.cpu().numpy() * 0.7 + 500.0 * 0.3 * sig_csf
    one, zero = np.ones(V, bool), np.zeros(V, bool)
    args = (plan, Y, np.full(V, 2), one, zero, peaks, 2, True, False, sig_csf, None, 0)
    lib = L.lib()
    got, cnt = [], []
    try:
        for images in (0, 2):
            lib.mfx_debug_set_k2s_images(images)
            got.append(engine.fit_batch(*args))
            # handed to the plain kernel, bound check fired, guard, audited pairs beyond a quarter of the margin, audited pairs
            cnt.append((lib.mfx_debug_last_counter(4), lib.mfx_debug_last_counter(5), lib.mfx_debug_last_guard_count(),
                        lib.mfx_debug_last_counter(8), lib.mfx_debug_last_counter(10)))
        lib.mfx_debug_set_k2s_images(0)
        lib.mfx_debug_set_k2x_screen(0)
        plain = engine.fit_batch(*args)
    finally:
        lib.mfx_debug_set_k2s_images(0)
        lib.mfx_debug_set_k2x_screen(1)
    for g, c, what in ((got[0], cnt[0], "as many images as fit"), (got[1], cnt[1], "two chunk images")):
        print("[N, N, 1] %s: handed back %d of %d, bound check %d, guard %d, audit beyond a quarter of the margin %d of %d pairs"
              % ((what, c[0], V) + c[1:]))
        assert np.array_equal(g, plain), "rows differ (%s): %s" % (what, np.flatnonzero(np.any(g != plain, axis=1))[:10])
        assert c[1] == 0 and c[2] == 0 and c[3] == 0, c
        # the screening pipeline itself must decide: every degenerate voxel (the second half of _voxels) may go back to the
        # plain kernel, of the 32 generic mixtures at most the 35 % tests/test_parity_stress_gpu.py allows its mixture
        assert c[0] <= 32 + 0.35 * 32, c
        assert c[4] >= V - c[0] - 32, c     # ... and it audits a pair of (nearly) every voxel it decides (as there: > V / 2)
    ns = 4
    ref = orc.fit_batch(_tables(ms), sch, Y[:ns], np.full(ns, 2), one[:ns], zero[:ns], peaks[:ns], 2, True, False, sig_csf, None, 0,
                        nthreads=4)
    # (atom indices are whole numbers: equal within 1e-5 relative means equal)
    assert got[0][:ns].shape == ref.shape and np.allclose(got[0][:ns], ref, rtol=RTOL_W, atol=1e-10), (got[0][:ns], ref)

"""The ingestion path every real fit enters through - MFModel.fit(<file>) -> nifti.load_raw -> mfx_fit_batch_volume /
mfx_volume_rows -> mfx_volume_gather_kernel - against NumPy in float64, bit for bit: the scalar types at their extremes,
the kernel's 64 x 64 tile edges, volumes that take more than two 64 MiB staging slices, and files whose headers carry
a scaling or the other byte order.  The referee is `x.astype(float64) * slope + inter` (two roundings) where the
header's scaling applies and `x.astype(float64)` where it does not."""
import numpy as np
import pytest

from _nifti_writer import write_nifti1

Z = np.array([0.0, 0.0, 1.0])
SLICE = 64 << 20        # bytes per staging slice (csrc/mfx_api.hip: pipe_setup(min(vol_bytes, 64 MiB)))

# (slope, inter, applies): `applies` is nibabel's rule written out by hand, not taken from the code under test
SCALINGS = [(0.0, 0.0, False), (1.0, 0.0, False), (1.0, 0.5, True), (-2.5e-3, 1e4, True),
            (float(np.float32(0.0173)), -3.5, True), (float("nan"), 0.0, False), (float("inf"), 0.0, False),
            (1e300, 0.0, True), (1e-320, 0.0, True), (2.25, float("nan"), True)]

_F4 = np.finfo(np.float32)
_F8 = np.finfo(np.float64)
SEAMS = {
    "u1": [0, 127, 128, 255],
    "i1": [-128, -1, 0, 127],
    "i2": [-32768, -1, 32767],
    "u2": [0, 32767, 32768, 65535],
    "i4": [-2 ** 31, -2 ** 24 - 1, 2 ** 24 + 1, 2 ** 31 - 1],
    "u4": [0, 2 ** 24 + 1, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 32 - 1],
    "f4": [_F4.smallest_subnormal, -_F4.smallest_subnormal, _F4.tiny, _F4.max, np.float32(0.0), np.float32(-0.0),
           np.float32(np.inf), np.float32(-np.inf), np.float32(np.nan)],
    "f8": [_F8.smallest_subnormal, -_F8.smallest_subnormal, _F8.tiny, _F8.max, 0.0, -0.0, np.inf, -np.inf, np.nan,
           1e300, float(_F4.smallest_subnormal), float(_F4.tiny), float(_F4.max)],
}


def _referee(x, slope, inter, applies):
    x = np.asarray(x).astype(np.float64)         # exact for every type here
    if not applies:
        return x
    with np.errstate(all="ignore"):
        return x * slope + inter


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _assert_same_bits(got, ref, what):
    """NaN where the referee has NaN, the same 64 bits (so the same sign of zero) everywhere else."""
    assert got.shape == ref.shape and got.dtype == np.float64, what
    gn, rn = np.isnan(got), np.isnan(ref)
    bad = (gn != rn) | (~rn & (_bits(got) != _bits(ref)))
    if bad.any():
        i = tuple(int(k) for k in np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d values differ, first at %s: got %r, referee %r"
                             % (what, int(bad.sum()), bad.size, i, got[i], ref[i]))


def _random_fill(rng, dt, shape):
    """Values over the whole range of ``dt`` as an array of ``shape`` in file (Fortran) order."""
    dt = np.dtype(dt)
    if dt.kind in "iu":
        info = np.iinfo(dt)
        a = rng.integers(info.min, info.max, shape[::-1], dtype=dt, endpoint=True)
    else:
        span = 37 if dt == np.float32 else 300
        with np.errstate(over="ignore"):             # a few values beyond float32's range become inf: welcome
            a = (rng.standard_normal(shape[::-1]) * 10.0 ** rng.uniform(-span, span, shape[::-1])).astype(dt)
    return a.T          # the transpose of a C-ordered array: Fortran-contiguous


# ---------------------------------------------------------------------------------------------------------------
# A. every scalar type at its extremes x every kind of header scaling
@pytest.mark.gpu
@pytest.mark.parametrize("key", ["u1", "i1", "i2", "u2", "i4", "u4", "f4", "f8"])
def test_gather_type_extremes_and_scalings(key):
    from microstructure_fingerprinting_amd import engine
    dt = np.dtype(key)
    rng = np.random.default_rng(100 + engine.FileOrderVolume.NIFTI_CODES[key])
    grid, M = (5, 7, 3), 70                           # 105 voxels; 70 images: one full tile of 64 and one of 6
    nvox = int(np.prod(grid))
    raw = _random_fill(rng, dt, grid + (M,))
    assert raw.flags.f_contiguous and not raw.flags.c_contiguous and raw.shape == grid + (M,) and raw.dtype == dt
    flat = raw.reshape(-1, M, order="F")              # a view: [voxel in file order, image]
    assert np.shares_memory(flat, raw)
    # the ROI: not sorted, with repeats, with the first and the last voxel
    vox = np.concatenate([[nvox - 1, 0, 57, 57], rng.permutation(nvox)[:60], [0, nvox - 1, 13, 57]]).astype(np.int64)
    seams = np.array(SEAMS[key], dtype=dt)
    # seam j sits in ROI row j (a voxel of its own), image (13 j + 5) mod 70: both tiles of images get some
    srow = np.arange(4, 4 + len(seams))
    assert len(set(vox[srow].tolist())) == len(seams)
    scol = (13 * np.arange(len(seams)) + 5) % M
    flat[vox[srow], scol] = seams
    assert _bits(raw.reshape(-1, M, order="F")[vox[srow], scol].astype(np.float64)).tolist() == _bits(seams.astype(np.float64)).tolist()
    if dt.kind in "iu":
        assert raw.min() == np.iinfo(dt).min and raw.max() == np.iinfo(dt).max
    for slope, inter, applies in SCALINGS:
        what = "%s, slope %r, inter %r" % (key, slope, inter)
        vol = engine.FileOrderVolume(raw, slope, inter)
        got = engine.volume_rows(vol, vox)
        for j, s in enumerate(seams):                 # the seams one by one: a failure names the type and the value
            ref_j = _referee(s, slope, inter, applies)
            g = got[srow[j], scol[j]]
            assert (np.isnan(g) and np.isnan(ref_j)) or _bits(g) == _bits(ref_j), \
                "%s: seam value %r came back as %r, referee %r" % (what, s, g, ref_j)
        ref = _referee(flat, slope, inter, applies)[vox]
        _assert_same_bits(got, ref, what)
        with np.errstate(all="ignore"):
            fdata = vol.get_fdata()
        _assert_same_bits(fdata.reshape(-1, M, order="F")[vox], ref, what + " (get_fdata)")


# ---------------------------------------------------------------------------------------------------------------
# B. partial tiles in both directions, and the component counts peaks / angles / tensors come with
@pytest.mark.gpu
@pytest.mark.parametrize("key", ["u2", "f4"])
def test_gather_tile_edges(key):
    from microstructure_fingerprinting_amd import engine
    dt = np.dtype(key)
    rng = np.random.default_rng(7 if key == "u2" else 8)
    nvox = 211
    slope, inter = float(np.float32(0.0173)), -3.5
    for ncomp in (1, 2, 3, 6, 63, 64, 65, 130):
        raw = _random_fill(rng, dt, (nvox, ncomp))
        assert raw.flags.f_contiguous and raw.shape == (nvox, ncomp)
        vol = engine.FileOrderVolume(raw, slope, inter)
        full = _referee(raw, slope, inter, True)
        for V in (0, 1, 63, 64, 65, 129):
            vox = rng.integers(0, nvox, V).astype(np.int64)
            if V > 1:
                vox[0], vox[-1] = nvox - 1, 0
            got = engine.volume_rows(vol, vox)
            assert got.shape == (V, ncomp)
            _assert_same_bits(got, full[vox], "%s, V = %d, ncomp = %d" % (key, V, ncomp))


# ---------------------------------------------------------------------------------------------------------------
# C. mfx_volume_rows over three staging slices
def _seam_elements(elem_bytes, n_elem):
    """Flat indices (file order) of the first element of every staging slice after the first."""
    assert SLICE % elem_bytes == 0
    return [o // elem_bytes for o in range(SLICE, n_elem * elem_bytes, SLICE)]


@pytest.mark.gpu
def test_volume_rows_across_staging_slices():
    from microstructure_fingerprinting_amd import _lib, engine
    nvox, ncomp = 47_000_003, 3
    rng = np.random.default_rng(21)
    raw = rng.integers(0, 255, (ncomp, nvox), dtype=np.uint8, endpoint=True).T      # 141 MB, file order
    assert raw.flags.f_contiguous and raw.shape == (nvox, ncomp)
    seams = _seam_elements(1, nvox * ncomp)
    assert len(seams) == 2 and raw.nbytes > 2 * SLICE                               # three slices: the loop's q >= 2 branch
    assert [(e // nvox, e % nvox) for e in seams] == [(1, 20_108_861), (2, 40_217_722)]   # (image, voxel) the seams fall in
    near = np.concatenate([np.arange(e % nvox - 2, e % nvox + 3) for e in seams])
    vox = np.concatenate([near, [0, nvox - 1], rng.integers(0, nvox, 20_000)]).astype(np.int64)
    slope, inter = float(np.float32(0.0173)), -3.5
    vol = engine.FileOrderVolume(raw, slope, inter)
    ref = _referee(raw[vox], slope, inter, True)
    _lib.check(_lib.lib().mfx_thread_release())       # staging buffers re-created at min(volume, 64 MiB) whatever ran before
    for turn in ("cold", "warm"):                     # warm: the pinned buffers and the device pool are reused
        got = engine.volume_rows(vol, vox)
        _assert_same_bits(got, ref, "uint8 volume of %d bytes, %s call" % (raw.nbytes, turn))
    del raw, vol
    _lib.check(_lib.lib().mfx_thread_release())


# ---------------------------------------------------------------------------------------------------------------
# D. mfx_fit_batch_volume over three staging slices (the other copy of the slice loop)
def _model(small, N=48, E=4):
    """small: a protocol of 30 rows (2 b0 + two shells of 14), so that a volume of > 128 MiB keeps a short fit;
    otherwise the protocol of tests/test_volume_e2e.py."""
    import microstructure_fingerprinting_amd as mf
    from microstructure_fingerprinting_amd import synth
    if small:
        rng = np.random.default_rng(3)
        sch = synth.make_scheme(rng, 2, [1000, 2000], [14, 14])
        dic = synth.make_dictionary(rng, sch, N)
    else:
        sch, dic, rng = synth.make_model("C2", N=N)
    md = {"dictionary": dic, "sch_mat": sch, "orientation": Z, "num_atom": N, "num_ear": E, "T2_csf": 2.0,
          "DIFF_csf": 3e-9, "T2_ear": 0.08, "DIFF_ear": np.linspace(0.2e-9, 1.2e-9, E), "fasc_propnames": ["rad", "fin"],
          "rad": rng.uniform(0.2e-6, 2e-6, N), "fin": rng.uniform(0.2, 0.9, N)}
    return mf.MFModel(md), sch, rng


@pytest.mark.gpu
def test_fit_batch_volume_across_staging_slices():
    from microstructure_fingerprinting_amd import _lib, engine
    model, sch, rng = _model(small=True)
    plan = model.ms_interpolator.plan_for(sch)
    M = sch.shape[0]
    assert M == 30
    nvox = (2 * SLICE + (3 << 20)) // (2 * M) + 1     # int16: 128 MiB and about 3 MiB more
    raw = rng.integers(-32768, 32767, (M, nvox), dtype=np.int16, endpoint=True).T
    assert raw.flags.f_contiguous and raw.shape == (nvox, M) and 2 * SLICE + (3 << 20) <= raw.nbytes < 2 * SLICE + (4 << 20)
    seams = _seam_elements(2, nvox * M)
    assert len(seams) == 2
    # voxels on both sides of either seam (in the image it falls in: every other image of these voxels lies well inside
    # a slice), the two ends, and voxels spread over the volume: 128 in all
    near = np.concatenate([np.arange(e % nvox - 2, e % nvox + 3) for e in seams])
    assert near.min() >= 0 and near.max() < nvox
    vox = np.concatenate([near, [0, nvox - 1]])
    vox = np.concatenate([vox, rng.choice(np.setdiff1d(np.arange(0, nvox, 997), vox), 128 - len(vox), replace=False)]).astype(np.int64)
    rng.shuffle(vox)
    assert len(vox) == 128 == len(set(vox.tolist()))
    slope, inter = float(np.float32(0.0173)), -3.5
    clean = 400 * model.dic["dictionary"][:, rng.integers(0, 48, 128)].T + rng.normal(0, 10, (128, M))
    q = np.rint((clean - inter) / slope)
    assert q.min() > -32768 and q.max() < 32767
    raw[vox] = q.astype(np.int16)                     # real signals, quantised, where the fit looks
    vol = engine.FileOrderVolume(raw, slope, inter)
    Yf = _referee(raw[vox], slope, inter, True)
    Kv = np.full(128, 1)
    pk = np.tile(Z, (128, 1))
    ref = engine.fit_batch(plan, Yf, Kv, None, None, pk, 1, False, False)
    assert np.all(ref[:, 0] > 0)                      # real fits, not rows of zeros
    _lib.check(_lib.lib().mfx_thread_release())       # staging buffers re-created at 64 MiB: three slices
    got = engine.fit_batch_volume(plan, vol, vox, Kv, None, None, pk, 1, False, False)
    assert np.array_equal(got, ref)
    _assert_same_bits(engine.volume_rows(vol, vox), Yf, "int16 volume of %d bytes" % raw.nbytes)
    del raw, vol
    _lib.check(_lib.lib().mfx_thread_release())


# ---------------------------------------------------------------------------------------------------------------
# E. MFModel.fit on files: scaling read from the header, little- and big-endian, compressed
@pytest.mark.gpu
def test_fit_from_scaled_and_big_endian_files(tmp_path):
    from microstructure_fingerprinting_amd import nifti
    from microstructure_fingerprinting_amd.engine import FileOrderVolume
    model, sch, rng = _model(small=False)
    M = sch.shape[0]
    grid = (20, 18, 16)
    ax = [(np.arange(n) + 0.5) / n * 2 - 1 for n in grid]
    mask = (ax[0][:, None, None] ** 2 + ax[1][None, :, None] ** 2 + ax[2][None, None, :] ** 2 <= 1.0).astype(np.float64)
    nvox = int(np.prod(grid))
    assert 2500 < mask.sum() < 3500
    clean = (400 * model.dic["dictionary"][:, rng.integers(0, 48, nvox)].T + rng.normal(0, 10, (nvox, M))).reshape(grid + (M,))
    peaks = np.broadcast_to(Z, grid + (3,)).copy()
    aff = np.diag([2.0, 2.0, 2.5, 1.0])
    s_u, i_u = float(np.float32(0.004)), -20.0        # uint16: signals above 111 have raw values above 32767
    s_i, i_i = float(np.float32(0.005)), 100.0        # int16: signals under 100 have negative raw values
    u16 = np.clip(np.rint((clean - i_u) / s_u), 0, 65535).astype(np.uint16)
    i16 = np.clip(np.rint((clean - i_i) / s_i), -32768, 32767).astype(np.int16)
    roi = mask > 0
    assert (u16[roi] > 32767).mean() > 0.1 and (i16[roi] < 0).mean() > 0.3 and (i16[roi] > 0).mean() > 0.1
    files = {"le_u16": (str(tmp_path / "le.nii"), u16, s_u, i_u, "<", True),
             "be_i16": (str(tmp_path / "be.nii"), i16, s_i, i_i, ">", False),
             "le_u16_gz": (str(tmp_path / "le.nii.gz"), u16, s_u, i_u, "<", True)}
    kw = dict(peaks=peaks, pgse_scheme=sch, verbose=0)
    for name, (path, arr, slope, inter, endian, device_path) in files.items():
        write_nifti1(path, arr, slope, inter, endian, aff)
        raw, s, i, _ = nifti.load_raw(path)
        assert (s, i) == (slope, inter) and np.array_equal(raw, arr), name
        assert FileOrderVolume.accepts(raw) == device_path, name      # which branch of MFModel.fit the file takes
        full = nifti.load(path)[0]
        assert np.array_equal(full, arr.astype(np.float64) * slope + inter), name
        fit = model.fit(path, mask, 1, **kw)
        fit_a = model.fit(np.ascontiguousarray(full), mask, 1, **kw)
        assert fit.params_in_mask.shape[0] == int(mask.sum())
        assert np.all(fit_a.params_in_mask[:, 0] > 0), name
        assert np.array_equal(fit.params_in_mask, fit_a.params_in_mask), name
        assert np.allclose(fit.affine, aff), name

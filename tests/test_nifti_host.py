"""The host side of volume ingestion without a GPU: nifti.load_raw / nifti.load on files whose headers carry a scaling
and either byte order (written by tests/_nifti_writer.py, not by nifti.save), and the rule that decides whether a
header's scl_slope / scl_inter apply."""
import numpy as np
import pytest

from _nifti_writer import write_nifti1

# (slope, inter, applies): the scalings of tests/test_volume_ingest_gpu.py; `applies` is nibabel's rule written out
SCALINGS = [(0.0, 0.0, False), (1.0, 0.0, False), (1.0, 0.5, True), (-2.5e-3, 1e4, True),
            (float(np.float32(0.0173)), -3.5, True), (float("nan"), 0.0, False), (float("inf"), 0.0, False),
            (1e300, 0.0, True), (1e-320, 0.0, True), (2.25, float("nan"), True)]


def _u16_volume(rng):
    a = rng.integers(0, 65535, (6, 5, 4, 7), endpoint=True).astype(np.uint16)
    a[0, 0, 0, :4] = (0, 32767, 32768, 65535)
    return a


@pytest.mark.parametrize("ext", [".nii", ".nii.gz"])
@pytest.mark.parametrize("endian", ["<", ">"])
def test_load_raw_and_load_honour_header_scaling_and_byte_order(tmp_path, endian, ext):
    from microstructure_fingerprinting_amd import nifti
    from microstructure_fingerprinting_amd.engine import FileOrderVolume
    rng = np.random.default_rng(11)
    aff = np.diag([2.0, 2.0, 2.5, 1.0]); aff[:3, 3] = [-6, -5, -4]
    i16 = rng.integers(-32768, 32767, (6, 5, 4, 7), endpoint=True).astype(np.int16)
    i16[0, 0, 0, :3] = (-32768, -1, 32767)
    for k, (a, slope, inter) in enumerate(((_u16_volume(rng), float(np.float32(0.0173)), -3.5), (i16, -0.25, 100.0),
                                           (rng.normal(0, 50, (6, 5, 4, 7)).astype(np.float32), 1.0, 0.5))):
        p = str(tmp_path / ("v%d%s" % (k, ext)))
        write_nifti1(p, a, slope, inter, endian, aff)
        raw, s, i, aff2 = nifti.load_raw(p)
        assert raw.dtype.newbyteorder("=") == a.dtype and raw.shape == a.shape and np.array_equal(raw, a)
        assert raw.flags.f_contiguous
        assert (s, i) == (slope, inter) and np.array_equal(aff2, aff)
        native = raw.dtype.isnative
        assert native == (endian == ("<" if np.little_endian else ">"))
        assert FileOrderVolume.accepts(raw) == native      # MFModel.fit: the device path / the host conversion
        full, aff3 = nifti.load(p)
        assert full.dtype == np.float64 and np.array_equal(aff3, aff)
        assert np.array_equal(full, a.astype(np.float64) * slope + inter)
        if native:
            assert np.array_equal(FileOrderVolume(raw, s, i).get_fdata(), full)


@pytest.mark.parametrize("endian", ["<", ">"])
def test_header_scalings_that_do_and_do_not_apply(tmp_path, endian):
    from microstructure_fingerprinting_amd import nifti
    a = _u16_volume(np.random.default_rng(12))
    a64 = a.astype(np.float64)
    for k, (slope, inter) in enumerate(((0.0, 7.0), (float("nan"), 7.0), (float("inf"), 7.0), (float("-inf"), 0.0), (1.0, 0.0))):
        p = str(tmp_path / ("n%d.nii" % k))
        write_nifti1(p, a, slope, inter, endian)
        raw, s, i, _ = nifti.load_raw(p)
        assert np.array_equal(raw, a) and (s == slope or (s != s and slope != slope)) and i == inter
        assert np.array_equal(nifti.load(p)[0], a64), (slope, inter)
    for k, (slope, inter) in enumerate(((1.0, -12.5), (-2.0, 0.0), (1.0, float("inf")))):
        p = str(tmp_path / ("s%d.nii" % k))
        write_nifti1(p, a, slope, inter, endian)
        assert np.array_equal(nifti.load(p)[0], a64 * slope + inter), (slope, inter)


def test_one_scaling_rule():
    """FileOrderVolume.scaled and nifti._scaled on every scaling of the GPU test, against the rule written out."""
    from microstructure_fingerprinting_amd import nifti
    from microstructure_fingerprinting_amd.engine import FileOrderVolume
    a = np.asfortranarray(np.arange(24, dtype=np.int16).reshape(2, 3, 4))
    for slope, inter, applies in SCALINGS:
        vol = FileOrderVolume(a, slope, inter)
        assert nifti._scaled(slope, inter) is applies, (slope, inter)
        assert vol.scaled is applies, (slope, inter)
        with np.errstate(all="ignore"):
            ref = a.astype(np.float64) * slope + inter if applies else a.astype(np.float64)
        assert np.array_equal(vol.get_fdata(), ref, equal_nan=True), (slope, inter)

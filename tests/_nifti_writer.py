"""A NIfTI-1 single-file writer for the tests, independent of the package's own: any byte order, any scl_slope /
scl_inter (nifti.save always writes little-endian files with slope 1, inter 0)."""
import gzip
import struct

import numpy as np

CODES = {"u1": 2, "i2": 4, "i4": 8, "f4": 16, "f8": 64, "i1": 256, "u2": 512, "u4": 768}


def write_nifti1(path, arr, slope, inter, endian="<", affine=None):
    """Write ``arr`` (its scalars as they are) to ``path`` (.nii or .nii.gz) in byte order ``endian`` ('<' or '>')
    with the header's scaling fields set to ``slope`` / ``inter`` and ``affine`` (default: identity) as sform."""
    arr = np.asarray(arr)
    key = arr.dtype.str[1:]
    aff = np.eye(4) if affine is None else np.asarray(affine, dtype=np.float64)
    e = endian
    hdr = bytearray(348)
    struct.pack_into(e + "i", hdr, 0, 348)                                               # sizeof_hdr
    struct.pack_into(e + "8h", hdr, 40, arr.ndim, *(list(arr.shape) + [1] * (7 - arr.ndim)))   # dim
    struct.pack_into(e + "hh", hdr, 70, CODES[key], arr.dtype.itemsize * 8)             # datatype, bitpix
    vox = np.sqrt(np.sum(aff[:3, :3] ** 2, axis=0))
    struct.pack_into(e + "8f", hdr, 76, 1.0, vox[0], vox[1], vox[2], 1.0, 1.0, 1.0, 1.0)   # pixdim
    struct.pack_into(e + "f", hdr, 108, 352.0)                                           # vox_offset
    struct.pack_into(e + "ff", hdr, 112, slope, inter)                                   # scl_slope, scl_inter
    struct.pack_into(e + "hh", hdr, 252, 0, 2)                                           # qform_code, sform_code
    for r in range(3):
        struct.pack_into(e + "4f", hdr, 280 + 16 * r, *aff[r])                           # srow_x, srow_y, srow_z
    hdr[344:348] = b"n+1\0"                                                              # magic
    body = np.asfortranarray(arr).astype(arr.dtype.newbyteorder(e), copy=False).tobytes(order="F")
    with (gzip.open(path, "wb", compresslevel=1) if str(path).endswith(".gz") else open(path, "wb")) as f:
        f.write(bytes(hdr) + b"\0\0\0\0" + body)

// class_batch.h -- the host side of a mixed batch, shared by mfx_fit2d_batch, mfx_wfit2d_batch, mfx_wfit_batch, mfx_rfit_batch
// and mfx_rfit2d_batch: voxels are binned by class (K fascicles, CSF flag), every class runs on contiguous copies of its
// voxels' rows, and the results go back by voxel index.  Pure host C++ on include/mfx.h and the standard library: no HIP,
// so that tests/class_batch_check.cpp exercises it as a stand-alone program.
//
// Order: bin 2 K + c, voxels ascending inside a bin; mfx_class_walk visits the bins ascending and a bin front to back.
#pragma once
#include "../../include/mfx.h"

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

int mfx_fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

typedef std::vector<std::vector<int64_t>> MfxClassBins;

// Bins the V voxels into 2 (maxfasc + 1) classes.  Per voxel K[v] is checked before the CSF flag and the first offending
// voxel is the one reported; csf null: no voxel is flagged; csf_allowed: the batch has csf_on and a CSF signal.
inline int mfx_class_bins(const char* fn, const int32_t* K, const uint8_t* csf, int maxfasc, bool csf_allowed, int64_t V,
                          MfxClassBins* bins) {
  bins->assign((size_t)2 * (maxfasc + 1), std::vector<int64_t>());
  for (int64_t v = 0; v < V; ++v) {
    const int c = csf && csf[v];
    if (K[v] < 0 || K[v] > maxfasc) return mfx_fail(MFX_ERR_ARG, "%s: K[%lld] = %d outside 0..%d", fn, (long long)v, K[v], maxfasc);
    if (c && !csf_allowed) return mfx_fail(MFX_ERR_ARG, "%s: voxels flagged CSF need csf_on and sig_csf", fn);
    (*bins)[(size_t)2 * K[v] + c].push_back(v);
  }
  return MFX_OK;
}

// body(k, c, ix, nv) on every non-empty bin in chunks of at most chunk_of(k) >= 1 voxels; the first non-zero return ends the walk
template <class ChunkOf, class Body>
int mfx_class_walk(const MfxClassBins& bins, ChunkOf chunk_of, Body body) {
  for (size_t b = 0; b < bins.size(); ++b) {
    const std::vector<int64_t>& all = bins[b];
    if (all.empty()) continue;
    const int k = (int)(b >> 1), c = (int)(b & 1);
    const size_t chunk = std::max<size_t>(1, chunk_of(k));
    for (size_t c0 = 0; c0 < all.size();) {
      const size_t nv = std::min(chunk, all.size() - c0);
      if (int rc = body(k, c, all.data() + c0, nv)) return rc;
      c0 += nv;
    }
  }
  return MFX_OK;
}
// the same chunk for every class; SIZE_MAX: a bin at a time
template <class Body>
int mfx_class_walk(const MfxClassBins& bins, size_t chunk, Body body) {
  return mfx_class_walk(bins, [chunk](int) { return chunk; }, body);
}

// dst [nv x width] = the first `width` entries of the rows ix[q] of src (leading dimension src_ld)
template <class T>
void gather_rows(T* dst, const T* src, const int64_t* ix, size_t nv, size_t src_ld, size_t width) {
  for (size_t q = 0; q < nv; ++q) std::memcpy(dst + q * width, src + (size_t)ix[q] * src_ld, sizeof(T) * width);
}
// rows ix[q] of dst (leading dimension width) = src [nv x width]
template <class T>
void scatter_rows(T* dst, const T* src, const int64_t* ix, size_t nv, size_t width) {
  for (size_t q = 0; q < nv; ++q) std::memcpy(dst + (size_t)ix[q] * width, src + q * width, sizeof(T) * width);
}

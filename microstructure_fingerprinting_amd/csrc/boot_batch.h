// boot_batch.h -- where a class's numbers land in a mixed batch of the bootstrap: the one definition of the parameter and
// statistic layouts, the two column maps class -> batch, the gather of the own fit's rows and the scatter of a class
// chunk's results into the caller's arrays, for mfx_boot_fit, mfx_wboot_fit, mfx_boot2d_fit and mfx_wboot2d_fit
// (boot_shared.h drives them).  Pure host C++ on include/mfx.h, include/mfx_boot.h and the standard library: no HIP, so
// that tests/boot_batch_check.cpp exercises it as a stand-alone program.
//
// Layouts (include/mfx.h, include/mfx_boot.h) for F fascicles, a CSF column (c) and the EAR columns (e):
//   parameters  M0 | nu_f [F] | index_f [F] | nu_csf [c] | nu_ear, index_ear [e] | MSE, R2
//   statistics  M0 | nu_f [F] | nu_csf [c] | nu_ear [e] | MSE | properties [F x nprop], fascicle-major
// The families without EAR pass e = 0.
#pragma once
#include "../../include/mfx.h"
#include "../../include/mfx_boot.h"

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

inline int boot_np(int F, int c, int e) { return 1 + 2 * F + c + 2 * e + 2; }                   // parameters of a row
inline int boot_c0(int F, int c, int e) { return 2 + F + c + e; }                               // statistic columns before the properties
inline int boot_ncol(int F, int c, int e, int nprop) { return boot_c0(F, c, e) + F * nprop; }   // statistic columns

// voxels per upload of a mixed batch: what four device chunks of replicate signals hold, 65536 at the most
inline size_t boot_upload_chunk(int64_t budget, int B, int M) {
  return (size_t)std::max<int64_t>(1, std::min<int64_t>(65536, 4 * std::max<int64_t>(1, budget / ((int64_t)B * M * 8))));
}

// The columns of a class (k fascicles, cf, e) inside a batch (F, csf_on, ear_on, nprop): class parameter j is the
// batch's parameter pmap[j], class statistic column c the batch's cmap[c].  Built once per class chunk.
struct BootColMap {
  int F, csf_on, ear_on, nprop;   // the batch
  int k, cf, e;                   // the class
  int npF, CF, npc, Cc;           // parameters and statistic columns of the batch and of the class
  std::vector<int> pmap, cmap;
  BootColMap(int F_, int csf_on_, int ear_on_, int nprop_, int k_, int cf_, int e_)
      : F(F_), csf_on(csf_on_), ear_on(ear_on_), nprop(nprop_), k(k_), cf(cf_), e(e_), npF(boot_np(F_, csf_on_, ear_on_)),
        CF(boot_ncol(F_, csf_on_, ear_on_, nprop_)), npc(boot_np(k_, cf_, e_)), Cc(boot_ncol(k_, cf_, e_, nprop_)), pmap(npc), cmap(Cc) {
    pmap[0] = 0;
    for (int f = 0; f < k; ++f) { pmap[1 + f] = 1 + f; pmap[1 + k + f] = 1 + F + f; }
    if (cf) pmap[1 + 2 * k] = 1 + 2 * F;
    if (e) { pmap[1 + 2 * k + cf] = 1 + 2 * F + csf_on; pmap[2 + 2 * k + cf] = 2 + 2 * F + csf_on; }
    pmap[npc - 2] = npF - 2; pmap[npc - 1] = npF - 1;
    cmap[0] = 0;
    for (int f = 0; f < k; ++f) cmap[1 + f] = 1 + f;
    if (cf) cmap[1 + k] = 1 + F;
    if (e) cmap[1 + k + cf] = 1 + F + csf_on;
    cmap[1 + k + cf + e] = 1 + F + csf_on + ear_on;
    for (int f = 0; f < k; ++f)
      for (int t = 0; t < nprop; ++t) cmap[boot_c0(k, cf, e) + f * nprop + t] = boot_c0(F, csf_on, ear_on) + f * nprop + t;
  }
};

// the own fit of the voxels ix[0 .. nv) in the class's layout: rows [nv x npc] out of params0 [V x npF]
inline std::vector<double> boot_gather_params0(const BootColMap& m, const double* params0, const int64_t* ix, size_t nv) {
  std::vector<double> rows(nv * m.npc);
  for (size_t i = 0; i < nv; ++i)
    for (int j = 0; j < m.npc; ++j) rows[i * m.npc + j] = params0[(size_t)ix[i] * m.npF + m.pmap[j]];
  return rows;
}

// the counter keys of the voxels ix[0 .. nv): the caller's batch indices vox[ix[i]], or the positions themselves
inline std::vector<int64_t> boot_vox_keys(const int64_t* vox, const int64_t* ix, size_t nv) {
  std::vector<int64_t> vi(nv);
  for (size_t i = 0; i < nv; ++i) vi[i] = vox ? vox[ix[i]] : ix[i];
  return vi;
}

// The downloaded results of a class chunk - hs [nv x Cc x NS] (NS = MFX_BOOT_NSTAT + Q), ha [nv x max(k, 1)], hst [nv],
// hk [nv x B x npc] or null - into the caller's stats [V x CF x NS], agree [V x F], status [V] and keep [V x B x npF] (or
// null) at the voxels ix.  Per voxel all CF columns are filled first with the statistics of a column the class does not
// have - a weight that is 0 in every replicate (n = B), a property that is never valid (n = 0); n = 0 everywhere for a
// voxel in a non-zero status - and the class's columns are copied over them; agree is 0 beyond the class's fascicles;
// a keep row is 0 (NaN for a non-zero status) outside the class's columns.
inline void boot_scatter(const BootColMap& m, const int64_t* ix, size_t nv, int B, int Q, const double* hs, const int32_t* ha,
                         const int32_t* hst, const double* hk, double* stats, int32_t* agree, int32_t* status, double* keep) {
  const int F = m.F, k = m.k, NS = MFX_BOOT_NSTAT + Q;
  const double qnan = __builtin_nan("");
  for (size_t i = 0; i < nv; ++i) {
    const size_t v = (size_t)ix[i];
    const bool ok = hst[i] == 0;
    status[v] = hst[i];
    double* sv = stats + v * m.CF * NS;
    for (int c = 0; c < m.CF; ++c) {
      double* s = sv + (size_t)c * NS;
      const bool weight = c < boot_c0(F, m.csf_on, m.ear_on);
      if (weight && ok) {
        s[0] = (double)B; s[1] = 0.0; s[2] = B > 1 ? 0.0 : qnan; s[3] = 0.0; s[4] = 0.0;
        for (int t = 0; t < Q; ++t) s[MFX_BOOT_NSTAT + t] = 0.0;
      } else {
        s[0] = 0.0;
        for (int t = 1; t < NS; ++t) s[t] = qnan;
      }
    }
    for (int c = 0; c < m.Cc; ++c) std::memcpy(sv + (size_t)m.cmap[c] * NS, hs + (i * m.Cc + c) * NS, sizeof(double) * NS);
    for (int f = 0; f < F; ++f) agree[v * F + f] = f < k ? ha[i * k + f] : 0;
    if (keep)
      for (int b = 0; b < B; ++b) {
        double* dst_row = keep + (v * B + b) * m.npF;
        for (int j = 0; j < m.npF; ++j) dst_row[j] = ok ? 0.0 : qnan;
        for (int j = 0; j < m.npc; ++j) dst_row[m.pmap[j]] = hk[(i * B + b) * m.npc + j];
      }
  }
}

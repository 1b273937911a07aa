// boot_batch_check.cpp -- stand-alone check of csrc/boot_batch.h (tests/test_boot_batch_host.py compiles it with the host
// compiler and -fsanitize=address,undefined and runs it): the layouts, the two column maps of every class in every batch,
// the gather of the own fit's rows, the scatter of a class chunk and the voxels-per-upload formula.  The expectations are
// written by column NAMES (include/mfx.h, include/mfx_boot.h), not by the header's index formulas.  Exit status 0 and "ok"
// on stdout when every check holds; else the failed lines.
#include "../microstructure_fingerprinting_amd/csrc/boot_batch.h"

#include <cmath>
#include <cstdio>
#include <string>

static int g_failed = 0;

#define CHECK(x)                                                   \
  do {                                                             \
    if (!(x)) { printf("line %d: %s\n", __LINE__, #x); ++g_failed; } \
  } while (0)

typedef std::vector<std::string> Names;

// a parameter row: M0, nu_f, index_f, nu_csf, nu_ear and its index, then the two trailing columns
static Names param_names(int F, int c, int e) {
  Names n;
  n.push_back("M0");
  for (int f = 0; f < F; ++f) n.push_back("nu_f" + std::to_string(f));
  for (int f = 0; f < F; ++f) n.push_back("index_f" + std::to_string(f));
  if (c) n.push_back("nu_csf");
  if (e) { n.push_back("nu_ear"); n.push_back("index_ear"); }
  n.push_back("MSE");
  n.push_back("R2");
  return n;
}
// the statistic columns: the weights (M0, nu_f, nu_csf, nu_ear, MSE), then the properties per fascicle
static Names stat_names(int F, int c, int e, int nprop) {
  Names n;
  n.push_back("M0");
  for (int f = 0; f < F; ++f) n.push_back("nu_f" + std::to_string(f));
  if (c) n.push_back("nu_csf");
  if (e) n.push_back("nu_ear");
  n.push_back("MSE");
  for (int f = 0; f < F; ++f)
    for (int t = 0; t < nprop; ++t) n.push_back("prop" + std::to_string(t) + "_f" + std::to_string(f));
  return n;
}
static int find(const Names& names, const std::string& s) {
  for (size_t i = 0; i < names.size(); ++i)
    if (names[i] == s) return (int)i;
  return -1;
}
static bool is_prop(const std::string& s) { return s.compare(0, 4, "prop") == 0; }
static bool same(double a, double b) { return (std::isnan(a) && std::isnan(b)) || a == b; }

// one map: inside its range, injective, and every class column on the batch column of the same name
static void check_one_map(const std::vector<int>& map, const Names& cls, const Names& batch) {
  CHECK(map.size() == cls.size());
  std::vector<int> hit(batch.size(), 0);
  for (size_t j = 0; j < map.size() && j < cls.size(); ++j) {
    CHECK(map[j] >= 0 && map[j] < (int)batch.size());
    if (map[j] < 0 || map[j] >= (int)batch.size()) continue;
    CHECK(++hit[map[j]] == 1);
    CHECK(map[j] == find(batch, cls[j]));
  }
}

static void check_maps() {
  const int nprops[3] = {0, 1, 3};
  int classes = 0;
  for (int F = 0; F <= 3; ++F)
    for (int csf_on = 0; csf_on <= 1; ++csf_on)
      for (int ear_on = 0; ear_on <= 1; ++ear_on)
        for (int nprop : nprops) {
          const Names pF = param_names(F, csf_on, ear_on), sF = stat_names(F, csf_on, ear_on, nprop);
          CHECK((int)pF.size() == boot_np(F, csf_on, ear_on));
          CHECK((int)sF.size() == boot_ncol(F, csf_on, ear_on, nprop));
          CHECK(boot_c0(F, csf_on, ear_on) == find(sF, "MSE") + 1);
          for (int k = 0; k <= F; ++k)
            for (int cf = 0; cf <= csf_on; ++cf)
              for (int e = 0; e <= ear_on; ++e) {
                const BootColMap m(F, csf_on, ear_on, nprop, k, cf, e);
                CHECK(m.npF == (int)pF.size() && m.CF == (int)sF.size());
                CHECK(m.npc == boot_np(k, cf, e) && m.Cc == boot_ncol(k, cf, e, nprop));
                check_one_map(m.pmap, param_names(k, cf, e), pF);
                check_one_map(m.cmap, stat_names(k, cf, e, nprop), sF);
                ++classes;
              }
        }
  CHECK(classes == 3 * (1 + 2 + 2 + 4) * (1 + 2 + 3 + 4));
}

// The fake batch of the scatter check: F = 2, CSF and EAR on, two property tables; 11 voxels over five classes, the voxels of
// a class in no particular order, one class with a single voxel.  The classes are scattered one after another into arrays full of a sentinel.
struct FakeClass { int k, cf, e; std::vector<int64_t> ix; };
static const int SF = 2, SCSF = 1, SEAR = 1, SNPROP = 2, SV = 11;
static std::vector<FakeClass> fake_classes() {
  return {{0, 0, 0, {7}}, {1, 1, 0, {9, 3, 0}}, {2, 0, 1, {10, 2}}, {2, 1, 1, {5, 8, 1}}, {1, 0, 0, {6, 4}}};
}
static int fake_status(int64_t v) { return v == 10 ? 4 : (v % 4 == 1 ? 2 : 0); }   // voxels 1, 5, 9 and 10 are not fine
static double stat_value(int64_t v, int c, int t) { return 1000.0 * (double)v + 10.0 * c + t + 0.5; }
static double keep_value(int64_t v, int b, int j) { return 10000.0 * (double)v + 100.0 * b + j + 0.25; }
static int agree_value(int64_t v, int f) { return 100 * (int)v + f + 1; }
static const double SENT = -77.0;

static void check_scatter(int B, int Q, bool with_keep) {
  const int NS = MFX_BOOT_NSTAT + Q;
  const Names pF = param_names(SF, SCSF, SEAR), sF = stat_names(SF, SCSF, SEAR, SNPROP);
  const int npF = (int)pF.size(), CF = (int)sF.size();
  std::vector<double> stats((size_t)SV * CF * NS, SENT), keep(with_keep ? (size_t)SV * B * npF : 0, SENT);
  std::vector<int32_t> agree((size_t)SV * SF, (int32_t)SENT), status(SV, (int32_t)SENT);
  const std::vector<FakeClass> classes = fake_classes();
  std::vector<int> done(SV, 0);
  int with_status = 0, without = 0;
  // every cell of a class's voxels, by name
  auto check_class = [&](const FakeClass& fc) {
    const Names pc = param_names(fc.k, fc.cf, fc.e), sc = stat_names(fc.k, fc.cf, fc.e, SNPROP);
    for (int64_t v : fc.ix) {
      const int st = fake_status(v);
      CHECK(status[v] == st);
      for (int J = 0; J < CF; ++J) {
        const double* s = &stats[((size_t)v * CF + J) * NS];
        const int c = find(sc, sF[J]);
        for (int t = 0; t < NS; ++t) {
          double want;
          if (c >= 0) want = stat_value(v, c, t);                      // a column of the class: what the device gave
          else if (!is_prop(sF[J]) && st == 0) want = t == 0 ? (double)B : (t == 2 && B == 1 ? NAN : 0.0);   // a weight that is 0 in every replicate
          else want = t == 0 ? 0.0 : NAN;                              // a property that is never valid; a voxel that is not fine
          CHECK(same(s[t], want));
        }
      }
      for (int f = 0; f < SF; ++f) CHECK(agree[v * SF + f] == (f < fc.k ? agree_value(v, f) : 0));
      if (with_keep)
        for (int b = 0; b < B; ++b)
          for (int J = 0; J < npF; ++J) {
            const int j = find(pc, pF[J]);
            const double want = j >= 0 ? keep_value(v, b, j) : (st == 0 ? 0.0 : NAN);
            CHECK(same(keep[((size_t)v * B + b) * npF + J], want));
          }
    }
  };
  for (const FakeClass& fc : classes) {
    const BootColMap m(SF, SCSF, SEAR, SNPROP, fc.k, fc.cf, fc.e);
    const size_t nv = fc.ix.size();
    std::vector<double> hs(nv * m.Cc * NS), hk(nv * B * m.npc);
    std::vector<int32_t> ha(nv * (size_t)std::max(fc.k, 1), -5), hst(nv);
    for (size_t i = 0; i < nv; ++i) {
      const int64_t v = fc.ix[i];
      hst[i] = fake_status(v);
      for (int c = 0; c < m.Cc; ++c)
        for (int t = 0; t < NS; ++t) hs[(i * m.Cc + c) * NS + t] = stat_value(v, c, t);
      for (int f = 0; f < fc.k; ++f) ha[i * fc.k + f] = agree_value(v, f);
      for (int b = 0; b < B; ++b)
        for (int j = 0; j < m.npc; ++j) hk[(i * B + b) * m.npc + j] = keep_value(v, b, j);
    }
    boot_scatter(m, fc.ix.data(), nv, B, Q, hs.data(), ha.data(), hst.data(), with_keep ? hk.data() : nullptr, stats.data(), agree.data(),
                 status.data(), with_keep ? keep.data() : nullptr);
    for (int64_t v : fc.ix) {
      CHECK(!done[v]);
      done[v] = 1;
      (fake_status(v) ? with_status : without)++;
    }
    check_class(fc);
    // the voxels no class has scattered yet still hold the sentinel, every cell
    for (int64_t v = 0; v < SV; ++v) {
      if (done[v]) continue;
      CHECK(status[v] == (int32_t)SENT);
      for (int x = 0; x < CF * NS; ++x) CHECK(stats[(size_t)v * CF * NS + x] == SENT);
      for (int f = 0; f < SF; ++f) CHECK(agree[v * SF + f] == (int32_t)SENT);
      if (with_keep)
        for (int x = 0; x < B * npF; ++x) CHECK(keep[(size_t)v * B * npF + x] == SENT);
    }
  }
  CHECK(with_status >= 3 && without >= 4 && with_status + without == SV);
  // after the last chunk every voxel still holds what its own class wrote: no later scatter reached into an earlier voxel
  for (const FakeClass& fc : classes) check_class(fc);
}

// gathering the own fit through pmap and scattering it back as a keep row restores the class's columns
static void check_round_trip() {
  const Names pF = param_names(SF, SCSF, SEAR);
  const int npF = (int)pF.size();
  std::vector<double> params0((size_t)SV * npF);
  for (size_t i = 0; i < params0.size(); ++i) params0[i] = 0.125 * (double)i + 3.0;
  for (const FakeClass& fc : fake_classes()) {
    const BootColMap m(SF, SCSF, SEAR, SNPROP, fc.k, fc.cf, fc.e);
    const size_t nv = fc.ix.size();
    const std::vector<double> rows = boot_gather_params0(m, params0.data(), fc.ix.data(), nv);
    CHECK(rows.size() == nv * m.npc);
    const Names pc = param_names(fc.k, fc.cf, fc.e);
    for (size_t i = 0; i < nv; ++i)
      for (int j = 0; j < m.npc; ++j) CHECK(rows[i * m.npc + j] == params0[(size_t)fc.ix[i] * npF + find(pF, pc[j])]);
    std::vector<double> stats((size_t)SV * m.CF * MFX_BOOT_NSTAT), keep((size_t)SV * npF, SENT), hs(nv * m.Cc * MFX_BOOT_NSTAT, 0.0);
    std::vector<int32_t> agree((size_t)SV * SF), status(SV), ha(nv * (size_t)std::max(fc.k, 1), 0), hst(nv, 0);
    boot_scatter(m, fc.ix.data(), nv, 1, 0, hs.data(), ha.data(), hst.data(), rows.data(), stats.data(), agree.data(), status.data(),
                 keep.data());
    for (int64_t v : fc.ix)
      for (int J = 0; J < npF; ++J) CHECK(keep[(size_t)v * npF + J] == (find(pc, pF[J]) >= 0 ? params0[(size_t)v * npF + J] : 0.0));
  }
  // the counter keys: the caller's indices where given, else the positions
  const int64_t ix[3] = {4, 0, 2}, vox[5] = {50, 51, 52, 53, 54};
  CHECK((boot_vox_keys(nullptr, ix, 3) == std::vector<int64_t>{4, 0, 2}));
  CHECK((boot_vox_keys(vox, ix, 3) == std::vector<int64_t>{54, 50, 52}));
}

static void check_upload_chunk() {
  const int B = 3, M = 7;
  const int64_t unit = 8 * (int64_t)B * M;   // bytes of a voxel's replicate signals
  CHECK(boot_upload_chunk(1, B, M) == 4);
  CHECK(boot_upload_chunk(unit - 1, B, M) == 4);          // budget < 8 B M: one voxel per device chunk, four per upload
  CHECK(boot_upload_chunk(unit, B, M) == 4);
  CHECK(boot_upload_chunk(2 * unit, B, M) == 8);
  CHECK(boot_upload_chunk(16383 * unit, B, M) == 65532);
  CHECK(boot_upload_chunk(16384 * unit, B, M) == 65536);  // exactly the cap
  CHECK(boot_upload_chunk(16384 * unit + unit - 1, B, M) == 65536);
  CHECK(boot_upload_chunk(16385 * unit, B, M) == 65536);  // one above: clamped
  CHECK(boot_upload_chunk((int64_t)256 << 20, 200, 64) == 4 * (((int64_t)256 << 20) / (8 * 200 * 64)));
}

int main() {
  check_maps();
  const int Bs[2] = {1, 3}, Qs[2] = {0, 2};
  for (int B : Bs)
    for (int Q : Qs)
      for (int with_keep = 0; with_keep <= 1; ++with_keep) check_scatter(B, Q, with_keep != 0);
  check_round_trip();
  check_upload_chunk();
  if (g_failed == 0) printf("ok\n");
  return g_failed ? 1 : 0;
}

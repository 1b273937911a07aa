// mfx_host.h -- host-side plumbing shared by the translation units of libmfx.so.
//
// The library is built from several translation units so that the kernel families compile in parallel
// (mfx_api.hip: C ABI, tables/plans, small kernels; tu_k2.hip: FP64 two-fascicle kernel; tu_k2s_*.hip: the
// screening kernel's instantiations; tu_k2x.hip: two fascicles + CSF/EAR).  Everything mutable that is not owned
// by a handle lives in ONE thread-local record: one host thread drives one GPU (mf.py:_fit_sharded), so the error
// string, the timing events and the diagnostic switches of a thread never meet those of another.
#pragma once
#include "../../include/mfx.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "class_batch.h"
#include "fit_k2.hip"
#include "fit_k2x.hip"

#define MFX_NCOUNTERS 12   // per-call counters (mfx_debug_last_counter): [0..7] hand-backs of the kernel families, [8..10] screening audit

struct MfxThread {
  std::string err;
  // timing hook (mfx_set_profiling / mfx_last_kernel_ms)
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  int ev_launches = 0;
  bool ev_valid = false;
  bool profiling = false;
  // diagnostics (mfx_debug_*)
  unsigned long long* stamps = nullptr;
  int k2_pipe = -1;        // MFX_K2_PIPE=0 selects the un-pipelined chunk loop of the FP64 kernel
  int k2_maxc = MFX_MAXC;  // FP64 kernel: short-list size beyond which its exhaustive exact pass runs
  int k2x_maxc = MFX_XMAXC;
  int k2s_nb = 0;          // 0: as many chunk images as fit; 2: force the two-image schedule
  int k2s_cap = 0;         // 0: MFX_S_CAP
  int force_generic = 0;   // 1: every voxel class through the explicit-dictionary solver (tests of the out-of-limits fallback)
  int k3_screen = 1;       // 0: three sub-dictionaries through the plain one-thread-per-tuple scan (no batched path, no relaxed-bound screen: the referee of the full-size test)
  int k3_cap = 0;          // > 0: candidate-list entries of the batched three-fascicle path (tests force the overflow fallback)
  int k3_batch = -1;       // MFX_K3_BATCH=0: three-fascicle voxels one by one through solve_k3.hip (no batched fit_k3.hip path)
  int k2_screen = -1;      // MFX_K2_SCREEN=0 disables the screening kernels
  int k2x_screen = -1;     // MFX_K2X_SCREEN=0: the [N, N, 1] class stays on the FP64 kernel (no screening pipeline)
  int k2_wide = -1;        // MFX_K2_WIDE: 1 forces the wide screening kernel (fit_k2w.hip) wherever it applies, 0 never uses it
  // hand-back counters of the last mfx_fit_batch* call: summed on the device over its launches, copied to pinned memory
  // behind the kernels and read only when somebody asks (mfx_debug_last_*_count): the _dev entry points never synchronise
  int* fb_dev = nullptr;           // device [MFX_NCOUNTERS]: [0] voxels handed back to an exact kernel, [1] of them by the screening-error guard
  int* fb_host = nullptr;          // pinned [MFX_NCOUNTERS]
  int fb_device = -1;              // device fb_dev lives on
  hipEvent_t fb_event = nullptr;
  bool fb_pending = false;
  // host pipeline of mfx_fit_batch (pinned staging, copy/compute streams), created on first use per device
  void* stage[2] = {nullptr, nullptr};
  size_t stage_bytes = 0;
  hipStream_t s_copy = nullptr, s_comp = nullptr;
  hipEvent_t ev_h2d[2] = {nullptr, nullptr};
  int pipe_device = -1;
  // device buffers of mfx_fit_batch (signals, directions, parameters, voxel lists): kept between calls and only ever
  // grown, so that a volume fitted slab by slab does not pay an allocation and a (synchronising) release per call;
  // mfx_thread_release() returns them
  void* pool[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // [4], [5]: a volume in its file's layout and the ROI's indices into it
  size_t pool_bytes[6] = {0, 0, 0, 0, 0, 0};
  // two internal streams of the voxel-by-voxel three-fascicle path (two voxels in flight: the launch gaps and the
  // tail of one voxel's kernels are covered by the other's), forked from and joined to the caller's stream by events
  // scratch arenas (mfx_scratch_alloc): one per (device, stream) this thread has launched on
  struct Arena {
    int device = -1;
    hipStream_t stream = nullptr;
    std::vector<void*> blocks;
    std::vector<size_t> sizes;
    size_t cur = 0, off = 0;   // block in use, bytes handed out of it
    int live = 0;              // allocations not yet released
    unsigned long long used = 0;   // (LRU stamp)
  };
  std::vector<Arena> arenas;
  unsigned long long arena_clock = 0;
  hipStream_t s_lane[4] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t ev_lane[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // [lane] join, [4] fork
  int lane_device = -1;
};

MfxThread& mfx_thread();
int mfx_fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
// what every compute entry point answers first where mfx_device_count() <= 0
inline int mfx_no_device() { return mfx_fail(MFX_ERR_NO_DEVICE, "no HIP device available (this library has no CPU path)"); }
// mfx_api.hip: the device count, then the range of `device`, then hipSetDevice
int mfx_require_device(int device);

#define HIPCHK(x)                                                                                   \
  do {                                                                                              \
    hipError_t e_ = (x);                                                                            \
    if (e_ != hipSuccess) return mfx_fail(MFX_ERR_HIP, "%s failed: %s", #x, hipGetErrorString(e_)); \
  } while (0)

// ---- host seams: where an entry point cuts a batch into pieces, the items a piece holds at the most.  The host code
// uses these very expressions and mfx_debug_seam (mfx_api.hip; `which` = the MFX_SEAM_* below) returns them, so that a
// test can size its batch from the library's own figure and cross the seam whatever the figure becomes.
enum {
  MFX_SEAM_ROTATE = 1,        // mfx_rotate_dev: directions per launch (gridDim.y)
  MFX_SEAM_K2SX_BIG = 2,      // launch_k2sx_pipeline: voxels per screening + list-mode launch
  MFX_SEAM_K2X_CHUNK = 3,     // launch_k2x_t and the pipeline's hand-back pass: voxels per plain launch (slab)
  MFX_SEAM_DENSE = 4,         // mfx_solve_dense_chunks: upper bound, voxels in the largest budget at per_vox bytes each
  MFX_SEAM_WFIT_UPLOAD = 5,   // mfx_wfit_batch: voxels per upload
  MFX_SEAM_RFIT_UPLOAD = 6,   // mfx_rfit_batch: voxels per upload
  MFX_SEAM_SOLVE_SOFT = 7,    // ss_chunk: signals per launch (gridDim.y)
  MFX_SEAM_BOOT2D = 8,        // b2_rows, shared-fit kernels: voxels per launch (gridDim.z)
  MFX_SEAM_RFIT2D_UPLOAD = 9, // mfx_rfit2d_batch: voxels per upload of a K-fascicle bin (per_vox carries K)
  MFX_SEAM_WBOOT2D = 10,      // wb2_rows, shared-fit kernels: voxels per launch (gridDim.z)
};
constexpr int MFX_ROT_DIRS_PER_LAUNCH = 32768;
constexpr int MFX_K2SX_VOX_PER_LAUNCH = 32768;
constexpr int MFX_K2X_VOX_PER_LAUNCH = 2048;
constexpr size_t MFX_DENSE_MAX_BYTES = (size_t)1 << 30;
constexpr size_t MFX_UPLOAD_BYTES = (size_t)256 << 20;   // the host entry points' byte budget per upload chunk
constexpr int64_t MFX_SS_SIGNALS_PER_LAUNCH = 65535;
constexpr int64_t MFX_B2_VOX_PER_LAUNCH = 65535;
constexpr int64_t MFX_WB2_VOX_PER_LAUNCH = 65535;
inline size_t mfx_wfit_upload_chunk(int M) { return std::max<size_t>(1, MFX_UPLOAD_BYTES / (sizeof(double) * 2 * (size_t)M)); }   // Y, W
inline size_t mfx_rfit_upload_chunk(int M) { return std::max<size_t>(1, MFX_UPLOAD_BYTES / (sizeof(double) * 4 * (size_t)M)); }   // Y, W0, W, prediction
// Y, W0, W, the prediction and the weighted fit's s and y' (8 M bytes each), the plan's records (28 K M) and the kernels'
// records (F2Rec, 32 K M; robust2d.hip asserts the size)
constexpr size_t MFX_F2REC_BYTES = 32;
inline size_t mfx_rfit2d_upload_chunk(int M, int k) {
  return MFX_UPLOAD_BYTES / ((size_t)M * (sizeof(double) * 6 + (size_t)k * (28 + MFX_F2REC_BYTES)));
}

// device allocation released on every exit path
struct DevMem {
  void* p = nullptr;
  DevMem() = default;
  DevMem(const DevMem&) = delete;
  DevMem& operator=(const DevMem&) = delete;
  ~DevMem() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 8); }
  void* release() { void* q = p; p = nullptr; return q; }
  template <class T> T* as() const { return (T*)p; }
};
// a device array of n elements of T and its copies from and to host memory, each one checked call (HIPCHK).  The row
// forms move the rows ix[0 .. nv) of a host array through a contiguous [nv x width] copy (class_batch.h).
template <class T>
struct DevBuf : DevMem {
  size_t n = 0;
  T* get() const { return (T*)p; }
  hipError_t alloc_n(size_t n_) { n = n_; return alloc(sizeof(T) * n); }
  hipError_t upload(const T* src, size_t n_) {
    const hipError_t e = alloc_n(n_);
    return e != hipSuccess ? e : hipMemcpy(p, src, sizeof(T) * n, hipMemcpyHostToDevice);
  }
  hipError_t download(T* dst) const { return hipMemcpy(dst, p, sizeof(T) * n, hipMemcpyDeviceToHost); }
  hipError_t upload_rows(const T* src, const int64_t* ix, size_t nv, size_t src_ld, size_t width) {
    std::vector<T> rows(nv * width);
    gather_rows(rows.data(), src, ix, nv, src_ld, width);
    return upload(rows.data(), rows.size());
  }
  hipError_t download_rows(T* dst, const int64_t* ix, size_t nv, size_t width) const {
    std::vector<T> rows(nv * width);
    const hipError_t e = download(rows.data());
    if (e == hipSuccess) scatter_rows(dst, rows.data(), ix, nv, width);
    return e;
  }
};
// the directions of a class chunk: the first 3 k of every [3 maxfasc] row of peaks -> [nv x 3 k]; for k = 0 three zeros
// per voxel, which nobody reads, so that no upload is empty
inline hipError_t mfx_upload_peaks(DevBuf<double>& d, const double* peaks, const int64_t* ix, size_t nv, int maxfasc, int k) {
  if (k > 0) return d.upload_rows(peaks, ix, nv, 3 * (size_t)maxfasc, 3 * (size_t)k);
  const std::vector<double> zeros(nv * 3, 0.0);
  return d.upload(zeros.data(), zeros.size());
}
// Scratch memory of a call (per-workgroup slabs, short lists, extra columns, Gram / candidate buffers) comes from an ARENA
// per (host thread, stream): a few device blocks (a new one whenever a request does not fit: hipMalloc, once), handed out
// by bumping an offset through them in order, and taken back when the call's last StreamMem dies.  Calls on one stream execute in order, so the next call may reuse the
// addresses while the previous one is still running; different streams and different host threads have their own arenas.
// No HIP allocator call in the steady state: on the MI355X boxes of round 2 memory of HIP's DEFAULT stream-ordered pool
// read back as zeros after being re-mapped (tools/micro/mempool_remap.hip), and hipFreeAsync - also into a
// pool that keeps its memory - blocked the host for a kernel's duration from the second call in flight on.
// MFX_POISON=<byte>: every scratch allocation is filled with that byte before use (developer check for reads of
// uninitialised scratch memory).
hipError_t mfx_scratch_alloc(void** p, size_t bytes, hipStream_t s);
void mfx_scratch_free(void* p, hipStream_t s);
// A call that keeps scratch alive over a loop of steps (robust2d.hip: the directions' records over the iterations) marks the
// arena's position behind what it keeps and rewinds to it after every step, once the step's own allocations are released
// (the rewind does nothing otherwise): the steps follow each other on the stream like separate calls, and the arena
// does not grow with their number.  mark: false when the stream has no live allocation.
struct ScratchMark { size_t cur = 0, off = 0; int live = 0; };
bool mfx_scratch_mark(hipStream_t s, ScratchMark* m);
void mfx_scratch_rewind(hipStream_t s, const ScratchMark& m);
// scratch allocation released on every exit path
struct StreamMem {
  void* p = nullptr;
  hipStream_t s;
  explicit StreamMem(hipStream_t s_) : s(s_) {}
  StreamMem(const StreamMem&) = delete;
  StreamMem& operator=(const StreamMem&) = delete;
  ~StreamMem() { if (p) mfx_scratch_free(p, s); }
  hipError_t alloc(size_t bytes) { return mfx_scratch_alloc(&p, bytes, s); }
  template <class T> T* as() const { return (T*)p; }
};

// event pair around the dominant kernel of a class launch (bench.py reads it through mfx_last_kernel_ms)
int mfx_prof_begin(hipStream_t st);
int mfx_prof_end(hipStream_t st);
// hand-back counters: zero the call's totals / add one launch's device counters [n <= 4 ints] / queue their copy to
// pinned memory, all in stream order behind the work on `st` (no host synchronisation)
int mfx_fb_begin(hipStream_t st);
int mfx_fb_accumulate(const int* d_counters, int n, hipStream_t st, int offset = 0);
int mfx_fb_accumulate_audit(const int* d_audit, hipStream_t st);   // [0] beyond DC/4 (+), [1] largest error (max), [2] audited pairs (+) -> counters 8..10
int mfx_fb_end(hipStream_t st);

// the device-side views of a plan and of its tables, and the device they live on (for translation units other than mfx_api.hip)
void mfx_plan_view(const mfx_plan* p, TablesDev* T, PlanDev* P, int* device);

// explicit-dictionary solver and params packing on a device-resident dictionary [M x (K N + has_csf)] (mfx_api.hip; for fit2d.hip)
int mfx_solve_dense_scratch_bytes(int M, int K, int N, int has_csf, size_t* bytes);
int mfx_solve_dense_dev(const double* d_A, int M, int K, int N, int has_csf, const double* d_y, int maxfasc, int csf_on,
                        double* d_row, const int* run_if, void* d_scratch, hipStream_t st);
// The explicit fallback of a class launcher (fit2d.hip, w2d.hip, fit_w.hip): the V voxels in chunks of nvc within a byte
// budget of min(free / 4, 1 GiB) at per_vox bytes a voxel, one scratch block of per_vox * nvc bytes for all chunks.  Per
// chunk: materialise(v0, nv, nvc, block, &y) enqueues the dictionaries [nv x M x (K N + has_csf)] at the front of the
// block and sets y to the signal of voxel v0 (stride M); the solver runs voxel by voxel where ok[v]; after(v0, nv)
// enqueues what follows a chunk.  Only enqueues, in that order.
template <class Materialise, class After>
int mfx_solve_dense_chunks(int M, int K, int N, int has_csf, size_t per_vox, int64_t V, int maxfasc, int csf_on, double* d_params,
                           const int* ok, hipStream_t st, Materialise materialise, After after) {
  const size_t Ntot = (size_t)K * N + has_csf;
  const int np = 1 + 2 * maxfasc + csf_on + 2;
  size_t free_b = 0, total_b = 0, scratch_b = 0;
  HIPCHK(hipMemGetInfo(&free_b, &total_b));
  if (int rc = mfx_solve_dense_scratch_bytes(M, K, N, has_csf, &scratch_b)) return rc;
  const size_t budget = std::min<size_t>(free_b / 4, MFX_DENSE_MAX_BYTES);
  const int64_t nvc = std::max<int64_t>(1, std::min<int64_t>(V, (int64_t)(budget / per_vox)));
  StreamMem dA(st), dS(st);
  HIPCHK(dA.alloc(per_vox * nvc));
  HIPCHK(dS.alloc(scratch_b));
  for (int64_t v0 = 0; v0 < V; v0 += nvc) {
    const int64_t nv = std::min(nvc, V - v0);
    const double* y = nullptr;
    if (int rc = materialise(v0, nv, nvc, dA.as<double>(), &y)) return rc;
    for (int64_t q = 0; q < nv; ++q)
      if (int rc = mfx_solve_dense_dev(dA.as<double>() + (size_t)q * M * Ntot, M, K, N, has_csf, y + (size_t)q * M, maxfasc, csf_on,
                                       d_params + (size_t)(v0 + q) * np, ok + v0 + q, dS.p, st)) return rc;
    if (int rc = after(v0, nv)) return rc;
  }
  return MFX_OK;
}

// class launchers for robust.hip: one homogeneous class (every voxel K fascicles, d_peaks [V x 3 K] contiguous, the CSF
// column d_xc or null) into rows of the (maxfasc, csf_on) layout; they only enqueue.
// mfx_api.hip: the unweighted class fit, the launch sequence mfx_fit_batch* runs for the class; rows must be zero before
int mfx_fit_class_plain_dev(const mfx_plan* p, const double* d_Y, const double* d_peaks, int K, const double* d_xc, int maxfasc,
                            int csf_on, int64_t V, double* d_params, hipStream_t st);
// fit_w.hip: the weighted class fit behind mfx_wfit_batch* (w_class_dev)
int mfx_wfit_class_dev(const mfx_plan* p, const double* d_Y, const double* d_W, int64_t wstride, const double* d_peaks, int K,
                       const double* d_xc, int maxfasc, int csf_on, int64_t V, double* d_params, int32_t* d_vstat, hipStream_t st);

// robust.hip, for robust2d.hip: the check of the rule's parameters, the reweighting kernel (mfx_robust_weights_dev without its
// argument checks), W = W0 spread to [V x M] (ones without W0), and *d_out = the number of non-zero flags; they only enqueue
int mfx_rob_check_rule(const char* fn, int loss, double c, int M);
int mfx_rob_launch_weights(int M, const double* d_Y, const double* d_P, const double* d_W0, int64_t w0_stride, int loss, double c,
                           int64_t V, const double* d_Wprev, double* d_W, double* d_scale, int32_t* d_state, int32_t* d_changed,
                           hipStream_t st);
int mfx_rob_spread(const double* d_W0, int64_t w0_stride, int M, int64_t V, double* d_W, hipStream_t st);
int mfx_rob_count(const int* d_flags, int64_t V, int* d_out, hipStream_t st);
// The robust loop of robust.hip and robust2d.hip: the first fit, then per iteration the reweighting and the weighted fit.
// steps: first_fit(), reweight(it), refit() (they only enqueue) and step_done(), which follows each of them.  The device
// entry points pass host = null and enqueue every iteration.  The host entry points go one iteration at a time: they read
// nchanged[it] (the copy waits for the default stream), add it to n_changed[it], and an iteration that changed nothing
// leaves its fit out when the parameters already are those of a weighted fit on these weights (any iteration but the
// first one after an unweighted fit): every later iteration would repeat it bit for bit.
struct MfxRobHostCount {
  const int32_t* d_nchanged;
  bool has_w0;
  int64_t* n_changed;
  int32_t* n_iter_used;   // raised to the iterations this chunk took
};
template <class Steps>
int mfx_rob_iterate(const Steps& s, int n_iter, const MfxRobHostCount* host) {
  if (int rc = s.first_fit()) return rc;
  s.step_done();
  for (int it = 0; it < n_iter; ++it) {
    if (int rc = s.reweight(it)) return rc;
    s.step_done();
    if (host) {
      int32_t nc = 0;
      HIPCHK(hipMemcpy(&nc, host->d_nchanged + it, sizeof(int32_t), hipMemcpyDeviceToHost));
      host->n_changed[it] += nc;
      *host->n_iter_used = std::max<int32_t>(*host->n_iter_used, it + 1);
      if (nc == 0 && (it > 0 || host->has_w0)) break;
    }
    if (int rc = s.refit()) return rc;
    s.step_done();
  }
  return MFX_OK;
}

// ---- kernel launchers, one translation unit each
// FP64 two-fascicle kernel (tu_k2.hip).  With a.list_count set, a.vox_list is a device-side list whose length only the
// device knows: the launch covers nvox blocks and those beyond *a.list_count exit at once.
int mfx_launch_k2_f64(const FitK2Args& a, int nvox, hipStream_t st, bool record_events);
bool mfx_k2_f64_fits(const FitK2Args& a);
// screening kernel (tu_k2s_*.hip): KS k-steps of 16 measurements, bracketed protocol or not, NB chunk images
size_t mfx_k2s_lds_bytes(int KS, int N, bool bracket, int NB);
int mfx_launch_k2s_ks4(const FitK2Args& a, int nvox, hipStream_t st, bool br, int NB);
int mfx_launch_k2s_ks8(const FitK2Args& a, int nvox, hipStream_t st, bool br, int NB);
int mfx_launch_k2s_ks13(const FitK2Args& a, int nvox, hipStream_t st, bool br, int NB);
int mfx_launch_k2s_ks16(const FitK2Args& a, int nvox, hipStream_t st, bool br, int NB);
// wide screening kernel (tu_k2w_*.hip): one wave per SIMD, TL row tiles per wave (fit_k2w.hip)
size_t mfx_k2sx_lds_bytes(int KS, int N, bool bracket, int NB);
int mfx_launch_k2sx_ks8(const FitK2Args& a, int nvox, hipStream_t st, bool br);
int mfx_launch_k2sx_ks13(const FitK2Args& a, int nvox, hipStream_t st, bool br);
size_t mfx_k2w_lds_bytes(int KS, int N, bool bracket, int NB, int TL);
size_t mfx_k2wx_lds_bytes(int KS, int N, bool bracket, int NB, int TL);
int mfx_launch_k2wx_ks24(const FitK2Args& a, int nvox, hipStream_t st, bool br);
int mfx_launch_k2wx_ks35(const FitK2Args& a, int nvox, hipStream_t st, bool br);
int mfx_launch_k2w_ks13(const FitK2Args& a, int nvox, hipStream_t st, bool br);
int mfx_launch_k2w_ks16(const FitK2Args& a, int nvox, hipStream_t st, bool br);
int mfx_launch_k2w_ks24(const FitK2Args& a, int nvox, hipStream_t st, bool br);
int mfx_launch_k2w_ks35(const FitK2Args& a, int nvox, hipStream_t st, bool br);
// two fascicles + CSF/EAR (tu_k2x.hip)
int mfx_launch_k2x(const FitK2XArgs& a, int nvox, hipStream_t st);

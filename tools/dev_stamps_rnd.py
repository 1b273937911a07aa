"""Diagnostic: duration of every round of the screening kernel (A-operand generation, sweep) from in-kernel stamps.
Needs `make stamps_rnd` (microstructure_fingerprinting_amd/libmfx_stamps_rnd.so)."""
import os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from microstructure_fingerprinting_amd import _lib as L
L.LIB_PATH = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else os.path.join(ROOT, "microstructure_fingerprinting_amd", "libmfx_stamps_rnd.so")
from microstructure_fingerprinting_amd import engine, synth
import bench
V = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
sch, dic, ms = bench.build_model(782)
dev = torch.device("cuda", 0)
ms.device = 0
plan = engine.Plan(ms.device_tables(), scheme=sch)
M, N = sch.shape[0], ms.num_subs
# order of the phases: the kernel sweeps a shared last row tile first (ntiles > 1 and ntiles % 8 == 1: fit_k2s.hip); a third
# argument "plain" is for a library from before that (the shared tile last), e.g. to measure a parent commit's build
NTILES = (N + 31) // 32
FUSED = NTILES > 1 and NTILES % 8 == 1 and not (len(sys.argv) > 3 and sys.argv[3] == "plain")
rng = np.random.default_rng(1000)
peaks_h = np.concatenate([synth.unit_vectors(rng, V), synth.unit_vectors(rng, V)], axis=1)
atoms_h = rng.integers(0, N, (V, 2)).astype(np.int32)
nu_h = rng.dirichlet(np.ones(2), V)
d_peaks = torch.from_numpy(peaks_h).to(dev)
d_Y = torch.zeros((V, M), dtype=torch.float64, device=dev)
for k in range(2):
    col = engine.rotate_columns_dev(plan, d_peaks[:, 3 * k:3 * k + 3].contiguous(), torch.from_numpy(atoms_h[:, k].copy()).to(dev))
    d_Y += 500.0 * torch.from_numpy(nu_h[:, k:k + 1].copy()).to(dev) * col
gen = torch.Generator(device=dev); gen.manual_seed(1234)
d_Y += torch.randn((V, M), dtype=torch.float64, device=dev, generator=gen) * (500.0 / 30.0)
out = torch.zeros((V, 7), dtype=torch.float64, device=dev)
st = torch.zeros((V, 16), dtype=torch.int64, device=dev)
lib = L.lib()
lib.mfx_debug_set_stamps(st.data_ptr())
def run(thr0=None):
    st.zero_()
    if thr0 is not None:
        st[:, 15] = thr0.view(torch.int64)
    L.check(lib.mfx_fit_batch_dev(plan.handle(), d_Y.data_ptr(), d_peaks.data_ptr(), 2, 0, 0, None, None, 0, V, out.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    raw = st.cpu().numpy().astype(np.float64)[V // 4: 3 * V // 4]
    x = raw[(raw[:, :9] > 0).all(axis=1)]
    # the shared last row tile (slots 7, 8) runs FIRST when the kernel fuses D2's statistics into it: FUSED below
    order = [0, 7, 8, 1, 2, 3, 4, 5, 6] if FUSED else list(range(9))
    nms = [names[6], names[7] + " + D2 statistics"] + names[:6] if FUSED else names
    d = np.diff(x[:, order], axis=1)
    print("  whole kernel up to the end of the last phase: median %7.0f cycles" % np.median(x[:, order[-1]] - x[:, 0]))
    sh = st.cpu().numpy()[V // 4: 3 * V // 4, 12]
    print("  shared last tile: accumulator tiles sent to the FP64 criteria: mean %.1f; register groups evaluated: mean %.1f" % ((sh & 0xffffffff).mean(), (sh >> 32).mean()))
    for k, nm in enumerate(nms):
        print("  %-26s median %7.0f  mean %7.0f  p90 %7.0f cycles" % (nm, np.median(d[:, k]), d[:, k].mean(), np.percentile(d[:, k], 90)))
    cnt = st.cpu().numpy()[V // 4: 3 * V // 4, 9:12]
    for r in range(3):
        fl, gr = cnt[:, r] & 0xffffffff, cnt[:, r] >> 32
        print("  round %d: accumulator tiles sent to the FP64 criteria (all 8 waves): median %d mean %.1f p90 %d; register groups evaluated: median %d mean %.1f" % (r, np.median(fl), fl.mean(), np.percentile(fl, 90), np.median(gr), gr.mean()))
names = ["A operand r0", "sweep r0", "A operand r1", "sweep r1", "A operand r2", "sweep r2", "A operand (shared tile)", "shared last tile"]
run(); print("as shipped:"); run()
ref = out.clone()
ysq = (d_Y * d_Y).sum(1)
thr0 = ysq - out[:, 5] * M - 4e-5 * ysq       # the optimum's score minus 4 margins
print("starting threshold = final optimum - 4 margins (experiment):"); run(thr0.contiguous())
print("outputs identical:", bool(torch.equal(ref, out)))

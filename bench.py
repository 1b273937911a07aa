#!/usr/bin/env python3
"""bench.py -- headline benchmark: voxels/s of the per-voxel fingerprint matcher.

Workload (BASELINE.json configs[1], "C2"): 1e5 voxels, 2 fascicles, 782-atom x 200-measurement
multishell dictionary, exhaustive 2-sub-dictionary NNLS.  One "step" = one pass of the hot path
(rotation + exhaustive NNLS + parameter packing) over the whole batch, inputs already resident in HBM.
With N GPUs: --scaling weak (default) gives every rank its own 1e5-voxel shard, --scaling strong splits
ONE 1e5-voxel ROI over the ranks (BASELINE config 3 as worded); no data-path collective either way, rank 0
builds the dictionary tables and broadcasts them once over RCCL.

    python bench.py --gpus 1 --steps 3 --warmup 1
    python bench.py --gpus N --steps K --warmup W [--scaling strong]      # starts the N ranks itself (see launch_ranks)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W [--scaling strong]

`--gpus N` with N > 1 and no WORLD_SIZE in the environment: this process touches no GPU; it starts
`torch.distributed.run` with N ranks of this same script as a CHILD process, passes their output through and exits with
their code.  Inside a rank, WORLD_SIZE must equal --gpus and (backend nccl) every rank must own a device, or the rank
exits non-zero: a line with `n_gpus: N` is never printed by fewer than N devices.

Prints ONE JSON line on rank 0.  A plain run sets up, warms up, times --steps steps and prints the line; nothing else.
`--full` adds, after the timed steps: the `roofline` (the dominant kernel's time by HIP events, over a profiled pass of
its own of --steps steps) and a range check of the atom ids; at N = 1 also, measured in the same process over a few
steps each: the FP64 kernel on the same voxels (`fp64_kernel`), BASELINE configs 4, 1 and 5 (`c4`, `c1`, `c5`), the two-fascicle + CSF class (`k2_csf`), the
PCIe-inclusive rate of the host entry point (`host_api`) and the CPU baseline on all host cores.

`--dump-outputs DIR` writes what the last timed step computed, as the caller of mfx_fit_batch_dev receives it: the
[V, 7] float64 parameter rows (M0, nu1, nu2, id1, id2, MSE, R2) as DIR/params.npy (DIR/params_rank<r>.npy with N > 1).
Beyond OUTPUT_BUDGET_BYTES in all, a fixed seeded sample of rows is written, with their row numbers in
DIR/params_rows.npy (float64).  The inputs depend only on the arguments (seeded), so two builds can be compared
output for output.
"""
import argparse
import json
import os
import platform
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FLOP_PER_VOXEL = 261.0e6      # 244.6 MFLOP Gram + 16.4 MFLOP vector work (the reference's FP64 count)
BYTES_PER_VOXEL = 1710.0      # y (1600 B) + peaks (48 B) + flags in, 56 B out
PEAK_FP64_MFMA_TFLOPS = 78.6  # AMD public spec, FP64 matrix (the CDNA4 guide lists no FP64 MFMA rate)
PEAK_FP64_VALU_TFLOPS = 62.0  # FP64 vector FMA as MEASURED on MI355X (tools/micro/f64_rates.hip, profiles/r01_micro_f64_rates.txt); no spec figure in the guide
PEAK_F16_MFMA_TFLOPS = 2500.0  # dense FP16/BF16 MFMA, MI355X_MICROARCH.md
PEAK_HBM_GBPS = 8000.0
# The dominant kernel (mfx_fit_k2s_kernel) ranks the atom pairs with a Gram computed from operands split in two
# FP16 halves: 3 MFMA products per 32x32x16 block over the padded problem (800 x 800 atoms x 208 rows).
EXEC_F16_FLOP_PER_VOXEL = 3 * 2.0 * 800 * 800 * 208
# FP32 screening table bytes a voxel pulls from L2: 6 passes over a rotated dictionary (200 rows x 782 atoms x 8 B) + the
# shared last tile's operand read by all 8 waves
L2_TABLE_BYTES_PER_VOXEL = 6 * 200 * 782 * 8.0 + 8 * 32 * 200 * 8.0
# config 4, sub-dictionaries [782, 782, 1, E]: the C2 Gram + 782^2 E four-column NNLS of ~150 flops
C4_E = 10
FLOP_PER_VOXEL_C4 = 244.6e6 + 782.0 * 782.0 * C4_E * 150.0
# config 5, sub-dictionaries [1500, 1500, 1500] x 300 measurements: three N x N cross-Grams + N^3 three-column solves of the
# reference's solve_exhaustive_posweights_3 (Cramer 3x3 + residual from the Gram scalars: ~40 flops each, mf_utils.py:540-600)
C5_N, C5_V = 1500, 64
FLOP_PER_VOXEL_C5 = 3 * 2.0 * C5_N * C5_N * 300 + 40.0 * float(C5_N) ** 3
PMC_PROFILE = os.path.join("profiles", "r03_pmc_traffic_k2s.json")
PMC_C4 = os.path.join("profiles", "r03_pmc_k2x.json")
PMC_C5 = os.path.join("profiles", "r03_pmc_k3_screen.json")
OUTPUT_BUDGET_BYTES = 64 * 1024 * 1024     # --dump-outputs: all ranks together


def _pmc_field(rel, key):
    """A figure from a committed rocprofv3 --pmc summary of the same binary and workload (PMC needs its own passes: not
    measured in this run; the line names the file), or None."""
    try:
        return json.load(open(os.path.join(ROOT, rel))).get(key)
    except Exception:
        return None


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--voxels", type=int, default=100000, help="voxels per GPU (weak) or in total (strong); default: BASELINE config 2")
    ap.add_argument("--atoms", type=int, default=782)
    ap.add_argument("--scaling", choices=["weak", "strong"], default="weak")
    ap.add_argument("--cpu-sample", type=int, default=0, help="voxels timed on the host cores (0: ~40 per core)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip the fp64_kernel / c4 / c1 / host_api measurements")
    ap.add_argument("--full", action="store_true",
                    help="after the headline: roofline (profiled pass), atom-id check, the other configurations and the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs as DIR/<name>.npy")
    a = ap.parse_args()
    if a.steps < 1:
        ap.error("--steps must be at least 1")
    if a.warmup < 0:
        ap.error("--warmup must not be negative")
    return a


def dump_outputs(d_out, outdir, rank, world):
    """The last timed step's parameter rows -> outdir/params[_rank<r>].npy (float64); a seeded sample of rows beyond this
    rank's share of OUTPUT_BUDGET_BYTES, with the row numbers beside it."""
    os.makedirs(outdir, exist_ok=True)
    suffix = "" if world == 1 else "_rank%d" % rank
    out = d_out.cpu().numpy().astype(np.float64, copy=False)
    max_rows = max(1, OUTPUT_BUDGET_BYTES // world // (out.shape[1] * 8 + 8))
    if out.shape[0] > max_rows:
        rows = np.sort(np.random.default_rng(4242 + rank).choice(out.shape[0], max_rows, replace=False))
        out = out[rows]
        np.save(os.path.join(outdir, "params%s_rows.npy" % suffix), rows.astype(np.float64))
    np.save(os.path.join(outdir, "params%s.npy" % suffix), np.ascontiguousarray(out))


def build_model(atoms):
    """Host-side, once: synthetic dense scheme + dictionary -> per-shell knot tables."""
    from microstructure_fingerprinting_amd import mf_utils as mfu
    from microstructure_fingerprinting_amd import synth
    sch, dic, rng = synth.make_model("C2", N=atoms)
    ms = mfu.init_PGSE_multishell_interp(dic, sch, np.array([0.0, 0.0, 1.0]))
    return sch, dic, ms


def synth_voxels(plan, V, N, M, dev, seed, K=2, extra_cols=None, snr=30.0):
    """Synthetic voxels generated on the device with the library's own rotation kernel (SURVEY.md section 8d recipe):
    y = 500 sum_k nu_k D_k[:, a_k] (+ nu_x x) + N(0, 500/snr)."""
    import torch
    from microstructure_fingerprinting_amd import engine, synth
    rng = np.random.default_rng(seed)
    peaks_h = np.concatenate([synth.unit_vectors(rng, V) for _ in range(K)], axis=1)
    atoms_h = rng.integers(0, N, (V, K)).astype(np.int32)
    ncomp = K + (extra_cols.shape[1] if extra_cols is not None else 0)
    nu_h = rng.dirichlet(np.ones(ncomp), V)
    d_peaks = torch.from_numpy(peaks_h).to(dev)
    d_Y = torch.zeros((V, M), dtype=torch.float64, device=dev)
    for k in range(K):
        col = engine.rotate_columns_dev(plan, d_peaks[:, 3 * k:3 * k + 3].contiguous(),
                                        torch.from_numpy(atoms_h[:, k].copy()).to(dev))      # [V, M]
        d_Y += 500.0 * torch.from_numpy(nu_h[:, k:k + 1].copy()).to(dev) * col
    if extra_cols is not None:
        d_Y += 500.0 * torch.from_numpy(nu_h[:, K:].copy()).to(dev) @ torch.from_numpy(np.ascontiguousarray(extra_cols.T)).to(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234 + seed)
    d_Y += torch.randn((V, M), dtype=torch.float64, device=dev, generator=gen) * (500.0 / snr)
    return peaks_h, d_peaks, d_Y


def timed(step, steps, warmup, dev, lib):
    """(seconds per step by the wall clock, ms of the dominant kernel by HIP events on the launch stream)."""
    import torch
    for _ in range(warmup):
        step()
    lib.mfx_set_profiling(1)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    kms = []
    for _ in range(steps):
        step()
        kms.append(lib.mfx_last_kernel_ms())
    torch.cuda.synchronize(dev)
    dt = (time.perf_counter() - t0) / steps
    lib.mfx_set_profiling(0)
    return dt, (float(np.mean(kms)) if kms and min(kms) > 0 else None)


def launch_ranks(a, argv):
    """`bench.py --gpus N` (N > 1) outside a launcher: start the N ranks as a CHILD process (the reference's analogue is
    `mp.Pool(cpu_count)`, mf.py:978-1009) and hand back its exit code.  Nothing in THIS process has touched or will touch
    the GPU (no torch.cuda call, the library is not loaded): a process that has initialised the GPU must not be replaced or
    forked, so the decision is taken before anything else runs.  Rank 0 prints the JSON line on the shared stdout."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")     # dmabuf IPC: RCCL needs it on this platform
    env.setdefault("OMP_NUM_THREADS", "1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(a.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    return subprocess.run(cmd, env=env).returncode


def stub_main(a, world, rank):
    """MFX_BENCH_STUB=1 (tests/test_bench_launcher.py, CPU only): the whole multi-rank skeleton of main() - rendezvous,
    dictionary broadcast, shard sizes, barriers around the timed region, MAX over ranks, one JSON line from rank 0 - with
    a step that computes nothing.  The line says so in `metric` and `data`; it is not a measurement."""
    import torch
    import torch.distributed as dist
    from microstructure_fingerprinting_amd import dist as mdist
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo")
    ms = sch = None
    if rank == 0:
        sch, dic, ms = build_model(min(a.atoms, 64))
    if world > 1:
        ms, sch = mdist.broadcast_interpolator(ms, sch, src=0)
    if a.scaling == "strong" and world > 1:
        lo, hi = mdist.shard_range(a.voxels, rank, world)
        V, global_V = hi - lo, a.voxels
    else:
        V, global_V = a.voxels, world * a.voxels
    acc = np.zeros(1)

    def step():
        acc[0] += float(ms.num_subs)      # nothing is fitted

    for _ in range(a.warmup):
        step()
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        step()
    if world > 1:
        dist.barrier()
    elapsed = max(time.perf_counter() - t0, 1e-9)
    vpr = [V]
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        vpr = [None] * world
        dist.all_gather_object(vpr, V)
    if rank == 0:
        print(json.dumps({"metric": "STUB - no kernel ran (launcher / rendezvous / sharding skeleton only)", "value": 0.0,
                          "unit": "voxels/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
                          "ms_per_step": round(elapsed / a.steps * 1e3, 6), "higher_is_better": True,
                          "scaling": a.scaling if world > 1 else "weak", "vs_baseline": None, "dtype": "none", "data": "stub",
                          "config": {"workload": "stub", "voxels_per_rank": vpr, "global_voxels": global_V,
                                     "ranks_in_group": dist.get_world_size() if world > 1 else 1,
                                     "table_atoms_after_broadcast": int(ms.num_subs)}}), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def main(a=None):
    a = a or parse()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != a.gpus:
        # the line must never claim more (or fewer) GPUs than ranks took part
        sys.stderr.write("bench.py: --gpus %d but WORLD_SIZE=%d: start it as `python bench.py --gpus N` (it launches the ranks "
                         "itself) or under torch.distributed.run with --nproc-per-node equal to --gpus\n" % (a.gpus, world))
        sys.exit(2)
    if os.environ.get("MFX_BENCH_STUB") == "1":
        return stub_main(a, world, rank)
    import torch
    import torch.distributed as dist
    from microstructure_fingerprinting_amd import _lib as L
    from microstructure_fingerprinting_amd import engine
    from microstructure_fingerprinting_amd import mf_utils as mfu

    backend = os.environ.get("MFX_BENCH_BACKEND", "nccl")     # "gloo" only for rehearsals on a 1-GPU box
    ndev = torch.cuda.device_count()
    if world > 1 and backend == "nccl" and ndev < world:
        sys.stderr.write("bench.py: %d ranks but only %d visible GPU(s): one process per GPU, no sharing\n" % (world, ndev))
        sys.exit(3)
    # MFX_BENCH_FORCE_DIST=1: a one-rank group goes through the same process-group calls as N ranks (rehearsal of the RCCL
    # path on a one-GPU box, under torch.distributed.run --nproc-per-node 1)
    use_dist = world > 1 or os.environ.get("MFX_BENCH_FORCE_DIST") == "1"
    dev_index = (local_rank % ndev) if world > 1 else 0
    dev = torch.device("cuda", dev_index)
    torch.cuda.set_device(dev)
    json_fd = None
    if use_dist:
        # RCCL prints a version banner on STDOUT when the first communicator is made (seen on the GPU box: five lines in
        # front of the result).  The contract is ONE JSON line on stdout: everything else this process and its libraries
        # print goes to stderr, the line itself is written to the saved descriptor.
        sys.stdout.flush()
        json_fd = os.dup(1)
        os.dup2(2, 1)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)

    # ---- dictionary tables: built on rank 0, broadcast once (RCCL over xGMI), then staged to HBM
    ms = sch = None
    if rank == 0:
        sch, dic, ms = build_model(a.atoms)
    if use_dist:
        from microstructure_fingerprinting_amd import dist as mdist
        ms, sch = mdist.broadcast_interpolator(ms, sch, src=0, device=dev if backend == "nccl" else None)
    ms.device = dev.index or 0
    plan = engine.Plan(ms.device_tables(), scheme=sch)
    M, N = sch.shape[0], ms.num_subs

    # ---- this rank's voxels: its own shard (weak) or its contiguous block of ONE global ROI (strong; the global ROI is
    # generated from per-block seeds, so that the set of voxels does not depend on how it is split only in its totals)
    if a.scaling == "strong" and world > 1:
        from microstructure_fingerprinting_amd import dist as mdist
        lo, hi = mdist.shard_range(a.voxels, rank, world)
        V, global_V = hi - lo, a.voxels
    else:
        V, global_V = a.voxels, world * a.voxels
    peaks_h, d_peaks, d_Y = synth_voxels(plan, V, N, M, dev, 1000 + rank)
    d_out = torch.zeros((V, 7), dtype=torch.float64, device=dev)
    lib = L.lib()
    stream = torch.cuda.current_stream(dev)

    def step():
        L.check(lib.mfx_fit_batch_dev(plan.handle(), d_Y.data_ptr(), d_peaks.data_ptr(), 2, 0, 0, None, None, 0, V,
                                      d_out.data_ptr(), stream.cuda_stream))

    for _ in range(a.warmup):
        step()
    # ---- timed region: barrier + sync on both sides, the steps queued back to back
    torch.cuda.synchronize(dev)
    if use_dist:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        step()
    torch.cuda.synchronize(dev)
    if use_dist:
        dist.barrier()
    t1 = time.perf_counter()
    L.check(lib.mfx_plan_status(plan.handle(), stream.cuda_stream))
    elapsed = t1 - t0
    if a.dump_outputs:
        dump_outputs(d_out, a.dump_outputs, rank, world)
    ranks_seen, vox_per_rank, dev_per_rank = 1, [V], [torch.cuda.get_device_name(dev)]
    if use_dist:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        # what the process group really was: ranks, their shard sizes, the device each one ran on (PCI bus id: two ranks
        # on one card would show the same id)
        ranks_seen = dist.get_world_size()
        info = [None] * world
        dist.all_gather_object(info, (V, "%s #%d %s" % (torch.cuda.get_device_name(dev), dev.index or 0,
                                                        getattr(torch.cuda.get_device_properties(dev), "pci_bus_id", ""))))
        vox_per_rank = [i[0] for i in info]
        dev_per_rank = [i[1] for i in info]
    ms_per_step = elapsed / a.steps * 1e3
    value = global_V * a.steps / elapsed

    if a.full:
        # sanity: selected atoms are plausible indices
        ids = d_out[:, 3:5]
        assert bool(((ids >= 0) & (ids < N)).all()), "atom ids out of range"

    res = None
    if rank == 0:
        screen = os.environ.get("MFX_K2_SCREEN", "1") != "0"
        kavg, handed_back = None, None
        if a.full:
            # the dominant kernel's time: HIP events on the launch stream, over a pass of its own after the timed steps
            _, kavg = timed(step, a.steps, 0, dev, lib)
            L.check(lib.mfx_plan_status(plan.handle(), stream.cuda_stream))
            handed_back = int(lib.mfx_debug_last_fallback_count())
        roof = None
        if kavg:
            ach = FLOP_PER_VOXEL * V / (kavg * 1e-3) / 1e12
            # HBM bytes per launch from the PMC counters: NOT measured in this run (rocprofv3 --pmc needs its own passes);
            # taken from the committed profile of the same binary and workload, and tagged as such
            traffic, tfrom = None, None
            tf = os.path.join(ROOT, PMC_PROFILE if screen else os.path.join("profiles", "r01_pmc_traffic.json"))
            if os.path.exists(tf) and V == 100000 and a.atoms == 782:
                try:
                    traffic, tfrom = json.load(open(tf)).get("hbm_bytes_per_launch"), os.path.relpath(tf, ROOT)
                except Exception:
                    traffic = None
            if screen:
                # achieved: the reference's algorithmic FP64 flop count per second, priced against the dense MFMA
                # peak of the type the dominant kernel multiplies in (FP16).  exec_*: what the matrix pipe really did.
                exe = EXEC_F16_FLOP_PER_VOXEL * V / (kavg * 1e-3) / 1e12
                pmc = {}
                try:
                    pmc = json.load(open(os.path.join(ROOT, PMC_PROFILE)))
                except Exception:
                    pass
                aud_n, aud_max, aud_over = (int(lib.mfx_debug_last_counter(10)), int(lib.mfx_debug_last_counter(9)) * 1e-11,
                                            int(lib.mfx_debug_last_counter(8)))
                # `achieved` / `frac` as the contract defines them: the reference's ALGORITHMIC FP64 flop count per second
                # against the dense MFMA peak of the type the dominant kernel multiplies in (FP16).  `frac_executed` is what
                # the matrix pipe really did (3 split-FP16 products per block over the padded 800 x 800 x 208 problem).
                roof = {"bound": "mfma", "achieved": round(ach, 3), "peak": PEAK_F16_MFMA_TFLOPS, "unit": "TFLOP/s",
                        "frac": round(ach / PEAK_F16_MFMA_TFLOPS, 4), "traffic": traffic, "traffic_from": tfrom,
                        "kernel": "mfx_fit_k2s_kernel<13, false, 3, false>", "kernel_ms": round(kavg, 3),
                        "flop_per_voxel": FLOP_PER_VOXEL,
                        "frac_is": "algorithmic: flop_per_voxel (SURVEY 8d, the reference's FP64 count) x voxels / kernel_ms / peak",
                        "frac_algorithmic": round(ach / PEAK_F16_MFMA_TFLOPS, 4),
                        "executed_f16_mfma_flop_per_voxel": EXEC_F16_FLOP_PER_VOXEL,
                        "executed_TFLOPs": round(exe, 1),
                        "frac_executed": round(exe / PEAK_F16_MFMA_TFLOPS, 4),
                        "frac_executed_is": "3 x 2 x 800 x 800 x 208 FP16-MFMA flop per voxel x voxels / kernel_ms / 2500 TFLOP/s",
                        "mfma_pipe_utilisation_pmc": pmc.get("mfma_pipe_utilisation"), "valu_per_mfma_pmc": pmc.get("valu_insts_per_mfma"),
                        "pmc_from": PMC_PROFILE if pmc else None,
                        "vs_fp64_mfma_peak": round(ach / PEAK_FP64_MFMA_TFLOPS, 3),
                        "note": "pair screening on split-FP16 MFMA + exact FP64 re-evaluation; the kernel is VALU-issue/L2 bound, "
                                "see DESIGN.md 4.1",
                        "hbm_bytes_per_voxel_algorithmic": BYTES_PER_VOXEL,
                        "achieved_hbm_GBps_algorithmic": round(BYTES_PER_VOXEL * V / (kavg * 1e-3) / 1e9, 3),
                        # second roofline: the FP32 screening table is re-read from L2 6.3 times per
                        # voxel (D2 five times, D1 once, the shared last tile's operand eight times) at M rows x N atoms
                        # x 8 B per pass; an XCD's L2 delivers 66-73 GB/s per CU (MI355X_MICROARCH.md), 68 x 256 here
                        "l2_table_bytes_per_voxel": L2_TABLE_BYTES_PER_VOXEL,
                        "l2_table_TBps": round(L2_TABLE_BYTES_PER_VOXEL * V / (kavg * 1e-3) / 1e12, 2),
                        "l2_table_frac_of_17.4TBps": round(L2_TABLE_BYTES_PER_VOXEL * V / (kavg * 1e-3) / 17.4e12, 3),
                        "handed_back_to_fp64_kernel": handed_back,
                        # population audit of the last timed step (k2s_shared.h): one pseudo-random pair per voxel, listed or
                        # not, split-FP16 cross product against its FP64 value (cosine units; the screening margin is 1e-5)
                        "screen_audit": {"pairs": aud_n, "max_abs_err": aud_max, "pairs_beyond_quarter_margin": aud_over,
                                         "margin": 1.5e-5}}
            else:
                roof = {"bound": "mfma", "achieved": round(ach, 3), "peak": PEAK_FP64_MFMA_TFLOPS, "unit": "TFLOP/s",
                        "frac": round(ach / PEAK_FP64_MFMA_TFLOPS, 4), "traffic": traffic, "traffic_from": tfrom,
                        "kernel": "mfx_fit_k2_kernel<50,false,true,8,2,2>", "kernel_ms": round(kavg, 3),
                        "flop_per_voxel": FLOP_PER_VOXEL, "hbm_bytes_per_voxel_algorithmic": BYTES_PER_VOXEL,
                        "achieved_hbm_GBps_algorithmic": round(BYTES_PER_VOXEL * V / (kavg * 1e-3) / 1e9, 3)}
        extras = {}
        if a.full and world == 1 and not a.no_extras:
            extras = extra_measurements(plan, ms, sch, d_Y, d_peaks, peaks_h, d_out, V, N, M, dev, lib, screen)
        cpu = None
        if a.full and world == 1 and not a.no_cpu_baseline:
            cpu = cpu_baseline(sch, ms, d_Y, peaks_h, d_out, V, a.cpu_sample)
        res = {"metric": "voxels/sec, 2-fascicle exhaustive NNLS, 782-atom x 200-measurement dictionary",
               "value": round(value, 1), "unit": "voxels/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
               "ms_per_step": round(ms_per_step, 3), "ms_per_voxel": round(ms_per_step / max(global_V // world, 1), 6),
               "higher_is_better": True, "scaling": a.scaling if world > 1 else "weak", "vs_baseline": None,
               "dtype": "f64" if not screen else "f64 (pairs ranked on split-f16 MFMA, short list re-evaluated in f64)",
               "data": "synthetic", "full": a.full,
               "config": {"workload": "C2: %d voxels%s, 2 fascicles, %d atoms x %d measurements"
                                      % (a.voxels, "/GPU" if a.scaling == "weak" else " in total", N, M),
                          "voxels_per_gpu": global_V // world, "global_voxels": global_V, "atoms": N, "measurements": M,
                          "ranks_in_group": ranks_seen, "backend": backend if use_dist else None,
                          "voxels_per_rank": vox_per_rank, "device_per_rank": dev_per_rank,
                          "sharding": "voxel shards, no data-path collective; dictionary broadcast once over RCCL"},
               "roofline": roof, "cpu_baseline": cpu}
        res.update(extras)
        if json_fd is not None:
            sys.stdout.flush()
            os.write(json_fd, (json.dumps(res) + "\n").encode())
        else:
            print(json.dumps(res), flush=True)
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()
    return res


def extra_measurements(plan, ms, sch, d_Y, d_peaks, peaks_h, d_out, V, N, M, dev, lib, screen):
    """The rest of the story in the same process, a few steps each (N = 1 only): the FP64 kernel on the same voxels,
    BASELINE configs 4 and 1, and the PCIe-inclusive rate of the host entry point."""
    import torch
    from microstructure_fingerprinting_amd import _lib as L
    from microstructure_fingerprinting_amd import engine, synth
    from microstructure_fingerprinting_amd import mf_utils as mfu
    st = torch.cuda.current_stream(dev).cuda_stream
    out = {}
    # ---- FP64 kernel (same arithmetic as the reference's Gram, on FP64 MFMA) on the bench voxels; outputs must be identical
    if screen:
        ref_out = d_out.clone()
        o2 = torch.zeros_like(d_out)
        lib.mfx_debug_set_k2_screen(0)
        try:
            dt, kms = timed(lambda: L.check(lib.mfx_fit_batch_dev(plan.handle(), d_Y.data_ptr(), d_peaks.data_ptr(), 2, 0, 0, None,
                                                                 None, 0, V, o2.data_ptr(), st)), 2, 1, dev, lib)
        finally:
            lib.mfx_debug_set_k2_screen(1)
        ach = FLOP_PER_VOXEL * V / ((kms or dt * 1e3) * 1e-3) / 1e12
        out["fp64_kernel"] = {"value": round(V / dt, 1), "unit": "voxels/s", "kernel": "mfx_fit_k2_kernel<50,false,true,8,2,2>",
                              "kernel_ms": round(kms, 3) if kms else None, "bound": "mfma_f64", "achieved_TFLOPs": round(ach, 2),
                              "peak_TFLOPs": PEAK_FP64_MFMA_TFLOPS, "frac": round(ach / PEAK_FP64_MFMA_TFLOPS, 4),
                              "outputs_identical_to_default_path": bool(torch.equal(o2, ref_out))}
    # ---- config 4: two fascicles + CSF + EAR, sub-dictionaries [782, 782, 1, 10] (20 000 voxels: the class is ~30x slower)
    V4 = min(V, 20000)
    gam = mfu.get_gyromagnetic_ratio('H')
    b = (gam * sch[:, 3] * sch[:, 5]) ** 2 * (sch[:, 4] - sch[:, 5] / 3)
    sig_csf = np.exp(-sch[:, 6] / 2.0) * np.exp(-b * 3.0e-9)
    sig_ear = np.ascontiguousarray(np.stack([np.exp(-sch[:, 6] / 0.08) * np.exp(-b * D) for D in np.linspace(0.2e-9, 1.2e-9, C4_E)], axis=1))
    xcols = np.concatenate([sig_csf[:, None], sig_ear[:, 3:4]], axis=1)
    _, d_pk4, d_Y4 = synth_voxels(plan, V4, N, M, dev, 2, K=2, extra_cols=xcols)
    d_csf, d_ear = torch.from_numpy(sig_csf).to(dev), torch.from_numpy(sig_ear).to(dev)
    o4 = torch.zeros((V4, engine.num_params(2, True, True)), dtype=torch.float64, device=dev)
    dt, kms = timed(lambda: L.check(lib.mfx_fit_batch_dev(plan.handle(), d_Y4.data_ptr(), d_pk4.data_ptr(), 2, 1, 1, d_csf.data_ptr(),
                                                         d_ear.data_ptr(), C4_E, V4, o4.data_ptr(), st)), 2, 1, dev, lib)
    ach = FLOP_PER_VOXEL_C4 * V4 / dt / 1e12
    out["c4"] = {"workload": "C4: %d voxels, 2 fascicles + CSF + EAR, sub-dictionaries [782, 782, 1, %d], %d measurements" % (V4, C4_E, M),
                 "value": round(V4 / dt, 1), "unit": "voxels/s", "kernel": "mfx_fit_k2x_kernel<50,false,8,2>", "bound": "valu issue (FP64 scoring + FP32 filter) beside the FP64-MFMA Gram",
                 "reference_flop_per_voxel": FLOP_PER_VOXEL_C4, "reference_TFLOPs_equivalent": round(ach, 2),
                 "reference_TFLOPs_is": "the REFERENCE's work (Gram + 782^2 E four-column NNLS of ~150 flop) per second; the kernel filters "
                                        ">99 % of the tuples with a 5-instruction FP32 test, so this is NOT a utilisation",
                 "issue_utilisation_pmc": _pmc_field(PMC_C4, "issue_utilisation"), "mfma_pipe_utilisation_pmc": _pmc_field(PMC_C4, "mfma_pipe_utilisation"),
                 "hbm_bytes_per_voxel_pmc": _pmc_field(PMC_C4, "hbm_bytes_per_voxel"), "pmc_from": PMC_C4 if os.path.exists(os.path.join(ROOT, PMC_C4)) else None,
                 "exhaustive_pass_voxels": int(lib.mfx_debug_last_fallback_count())}
    # ---- two fascicles + CSF, sub-dictionaries [782, 782, 1]: the screening pipeline (fit_k2s.hip in its XC form -> short
    # lists -> fit_k2x.hip's exact stage; handed-back voxels on the FP64 kernel of the class), checked against that kernel
    _, d_pk3, d_Y3 = synth_voxels(plan, V4, N, M, dev, 3, K=2, extra_cols=sig_csf[:, None])
    o3 = torch.zeros((V4, engine.num_params(2, True, False)), dtype=torch.float64, device=dev)
    run3 = lambda: L.check(lib.mfx_fit_batch_dev(plan.handle(), d_Y3.data_ptr(), d_pk3.data_ptr(), 2, 1, 0, d_csf.data_ptr(), None, 0, V4,
                                                 o3.data_ptr(), st))
    dt, kms = timed(run3, 3, 1, dev, lib)
    handed = int(lib.mfx_debug_last_counter(4))
    ref3 = o3.clone()
    lib.mfx_debug_set_k2x_screen(0)
    try:
        dt_plain, _ = timed(run3, 1, 0, dev, lib)
    finally:
        lib.mfx_debug_set_k2x_screen(1)
    out["k2_csf"] = {"workload": "%d voxels, 2 fascicles + CSF, sub-dictionaries [782, 782, 1], %d measurements" % (V4, M),
                     "value": round(V4 / dt, 1), "unit": "voxels/s", "kernel": "mfx_fit_k2s_kernel<13,false,3,true> + mfx_fit_k2x_kernel<50,false,8,2,true>",
                     "handed_to_fp64_kernel": handed, "fp64_kernel_value": round(V4 / dt_plain, 1),
                     "outputs_identical_to_fp64_kernel": bool(torch.equal(o3, ref3))}
    # ---- config 1: 1 000 voxels, one fascicle, 100 atoms x 60 measurements (the reference's CPU-runnable plumbing case)
    sch1, dic1, _ = synth.make_model("C1")
    ms1 = mfu.init_PGSE_multishell_interp(dic1, sch1, np.array([0.0, 0.0, 1.0]))
    ms1.device = dev.index or 0
    plan1 = engine.Plan(ms1.device_tables(), scheme=sch1)
    V1, M1, N1 = 1000, sch1.shape[0], ms1.num_subs
    _, d_pk1, d_Y1 = synth_voxels(plan1, V1, N1, M1, dev, 0, K=1)
    o1 = torch.zeros((V1, engine.num_params(1, False, False)), dtype=torch.float64, device=dev)
    dt, kms = timed(lambda: L.check(lib.mfx_fit_batch_dev(plan1.handle(), d_Y1.data_ptr(), d_pk1.data_ptr(), 1, 0, 0, None, None, 0,
                                                         V1, o1.data_ptr(), st)), 20, 3, dev, lib)
    byt = (M1 * 8 + 24 + 5 * 8) * V1
    out["c1"] = {"workload": "C1: %d voxels, 1 fascicle, %d atoms x %d measurements" % (V1, N1, M1), "value": round(V1 / dt, 1),
                 "unit": "voxels/s", "kernel": "mfx_fit_small_kernel<false>", "kernel_us": round(kms * 1e3, 1) if kms else None,
                 "bound": "launch latency (one 1000-workgroup launch; HBM roofline for reference)",
                 "achieved_GBps": round(byt / dt / 1e9, 3), "peak_GBps": PEAK_HBM_GBPS, "frac": round(byt / dt / 1e9 / PEAK_HBM_GBPS, 6)}
    # ---- config 5: three fascicles, 1500 atoms x 300 measurements (3.4e9 triples per voxel), the dictionary sampled on the
    # subject's own protocol and rotated per voxel with rotate_atom's tables (mf_utils.py:1205-1437: an explicit row plan with
    # the free-diffusion knot, DIFF = 2e-9, S0 = the atoms' b0 signal), as BASELINE words config 5; batched three-fascicle path
    # (fit_k3.hip: rotation, Gram cross blocks on FP64 MFMA, triple screen on FP16 MFMA, exact finalize); opt-in maxfasc = 3
    rng5 = np.random.default_rng(5)
    sch5 = synth.make_scheme(rng5, 1, [1000, 2000, 3000, 4000], [75, 75, 75, 74])
    dic5 = synth.make_dictionary(rng5, sch5, C5_N)
    S05 = np.ascontiguousarray(np.repeat(dic5[:1, :], sch5.shape[0], axis=0))      # b0 signal of every atom, constant within a shell
    rt5 = mfu.RotateAtomTables(np.ascontiguousarray(dic5), sch5, np.array([0.0, 0.0, 1.0]), 2.0e-9, S05, warnings=False, device=dev.index or 0)
    plan5 = rt5.plan
    _, d_pk5, d_Y5 = synth_voxels(plan5, C5_V, C5_N, sch5.shape[0], dev, 7, K=3)
    o5 = torch.zeros((C5_V, engine.num_params(3, False, False)), dtype=torch.float64, device=dev)
    dt, kms = timed(lambda: L.check(lib.mfx_fit_batch_dev(plan5.handle(), d_Y5.data_ptr(), d_pk5.data_ptr(), 3, 0, 0, None, None, 0,
                                                         C5_V, o5.data_ptr(), st)), 2, 1, dev, lib)
    ach = FLOP_PER_VOXEL_C5 * C5_V / dt / 1e12
    out["c5"] = {"workload": "C5: %d voxels, 3 fascicles, sub-dictionaries [%d, %d, %d], %d measurements (%.2e triples per voxel), explicit rotate_atom plan"
                             % (C5_V, C5_N, C5_N, C5_N, sch5.shape[0], float(C5_N) ** 3),
                 "value": round(C5_V / dt, 1), "unit": "voxels/s", "ms_per_voxel": round(dt / C5_V * 1e3, 3),
                 "kernel": "mfx_k3b_screen_kernel (+ mfx_k3b_gram_kernel, mfx_k3b_items_kernel, mfx_k3b_finalize_kernel), batches of 32 voxels", "bound": "valu issue",
                 "reference_flop_per_voxel": FLOP_PER_VOXEL_C5, "reference_TFLOPs_equivalent": round(ach, 2),
                 "reference_TFLOPs_is": "the REFERENCE's work (three cross-Grams + N^3 three-column solves of ~40 flop) per second; the "
                                        "screen decides 1024 triples with one FP16 MFMA and ~25 vector instructions (most of them building its operands), so this is NOT a utilisation",
                 "issue_utilisation_pmc": _pmc_field(PMC_C5, "issue_utilisation"), "mfma_pipe_utilisation_pmc": _pmc_field(PMC_C5, "mfma_pipe_utilisation"),
                 "pmc_from": PMC_C5 if os.path.exists(os.path.join(ROOT, PMC_C5)) else None}
    del plan5, rt5, d_Y5, d_pk5, o5
    # ---- PCIe-inclusive: the host entry point (pinned double-buffered upload overlapped with the kernels), NumPy buffers in and out
    Yh, pkh = d_Y.cpu().numpy(), np.ascontiguousarray(peaks_h)
    Kh = np.full(V, 2, dtype=np.int32)
    t0 = time.perf_counter()
    engine.fit_batch(plan, Yh, Kh, None, None, pkh, 2, False, False)    # first call of the thread: allocates its staging and device buffers
    dt_first = time.perf_counter() - t0
    t0 = time.perf_counter()
    ph = engine.fit_batch(plan, Yh, Kh, None, None, pkh, 2, False, False)
    dt = time.perf_counter() - t0
    out["host_api"] = {"value": round(V / dt, 1), "unit": "voxels/s", "what": "mfx_fit_batch_rows on host ndarrays (H2D + kernels + D2H), buffers of the thread in place",
                       "ms": round(dt * 1e3, 2), "first_call_ms": round(dt_first * 1e3, 2),
                       "outputs_identical_to_device_path": bool(np.array_equal(ph, d_out.cpu().numpy()))}
    return out


def cpu_quota():
    """CPUs the container may use at once (cgroup v2 cpu.max / v1 cfs quota), or None: on the GPU boxes the affinity mask shows
    every hardware thread while the quota is a 16-CPU share, which is why more than 16 oracle threads run no faster."""
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        return None if q == "max" else round(float(q) / float(p), 2)
    except Exception:
        pass
    try:
        q = float(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
        p = float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        return None if q <= 0 else round(q / p, 2)
    except Exception:
        return None


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except Exception:
        pass
    return platform.processor() or "unknown"


def cpu_baseline(sch, ms, d_Y, peaks_h, d_out, V, nsample):
    """Time the CPU oracle (compiled restatement of the reference algorithm) on a bounded sample of the same voxels:
    one thread (the reference's parallel=False loop, mf.py:1017-1028) and 16 / 32 / 64 / all usable host threads (one worker
    per core: the analogue of mp.Pool(cpu_count), mf.py:978-1009).  `value` is the BEST of the multi-thread legs - with two
    hardware threads per core the working set of a voxel (2.5 MB of rotated dictionaries swept 782 times by the reference's
    Gram loop, mf_utils.py:315-319) falls out of the cores' shared L3 and the all-thread leg can be slower than the
    one-per-core leg; every leg is listed.  The GPU result is checked against the oracle on the largest sample."""
    from oracle import oracle as orc
    cores = os.cpu_count() or 1
    try:
        cores = len(os.sched_getaffinity(0))
    except Exception:
        pass
    nmax = max(1, min(cores, orc.max_threads()))
    T = {"S": ms.S, "N": ms.num_subs, "G_un": ms.Gms_un, "off": ms.off, "x": ms.x_flat, "Y": ms.Y_flat}
    legs_nt = sorted({n for n in (16, 32, 64, nmax) if n <= nmax} | {nmax})
    per = nsample // max(len(legs_nt), 1) if nsample > 0 else 0
    nbig = min(V, max((per if per > 0 else 30 * n) for n in legs_nt))
    Ys = d_Y[:nbig].cpu().numpy()
    pk = np.ascontiguousarray(peaks_h[:nbig])
    K = np.full(nbig, 2, dtype=np.int32)
    z = np.zeros(nbig, dtype=np.uint8)

    def run(n, nt):
        t0 = time.perf_counter()
        r = orc.fit_batch(T, sch, Ys[:n], K[:n], z[:n], z[:n], pk[:n], 2, False, False, None, None, 0, nthreads=nt)
        return n / (time.perf_counter() - t0), r

    n1 = min(nbig, 48)
    single, _ = run(n1, 1)
    legs, ref, nref = [], None, 0
    for nt in legs_nt:
        n = min(nbig, per if per > 0 else 30 * nt)     # ~20 voxels/s/thread: 1.5-3 s of wall clock per leg, whatever the box
        rate, r = run(n, nt)
        legs.append({"threads": nt, "voxels": n, "value": round(rate, 2), "per_thread": round(rate / nt, 3),
                     "efficiency_vs_single_thread": round(rate / (nt * single), 3)})
        if n >= nref:
            ref, nref = r, n
    best = max(legs, key=lambda l: l["value"])
    got = d_out[:nref].cpu().numpy()
    ids_equal = bool(np.array_equal(got[:, 3:5], ref[:, 3:5]))
    relerr = float(np.max(np.abs(got[:, :3] - ref[:, :3]) / np.maximum(np.abs(ref[:, :3]), 1e-300)))
    return {"value": best["value"], "unit": "voxels/s", "cores": best["threads"], "cores_total": os.cpu_count(),
            "cpu_model": cpu_model(), "cpu_quota": cpu_quota(), "kind": "port",
            "sample": "%d voxels of the same workload on %d OpenMP threads (best of the legs below; one worker per thread: "
                      "mp.Pool analogue); single-thread leg: %d voxels" % (best["voxels"], best["threads"], n1),
            "single_thread_value": round(single, 3), "legs": legs,
            "parity_on_sample": {"voxels": nref, "atom_ids_equal": ids_equal, "max_rel_err_weights": relerr}}


if __name__ == "__main__":
    _a = parse()
    if _a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(_a, sys.argv[1:]))      # before any GPU call in this process
    main(_a)

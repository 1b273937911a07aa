"""The screening kernel's 16-row form: a shared last row tile with at most 16 atoms runs on v_mfma_f32_16x16x32_f16 (two
16-column sub-tiles per column tile, one 16-byte table load per lane and row) instead of the 32-row form.  Voxel recipe and
comparison of tests/test_k2s_fused_tail_gpu.py: 64 voxels per case (generic mixtures, single-fascicle voxels whose atom lies
in the last tile of either dictionary, the duplicate-column first-index case, identical and 0.2-degree-apart peaks, noise-free
voxels, a zero signal); the screening kernel under both chunk-image schedules bit for bit equal to the FP64 kernel, the first
4 voxels equal to the oracle, no guard hit and no audited pair beyond a quarter of the margin.  All shapes have nine tiles:
one full round and the shared pass."""
import numpy as np
import pytest

from test_k2s_fused_tail_gpu import _compare, _model, _voxels

pytestmark = pytest.mark.gpu


# 257, 270, 272: 1, 14 and 16 atoms in the last tile - the 16-row form; 273: 17 atoms, the first shape that stays on the
# 32-row form.  [12,12,12]: KS = 4 (an even number of k-steps: 2 full steps of 32); [66,66,66]: 200 measurements, KS = 13,
# the half-empty last step; [40,40,40]: KS = 8; [80,80,80]: KS = 16.
@pytest.mark.parametrize("N,dirs", [(257, [12, 12, 12]), (270, [12, 12, 12]), (272, [12, 12, 12]), (273, [12, 12, 12]),
                                    (270, [66, 66, 66]), (272, [66, 66, 66]), (270, [40, 40, 40]), (270, [80, 80, 80])])
def test_tail16_shapes(N, dirs):
    rng, sch, ms = _model(N, dirs, 5000 + N + dirs[0], dup=True)
    plan = ms.plan_for(sch)
    peaks, d_pk, d_Y = _voxels(rng, plan, N, sch.shape[0])
    res, _ = _compare(ms, sch, plan, peaks, d_pk, d_Y)
    # first index on ties: the voxels made of atom 3 alone (column N - 1, in the last tile, is its copy) name atom 3
    assert np.all(res[0][40:42, 3] == 3) and np.all(res[0][42:44, 4] == 3), res[0][40:44, 1:5]


@pytest.mark.parametrize("dirs", [[12, 12, 12], [66, 66, 66]])
def test_tail16_bracketed_rows(dirs):
    """G-bracketed protocol (BR = true), built as in test_fused_tail_bracketed_rows, at N = 270."""
    rng, sch_ms, ms = _model(270, dirs, 5600 + dirs[0])
    Gs = ms["Gms_un"]
    sch = sch_ms.copy()
    nz = np.where(sch[:, 3] > 0)[0]
    between = [0.3 * Gs[1] + 0.7 * Gs[2], 0.55 * Gs[2] + 0.45 * Gs[3], 0.9 * Gs[2] + 0.1 * Gs[3], 0.5 * (Gs[1] + Gs[2])]
    sch[nz[::2], 3] = rng.choice(between, size=nz[::2].size)
    plan = ms.plan_for(sch)
    peaks, d_pk, d_Y = _voxels(rng, plan, 270, sch.shape[0])
    _compare(ms, sch, plan, peaks, d_pk, d_Y)


def test_tail16_ring_overflow_hands_back():
    """A ring of 16 entries at N = 270: voxels are handed back under both schedules; results still identical."""
    rng, sch, ms = _model(270, [12, 12, 12], 5700)
    plan = ms.plan_for(sch)
    peaks, d_pk, d_Y = _voxels(rng, plan, 270, sch.shape[0])
    _, cnt = _compare(ms, sch, plan, peaks, d_pk, d_Y, cap=16)
    assert cnt[0][0] > 0 and cnt[1][0] > 0, cnt

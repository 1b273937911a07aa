"""engine.py's argument checks and ctypes marshalling, entry point by entry point, without a GPU.  Two tables of calls:
malformed ones, whose exception class and message are pinned (a call with two faults pins the order of the checks), and
valid ones against a recording stand-in for the library, whose C calls are pinned argument by argument.  The expected
values were recorded from the engine.py that preceded the shared argument helpers and stand here as literals."""
import numpy as np
import pytest
import torch

from microstructure_fingerprinting_amd import _lib, engine as E

V, M, N = 4, 8, 5


class Stand:
    """Stands for an engine.Plan and for a mf_utils.RotateAtom2DTables.  Without ``h`` asking for the handle is a device
    call and fails; with it the handle is that marker."""
    def __init__(self, h=None, scheme=None):
        self.M, self.N, self.tables, self.scheme, self.h = M, N, self, scheme, h

    def handle(self):
        if self.h is None:
            raise AssertionError("the device was touched before the arguments were checked")
        return self.h


class OnDevice(torch.Tensor):
    """A CPU tensor that says it is a CUDA one: reaches the checks that follow the is_cuda asserts."""
    is_cuda = True


def cpu(*shape, dtype=torch.float64):
    return torch.zeros(shape, dtype=dtype)


def dev(*shape, dtype=torch.float64):
    return torch.zeros(shape, dtype=dtype).as_subclass(OnDevice)


def volume(m=M):
    return E.FileOrderVolume(np.asfortranarray(np.arange(6 * m, dtype=np.float32).reshape(3, 2, 1, m)), 2.0, 1.0)


def error_cases():
    P = T = Stand()
    Y, W, w = np.ones((V, M)), np.ones((V, M)), np.ones(M)
    pk1, pk2 = np.tile([0.0, 0.0, 1.0], (V, 1)), np.tile([0.0, 0.0, 1.0, 0.0, 0.6, 0.8], (V, 1))
    K, Kbad, csf, sc, se = np.array([1, 2, 0, 2]), np.array([1, 2, 3, 0]), np.array([0, 1, 0, 0]), np.ones(M), np.ones((M, 2))
    vox = np.arange(V)
    prm2 = np.zeros((V, E.num_params(2, False, False)))
    tY, tW, tw, tpk1, tpk2, tT = cpu(V, M), cpu(V, M), cpu(M), cpu(V, 3), cpu(V, 6), cpu(V)
    dY, dW, dw, dpk1, dpk2, dT = dev(V, M), dev(V, M), dev(M), dev(V, 3), dev(V, 6), dev(V)
    dprm2, tprm2 = dev(V, prm2.shape[1]), cpu(V, prm2.shape[1])
    c = {}
    # ---- the plain fit
    c["fit_batch/Y-1d"] = lambda: E.fit_batch(P, np.ones(M), K, None, None, pk2, 2, False, False)
    c["fit_batch/rows-range"] = lambda: E.fit_batch(P, Y, K, None, None, pk2, 2, False, False, rows=np.array([0, 1, 2, V]))
    c["fit_batch/M"] = lambda: E.fit_batch(P, Y[:, :-1], K, None, None, pk2, 2, False, False)
    c["fit_batch/K-length"] = lambda: E.fit_batch(P, Y, K[:3], None, None, pk2, 2, False, False)
    c["fit_batch/peaks-2"] = lambda: E.fit_batch(P, Y, K, None, None, pk1, 2, False, False)
    c["fit_batch/peaks-0-ignored"] = lambda: E.fit_batch(P, Y, np.zeros(V), None, None, None, 0, False, False)
    c["fit_batch/M+K-length"] = lambda: E.fit_batch(P, Y[:, :-1], K[:3], None, None, pk2, 2, False, False)
    c["fit_batch/K-length+peaks"] = lambda: E.fit_batch(P, Y, K[:3], None, None, pk1, 2, False, False)
    c["fit_batch/rows-range+M"] = lambda: E.fit_batch(P, Y[:, :-1], K, None, None, pk2, 2, False, False, rows=np.array([-1, 0, 1, 2]))
    c["fit_batch_volume/M"] = lambda: E.fit_batch_volume(P, volume(M - 1), vox, K, None, None, pk2, 2, False, False)
    c["fit_batch_volume/vox-range"] = lambda: E.fit_batch_volume(P, volume(), np.array([0, 1, 2, 6]), K, None, None, pk2, 2, False, False)
    c["fit_batch_volume/K-length"] = lambda: E.fit_batch_volume(P, volume(), vox, K[:3], None, None, pk2, 2, False, False)
    c["fit_batch_volume/peaks-2"] = lambda: E.fit_batch_volume(P, volume(), vox, K, None, None, pk1, 2, False, False)
    c["fit_batch_volume/peaks-0-ignored"] = lambda: E.fit_batch_volume(P, volume(), vox, np.zeros(V), None, None, None, 0, False, False)
    c["fit_batch_volume/M+vox-range"] = lambda: E.fit_batch_volume(P, volume(M - 1), -vox, K, None, None, pk2, 2, False, False)
    c["fit_batch_volume/vox-range+K-length"] = lambda: E.fit_batch_volume(P, volume(), -vox, K[:3], None, None, pk2, 2, False, False)
    c["fit_batch_volume/K-length+peaks"] = lambda: E.fit_batch_volume(P, volume(), vox, K[:3], None, None, pk1, 2, False, False)
    c["volume_rows/vox-range"] = lambda: E.volume_rows(volume(), np.array([0, 6]))
    c["fit_batch_dev/not-cuda"] = lambda: E.fit_batch_dev(P, tY, tpk2, 2)
    c["fit_batch_dev/M"] = lambda: E.fit_batch_dev(P, dev(V, M - 1), dpk2, 2)
    c["fit_batch_dev/peaks-not-cuda"] = lambda: E.fit_batch_dev(P, dY, tpk2, 2)
    c["fit_batch_dev/peaks-2"] = lambda: E.fit_batch_dev(P, dY, dpk1, 2)
    c["fit_batch_dev/not-cuda+M"] = lambda: E.fit_batch_dev(P, cpu(V, M - 1), tpk2, 2)
    c["fit_batch_dev/M+peaks-not-cuda"] = lambda: E.fit_batch_dev(P, dev(V, M - 1), tpk2, 2)
    c["rotate_columns_dev/not-cuda"] = lambda: E.rotate_columns_dev(P, cpu(V, 3), cpu(V, dtype=torch.int32))
    # ---- the forward model
    c["predict/maxfasc"] = lambda: E.predict(P, prm2, pk2, 4)
    c["predict/params"] = lambda: E.predict(P, prm2[:, :-1], pk2, 2)
    c["predict/peaks"] = lambda: E.predict(P, prm2, pk1, 2)
    c["predict/sig_csf"] = lambda: E.predict(P, np.zeros((V, 8)), pk2, 2, csf_on=True, sig_csf=sc[:-1])
    c["predict/sig_ear"] = lambda: E.predict(P, np.zeros((V, 9)), pk2, 2, ear_on=True, sig_ear=se, E=3)
    c["predict/Y"] = lambda: E.predict(P, prm2, pk2, 2, Y=Y[:3])
    c["predict/sigma-missing"] = lambda: E.predict(P, prm2, pk2, 2, ncoils=2)
    c["predict/sigma-shape"] = lambda: E.predict(P, prm2, pk2, 2, ncoils=2, sigma_g=np.ones(3))
    c["predict/maxfasc+params"] = lambda: E.predict(P, prm2[:, :-1], pk2, -1)
    c["predict/params+peaks"] = lambda: E.predict(P, prm2[:, :-1], pk1, 2)
    c["predict/Y+sigma-missing"] = lambda: E.predict(P, prm2, pk2, 2, Y=Y[:3], ncoils=1)
    c["predict_dev/not-cuda"] = lambda: E.predict_dev(P, tprm2, tpk2, 2)
    c["predict_dev/peaks-not-cuda"] = lambda: E.predict_dev(P, dprm2, tpk2, 2)
    c["predict_dev/params"] = lambda: E.predict_dev(P, dev(V, 6), dpk2, 2)
    c["predict_dev/peaks"] = lambda: E.predict_dev(P, dprm2, dpk1, 2)
    c["predict_dev/sigma-missing"] = lambda: E.predict_dev(P, dprm2, dpk2, 2, ncoils=1)
    c["predict_dev/out-shape"] = lambda: E.predict_dev(P, dprm2, dpk2, 2, out=dev(V, M + 1))
    c["predict_dev/not-cuda+params"] = lambda: E.predict_dev(P, cpu(V, 6), tpk2, 2)
    c["predict_dev/Y-not-cuda+peaks"] = lambda: E.predict_dev(P, dprm2, dpk1, 2, d_Y=tY)
    c["predict_dev/sigma-missing+out-shape"] = lambda: E.predict_dev(P, dprm2, dpk2, 2, ncoils=1, out=dev(V, M + 1))
    c["sos_noise/sigma-shape"] = lambda: E.sos_noise(Y, np.ones(3))
    c["sos_noise_dev/not-cuda"] = lambda: E.sos_noise_dev(tY, 1.0)
    c["sos_noise_dev/sigma-shape"] = lambda: E.sos_noise_dev(dY, cpu(3))
    c["sos_noise_dev/ncoils"] = lambda: E.sos_noise_dev(dY, 1.0, ncoils=0)
    c["sos_noise_dev/out-shape"] = lambda: E.sos_noise_dev(dY, 1.0, out=dev(V, M + 1))
    c["sos_noise_dev/not-cuda+sigma-shape"] = lambda: E.sos_noise_dev(tY, cpu(3))
    c["sos_noise_dev/sigma-shape+ncoils"] = lambda: E.sos_noise_dev(dY, cpu(3), ncoils=0)
    c["predict2d/maxfasc"] = lambda: E.predict2d(T, prm2, pk2, 4)
    c["predict2d/params"] = lambda: E.predict2d(T, prm2[:, :-1], pk2, 2)
    c["predict2d/peaks"] = lambda: E.predict2d(T, prm2, pk1, 2)
    c["predict2d/sig_csf"] = lambda: E.predict2d(T, np.zeros((V, 8)), pk2, 2, csf_on=True, sig_csf=sc[:-1])
    c["predict2d/Y"] = lambda: E.predict2d(T, prm2, pk2, 2, Y=Y[:3])
    c["predict2d/sigma-missing"] = lambda: E.predict2d(T, prm2, pk2, 2, ncoils=2)
    c["predict2d/sigma-shape"] = lambda: E.predict2d(T, prm2, pk2, 2, ncoils=2, sigma_g=np.ones(3))
    c["predict2d/maxfasc+params"] = lambda: E.predict2d(T, prm2[:, :-1], pk2, 4)
    c["predict2d_dev/not-cuda"] = lambda: E.predict2d_dev(T, tprm2, tpk2, 2)
    c["predict2d_dev/params"] = lambda: E.predict2d_dev(T, dev(V, 6), dpk2, 2)
    c["predict2d_dev/out-shape"] = lambda: E.predict2d_dev(T, dprm2, dpk2, 2, out=dev(V, M + 1))
    c["predict2d_dev/not-cuda+params"] = lambda: E.predict2d_dev(T, cpu(V, 6), tpk2, 2)
    c["predict2d_dev/sigma-missing+out-shape"] = lambda: E.predict2d_dev(T, dprm2, dpk2, 2, ncoils=1, out=dev(V, M + 1))
    # ---- profiles, pair objectives and posteriors
    for name, f, fd, extra in (("profile", E.profile, E.profile_dev, ()), ("posterior", E.posterior, E.posterior_dev, (tT, tT))):
        hx = (1.0,) if extra else ()
        c[name + "/data"] = lambda f=f, hx=hx: f(P, Y[:, :-1], K, csf, pk2, 2, True, sc, *hx)
        c[name + "/K-length"] = lambda f=f, hx=hx: f(P, Y, K[:3], csf, pk2, 2, True, sc, *hx)
        c[name + "/weights-VM"] = lambda f=f, hx=hx: f(P, Y, K, csf, pk2, 2, True, sc, *hx, W=W[:, :-1])
        c[name + "/weights-M"] = lambda f=f, hx=hx: f(P, Y, K, csf, pk2, 2, True, sc, *hx, W=np.ones(M + 1))
        c[name + "/peaks-2"] = lambda f=f, hx=hx: f(P, Y, K, csf, pk1, 2, True, sc, *hx)
        c[name + "/csf-no-csf_on"] = lambda f=f, hx=hx: f(P, Y, K, csf, pk2, 2, False, sc, *hx)
        c[name + "/csf-no-sig_csf"] = lambda f=f, hx=hx: f(P, Y, K, csf, pk2, 2, True, None, *hx)
        c[name + "/sig_csf-length"] = lambda f=f, hx=hx: f(P, Y, K, csf, pk2, 2, True, sc[:-1], *hx)
        c[name + "/csf-length"] = lambda f=f, hx=hx: f(P, Y, K, csf[:3], pk2, 2, True, sc, *hx)
        c[name + "/K-range"] = lambda f=f, hx=hx: f(P, Y, Kbad, csf, pk2, 2, True, sc, *hx)
        c[name + "/data+K-length"] = lambda f=f, hx=hx: f(P, Y[:, :-1], K[:3], csf, pk2, 2, True, sc, *hx)
        c[name + "/K-length+weights"] = lambda f=f, hx=hx: f(P, Y, K[:3], csf, pk2, 2, True, sc, *hx, W=W[:3])
        c[name + "/weights+peaks"] = lambda f=f, hx=hx: f(P, Y, K, csf, pk1, 2, True, sc, *hx, W=W[:3])
        c[name + "/peaks+csf"] = lambda f=f, hx=hx: f(P, Y, K, csf, pk1, 2, False, sc, *hx)
        c[name + "/csf+sig_csf-length"] = lambda f=f, hx=hx: f(P, Y, K, csf, pk2, 2, False, sc[:-1], *hx)
        c[name + "/sig_csf-length+K-range"] = lambda f=f, hx=hx: f(P, Y, Kbad, csf, pk2, 2, True, sc[:-1], *hx)
        dx = (dT, dT) if extra else ()
        c[name + "_dev/csf_on-alone"] = lambda fd=fd, extra=extra: fd(P, tY, tpk2, 2, *extra, csf_on=True)
        c[name + "_dev/K"] = lambda fd=fd, extra=extra: fd(P, tY, cpu(V, 9), 3, *extra)
        c[name + "_dev/data"] = lambda fd=fd, extra=extra: fd(P, tY[:, :-1], tpk2, 2, *extra)
        c[name + "_dev/peaks"] = lambda fd=fd, extra=extra: fd(P, tY, tpk1, 2, *extra)
        c[name + "_dev/sig_csf-length"] = lambda fd=fd, extra=extra: fd(P, tY, tpk2, 2, *extra, csf_on=True, d_sig_csf=cpu(M - 1))
        c[name + "_dev/weights-VM"] = lambda fd=fd, extra=extra: fd(P, tY, tpk2, 2, *extra, d_W=cpu(V, M - 1))
        c[name + "_dev/weights-M"] = lambda fd=fd, extra=extra: fd(P, tY, tpk2, 2, *extra, d_W=cpu(M + 1))
        c[name + "_dev/not-cuda"] = lambda fd=fd, extra=extra: fd(P, tY, tpk2, 2, *extra)
        c[name + "_dev/weights-not-cuda"] = lambda fd=fd, dx=dx: fd(P, dY, dpk2, 2, *dx, d_W=tw)
        c[name + "_dev/sig_csf-not-cuda"] = lambda fd=fd, dx=dx: fd(P, dY, dpk2, 2, *dx, csf_on=True, d_sig_csf=cpu(M))
        c[name + "_dev/csf_on-alone+K"] = lambda fd=fd, extra=extra: fd(P, tY, cpu(V, 9), 3, *extra, csf_on=True)
        c[name + "_dev/K+data"] = lambda fd=fd, extra=extra: fd(P, tY[:, :-1], cpu(V, 9), 3, *extra)
        c[name + "_dev/peaks+weights"] = lambda fd=fd, extra=extra: fd(P, tY, tpk1, 2, *extra, d_W=cpu(M + 1))
        c[name + "_dev/weights+not-cuda"] = lambda fd=fd, extra=extra: fd(P, tY, tpk2, 2, *extra, d_W=cpu(V, M - 1))
    c["profile_dev/out-shape"] = lambda: E.profile_dev(P, dY, dpk2, 2, out=dev(V, 2, N + 1))
    c["profile_dev/weights+out-shape"] = lambda: E.profile_dev(P, dY, dpk2, 2, out=dev(V, 2, N + 1), d_W=dev(M + 1))
    c["posterior/sigma"] = lambda: E.posterior(P, Y, K, csf, pk2, 2, True, sc, np.ones(3))
    c["posterior/shift"] = lambda: E.posterior(P, Y, K, csf, pk2, 2, True, sc, 1.0, shift=np.ones(3))
    c["posterior/K-range+sigma"] = lambda: E.posterior(P, Y, Kbad, csf, pk2, 2, True, sc, np.ones(3))
    c["posterior_dev/T"] = lambda: E.posterior_dev(P, tY, tpk2, 2, tT[:3], tT)
    c["posterior_dev/shift"] = lambda: E.posterior_dev(P, tY, tpk2, 2, tT, 0.0)
    c["posterior_dev/T+weights"] = lambda: E.posterior_dev(P, tY, tpk2, 2, tT[:3], tT, d_W=cpu(M + 1))
    c["posterior_dev/peaks+T"] = lambda: E.posterior_dev(P, tY, tpk1, 2, tT[:3], tT)
    c["pair_objectives/csf_on-alone"] = lambda: E.pair_objectives(P, Y, pk2, csf_on=True)
    c["pair_objectives/data"] = lambda: E.pair_objectives(P, Y[:, :-1], pk2)
    c["pair_objectives/peaks"] = lambda: E.pair_objectives(P, Y, pk1)
    c["pair_objectives/sig_csf-length"] = lambda: E.pair_objectives(P, Y, pk2, csf_on=True, sig_csf=sc[:-1])
    c["pair_objectives/weights-VM"] = lambda: E.pair_objectives(P, Y, pk2, W=W[:, :-1])
    c["pair_objectives/weights-M"] = lambda: E.pair_objectives(P, Y, pk2, W=np.ones(M + 1))
    c["pair_objectives/data+peaks"] = lambda: E.pair_objectives(P, Y[:, :-1], pk1)
    c["pair_objectives/sig_csf-length+weights"] = lambda: E.pair_objectives(P, Y, pk2, csf_on=True, sig_csf=sc[:-1], W=W[:3])
    c["pair_objectives_dev/csf_on-alone"] = lambda: E.pair_objectives_dev(P, tY, tpk2, csf_on=True)
    c["pair_objectives_dev/data"] = lambda: E.pair_objectives_dev(P, tY[:, :-1], tpk2)
    c["pair_objectives_dev/peaks"] = lambda: E.pair_objectives_dev(P, tY, tpk1)
    c["pair_objectives_dev/weights-VM"] = lambda: E.pair_objectives_dev(P, tY, tpk2, d_W=cpu(V, M - 1))
    c["pair_objectives_dev/weights-M"] = lambda: E.pair_objectives_dev(P, tY, tpk2, d_W=cpu(M + 1))
    c["pair_objectives_dev/not-cuda"] = lambda: E.pair_objectives_dev(P, tY, tpk2)
    c["pair_objectives_dev/weights-not-cuda"] = lambda: E.pair_objectives_dev(P, dY, dpk2, d_W=tW)
    c["pair_objectives_dev/peaks+weights"] = lambda: E.pair_objectives_dev(P, tY, tpk1, d_W=cpu(M + 1))
    c["profile_classes/lengths"] = lambda: E.profile_classes(K, csf[:3], None, 2)
    c["profile_classes/K-range"] = lambda: E.profile_classes(Kbad, csf, None, 2)
    # ---- 2-D protocols: rotation, fits, soft fits and profiles
    c["rotate2d_dev/not-cuda"] = lambda: E.rotate2d_dev(T, cpu(V, 3))
    c["fit2d_dev/not-cuda"] = lambda: E.fit2d_dev(T, tY, tpk2, 2)
    c["fit2d_dev/peaks-not-cuda"] = lambda: E.fit2d_dev(T, dY, tpk2, 2)
    c["fit2d_dev/maxfasc"] = lambda: E.fit2d_dev(T, dY, dev(V, 12), 4)
    c["fit2d_dev/data"] = lambda: E.fit2d_dev(T, dev(V, M - 1), dpk2, 2)
    c["fit2d_dev/peaks"] = lambda: E.fit2d_dev(T, dY, dpk1, 2)
    c["fit2d_dev/out-shape"] = lambda: E.fit2d_dev(T, dY, dpk2, 2, out=dev(V, 6))
    c["fit2d_dev/not-cuda+maxfasc"] = lambda: E.fit2d_dev(T, tY, cpu(V, 12), 4)
    c["fit2d_dev/peaks+out-shape"] = lambda: E.fit2d_dev(T, dY, dpk1, 2, out=dev(V, 6))
    c["fit2d_weighted_dev/maxfasc"] = lambda: E.fit2d_weighted_dev(T, tY, tW, cpu(V, 12), 4)
    c["fit2d_weighted_dev/data"] = lambda: E.fit2d_weighted_dev(T, tY[:, :-1], tW, tpk2, 2)
    c["fit2d_weighted_dev/peaks"] = lambda: E.fit2d_weighted_dev(T, tY, tW, tpk1, 2)
    c["fit2d_weighted_dev/weights-VM"] = lambda: E.fit2d_weighted_dev(T, tY, cpu(V, M - 1), tpk2, 2)
    c["fit2d_weighted_dev/weights-M"] = lambda: E.fit2d_weighted_dev(T, tY, cpu(M + 1), tpk2, 2)
    c["fit2d_weighted_dev/not-cuda"] = lambda: E.fit2d_weighted_dev(T, tY, tW, tpk2, 2)
    c["fit2d_weighted_dev/out-shape"] = lambda: E.fit2d_weighted_dev(T, dY, dw, dpk2, 2, out=dev(V, 6))
    c["fit2d_weighted_dev/peaks+weights"] = lambda: E.fit2d_weighted_dev(T, tY, cpu(M + 1), tpk1, 2)
    c["fit2d_weighted_dev/weights+not-cuda"] = lambda: E.fit2d_weighted_dev(T, tY, cpu(M + 1), tpk2, 2)
    c["fit_weighted_dev/not-cuda"] = lambda: E.fit_weighted_dev(P, tY, tW, tpk2, 2)
    c["fit_weighted_dev/maxfasc"] = lambda: E.fit_weighted_dev(P, dY, dW, dev(V, 12), 4)
    c["fit_weighted_dev/data"] = lambda: E.fit_weighted_dev(P, dev(V, M - 1), dW, dpk2, 2)
    c["fit_weighted_dev/weights-VM"] = lambda: E.fit_weighted_dev(P, dY, dev(V, M - 1), dpk2, 2)
    c["fit_weighted_dev/weights-M"] = lambda: E.fit_weighted_dev(P, dY, dev(M + 1), dpk2, 2)
    c["fit_weighted_dev/peaks"] = lambda: E.fit_weighted_dev(P, dY, dw, dpk1, 2)
    c["fit_weighted_dev/out-shape"] = lambda: E.fit_weighted_dev(P, dY, dw, dpk2, 2, out=dev(V, 6))
    c["fit_weighted_dev/not-cuda+weights"] = lambda: E.fit_weighted_dev(P, tY, cpu(M + 1), tpk2, 2)
    c["fit_weighted_dev/weights+peaks"] = lambda: E.fit_weighted_dev(P, dY, dev(M + 1), dpk1, 2)
    c["fit_weighted_dev/peaks+out-shape"] = lambda: E.fit_weighted_dev(P, dY, dw, dpk1, 2, out=dev(V, 6))
    # the mixed-batch forms: (name, call with (Y, K, csf, peaks, maxfasc, csf_on, sig_csf, W or W0), its weights are optional)
    mixed = (("fit2d", lambda y, k, cf, pk, mf, on, s, wt: E.fit2d(T, y, k, cf, pk, mf, on, s), None),
             ("fit2d_weighted", lambda y, k, cf, pk, mf, on, s, wt: E.fit2d_weighted(T, y, wt, k, cf, pk, mf, on, s), False),
             ("fit_weighted", lambda y, k, cf, pk, mf, on, s, wt: E.fit_weighted(P, y, wt, k, cf, pk, mf, on, s), False),
             ("fit_robust", lambda y, k, cf, pk, mf, on, s, wt: E.fit_robust(P, y, k, cf, pk, mf, on, s, W0=wt), True),
             ("fit2d_robust", lambda y, k, cf, pk, mf, on, s, wt: E.fit2d_robust(T, y, k, cf, pk, mf, on, s, W0=wt), True))
    for name, f, optional in mixed:
        c[name + "/maxfasc"] = lambda f=f: f(Y, K, csf, np.ones((V, 12)), 4, True, sc, W)
        c[name + "/data"] = lambda f=f: f(Y[:, :-1], K, csf, pk2, 2, True, sc, W)
        c[name + "/peaks-2"] = lambda f=f: f(Y, K, csf, pk1, 2, True, sc, W)
        c[name + "/peaks-0-ignored"] = lambda f=f: f(Y, np.zeros(V), None, pk1, 0, False, None, w)
        c[name + "/K-length"] = lambda f=f: f(Y, K[:3], csf, pk2, 2, True, sc, W)
        c[name + "/K-range"] = lambda f=f: f(Y, Kbad, csf, pk2, 2, True, sc, W)
        c[name + "/K-negative"] = lambda f=f: f(Y, -K, csf, pk2, 2, True, sc, W)
        c[name + "/csf-length"] = lambda f=f: f(Y, K, csf[:3], pk2, 2, True, sc, W)
        c[name + "/csf-no-csf_on"] = lambda f=f: f(Y, K, csf, pk2, 2, False, sc, W)
        c[name + "/csf-no-sig_csf"] = lambda f=f: f(Y, K, csf, pk2, 2, True, None, W)
        c[name + "/csf_on-no-sig_csf"] = lambda f=f: f(Y, K, None, pk2, 2, True, None, W)
        c[name + "/sig_csf-length"] = lambda f=f: f(Y, K, csf, pk2, 2, True, sc[:-1], W)
        c[name + "/sig_csf-length-unused"] = lambda f=f: f(Y, K, None, pk2, 2, False, sc[:-1], W)
        c[name + "/data+K-length"] = lambda f=f: f(Y[:, :-1], K[:3], csf, pk2, 2, True, sc, W)
        c[name + "/K-length+K-range"] = lambda f=f: f(Y, Kbad[:3], csf, pk2, 2, True, sc, W)
        c[name + "/K-range+csf-length"] = lambda f=f: f(Y, Kbad, csf[:3], pk2, 2, True, sc, W)
        c[name + "/csf-length+csf-no-csf_on"] = lambda f=f: f(Y, K, np.ones(3), pk2, 2, False, sc, W)
        c[name + "/csf-no-sig_csf+sig_csf-length"] = lambda f=f: f(Y, K, csf, pk2, 2, False, sc[:-1], W)
        if optional is not None:
            c[name + "/weights-VM"] = lambda f=f: f(Y, K, csf, pk2, 2, True, sc, W[:, :-1])
            c[name + "/weights-M"] = lambda f=f: f(Y, K, csf, pk2, 2, True, sc, np.ones(M + 1))
            c[name + "/weights+K-length"] = lambda f=f: f(Y, K[:3], csf, pk2, 2, True, sc, W[:3])
            c[name + "/peaks+weights"] = lambda f=f: f(Y, K, csf, pk1, 2, True, sc, W[:3])
            c[name + "/data+weights"] = lambda f=f: f(Y[:, :-1], K, csf, pk2, 2, True, sc, W[:3])
        if optional:
            c[name + "/loss"] = lambda f=f: f(Y[:, :-1], K, csf, pk2, 2, True, sc, None)
    c["fit_weighted/ear"] = lambda: E.fit_weighted(P, Y[:, :-1], W, K, csf, pk2, 2, True, sc, ear=np.array([0, 1, 1, 0]))
    c["fit_robust/ear+loss"] = lambda: E.fit_robust(P, Y, K, csf, pk2, 2, True, sc, loss='l2', ear=np.array([0, 1, 1, 0]))
    c["fit_robust/loss+data"] = lambda: E.fit_robust(P, Y[:, :-1], K, csf, pk2, 2, True, sc, loss='l2')
    c["fit_robust/c"] = lambda: E.fit_robust(P, Y, K, csf, pk2, 2, True, sc, c=0.5)
    c["fit_robust/n_iter"] = lambda: E.fit_robust(P, Y, K, csf, pk2, 2, True, sc, n_iter=-1)
    c["fit2d_robust/loss+data"] = lambda: E.fit2d_robust(T, Y[:, :-1], K, csf, pk2, 2, True, sc, loss='l2')
    for name, fd, S in (("fit_robust_dev", E.fit_robust_dev, P), ("fit2d_robust_dev", E.fit2d_robust_dev, T)):
        c[name + "/loss"] = lambda fd=fd, S=S: fd(S, tY, tpk2, 2, loss='l2')
        c[name + "/not-cuda"] = lambda fd=fd, S=S: fd(S, tY, tpk2, 2)
        c[name + "/W0-not-cuda"] = lambda fd=fd, S=S: fd(S, dY, dpk2, 2, d_W0=tw)
        c[name + "/maxfasc"] = lambda fd=fd, S=S: fd(S, dY, dev(V, 12), 4)
        c[name + "/data"] = lambda fd=fd, S=S: fd(S, dev(V, M - 1), dpk2, 2)
        c[name + "/peaks"] = lambda fd=fd, S=S: fd(S, dY, dpk1, 2)
        c[name + "/weights-VM"] = lambda fd=fd, S=S: fd(S, dY, dpk2, 2, d_W0=dev(V, M - 1))
        c[name + "/weights-M"] = lambda fd=fd, S=S: fd(S, dY, dpk2, 2, d_W0=dev(M + 1))
        c[name + "/loss+not-cuda"] = lambda fd=fd, S=S: fd(S, tY, tpk2, 2, c=0.0)
        c[name + "/not-cuda+data"] = lambda fd=fd, S=S: fd(S, tY[:, :-1], tpk2, 2)
        c[name + "/peaks+weights"] = lambda fd=fd, S=S: fd(S, dY, dpk1, 2, d_W0=dev(M + 1))
    for name, f, fd, extra in (("profile2d", E.profile2d, E.profile2d_dev, ()), ("posterior2d", E.posterior2d, E.posterior2d_dev, (tT, tT))):
        hx = (1.0,) if extra else ()
        c[name + "/data"] = lambda f=f, hx=hx: f(T, Y[:, :-1], K, pk2, 2, *hx)
        c[name + "/K-length"] = lambda f=f, hx=hx: f(T, Y, K[:3], pk2, 2, *hx)
        c[name + "/peaks-2"] = lambda f=f, hx=hx: f(T, Y, K, pk1, 2, *hx)
        c[name + "/K-range"] = lambda f=f, hx=hx: f(T, Y, Kbad, pk2, 2, *hx)
        c[name + "/csf-length"] = lambda f=f, hx=hx: f(T, Y, K, pk2, 2, *hx, csf=csf[:3])
        c[name + "/weights-VM"] = lambda f=f, hx=hx: f(T, Y, K, pk2, 2, *hx, W=W[:, :-1])
        c[name + "/weights-M"] = lambda f=f, hx=hx: f(T, Y, K, pk2, 2, *hx, W=np.ones(M + 1))
        c[name + "/data+K-length"] = lambda f=f, hx=hx: f(T, Y[:, :-1], K[:3], pk2, 2, *hx)
        c[name + "/K-length+peaks"] = lambda f=f, hx=hx: f(T, Y, K[:3], pk1, 2, *hx)
        c[name + "/peaks+K-range"] = lambda f=f, hx=hx: f(T, Y, Kbad, pk1, 2, *hx)
        c[name + "/K-range+csf-length"] = lambda f=f, hx=hx: f(T, Y, Kbad, pk2, 2, *hx, csf=csf[:3])
        c[name + "/csf-length+weights"] = lambda f=f, hx=hx: f(T, Y, K, pk2, 2, *hx, csf=csf[:3], W=W[:3])
        dx = (dT, dT) if extra else ()
        c[name + "_dev/K"] = lambda fd=fd, extra=extra: fd(T, tY, cpu(V, 9), 3, *extra)
        c[name + "_dev/data"] = lambda fd=fd, extra=extra: fd(T, tY[:, :-1], tpk2, 2, *extra)
        c[name + "_dev/peaks"] = lambda fd=fd, extra=extra: fd(T, tY, tpk1, 2, *extra)
        c[name + "_dev/weights-VM"] = lambda fd=fd, extra=extra: fd(T, tY, tpk2, 2, *extra, d_W=cpu(V, M - 1))
        c[name + "_dev/weights-M"] = lambda fd=fd, extra=extra: fd(T, tY, tpk2, 2, *extra, d_W=cpu(M + 1))
        c[name + "_dev/not-cuda"] = lambda fd=fd, extra=extra: fd(T, tY, tpk2, 2, *extra)
        c[name + "_dev/weights-not-cuda"] = lambda fd=fd, dx=dx: fd(T, dY, dpk2, 2, *dx, d_W=tw)
        c[name + "_dev/K+data"] = lambda fd=fd, extra=extra: fd(T, tY[:, :-1], cpu(V, 9), 3, *extra)
        c[name + "_dev/peaks+weights"] = lambda fd=fd, extra=extra: fd(T, tY, tpk1, 2, *extra, d_W=cpu(M + 1))
        c[name + "_dev/weights+not-cuda"] = lambda fd=fd, extra=extra: fd(T, tY, tpk2, 2, *extra, d_W=cpu(V, M - 1))
    c["profile2d_dev/out-shape"] = lambda: E.profile2d_dev(T, dY, dpk2, 2, out=dev(V, 2, N + 1))
    c["profile2d_dev/weights+out-shape"] = lambda: E.profile2d_dev(T, dY, dpk2, 2, out=dev(V, 2, N + 1), d_W=dev(M + 1))
    c["posterior2d/sigma"] = lambda: E.posterior2d(T, Y, K, pk2, 2, np.ones(3))
    c["posterior2d/weights+sigma"] = lambda: E.posterior2d(T, Y, K, pk2, 2, np.ones(3), W=W[:3])
    c["posterior2d_dev/T"] = lambda: E.posterior2d_dev(T, tY, tpk2, 2, tT[:3], tT)
    c["posterior2d_dev/shift"] = lambda: E.posterior2d_dev(T, tY, tpk2, 2, tT, 0.0)
    c["posterior2d_dev/T+weights"] = lambda: E.posterior2d_dev(T, tY, tpk2, 2, tT[:3], tT, d_W=cpu(M + 1))
    # ---- the robust weight rule and the bootstrap
    c["robust_weights_dev/loss"] = lambda: E.robust_weights_dev(tY, tY, loss='l2')
    c["robust_weights_dev/not-cuda"] = lambda: E.robust_weights_dev(tY, tY)
    c["robust_weights_dev/prediction"] = lambda: E.robust_weights_dev(dY, dev(V, M - 1))
    c["robust_weights_dev/base-weights"] = lambda: E.robust_weights_dev(dY, dY, dev(M + 1))
    c["robust_weights_dev/previous"] = lambda: E.robust_weights_dev(dY, dY, d_Wprev=dev(V, M - 1))
    c["robust_weights_dev/out-shape"] = lambda: E.robust_weights_dev(dY, dY, out=dev(V, M + 1))
    c["robust_weights_dev/out-not-cuda+prediction"] = lambda: E.robust_weights_dev(dY, dev(V, M - 1), out=tY)
    c["robust_weights/loss+prediction"] = lambda: E.robust_weights(Y, Y[:, :-1], loss='l2')
    c["robust_weights/prediction"] = lambda: E.robust_weights(Y, Y[:, :-1])
    c["robust_weights/base-weights"] = lambda: E.robust_weights(Y, Y, np.ones(M + 1))
    fb = lambda *a, **kw: E.fit_bootstrap(P, *a, **kw)
    ear = np.array([0, 0, 1, 0])
    c["fit_bootstrap/B"] = lambda: fb(Y, K, None, None, pk2, 2, False, False, B=0)
    c["fit_bootstrap/maxfasc"] = lambda: fb(Y, K, None, None, pk2, 4, False, False, B=4)
    c["fit_bootstrap/data"] = lambda: fb(Y[:, :-1], K, None, None, pk2, 2, False, False, B=4)
    c["fit_bootstrap/K-length"] = lambda: fb(Y, K[:3], None, None, pk2, 2, False, False, B=4)
    c["fit_bootstrap/K-range"] = lambda: fb(Y, Kbad, None, None, pk2, 2, False, False, B=4)
    c["fit_bootstrap/csf-length"] = lambda: fb(Y, K, csf[:3], None, pk2, 2, True, False, sc, B=4)
    c["fit_bootstrap/csf-no-csf_on"] = lambda: fb(Y, K, csf, None, pk2, 2, False, False, sc, B=4)
    c["fit_bootstrap/ear-length"] = lambda: fb(Y, K, None, ear[:3], pk2, 2, False, True, None, se, 2, B=4)
    c["fit_bootstrap/ear-no-ear_on"] = lambda: fb(Y, K, None, ear, pk2, 2, False, False, None, se, 2, B=4)
    c["fit_bootstrap/peaks"] = lambda: fb(Y, K, None, None, pk1, 2, False, False, B=4)
    c["fit_bootstrap/csf_on-no-sig_csf"] = lambda: fb(Y, K, csf, None, pk2, 2, True, False, B=4)
    c["fit_bootstrap/sig_csf-length"] = lambda: fb(Y, K, csf, None, pk2, 2, True, False, sc[:-1], B=4)
    c["fit_bootstrap/sig_ear"] = lambda: fb(Y, K, None, ear, pk2, 2, False, True, None, se, 3, B=4)
    c["fit_bootstrap/params"] = lambda: fb(Y, K, None, None, pk2, 2, False, False, B=4, params=prm2[:, :-1])
    c["fit_bootstrap/vox"] = lambda: fb(Y, K, None, None, pk2, 2, False, False, B=4, vox=np.arange(3))
    c["fit_bootstrap/props"] = lambda: fb(Y, K, None, None, pk2, 2, False, False, B=4, props=np.ones((2, N + 1)))
    c["fit_bootstrap/groups-missing"] = lambda: fb(Y, K, None, None, pk2, 2, False, False, B=4, kind='residual')
    c["fit_bootstrap/groups-shape"] = lambda: fb(Y, K, None, None, pk2, 2, False, False, B=4, kind='residual', groups=np.arange(M - 1))
    c["fit_bootstrap/B+maxfasc"] = lambda: fb(Y, K, None, None, pk2, 4, False, False, B=0)
    c["fit_bootstrap/maxfasc+data"] = lambda: fb(Y[:, :-1], K, None, None, pk2, 4, False, False, B=4)
    c["fit_bootstrap/data+K-length"] = lambda: fb(Y[:, :-1], K[:3], None, None, pk2, 2, False, False, B=4)
    c["fit_bootstrap/K-length+K-range"] = lambda: fb(Y, Kbad[:3], None, None, pk2, 2, False, False, B=4)
    c["fit_bootstrap/K-range+csf-length"] = lambda: fb(Y, Kbad, csf[:3], None, pk2, 2, True, False, sc, B=4)
    c["fit_bootstrap/csf-no-csf_on+peaks"] = lambda: fb(Y, K, csf, None, pk1, 2, False, False, sc, B=4)
    c["fit_bootstrap/peaks+sig_csf-length"] = lambda: fb(Y, K, csf, None, pk1, 2, True, False, sc[:-1], B=4)
    c["fit_bootstrap/params+vox"] = lambda: fb(Y, K, None, None, pk2, 2, False, False, B=4, params=prm2[:, :-1], vox=np.arange(3))
    fbd = lambda *a, **kw: E.fit_bootstrap_dev(P, *a, **kw)
    c["fit_bootstrap_dev/B"] = lambda: fbd(tY, tpk2, 2, B=0)
    c["fit_bootstrap_dev/maxfasc"] = lambda: fbd(tY, tpk2, 4, B=4)
    c["fit_bootstrap_dev/not-cuda"] = lambda: fbd(tY, tpk2, 2, B=4)
    c["fit_bootstrap_dev/params-not-cuda"] = lambda: fbd(dY, dpk2, 2, B=4, d_params=tprm2)
    c["fit_bootstrap_dev/data"] = lambda: fbd(dev(V, M - 1), dpk2, 2, B=4)
    c["fit_bootstrap_dev/peaks"] = lambda: fbd(dY, dpk1, 2, B=4)
    c["fit_bootstrap_dev/sig_csf"] = lambda: fbd(dY, dpk2, 2, csf_on=True, d_sig_csf=dev(M - 1), B=4)
    c["fit_bootstrap_dev/sig_ear"] = lambda: fbd(dY, dpk2, 2, ear_on=True, d_sig_ear=dev(M, 2), E=3, B=4)
    c["fit_bootstrap_dev/params"] = lambda: fbd(dY, dpk2, 2, B=4, d_params=dev(V, 6))
    c["fit_bootstrap_dev/pred"] = lambda: fbd(dY, dpk2, 2, B=4, d_pred=dY)
    c["fit_bootstrap_dev/props"] = lambda: fbd(dY, dpk2, 2, B=4, d_props=dev(2, N + 1))
    c["fit_bootstrap_dev/groups-missing"] = lambda: fbd(dY, dpk2, 2, B=4, kind='residual')
    c["fit_bootstrap_dev/groups-not-cuda"] = lambda: fbd(dY, dpk2, 2, B=4, kind='residual', d_groups=cpu(M, dtype=torch.int32))
    c["fit_bootstrap_dev/groups-shape"] = lambda: fbd(dY, dpk2, 2, B=4, kind='residual', d_groups=dev(M - 1, dtype=torch.int32))
    c["fit_bootstrap_dev/vox-dtype"] = lambda: fbd(dY, dpk2, 2, B=4, d_vox=dev(V, dtype=torch.int32))
    c["fit_bootstrap_dev/vox"] = lambda: fbd(dY, dpk2, 2, B=4, d_vox=dev(3, dtype=torch.int64))
    c["fit_bootstrap_dev/maxfasc+not-cuda"] = lambda: fbd(tY, tpk2, -1, B=4)
    c["fit_bootstrap_dev/not-cuda+data"] = lambda: fbd(cpu(V, M - 1), tpk2, 2, B=4)
    c["fit_bootstrap_dev/peaks+params"] = lambda: fbd(dY, dpk1, 2, B=4, d_params=dev(V, 6))
    brd = E.boot_resample_dev
    c["boot_resample_dev/B"] = lambda: brd(tY, tY, tprm2, 2, B=0)
    c["boot_resample_dev/maxfasc"] = lambda: brd(tY, tY, tprm2, 4, B=4)
    c["boot_resample_dev/not-cuda"] = lambda: brd(tY, tY, tprm2, 2, B=4)
    c["boot_resample_dev/prediction"] = lambda: brd(dY, dev(V, M - 1), dprm2, 2, B=4)
    c["boot_resample_dev/params"] = lambda: brd(dY, dY, dev(V, 6), 2, B=4)
    c["boot_resample_dev/peaks"] = lambda: brd(dY, dY, dprm2, 2, B=4, d_peaks=dpk1)
    c["boot_resample_dev/groups-missing"] = lambda: brd(dY, dY, dprm2, 2, B=4, kind='residual')
    c["boot_resample_dev/vox"] = lambda: brd(dY, dY, dprm2, 2, B=4, d_vox=dev(3, dtype=torch.int64))
    c["boot_resample_dev/maxfasc+not-cuda"] = lambda: brd(tY, tY, tprm2, 4, B=4)
    c["boot_resample_dev/not-cuda+prediction"] = lambda: brd(tY, cpu(V, M - 1), tprm2, 2, B=4)
    c["boot_reduce_dev/X"] = lambda: E.boot_reduce_dev(cpu(V, 4), cpu(V, 4, dtype=torch.uint8))
    c["boot_reduce_dev/valid"] = lambda: E.boot_reduce_dev(cpu(V, 4, 3), cpu(V, 4, 2, dtype=torch.uint8))
    c["boot_reduce_dev/q"] = lambda: E.boot_reduce_dev(cpu(V, 4, 3), cpu(V, 4, 3, dtype=torch.uint8), q=(1.5,))
    c["boot_reduce_dev/not-cuda"] = lambda: E.boot_reduce_dev(cpu(V, 4, 3), cpu(V, 4, 3, dtype=torch.uint8))
    c["boot_reduce_dev/valid-dtype"] = lambda: E.boot_reduce_dev(dev(V, 4, 3), dev(V, 4, 3))
    c["boot_reduce_dev/q+valid"] = lambda: E.boot_reduce_dev(cpu(V, 4, 3), cpu(V, 4, 2, dtype=torch.uint8), q=(1.5,))
    c["cleanup_select/shapes"] = lambda: E.cleanup_select(np.ones(3), np.ones(2), np.ones((3, 3)), np.ones((3, 3)), 0.9, 2.0, 0.1, 0.05)
    return c


def outcome(thunk):
    """(exception class name, message) of a call that has to fail before it reaches the library."""
    try:
        thunk()
    except Exception as e:      # noqa: BLE001 - the class is what is recorded
        return type(e).__name__, str(e)
    return None, None


# ---------------------------------------------------------------------------------------------------------------------------
# marshalling: every NumPy entry point against a library that records its calls
class Recorder:
    """Stands for the ctypes library: every function records (name, arguments as ``render`` shows them) and returns MFX_OK."""
    def __init__(self, addresses):
        self.calls, self.addresses = [], addresses

    def render(self, a):
        if a is None or isinstance(a, (str, bool)):
            return a
        if hasattr(a, "contents"):                 # a typed pointer: its C type and the element it addresses
            return (type(a)._type_.__name__[2:], a[0])
        if isinstance(a, int) and a in self.addresses:
            return self.addresses[a]
        assert isinstance(a, (int, float)), a
        return a

    def __getattr__(self, name):
        def f(*args):
            self.calls.append((name, tuple(self.render(a) for a in args)))
            return _lib.MFX_OK
        return f


def marshal_cases():
    """name -> call taking (plan, tables, addresses).  Every input array starts with a value of its own, and the rows of the
    per-voxel ones do too, so that a pointer's first element names the array (and the row of a class's chunk)."""
    Y = 100.0 + np.arange(V * M, dtype=np.float64).reshape(V, M)
    W = 200.0 + np.arange(V * M, dtype=np.float64).reshape(V, M)
    w = 300.0 + np.arange(M, dtype=np.float64)
    pk1 = 400.0 + np.arange(V * 3, dtype=np.float64).reshape(V, 3)
    pk2 = 500.0 + np.arange(V * 6, dtype=np.float64).reshape(V, 6)
    sc, se = 600.0 + np.arange(M), 700.0 + np.arange(M * 2, dtype=np.float64).reshape(M, 2)
    K, Kfull, csf, ear = np.array([1, 2, 2, 1]), np.array([2, 2, 2, 2]), np.array([0, 1, 0, 0]), np.array([0, 0, 1, 0])
    prm = lambda mf, on=False, e=False: 800.0 + np.arange(V * E.num_params(mf, on, e), dtype=np.float64).reshape(V, -1)
    sig, shift = np.array([1.0, 2.0, 3.0, 4.0]), 900.0 + np.arange(V)
    props, groups, vx = 1000.0 + np.arange(2 * N, dtype=np.float64).reshape(2, N), np.arange(M) % 3 + 7, np.array([40, 41, 42, 43])
    c = {}

    def vol_call(f):
        def g(P, T, addr):
            vol = volume()
            addr[vol.array.ctypes.data] = "volume"
            return f(P, vol)
        return g
    c["volume_rows"] = vol_call(lambda P, vol: E.volume_rows(vol, np.array([5, 0, 3]), device=2))
    c["fit_batch_volume"] = vol_call(lambda P, vol: E.fit_batch_volume(P, vol, np.array([5, 0, 3, 1]), K, csf, ear, pk2, 2, True, True, sc, se, 2))
    c["fit_batch_volume/bare"] = vol_call(lambda P, vol: E.fit_batch_volume(P, vol, np.array([5, 0, 3, 1]), np.zeros(V), None, None, None, 0, False, False))
    c["fit_batch"] = lambda P, T, addr: E.fit_batch(P, Y, K, csf, ear, pk2, 2, True, True, sc, se, 2)
    c["fit_batch/rows"] = lambda P, T, addr: E.fit_batch(P, Y, K[:2], None, None, pk2[:2], 2, False, False, rows=np.array([3, 1]))
    c["fit_batch/bare"] = lambda P, T, addr: E.fit_batch(P, Y, np.zeros(V), None, None, None, 0, False, False)
    c["predict"] = lambda P, T, addr: E.predict(P, prm(2, True, True), pk2, 2, True, True, sc, se, 2, Y=Y, sigma_g=sig, ncoils=3, seed=-1, offset=5)
    c["predict/bare"] = lambda P, T, addr: E.predict(P, prm(0), None, 0)
    c["sos_noise"] = lambda P, T, addr: E.sos_noise(Y, 2.5, ncoils=2, seed=9, offset=1 << 40, device=1)
    c["sos_noise/element"] = lambda P, T, addr: E.sos_noise(Y, W)
    for tag, wt in (("", None), ("/W-VM", W), ("/W-M", w)):
        c["profile" + tag] = lambda P, T, addr, wt=wt: E.profile(P, Y, K, csf, pk2, 2, True, sc, W=wt)
        c["profile/partner" + tag] = lambda P, T, addr, wt=wt: E.profile(P, Y, K, csf, pk2, 2, True, sc, partner=True, W=wt)
        c["pair_objectives" + tag] = lambda P, T, addr, wt=wt: E.pair_objectives(P, Y, pk2, W=wt)
        c["pair_objectives/csf" + tag] = lambda P, T, addr, wt=wt: E.pair_objectives(P, Y, pk2, True, sc, W=wt)
        c["posterior" + tag] = lambda P, T, addr, wt=wt: E.posterior(P, Y, K, csf, pk2, 2, True, sc, sig, shift=shift, W=wt)
        c["posterior/own-shift" + tag] = lambda P, T, addr, wt=wt: E.posterior(P, Y, K, csf, pk2, 2, True, sc, 0.5, W=wt)
        c["posterior2d" + tag] = lambda P, T, addr, wt=wt: E.posterior2d(T, Y, K, pk2, 2, sig, shift=shift, W=wt)
        c["posterior2d/own-shift" + tag] = lambda P, T, addr, wt=wt: E.posterior2d(T, Y, K, pk2, 2, 0.5, csf=csf, W=wt)
        c["profile2d" + tag] = lambda P, T, addr, wt=wt: E.profile2d(T, Y, K, pk2, 2, W=wt)
        c["profile2d/partner" + tag] = lambda P, T, addr, wt=wt: E.profile2d(T, Y, K, pk2, 2, partner=True, csf=csf, W=wt)
        c["fit_robust" + tag] = lambda P, T, addr, wt=wt: E.fit_robust(P, Y, K, csf, pk2, 2, True, sc, W0=wt, loss='huber', c=2.0, n_iter=2)
        c["fit2d_robust" + tag] = lambda P, T, addr, wt=wt: E.fit2d_robust(T, Y, K, csf, pk2, 2, True, sc, W0=wt, loss='tukey', c=3.0, n_iter=0)
        if wt is not None:
            c["fit2d_weighted" + tag] = lambda P, T, addr, wt=wt: E.fit2d_weighted(T, Y, wt, K, csf, pk2, 2, True, sc)
            c["fit_weighted" + tag] = lambda P, T, addr, wt=wt: E.fit_weighted(P, Y, wt, K, csf, pk2, 2, True, sc)
    c["fit2d"] = lambda P, T, addr: E.fit2d(T, Y, K, csf, pk2, 2, True, sc)
    c["fit2d/bare"] = lambda P, T, addr: E.fit2d(T, Y, np.zeros(V), None, None, 0, False)
    c["fit2d_weighted/bare"] = lambda P, T, addr: E.fit2d_weighted(T, Y, w, np.zeros(V), None, None, 0, False)
    c["fit_weighted/bare"] = lambda P, T, addr: E.fit_weighted(P, Y, w, np.zeros(V), None, None, 0, False)
    c["fit_robust/bare"] = lambda P, T, addr: E.fit_robust(P, Y, np.zeros(V), None, None, 0, False, n_iter=0)
    c["fit2d_robust/bare"] = lambda P, T, addr: E.fit2d_robust(T, Y, np.zeros(V), None, None, 0, False)
    c["predict2d"] = lambda P, T, addr: E.predict2d(T, prm(2, True), pk2, 2, True, sc, Y=Y, sigma_g=sig, ncoils=3, seed=-1, offset=5)
    c["predict2d/bare"] = lambda P, T, addr: E.predict2d(T, prm(0), None, 0)
    c["fit_bootstrap"] = lambda P, T, addr: E.fit_bootstrap(P, Y, K, csf, ear, pk2, 2, True, True, sc, se, 2, B=4, kind='residual', seed=-3,
                                                            inflate=False, offset=11, q=(0.1, 0.9), props=props, groups=groups,
                                                            params=prm(2, True, True), vox=vx, max_bytes=1 << 20, keep=True)
    c["fit_bootstrap/bare"] = lambda P, T, addr: E.fit_bootstrap(P, Y, np.zeros(V), None, None, None, 0, False, False, B=3, q=())
    c["fit_bootstrap/flags-unused"] = lambda P, T, addr: E.fit_bootstrap(P, Y, Kfull, None, None, pk2, 2, False, False, sc, se, 2, B=2)
    c["cleanup_select"] = lambda P, T, addr: E.cleanup_select(Y[:, 0], W[:, 0], pk1, pk2[:, :3], 0.9, 2, 0.25, 0.125, device=3)
    return c


def recorded(call, monkeypatch):
    addr = {}
    rec = Recorder(addr)
    monkeypatch.setattr(E.L, "lib", lambda: rec)
    call(Stand("plan"), Stand("tables"), addr)
    return rec.calls


ERROR_CASES, MARSHAL_CASES = error_cases(), marshal_cases()


def test_tables_cover_the_recorded_expectations():
    assert sorted(ERROR_CASES) == sorted(EXPECTED_ERRORS) and sorted(MARSHAL_CASES) == sorted(EXPECTED_CALLS)
    assert all(cls is not None for cls, _ in EXPECTED_ERRORS.values())


@pytest.mark.parametrize("name", list(ERROR_CASES))
def test_malformed_call_raises_what_it_always_raised(name):
    assert outcome(ERROR_CASES[name]) == EXPECTED_ERRORS[name]


@pytest.mark.parametrize("name", list(MARSHAL_CASES))
def test_valid_call_reaches_the_library_as_it_always_did(name, monkeypatch):
    assert recorded(MARSHAL_CASES[name], monkeypatch) == EXPECTED_CALLS[name]


# ---------------------------------------------------------------------------------------------------------------------------
# recorded from the engine.py before the shared helpers: name -> (exception class, message), and name -> the C calls made,
# each (function, arguments): a scalar as it is, None for a null pointer, (C type, first element) for a pointer
EXPECTED_ERRORS = {'fit_batch/Y-1d': ('ValueError', 'Y should be a 2-D array [voxels x measurements]'),
 'fit_batch/rows-range': ('ValueError', 'rows out of range'),
 'fit_batch/M': ('ValueError', 'data has 7 measurements, protocol has 8'),
 'fit_batch/K-length': ('ValueError', 'K should have one entry per voxel'),
 'fit_batch/peaks-2': ('ValueError', 'peaks should have 6 columns'),
 'fit_batch/peaks-0-ignored': ('AssertionError', 'the device was touched before the arguments were checked'),
 'fit_batch/M+K-length': ('ValueError', 'data has 7 measurements, protocol has 8'),
 'fit_batch/K-length+peaks': ('ValueError', 'K should have one entry per voxel'),
 'fit_batch/rows-range+M': ('ValueError', 'rows out of range'),
 'fit_batch_volume/M': ('ValueError', 'data has 7 measurements, protocol has 8'),
 'fit_batch_volume/vox-range': ('ValueError', 'voxel indices out of range'),
 'fit_batch_volume/K-length': ('ValueError', 'K should have one entry per voxel'),
 'fit_batch_volume/peaks-2': ('ValueError', 'peaks should have 6 columns'),
 'fit_batch_volume/peaks-0-ignored': ('AssertionError', 'the device was touched before the arguments were checked'),
 'fit_batch_volume/M+vox-range': ('ValueError', 'data has 7 measurements, protocol has 8'),
 'fit_batch_volume/vox-range+K-length': ('ValueError', 'voxel indices out of range'),
 'fit_batch_volume/K-length+peaks': ('ValueError', 'K should have one entry per voxel'),
 'volume_rows/vox-range': ('ValueError', 'voxel indices out of range'),
 'fit_batch_dev/not-cuda': ('AssertionError', ''),
 'fit_batch_dev/M': ('ValueError', 'data has 7 measurements, protocol has 8'),
 'fit_batch_dev/peaks-not-cuda': ('AssertionError', ''),
 'fit_batch_dev/peaks-2': ('ValueError', 'peaks should have shape (4, 6)'),
 'fit_batch_dev/not-cuda+M': ('AssertionError', ''),
 'fit_batch_dev/M+peaks-not-cuda': ('ValueError', 'data has 7 measurements, protocol has 8'),
 'rotate_columns_dev/not-cuda': ('AssertionError', ''),
 'predict/maxfasc': ('ValueError', 'maxfasc must be 0..3'),
 'predict/params': ('ValueError',
                    'params should have 7 columns (maxfasc = 2, csf_on = False, ear_on = False), got shape (4, 6)'),
 'predict/peaks': ('ValueError', 'peaks should have shape (4, 6)'),
 'predict/sig_csf': ('ValueError', 'sig_csf has 7 entries, protocol has 8'),
 'predict/sig_ear': ('ValueError', 'sig_ear should have shape (8, E) with E >= 1'),
 'predict/Y': ('ValueError', 'data has shape (3, 8), protocol has 8 measurements for 4 voxels'),
 'predict/sigma-missing': ('ValueError', 'noise (ncoils > 0) needs sigma_g'),
 'predict/sigma-shape': ('ValueError',
                         'sigma_g should be a scalar, one value per voxel (4) or one per element (4, 8), got shape (3,)'),
 'predict/maxfasc+params': ('ValueError', 'maxfasc must be 0..3'),
 'predict/params+peaks': ('ValueError',
                          'params should have 7 columns (maxfasc = 2, csf_on = False, ear_on = False), got shape (4, 6)'),
 'predict/Y+sigma-missing': ('ValueError', 'data has shape (3, 8), protocol has 8 measurements for 4 voxels'),
 'predict_dev/not-cuda': ('AssertionError', ''),
 'predict_dev/peaks-not-cuda': ('AssertionError', ''),
 'predict_dev/params': ('ValueError',
                        'params should have 7 columns (maxfasc = 2, csf_on = False, ear_on = False), got shape (4, 6)'),
 'predict_dev/peaks': ('ValueError', 'peaks should have shape (4, 6)'),
 'predict_dev/sigma-missing': ('ValueError', 'noise (ncoils > 0) needs sigma_g'),
 'predict_dev/out-shape': ('AssertionError', ''),
 'predict_dev/not-cuda+params': ('AssertionError', ''),
 'predict_dev/Y-not-cuda+peaks': ('AssertionError', ''),
 'predict_dev/sigma-missing+out-shape': ('ValueError', 'noise (ncoils > 0) needs sigma_g'),
 'sos_noise/sigma-shape': ('ValueError', 'sigma_g should be a scalar or have the shape (4, 8) of S0, got (3,)'),
 'sos_noise_dev/not-cuda': ('AssertionError', ''),
 'sos_noise_dev/sigma-shape': ('ValueError', 'sigma_g should be a scalar or have the shape (4, 8) of S0, got (3,)'),
 'sos_noise_dev/ncoils': ('ValueError', 'ncoils should be at least 1'),
 'sos_noise_dev/out-shape': ('AssertionError', ''),
 'sos_noise_dev/not-cuda+sigma-shape': ('AssertionError', ''),
 'sos_noise_dev/sigma-shape+ncoils': ('ValueError', 'sigma_g should be a scalar or have the shape (4, 8) of S0, got (3,)'),
 'predict2d/maxfasc': ('NotImplementedError', 'the 2-D protocol prediction serves 0 to 3 fascicles per voxel (maxfasc = 4)'),
 'predict2d/params': ('ValueError', 'params should have 7 columns (maxfasc = 2, csf_on = False), got shape (4, 6)'),
 'predict2d/peaks': ('ValueError', 'peaks should have shape (4, 6)'),
 'predict2d/sig_csf': ('ValueError', 'sig_csf has 7 entries, protocol has 8'),
 'predict2d/Y': ('ValueError', 'data has shape (3, 8), protocol has 8 measurements for 4 voxels'),
 'predict2d/sigma-missing': ('ValueError', 'noise (ncoils > 0) needs sigma_g'),
 'predict2d/sigma-shape': ('ValueError',
                           'sigma_g should be a scalar, one value per voxel (4) or one per element (4, 8), got shape (3,)'),
 'predict2d/maxfasc+params': ('NotImplementedError',
                              'the 2-D protocol prediction serves 0 to 3 fascicles per voxel (maxfasc = 4)'),
 'predict2d_dev/not-cuda': ('AssertionError', ''),
 'predict2d_dev/params': ('ValueError', 'params should have 7 columns (maxfasc = 2, csf_on = False), got shape (4, 6)'),
 'predict2d_dev/out-shape': ('AssertionError', ''),
 'predict2d_dev/not-cuda+params': ('AssertionError', ''),
 'predict2d_dev/sigma-missing+out-shape': ('ValueError', 'noise (ncoils > 0) needs sigma_g'),
 'profile/data': ('ValueError', 'data has shape (4, 7), protocol has 8 measurements'),
 'profile/K-length': ('ValueError', 'K should have one entry per voxel'),
 'profile/weights-VM': ('ValueError', 'weights should have shape (4, 8) or (8,), got (4, 7) (4 voxels)'),
 'profile/weights-M': ('ValueError', 'weights should have shape (4, 8) or (8,), got (9,) (4 voxels)'),
 'profile/peaks-2': ('ValueError', 'peaks should have 6 columns'),
 'profile/csf-no-csf_on': ('ValueError', 'voxels flagged CSF need csf_on and sig_csf'),
 'profile/csf-no-sig_csf': ('ValueError', 'voxels flagged CSF need csf_on and sig_csf'),
 'profile/sig_csf-length': ('ValueError', 'sig_csf has 7 entries, protocol has 8'),
 'profile/csf-length': ('ValueError', 'K, csf and ear should have one entry per voxel'),
 'profile/K-range': ('ValueError', 'K exceeds maxfasc = 2'),
 'profile/data+K-length': ('ValueError', 'data has shape (4, 7), protocol has 8 measurements'),
 'profile/K-length+weights': ('ValueError', 'K should have one entry per voxel'),
 'profile/weights+peaks': ('ValueError', 'weights should have shape (4, 8) or (8,), got (3, 8) (4 voxels)'),
 'profile/peaks+csf': ('ValueError', 'peaks should have 6 columns'),
 'profile/csf+sig_csf-length': ('ValueError', 'voxels flagged CSF need csf_on and sig_csf'),
 'profile/sig_csf-length+K-range': ('ValueError', 'sig_csf has 7 entries, protocol has 8'),
 'profile_dev/csf_on-alone': ('ValueError', 'csf_on without d_sig_csf'),
 'profile_dev/K': ('NotImplementedError',
                   'objective profiles serve K = 1 or 2 fascicles (got 3): three fascicles and voxels without one are out '
                   'of scope'),
 'profile_dev/data': ('ValueError', 'data has shape (4, 7), protocol has 8 measurements'),
 'profile_dev/peaks': ('ValueError', 'peaks should have shape (4, 6)'),
 'profile_dev/sig_csf-length': ('ValueError', 'sig_csf has 7 entries, protocol has 8'),
 'profile_dev/weights-VM': ('ValueError', 'weights should have shape (4, 8) or (8,), got (4, 7) (4 voxels)'),
 'profile_dev/weights-M': ('ValueError', 'weights should have shape (4, 8) or (8,), got (9,) (4 voxels)'),
 'profile_dev/not-cuda': ('AssertionError', ''),
 'profile_dev/weights-not-cuda': ('AssertionError', ''),
 'profile_dev/sig_csf-not-cuda': ('AssertionError', ''),
 'profile_dev/csf_on-alone+K': ('ValueError', 'csf_on without d_sig_csf'),
 'profile_dev/K+data': ('NotImplementedError',
                        'objective profiles serve K = 1 or 2 fascicles (got 3): three fascicles and voxels without one are '
                        'out of scope'),
 'profile_dev/peaks+weights': ('ValueError', 'peaks should have shape (4, 6)'),
 'profile_dev/weights+not-cuda': ('ValueError', 'weights should have shape (4, 8) or (8,), got (4, 7) (4 voxels)'),
 'posterior/data': ('ValueError', 'data has shape (4, 7), protocol has 8 measurements'),
 'posterior/K-length': ('ValueError', 'K should have one entry per voxel'),
 'posterior/weights-VM': ('ValueError', 'weights should have shape (4, 8) or (8,), got (4, 7) (4 voxels)'),
 'posterior/weights-M': ('ValueError', 'weights should have shape (4, 8) or (8,), got (9,) (4 voxels)'),
 'posterior/peaks-2': ('ValueError', 'peaks should have 6 columns'),
 'posterior/csf-no-csf_on': ('ValueError', 'voxels flagged CSF need csf_on and sig_csf'),
 'posterior/csf-no-sig_csf': ('ValueError', 'voxels flagged CSF need csf_on and sig_csf'),
 'posterior/sig_csf-length': ('ValueError', 'sig_csf has 7 entries, protocol has 8'),
 'posterior/csf-length': ('ValueError', 'K, csf and ear should have one entry per voxel'),
 'posterior/K-range': ('ValueError', 'K exceeds maxfasc = 2'),
 'posterior/data+K-length': ('ValueError', 'data has shape (4, 7), protocol has 8 measurements'),
 'posterior/K-length+weights': ('ValueError', 'K should have one entry per voxel'),
 'posterior/weights+peaks': ('ValueError', 'weights should have shape (4, 8) or (8,), got (3, 8) (4 voxels)'),
 'posterior/peaks+csf': ('ValueError', 'peaks should have 6 columns'),
 'posterior/csf+sig_csf-length': ('ValueError', 'voxels flagged CSF need csf_on and sig_csf'),
 'posterior/sig_csf-length+K-range': ('ValueError', 'sig_csf has 7 entries, protocol has 8'),
 'posterior_dev/csf_on-alone': ('ValueError', 'csf_on without d_sig_csf'),
 'posterior_dev/K': ('NotImplementedError',
                     'objective profiles serve K = 1 or 2 fascicles (got 3): three fascicles and voxels without one are out '
                     'of scope'),
 'posterior_dev/data': ('ValueError', 'data has shape (4, 7), protocol has 8 measurements'),
 'posterior_dev/peaks': ('ValueError', 'peaks should have shape (4, 6)'),
 'posterior_dev/sig_csf-length': ('ValueError', 'sig_csf has 7 entries, protocol has 8'),
 'posterior_dev/weights-VM': ('ValueError', 'weights should have shape (4, 8) or (8,), got (4, 7) (4 voxels)'),
 'posterior_dev/weights-M': ('ValueError', 'weights should have shape (4, 8) or (8,), got (9,) (4 voxels)'),
 'posterior_dev/not-cuda': ('AssertionError', ''),
 'posterior_dev/weights-not-cuda': ('AssertionError', ''),
 'posterior_dev/sig_csf-not-cuda': ('AssertionError', ''),
 'posterior_dev/csf_on-alone+K': ('ValueError', 'csf_on without d_sig_csf'),
 'posterior_dev/K+data': ('NotImplementedError',
                          'objective profiles serve K = 1 or 2 fascicles (got 3): three fascicles and voxels without one '
                          'are out of scope'),
 'posterior_dev/peaks+weights': ('ValueError', 'peaks should have shape (4, 6)'),
 'posterior_dev/weights+not-cuda': ('ValueError', 'weights should have shape (4, 8) or (8,), got (4, 7) (4 voxels)'),
 'profile_dev/out-shape': ('AssertionError', ''),
 'profile_dev/weights+out-shape': ('ValueError', 'weights should have shape (4, 8) or (8,), got (9,) (4 voxels)'),
 'posterior/sigma': ('ValueError', 'sigma should be a scalar or have one entry per voxel (4), got shape (3,)'),
 'posterior/shift': ('ValueError', 'shift should be a scalar or have one entry per voxel (4), got shape (3,)'),
 'posterior/K-range+sigma': ('ValueError', 'sigma should be a scalar or have one entry per voxel (4), got shape (3,)'),
 'posterior_dev/T': ('ValueError', 'T should be a tensor with one entry per voxel (4)'),
 'posterior_dev/shift': ('ValueError', 'shift should be a tensor with one entry per voxel (4)'),
 'posterior_dev/T+weights': ('ValueError', 'T should be a tensor with one entry per voxel (4)'),
 'posterior_dev/peaks+T': ('ValueError', 'peaks should have shape (4, 6)'),
 'pair_objectives/csf_on-alone': ('ValueError', 'csf_on without sig_csf'),
 'pair_objectives/data': ('ValueError', 'data has shape (4, 7), protocol has 8 measurements'),
 'pair_objectives/peaks': ('ValueError', 'peaks should have shape (4, 6)'),
 'pair_objectives/sig_csf-length': ('ValueError', 'sig_csf has 7 entries, protocol has 8'),
 'pair_objectives/weights-VM': ('ValueError', 'weights should have shape (4, 8) or (8,), got (4, 7) (4 voxels)'),
 'pair_objectives/weights-M': ('ValueError', 'weights should have shape (4, 8) or (8,), got (9,) (4 voxels)'),
 'pair_objectives/data+peaks': ('ValueError', 'data has shape (4, 7), protocol has 8 measurements'),
 'pair_objectives/sig_csf-length+weights': ('ValueError', 'sig_csf has 7 entries, protocol has 8'),
 'pair_objectives_dev/csf_on-alone': ('ValueError', 'csf_on without d_sig_csf'),
 'pair_objectives_dev/data': ('ValueError', 'data has shape (4, 7), protocol has 8 measurements'),
 'pair_objectives_dev/peaks': ('ValueError', 'peaks should have shape (4, 6)'),
 'pair_objectives_dev/weights-VM': ('ValueError', 'weights should have shape (4, 8) or (8,), got (4, 7) (4 voxels)'),
 'pair_objectives_dev/weights-M': ('ValueError', 'weights should have shape (4, 8) or (8,), got (9,) (4 voxels)'),
 'pair_objectives_dev/not-cuda': ('AssertionError', ''),
 'pair_objectives_dev/weights-not-cuda': ('AssertionError', ''),
 'pair_objectives_dev/peaks+weights': ('ValueError', 'peaks should have shape (4, 6)'),
 'profile_classes/lengths': ('ValueError', 'K, csf and ear should have one entry per voxel'),
 'profile_classes/K-range': ('ValueError', 'K exceeds maxfasc = 2'),
 'rotate2d_dev/not-cuda': ('AssertionError', ''),
 'fit2d_dev/not-cuda': ('AssertionError', ''),
 'fit2d_dev/peaks-not-cuda': ('AssertionError', ''),
 'fit2d_dev/maxfasc': ('NotImplementedError', 'the 2-D protocol fit serves 0 to 3 fascicles per voxel (maxfasc = 4)'),
 'fit2d_dev/data': ('ValueError', 'data has shape (4, 7), protocol has 8 measurements'),
 'fit2d_dev/peaks': ('ValueError', 'peaks should have shape (4, 6)'),
 'fit2d_dev/out-shape': ('AssertionError', ''),
 'fit2d_dev/not-cuda+maxfasc': ('AssertionError', ''),
 'fit2d_dev/peaks+out-shape': ('ValueError', 'peaks should have shape (4, 6)'),
 'fit2d_weighted_dev/maxfasc': ('NotImplementedError',
                                'the 2-D protocol fit serves 0 to 3 fascicles per voxel (maxfasc = 4)'),
 'fit2d_weighted_dev/data': ('ValueError', 'data has shape (4, 7), protocol has 8 measurements'),
 'fit2d_weighted_dev/peaks': ('ValueError', 'peaks should have shape (4, 6)'),
 'fit2d_weighted_dev/weights-VM': ('ValueError', 'weights should have shape (4, 8) or (8,), got (4, 7) (4 voxels)'),
 'fit2d_weighted_dev/weights-M': ('ValueError', 'weights should have shape (4, 8) or (8,), got (9,) (4 voxels)'),
 'fit2d_weighted_dev/not-cuda': ('AssertionError', ''),
 'fit2d_weighted_dev/out-shape': ('AssertionError', ''),
 'fit2d_weighted_dev/peaks+weights': ('ValueError', 'peaks should have shape (4, 6)'),
 'fit2d_weighted_dev/weights+not-cuda': ('ValueError', 'weights should have shape (4, 8) or (8,), got (9,) (4 voxels)'),
 'fit_weighted_dev/not-cuda': ('AssertionError', ''),
 'fit_weighted_dev/maxfasc': ('ValueError',
                              'the weighted fit is not served for maxfasc = 4: it takes 0 to 3 fascicles per voxel'),
 'fit_weighted_dev/data': ('ValueError', 'data has shape (4, 7), protocol has 8 measurements'),
 'fit_weighted_dev/weights-VM': ('ValueError', 'weights should have shape (4, 8) or (8,), got (4, 7) (4 voxels)'),
 'fit_weighted_dev/weights-M': ('ValueError', 'weights should have shape (4, 8) or (8,), got (9,) (4 voxels)'),
 'fit_weighted_dev/peaks': ('ValueError', 'peaks should have shape (4, 6)'),
 'fit_weighted_dev/out-shape': ('AssertionError', ''),
 'fit_weighted_dev/not-cuda+weights': ('AssertionError', ''),
 'fit_weighted_dev/weights+peaks': ('ValueError', 'weights should have shape (4, 8) or (8,), got (9,) (4 voxels)'),
 'fit_weighted_dev/peaks+out-shape': ('ValueError', 'peaks should have shape (4, 6)'),
 'fit2d/maxfasc': ('NotImplementedError', 'the 2-D protocol fit serves 0 to 3 fascicles per voxel (maxfasc = 4)'),
 'fit2d/data': ('ValueError', 'data has shape (4, 7), protocol has 8 measurements'),
 'fit2d/peaks-2': ('ValueError', 'peaks should have shape (4, 6)'),
 'fit2d/peaks-0-ignored': ('AssertionError', 'the device was touched before the arguments were checked'),
 'fit2d/K-length': ('ValueError', 'K should have one entry per voxel'),
 'fit2d/K-range': ('ValueError', 'K should lie in 0..maxfasc = 2'),
 'fit2d/K-negative': ('ValueError', 'K should lie in 0..maxfasc = 2'),
 'fit2d/csf-length': ('ValueError', 'csf should have one entry per voxel'),
 'fit2d/csf-no-csf_on': ('ValueError', 'voxels flagged CSF need csf_on and sig_csf'),
 'fit2d/csf-no-sig_csf': ('ValueError', 'voxels flagged CSF need csf_on and sig_csf'),
 'fit2d/csf_on-no-sig_csf': ('AssertionError', 'the device was touched before the arguments were checked'),
 'fit2d/sig_csf-length': ('ValueError', 'sig_csf has 7 entries, protocol has 8'),
 'fit2d/sig_csf-length-unused': ('ValueError', 'sig_csf has 7 entries, protocol has 8'),
 'fit2d/data+K-length': ('ValueError', 'data has shape (4, 7), protocol has 8 measurements'),
 'fit2d/K-length+K-range': ('ValueError', 'K should have one entry per voxel'),
 'fit2d/K-range+csf-length': ('ValueError', 'K should lie in 0..maxfasc = 2'),
 'fit2d/csf-length+csf-no-csf_on': ('ValueError', 'csf should have one entry per voxel'),
 'fit2d/csf-no-sig_csf+sig_csf-length': ('ValueError', 'voxels flagged CSF need csf_on and sig_csf'),
 'fit2d_weighted/maxfasc': ('NotImplementedError', 'the 2-D protocol fit serves 0 to 3 fascicles per voxel (maxfasc = 4)'),
 'fit2d_weighted/data': ('ValueError', 'data has shape (4, 7), protocol has 8 measurements'),
 'fit2d_weighted/peaks-2': ('ValueError', 'peaks should have shape (4, 6)'),
 'fit2d_weighted/peaks-0-ignored': ('AssertionError', 'the device was touched before the arguments were checked'),
 'fit2d_weighted/K-length': ('ValueError', 'K should have one entry per voxel'),
 'fit2d_weighted/K-range': ('ValueError', 'K should lie in 0..maxfasc = 2'),
 'fit2d_weighted/K-negative': ('ValueError', 'K should lie in 0..maxfasc = 2'),
 'fit2d_weighted/csf-length': ('ValueError', 'csf should have one entry per voxel'),
 'fit2d_weighted/csf-no-csf_on': ('ValueError', 'voxels flagged CSF need csf_on and sig_csf'),
 'fit2d_weighted/csf-no-sig_csf': ('ValueError', 'voxels flagged CSF need csf_on and sig_csf'),
 'fit2d_weighted/csf_on-no-sig_csf': ('AssertionError', 'the device was touched before the arguments were checked'),
 'fit2d_weighted/sig_csf-length': ('ValueError', 'sig_csf has 7 entries, protocol has 8'),
 'fit2d_weighted/sig_csf-length-unused': ('ValueError', 'sig_csf has 7 entries, protocol has 8'),
 'fit2d_weighted/data+K-length': ('ValueError', 'data has shape (4, 7), protocol has 8 measurements'),
 'fit2d_weighted/K-length+K-range': ('ValueError', 'K should have one entry per voxel'),
 'fit2d_weighted/K-range+csf-length': ('ValueError', 'K should lie in 0..maxfasc = 2'),
 'fit2d_weighted/csf-length+csf-no-csf_on': ('ValueError', 'csf should have one entry per voxel'),
 'fit2d_weighted/csf-no-sig_csf+sig_csf-length': ('ValueError', 'voxels flagged CSF need csf_on and sig_csf'),
 'fit2d_weighted/weights-VM': ('ValueError', 'weights should have shape (4, 8) or (8,), got (4, 7) (4 voxels)'),
 'fit2d_weighted/weights-M': ('ValueError', 'weights should have shape (4, 8) or (8,), got (9,) (4 voxels)'),
 'fit2d_weighted/weights+K-length': ('ValueError', 'weights should have shape (4, 8) or (8,), got (3, 8) (4 voxels)'),
 'fit2d_weighted/peaks+weights': ('ValueError', 'peaks should have shape (4, 6)'),
 'fit2d_weighted/data+weights': ('ValueError', 'data has shape (4, 7), protocol has 8 measurements'),
 'fit_weighted/maxfasc': ('ValueError',
                          'the weighted fit is not served for maxfasc = 4: it takes 0 to 3 fascicles per voxel'),
 'fit_weighted/data': ('ValueError', 'data has shape (4, 7), protocol has 8 measurements'),
 'fit_weighted/peaks-2': ('ValueError', 'peaks should have shape (4, 6)'),
 'fit_weighted/peaks-0-ignored': ('AssertionError', 'the device was touched before the arguments were checked'),
 'fit_weighted/K-length': ('ValueError', 'K should have one entry per voxel'),
 'fit_weighted/K-range': ('ValueError', 'K should lie in 0..maxfasc = 2'),
 'fit_weighted/K-negative': ('ValueError', 'K should lie in 0..maxfasc = 2'),
 'fit_weighted/csf-length': ('ValueError', 'csf should have one entry per voxel'),
 'fit_weighted/csf-no-csf_on': ('ValueError', 'voxels flagged CSF need csf_on and sig_csf'),
 'fit_weighted/csf-no-sig_csf': ('ValueError', 'voxels flagged CSF need csf_on and sig_csf'),
 'fit_weighted/csf_on-no-sig_csf': ('AssertionError', 'the device was touched before the arguments were checked'),
 'fit_weighted/sig_csf-length': ('ValueError', 'sig_csf has 7 entries, protocol has 8'),
 'fit_weighted/sig_csf-length-unused': ('ValueError', 'sig_csf has 7 entries, protocol has 8'),
 'fit_weighted/data+K-length': ('ValueError', 'data has shape (4, 7), protocol has 8 measurements'),
 'fit_weighted/K-length+K-range': ('ValueError', 'K should have one entry per voxel'),
 'fit_weighted/K-range+csf-length': ('ValueError', 'K should lie in 0..maxfasc = 2'),
 'fit_weighted/csf-length+csf-no-csf_on': ('ValueError', 'csf should have one entry per voxel'),
 'fit_weighted/csf-no-sig_csf+sig_csf-length': ('ValueError', 'voxels flagged CSF need csf_on and sig_csf'),
 'fit_weighted/weights-VM': ('ValueError', 'weights should have shape (4, 8) or (8,), got (4, 7) (4 voxels)'),
 'fit_weighted/weights-M': ('ValueError', 'weights should have shape (4, 8) or (8,), got (9,) (4 voxels)'),
 'fit_weighted/weights+K-length': ('ValueError', 'weights should have shape (4, 8) or (8,), got (3, 8) (4 voxels)'),
 'fit_weighted/peaks+weights': ('ValueError', 'weights should have shape (4, 8) or (8,), got (3, 8) (4 voxels)'),
 'fit_weighted/data+weights': ('ValueError', 'data has shape (4, 7), protocol has 8 measurements'),
 'fit_robust/maxfasc': ('ValueError', 'the weighted fit is not served for maxfasc = 4: it takes 0 to 3 fascicles per voxel'),
 'fit_robust/data': ('ValueError', 'data has shape (4, 7), protocol has 8 measurements'),
 'fit_robust/peaks-2': ('ValueError', 'peaks should have shape (4, 6)'),
 'fit_robust/peaks-0-ignored': ('AssertionError', 'the device was touched before the arguments were checked'),
 'fit_robust/K-length': ('ValueError', 'K should have one entry per voxel'),
 'fit_robust/K-range': ('ValueError', 'K should lie in 0..maxfasc = 2'),
 'fit_robust/K-negative': ('ValueError', 'K should lie in 0..maxfasc = 2'),
 'fit_robust/csf-length': ('ValueError', 'csf should have one entry per voxel'),
 'fit_robust/csf-no-csf_on': ('ValueError', 'voxels flagged CSF need csf_on and sig_csf'),
 'fit_robust/csf-no-sig_csf': ('ValueError', 'voxels flagged CSF need csf_on and sig_csf'),
 'fit_robust/csf_on-no-sig_csf': ('ValueError', 'csf_on needs sig_csf'),
 'fit_robust/sig_csf-length': ('ValueError', 'sig_csf has 7 entries, protocol has 8'),
 'fit_robust/sig_csf-length-unused': ('ValueError', 'sig_csf has 7 entries, protocol has 8'),
 'fit_robust/data+K-length': ('ValueError', 'data has shape (4, 7), protocol has 8 measurements'),
 'fit_robust/K-length+K-range': ('ValueError', 'K should have one entry per voxel'),
 'fit_robust/K-range+csf-length': ('ValueError', 'K should lie in 0..maxfasc = 2'),
 'fit_robust/csf-length+csf-no-csf_on': ('ValueError', 'csf should have one entry per voxel'),
 'fit_robust/csf-no-sig_csf+sig_csf-length': ('ValueError', 'voxels flagged CSF need csf_on and sig_csf'),
 'fit_robust/weights-VM': ('ValueError', 'weights should have shape (4, 8) or (8,), got (4, 7) (4 voxels)'),
 'fit_robust/weights-M': ('ValueError', 'weights should have shape (4, 8) or (8,), got (9,) (4 voxels)'),
 'fit_robust/weights+K-length': ('ValueError', 'weights should have shape (4, 8) or (8,), got (3, 8) (4 voxels)'),
 'fit_robust/peaks+weights': ('ValueError', 'weights should have shape (4, 8) or (8,), got (3, 8) (4 voxels)'),
 'fit_robust/data+weights': ('ValueError', 'data has shape (4, 7), protocol has 8 measurements'),
 'fit_robust/loss': ('ValueError', 'data has shape (4, 7), protocol has 8 measurements'),
 'fit2d_robust/maxfasc': ('NotImplementedError', 'the 2-D protocol fit serves 0 to 3 fascicles per voxel (maxfasc = 4)'),
 'fit2d_robust/data': ('ValueError', 'data has shape (4, 7), protocol has 8 measurements'),
 'fit2d_robust/peaks-2': ('ValueError', 'peaks should have shape (4, 6)'),
 'fit2d_robust/peaks-0-ignored': ('AssertionError', 'the device was touched before the arguments were checked'),
 'fit2d_robust/K-length': ('ValueError', 'K should have one entry per voxel'),
 'fit2d_robust/K-range': ('ValueError', 'K should lie in 0..maxfasc = 2'),
 'fit2d_robust/K-negative': ('ValueError', 'K should lie in 0..maxfasc = 2'),
 'fit2d_robust/csf-length': ('ValueError', 'csf should have one entry per voxel'),
 'fit2d_robust/csf-no-csf_on': ('ValueError', 'voxels flagged CSF need csf_on and sig_csf'),
 'fit2d_robust/csf-no-sig_csf': ('ValueError', 'voxels flagged CSF need csf_on and sig_csf'),
 'fit2d_robust/csf_on-no-sig_csf': ('ValueError', 'csf_on needs sig_csf'),
 'fit2d_robust/sig_csf-length': ('ValueError', 'sig_csf has 7 entries, protocol has 8'),
 'fit2d_robust/sig_csf-length-unused': ('ValueError', 'sig_csf has 7 entries, protocol has 8'),
 'fit2d_robust/data+K-length': ('ValueError', 'data has shape (4, 7), protocol has 8 measurements'),
 'fit2d_robust/K-length+K-range': ('ValueError', 'K should have one entry per voxel'),
 'fit2d_robust/K-range+csf-length': ('ValueError', 'K should lie in 0..maxfasc = 2'),
 'fit2d_robust/csf-length+csf-no-csf_on': ('ValueError', 'csf should have one entry per voxel'),
 'fit2d_robust/csf-no-sig_csf+sig_csf-length': ('ValueError', 'voxels flagged CSF need csf_on and sig_csf'),
 'fit2d_robust/weights-VM': ('ValueError', 'weights should have shape (4, 8) or (8,), got (4, 7) (4 voxels)'),
 'fit2d_robust/weights-M': ('ValueError', 'weights should have shape (4, 8) or (8,), got (9,) (4 voxels)'),
 'fit2d_robust/weights+K-length': ('ValueError', 'weights should have shape (4, 8) or (8,), got (3, 8) (4 voxels)'),
 'fit2d_robust/peaks+weights': ('ValueError', 'peaks should have shape (4, 6)'),
 'fit2d_robust/data+weights': ('ValueError', 'data has shape (4, 7), protocol has 8 measurements'),
 'fit2d_robust/loss': ('ValueError', 'data has shape (4, 7), protocol has 8 measurements'),
 'fit_weighted/ear': ('ValueError', 'the weighted fit is not served for voxels with an EAR compartment (2 flagged)'),
 'fit_robust/ear+loss': ('ValueError', 'the robust fit is not served for voxels with an EAR compartment (2 flagged)'),
 'fit_robust/loss+data': ('ValueError', "robust loss should be one of 'cutoff', 'huber', 'tukey', got 'l2'"),
 'fit_robust/c': ('ValueError', 'robust c should be a finite number >= 1, got 0.5'),
 'fit_robust/n_iter': ('ValueError', 'robust n_iter should be a non-negative integer, got -1'),
 'fit2d_robust/loss+data': ('ValueError', "robust loss should be one of 'cutoff', 'huber', 'tukey', got 'l2'"),
 'fit_robust_dev/loss': ('ValueError', "robust loss should be one of 'cutoff', 'huber', 'tukey', got 'l2'"),
 'fit_robust_dev/not-cuda': ('AssertionError', ''),
 'fit_robust_dev/W0-not-cuda': ('AssertionError', ''),
 'fit_robust_dev/maxfasc': ('ValueError',
                            'the weighted fit is not served for maxfasc = 4: it takes 0 to 3 fascicles per voxel'),
 'fit_robust_dev/data': ('ValueError', 'data has shape (4, 7), protocol has 8 measurements'),
 'fit_robust_dev/peaks': ('ValueError', 'peaks should have shape (4, 6)'),
 'fit_robust_dev/weights-VM': ('ValueError', 'weights should have shape (4, 8) or (8,), got (4, 7) (4 voxels)'),
 'fit_robust_dev/weights-M': ('ValueError', 'weights should have shape (4, 8) or (8,), got (9,) (4 voxels)'),
 'fit_robust_dev/loss+not-cuda': ('ValueError', 'robust c should be a finite number >= 1, got 0.0'),
 'fit_robust_dev/not-cuda+data': ('AssertionError', ''),
 'fit_robust_dev/peaks+weights': ('ValueError', 'weights should have shape (4, 8) or (8,), got (9,) (4 voxels)'),
 'fit2d_robust_dev/loss': ('ValueError', "robust loss should be one of 'cutoff', 'huber', 'tukey', got 'l2'"),
 'fit2d_robust_dev/not-cuda': ('AssertionError', ''),
 'fit2d_robust_dev/W0-not-cuda': ('AssertionError', ''),
 'fit2d_robust_dev/maxfasc': ('NotImplementedError', 'the 2-D protocol fit serves 0 to 3 fascicles per voxel (maxfasc = 4)'),
 'fit2d_robust_dev/data': ('ValueError', 'data has shape (4, 7), protocol has 8 measurements'),
 'fit2d_robust_dev/peaks': ('ValueError', 'peaks should have shape (4, 6)'),
 'fit2d_robust_dev/weights-VM': ('ValueError', 'weights should have shape (4, 8) or (8,), got (4, 7) (4 voxels)'),
 'fit2d_robust_dev/weights-M': ('ValueError', 'weights should have shape (4, 8) or (8,), got (9,) (4 voxels)'),
 'fit2d_robust_dev/loss+not-cuda': ('ValueError', 'robust c should be a finite number >= 1, got 0.0'),
 'fit2d_robust_dev/not-cuda+data': ('AssertionError', ''),
 'fit2d_robust_dev/peaks+weights': ('ValueError', 'peaks should have shape (4, 6)'),
 'profile2d/data': ('ValueError', 'data has shape (4, 7), protocol has 8 measurements'),
 'profile2d/K-length': ('ValueError', 'K should have one entry per voxel'),
 'profile2d/peaks-2': ('ValueError', 'peaks should have 6 columns'),
 'profile2d/K-range': ('ValueError', 'K should lie in 0..maxfasc = 2'),
 'profile2d/csf-length': ('ValueError', 'csf should have one entry per voxel'),
 'profile2d/weights-VM': ('ValueError', 'weights should have shape (4, 8) or (8,), got (4, 7) (4 voxels)'),
 'profile2d/weights-M': ('ValueError', 'weights should have shape (4, 8) or (8,), got (9,) (4 voxels)'),
 'profile2d/data+K-length': ('ValueError', 'data has shape (4, 7), protocol has 8 measurements'),
 'profile2d/K-length+peaks': ('ValueError', 'K should have one entry per voxel'),
 'profile2d/peaks+K-range': ('ValueError', 'peaks should have 6 columns'),
 'profile2d/K-range+csf-length': ('ValueError', 'K should lie in 0..maxfasc = 2'),
 'profile2d/csf-length+weights': ('ValueError', 'csf should have one entry per voxel'),
 'profile2d_dev/K': ('NotImplementedError',
                     'soft fits and profiles of 2-D protocols serve K = 1 or 2 fascicles (got 3): three fascicles and '
                     'voxels without one are out of scope'),
 'profile2d_dev/data': ('ValueError', 'data has shape (4, 7), protocol has 8 measurements'),
 'profile2d_dev/peaks': ('ValueError', 'peaks should have shape (4, 6)'),
 'profile2d_dev/weights-VM': ('ValueError', 'weights should have shape (4, 8) or (8,), got (4, 7) (4 voxels)'),
 'profile2d_dev/weights-M': ('ValueError', 'weights should have shape (4, 8) or (8,), got (9,) (4 voxels)'),
 'profile2d_dev/not-cuda': ('AssertionError', ''),
 'profile2d_dev/weights-not-cuda': ('AssertionError', ''),
 'profile2d_dev/K+data': ('NotImplementedError',
                          'soft fits and profiles of 2-D protocols serve K = 1 or 2 fascicles (got 3): three fascicles and '
                          'voxels without one are out of scope'),
 'profile2d_dev/peaks+weights': ('ValueError', 'peaks should have shape (4, 6)'),
 'profile2d_dev/weights+not-cuda': ('ValueError', 'weights should have shape (4, 8) or (8,), got (4, 7) (4 voxels)'),
 'posterior2d/data': ('ValueError', 'data has shape (4, 7), protocol has 8 measurements'),
 'posterior2d/K-length': ('ValueError', 'K should have one entry per voxel'),
 'posterior2d/peaks-2': ('ValueError', 'peaks should have 6 columns'),
 'posterior2d/K-range': ('ValueError', 'K should lie in 0..maxfasc = 2'),
 'posterior2d/csf-length': ('ValueError', 'csf should have one entry per voxel'),
 'posterior2d/weights-VM': ('ValueError', 'weights should have shape (4, 8) or (8,), got (4, 7) (4 voxels)'),
 'posterior2d/weights-M': ('ValueError', 'weights should have shape (4, 8) or (8,), got (9,) (4 voxels)'),
 'posterior2d/data+K-length': ('ValueError', 'data has shape (4, 7), protocol has 8 measurements'),
 'posterior2d/K-length+peaks': ('ValueError', 'K should have one entry per voxel'),
 'posterior2d/peaks+K-range': ('ValueError', 'peaks should have 6 columns'),
 'posterior2d/K-range+csf-length': ('ValueError', 'K should lie in 0..maxfasc = 2'),
 'posterior2d/csf-length+weights': ('ValueError', 'csf should have one entry per voxel'),
 'posterior2d_dev/K': ('NotImplementedError',
                       'soft fits and profiles of 2-D protocols serve K = 1 or 2 fascicles (got 3): three fascicles and '
                       'voxels without one are out of scope'),
 'posterior2d_dev/data': ('ValueError', 'data has shape (4, 7), protocol has 8 measurements'),
 'posterior2d_dev/peaks': ('ValueError', 'peaks should have shape (4, 6)'),
 'posterior2d_dev/weights-VM': ('ValueError', 'weights should have shape (4, 8) or (8,), got (4, 7) (4 voxels)'),
 'posterior2d_dev/weights-M': ('ValueError', 'weights should have shape (4, 8) or (8,), got (9,) (4 voxels)'),
 'posterior2d_dev/not-cuda': ('AssertionError', ''),
 'posterior2d_dev/weights-not-cuda': ('AssertionError', ''),
 'posterior2d_dev/K+data': ('NotImplementedError',
                            'soft fits and profiles of 2-D protocols serve K = 1 or 2 fascicles (got 3): three fascicles '
                            'and voxels without one are out of scope'),
 'posterior2d_dev/peaks+weights': ('ValueError', 'peaks should have shape (4, 6)'),
 'posterior2d_dev/weights+not-cuda': ('ValueError', 'weights should have shape (4, 8) or (8,), got (4, 7) (4 voxels)'),
 'profile2d_dev/out-shape': ('AssertionError', ''),
 'profile2d_dev/weights+out-shape': ('ValueError', 'weights should have shape (4, 8) or (8,), got (9,) (4 voxels)'),
 'posterior2d/sigma': ('ValueError', 'sigma should be a scalar or have one entry per voxel (4), got shape (3,)'),
 'posterior2d/weights+sigma': ('ValueError', 'weights should have shape (4, 8) or (8,), got (3, 8) (4 voxels)'),
 'posterior2d_dev/T': ('ValueError', 'T should be a tensor with one entry per voxel (4)'),
 'posterior2d_dev/shift': ('ValueError', 'shift should be a tensor with one entry per voxel (4)'),
 'posterior2d_dev/T+weights': ('ValueError', 'T should be a tensor with one entry per voxel (4)'),
 'robust_weights_dev/loss': ('ValueError', "robust loss should be one of 'cutoff', 'huber', 'tukey', got 'l2'"),
 'robust_weights_dev/not-cuda': ('AssertionError', ''),
 'robust_weights_dev/prediction': ('ValueError', "prediction should have the data's shape (4, 8), got (4, 7)"),
 'robust_weights_dev/base-weights': ('ValueError', 'base weights should have shape (4, 8) or (8,), got (9,) (4 voxels)'),
 'robust_weights_dev/previous': ('ValueError', 'previous weights should have shape (4, 8), got (4, 7)'),
 'robust_weights_dev/out-shape': ('AssertionError', ''),
 'robust_weights_dev/out-not-cuda+prediction': ('AssertionError', ''),
 'robust_weights/loss+prediction': ('ValueError', "robust loss should be one of 'cutoff', 'huber', 'tukey', got 'l2'"),
 'robust_weights/prediction': ('ValueError', "prediction should have the data's shape (4, 8), got (4, 7)"),
 'robust_weights/base-weights': ('ValueError', 'base weights should have shape (4, 8) or (8,), got (9,) (4 voxels)'),
 'fit_bootstrap/B': ('ValueError', 'bootstrap B should be an integer >= 1, got 0'),
 'fit_bootstrap/maxfasc': ('ValueError', 'maxfasc must be 0..3'),
 'fit_bootstrap/data': ('ValueError', 'data should have shape (voxels, 8), got (4, 7)'),
 'fit_bootstrap/K-length': ('ValueError', 'K should have one entry per voxel'),
 'fit_bootstrap/K-range': ('ValueError', 'K should lie in 0..maxfasc = 2'),
 'fit_bootstrap/csf-length': ('ValueError', 'csf should have one entry per voxel'),
 'fit_bootstrap/csf-no-csf_on': ('ValueError', 'voxels flagged CSF need csf_on'),
 'fit_bootstrap/ear-length': ('ValueError', 'ear should have one entry per voxel'),
 'fit_bootstrap/ear-no-ear_on': ('ValueError', 'voxels flagged EAR need ear_on'),
 'fit_bootstrap/peaks': ('ValueError', 'peaks should have shape (4, 6)'),
 'fit_bootstrap/csf_on-no-sig_csf': ('ValueError', 'csf_on needs sig_csf with 8 entries'),
 'fit_bootstrap/sig_csf-length': ('ValueError', 'csf_on needs sig_csf with 8 entries'),
 'fit_bootstrap/sig_ear': ('ValueError', 'sig_ear should have shape (8, E) with E >= 1'),
 'fit_bootstrap/params': ('ValueError', 'params should have shape (4, 7), got (4, 6)'),
 'fit_bootstrap/vox': ('ValueError', 'vox should have one entry per voxel'),
 'fit_bootstrap/props': ('ValueError', 'props should have shape (nprop, 5), got (2, 6)'),
 'fit_bootstrap/groups-missing': ('ValueError',
                                  'the residual bootstrap needs groups (the plan knows no scheme to derive them from)'),
 'fit_bootstrap/groups-shape': ('ValueError', 'groups should be 8 integers (one per measurement), got shape (7,)'),
 'fit_bootstrap/B+maxfasc': ('ValueError', 'bootstrap B should be an integer >= 1, got 0'),
 'fit_bootstrap/maxfasc+data': ('ValueError', 'maxfasc must be 0..3'),
 'fit_bootstrap/data+K-length': ('ValueError', 'data should have shape (voxels, 8), got (4, 7)'),
 'fit_bootstrap/K-length+K-range': ('ValueError', 'K should have one entry per voxel'),
 'fit_bootstrap/K-range+csf-length': ('ValueError', 'K should lie in 0..maxfasc = 2'),
 'fit_bootstrap/csf-no-csf_on+peaks': ('ValueError', 'voxels flagged CSF need csf_on'),
 'fit_bootstrap/peaks+sig_csf-length': ('ValueError', 'peaks should have shape (4, 6)'),
 'fit_bootstrap/params+vox': ('ValueError', 'params should have shape (4, 7), got (4, 6)'),
 'fit_bootstrap_dev/B': ('ValueError', 'bootstrap B should be an integer >= 1, got 0'),
 'fit_bootstrap_dev/maxfasc': ('ValueError', 'maxfasc must be 0..3'),
 'fit_bootstrap_dev/not-cuda': ('AssertionError', ''),
 'fit_bootstrap_dev/params-not-cuda': ('AssertionError', ''),
 'fit_bootstrap_dev/data': ('ValueError', 'data should have shape (voxels, 8), got (4, 7)'),
 'fit_bootstrap_dev/peaks': ('ValueError', 'peaks should have shape (4, 6)'),
 'fit_bootstrap_dev/sig_csf': ('ValueError', 'csf_on needs sig_csf with 8 entries'),
 'fit_bootstrap_dev/sig_ear': ('ValueError', 'sig_ear should have shape (8, E) with E >= 1'),
 'fit_bootstrap_dev/params': ('ValueError', 'params should have shape (4, 7), got (4, 6)'),
 'fit_bootstrap_dev/pred': ('ValueError', "a prediction needs the parameters it was made from and the data's shape (4, 8)"),
 'fit_bootstrap_dev/props': ('ValueError', 'props should have shape (nprop, 5), got (2, 6)'),
 'fit_bootstrap_dev/groups-missing': ('ValueError',
                                      'the residual bootstrap needs groups (the plan knows no scheme to derive them from)'),
 'fit_bootstrap_dev/groups-not-cuda': ('AssertionError', ''),
 'fit_bootstrap_dev/groups-shape': ('ValueError', 'groups should be 8 integers (one per measurement), got shape (7,)'),
 'fit_bootstrap_dev/vox-dtype': ('AssertionError', ''),
 'fit_bootstrap_dev/vox': ('ValueError', 'vox should have one entry per voxel'),
 'fit_bootstrap_dev/maxfasc+not-cuda': ('ValueError', 'maxfasc must be 0..3'),
 'fit_bootstrap_dev/not-cuda+data': ('AssertionError', ''),
 'fit_bootstrap_dev/peaks+params': ('ValueError', 'peaks should have shape (4, 6)'),
 'boot_resample_dev/B': ('ValueError', 'bootstrap B should be an integer >= 1, got 0'),
 'boot_resample_dev/maxfasc': ('ValueError', 'maxfasc must be 0..3'),
 'boot_resample_dev/not-cuda': ('AssertionError', ''),
 'boot_resample_dev/prediction': ('ValueError', "prediction should have the data's shape (4, 8), got (4, 7)"),
 'boot_resample_dev/params': ('ValueError', 'params should have shape (4, 7), got (4, 6)'),
 'boot_resample_dev/peaks': ('ValueError', 'peaks should have shape (4, 6)'),
 'boot_resample_dev/groups-missing': ('ValueError', 'the residual bootstrap needs groups'),
 'boot_resample_dev/vox': ('ValueError', 'vox should have one entry per voxel'),
 'boot_resample_dev/maxfasc+not-cuda': ('ValueError', 'maxfasc must be 0..3'),
 'boot_resample_dev/not-cuda+prediction': ('AssertionError', ''),
 'boot_reduce_dev/X': ('ValueError', 'X should have shape (voxels, replicates, columns), got (4, 4)'),
 'boot_reduce_dev/valid': ('ValueError', 'valid should have the shape of X (4, 4, 3), got (4, 4, 2)'),
 'boot_reduce_dev/q': ('ValueError', 'bootstrap q should lie in [0, 1], got (1.5,)'),
 'boot_reduce_dev/not-cuda': ('AssertionError', ''),
 'boot_reduce_dev/valid-dtype': ('AssertionError', ''),
 'boot_reduce_dev/q+valid': ('ValueError', 'bootstrap q should lie in [0, 1], got (1.5,)'),
 'cleanup_select/shapes': ('ValueError', 'cleanup_select: f1, f2 should have shape (n,), p1, p2 (n, 3)')}

EXPECTED_CALLS = {'volume_rows': [('mfx_volume_rows', ('volume', 16, 2.0, 1.0, 6, 8, ('long', 5), 3, ('double', 0.0), 2))],
 'fit_batch_volume': [('mfx_fit_batch_volume',
                       ('plan', 'volume', 16, 2.0, 1.0, 6, ('long', 5), ('int', 1), ('ubyte', 0), ('ubyte', 0),
                        ('double', 500.0), 2, 1, 1, ('double', 600.0), ('double', 700.0), 2, 4, ('double', 0.0)))],
 'fit_batch_volume/bare': [('mfx_fit_batch_volume',
                            ('plan', 'volume', 16, 2.0, 1.0, 6, ('long', 5), ('int', 0), ('ubyte', 0), ('ubyte', 0),
                             ('double', 0.0), 0, 0, 0, None, None, 0, 4, ('double', 0.0)))],
 'fit_batch': [('mfx_fit_batch_rows',
                ('plan', ('double', 100.0), None, ('int', 1), ('ubyte', 0), ('ubyte', 0), ('double', 500.0), 2, 1, 1,
                 ('double', 600.0), ('double', 700.0), 2, 4, ('double', 0.0)))],
 'fit_batch/rows': [('mfx_fit_batch_rows',
                     ('plan', ('double', 100.0), ('long', 3), ('int', 1), ('ubyte', 0), ('ubyte', 0), ('double', 500.0), 2,
                      0, 0, None, None, 0, 2, ('double', 0.0)))],
 'fit_batch/bare': [('mfx_fit_batch_rows',
                     ('plan', ('double', 100.0), None, ('int', 0), ('ubyte', 0), ('ubyte', 0), ('double', 0.0), 0, 0, 0,
                      None, None, 0, 4, ('double', 0.0)))],
 'predict': [('mfx_predict',
              ('plan', ('double', 800.0), ('double', 500.0), 2, 1, 1, ('double', 600.0), ('double', 700.0), 2, 4,
               ('double', 100.0), ('double', 1.0), 1, 3, 18446744073709551615, 5, ('double', 0.0), ('double', 0.0)))],
 'predict/bare': [('mfx_predict',
                   ('plan', ('double', 800.0), None, 0, 0, 0, None, None, 0, 4, None, None, 0, 0, 0, 0, ('double', 0.0),
                    None))],
 'sos_noise': [('mfx_sos_noise', (('double', 100.0), 32, ('double', 2.5), 0, 2, 9, 1099511627776, ('double', 0.0), 1))],
 'sos_noise/element': [('mfx_sos_noise', (('double', 100.0), 32, ('double', 200.0), 2, 1, 0, 0, ('double', 0.0), 0))],
 'profile': [('mfx_profile', ('plan', ('double', 100.0), ('double', 500.0), 1, 0, None, 2, ('double', 0.0), None)),
             ('mfx_profile', ('plan', ('double', 116.0), ('double', 512.0), 2, 0, None, 1, ('double', 0.0), None)),
             ('mfx_profile',
              ('plan', ('double', 108.0), ('double', 506.0), 2, 1, ('double', 600.0), 1, ('double', 0.0), None))],
 'profile/partner': [('mfx_profile',
                      ('plan', ('double', 100.0), ('double', 500.0), 1, 0, None, 2, ('double', 0.0), ('int', 0))),
                     ('mfx_profile',
                      ('plan', ('double', 116.0), ('double', 512.0), 2, 0, None, 1, ('double', 0.0), ('int', 0))),
                     ('mfx_profile',
                      ('plan', ('double', 108.0), ('double', 506.0), 2, 1, ('double', 600.0), 1, ('double', 0.0),
                       ('int', 0)))],
 'pair_objectives': [('mfx_pair_objectives', ('plan', ('double', 100.0), ('double', 500.0), 0, None, 4, ('double', 0.0)))],
 'pair_objectives/csf': [('mfx_pair_objectives',
                          ('plan', ('double', 100.0), ('double', 500.0), 1, ('double', 600.0), 4, ('double', 0.0)))],
 'posterior': [('mfx_post',
                ('plan', ('double', 100.0), ('double', 500.0), 1, 0, None, ('double', 2.0), ('double', 900.0), 2,
                 ('double', 0.0), ('double', 0.0), ('int', 0))),
               ('mfx_post',
                ('plan', ('double', 116.0), ('double', 512.0), 2, 0, None, ('double', 18.0), ('double', 902.0), 1,
                 ('double', 0.0), ('double', 0.0), ('int', 0))),
               ('mfx_post',
                ('plan', ('double', 108.0), ('double', 506.0), 2, 1, ('double', 600.0), ('double', 8.0), ('double', 901.0),
                 1, ('double', 0.0), ('double', 0.0), ('int', 0)))],
 'posterior/own-shift': [('mfx_fit_batch_rows',
                          ('plan', ('double', 100.0), None, ('int', 1), ('ubyte', 0), ('ubyte', 0), ('double', 500.0), 1, 0,
                           0, None, None, 0, 2, ('double', 0.0))),
                         ('mfx_post',
                          ('plan', ('double', 100.0), ('double', 500.0), 1, 0, None, ('double', 0.5), ('double', 0.0), 2,
                           ('double', 0.0), ('double', 0.0), ('int', 0))),
                         ('mfx_fit_batch_rows',
                          ('plan', ('double', 116.0), None, ('int', 2), ('ubyte', 0), ('ubyte', 0), ('double', 512.0), 2, 0,
                           0, None, None, 0, 1, ('double', 0.0))),
                         ('mfx_post',
                          ('plan', ('double', 116.0), ('double', 512.0), 2, 0, None, ('double', 0.5), ('double', 0.0), 1,
                           ('double', 0.0), ('double', 0.0), ('int', 0))),
                         ('mfx_fit_batch_rows',
                          ('plan', ('double', 108.0), None, ('int', 2), ('ubyte', 1), ('ubyte', 0), ('double', 506.0), 2, 1,
                           0, ('double', 600.0), None, 0, 1, ('double', 0.0))),
                         ('mfx_post',
                          ('plan', ('double', 108.0), ('double', 506.0), 2, 1, ('double', 600.0), ('double', 0.5),
                           ('double', 0.0), 1, ('double', 0.0), ('double', 0.0), ('int', 0)))],
 'posterior2d': [('mfx_post2d',
                  ('tables', ('double', 100.0), ('double', 500.0), 1, ('double', 2.0), ('double', 900.0), 2, ('double', 0.0),
                   ('double', 0.0), ('int', 0), ('int', 0))),
                 ('mfx_post2d',
                  ('tables', ('double', 108.0), ('double', 506.0), 2, ('double', 8.0), ('double', 901.0), 2, ('double', 0.0),
                   ('double', 0.0), ('int', 0), ('int', 0)))],
 'posterior2d/own-shift': [('mfx_fit2d_batch',
                            ('tables', ('double', 100.0), ('int', 1), None, ('double', 500.0), 1, 0, None, 2,
                             ('double', 0.0), ('int', 0))),
                           ('mfx_post2d',
                            ('tables', ('double', 100.0), ('double', 500.0), 1, ('double', 0.5), ('double', 0.0), 2,
                             ('double', 0.0), ('double', 0.0), ('int', 0), ('int', 0))),
                           ('mfx_fit2d_batch',
                            ('tables', ('double', 116.0), ('int', 2), None, ('double', 512.0), 2, 0, None, 1,
                             ('double', 0.0), ('int', 0))),
                           ('mfx_post2d',
                            ('tables', ('double', 116.0), ('double', 512.0), 2, ('double', 0.5), ('double', 0.0), 1,
                             ('double', 0.0), ('double', 0.0), ('int', 0), ('int', 0)))],
 'profile2d': [('mfx_profile2d', ('tables', ('double', 100.0), ('double', 500.0), 1, 2, ('double', 0.0), None, ('int', 0))),
               ('mfx_profile2d', ('tables', ('double', 108.0), ('double', 506.0), 2, 2, ('double', 0.0), None, ('int', 0)))],
 'profile2d/partner': [('mfx_profile2d',
                        ('tables', ('double', 100.0), ('double', 500.0), 1, 2, ('double', 0.0), ('int', 0), ('int', 0))),
                       ('mfx_profile2d',
                        ('tables', ('double', 116.0), ('double', 512.0), 2, 1, ('double', 0.0), ('int', 0), ('int', 0)))],
 'fit_robust': [('mfx_rfit_batch',
                 ('plan', ('double', 100.0), None, 0, ('int', 1), ('ubyte', 0), ('double', 500.0), 2, 1, ('double', 600.0),
                  1, 2.0, 2, 4, ('double', 0.0), ('double', 0.0), ('double', 0.0), ('int', 0), ('int', 0), ('long', 0),
                  ('int', 0))),
                ('mfx_plan_status', ('plan', None))],
 'fit2d_robust': [('mfx_rfit2d_batch',
                   ('tables', ('double', 100.0), None, 0, ('int', 1), ('ubyte', 0), ('double', 500.0), 2, 1,
                    ('double', 600.0), 2, 3.0, 0, 4, ('double', 0.0), ('double', 0.0), ('double', 0.0), ('int', 0),
                    ('int', 0), ('int', 0), ('long', 0), ('int', 0)))],
 'profile/W-VM': [('mfx_wprofile',
                   ('plan', ('double', 100.0), ('double', 200.0), 8, ('double', 500.0), 1, 0, None, 2, ('double', 0.0),
                    None)),
                  ('mfx_wprofile',
                   ('plan', ('double', 116.0), ('double', 216.0), 8, ('double', 512.0), 2, 0, None, 1, ('double', 0.0),
                    None)),
                  ('mfx_wprofile',
                   ('plan', ('double', 108.0), ('double', 208.0), 8, ('double', 506.0), 2, 1, ('double', 600.0), 1,
                    ('double', 0.0), None))],
 'profile/partner/W-VM': [('mfx_wprofile',
                           ('plan', ('double', 100.0), ('double', 200.0), 8, ('double', 500.0), 1, 0, None, 2,
                            ('double', 0.0), ('int', 0))),
                          ('mfx_wprofile',
                           ('plan', ('double', 116.0), ('double', 216.0), 8, ('double', 512.0), 2, 0, None, 1,
                            ('double', 0.0), ('int', 0))),
                          ('mfx_wprofile',
                           ('plan', ('double', 108.0), ('double', 208.0), 8, ('double', 506.0), 2, 1, ('double', 600.0), 1,
                            ('double', 0.0), ('int', 0)))],
 'pair_objectives/W-VM': [('mfx_wpair_objectives',
                           ('plan', ('double', 100.0), ('double', 200.0), 8, ('double', 500.0), 0, None, 4,
                            ('double', 0.0)))],
 'pair_objectives/csf/W-VM': [('mfx_wpair_objectives',
                               ('plan', ('double', 100.0), ('double', 200.0), 8, ('double', 500.0), 1, ('double', 600.0), 4,
                                ('double', 0.0)))],
 'posterior/W-VM': [('mfx_wpost',
                     ('plan', ('double', 100.0), ('double', 200.0), 8, ('double', 500.0), 1, 0, None, ('double', 2.0),
                      ('double', 900.0), 2, ('double', 0.0), ('double', 0.0), ('int', 0))),
                    ('mfx_wpost',
                     ('plan', ('double', 116.0), ('double', 216.0), 8, ('double', 512.0), 2, 0, None, ('double', 18.0),
                      ('double', 902.0), 1, ('double', 0.0), ('double', 0.0), ('int', 0))),
                    ('mfx_wpost',
                     ('plan', ('double', 108.0), ('double', 208.0), 8, ('double', 506.0), 2, 1, ('double', 600.0),
                      ('double', 8.0), ('double', 901.0), 1, ('double', 0.0), ('double', 0.0), ('int', 0)))],
 'posterior/own-shift/W-VM': [('mfx_wfit_batch',
                               ('plan', ('double', 100.0), ('double', 200.0), 8, ('int', 1), ('ubyte', 0), ('double', 500.0),
                                1, 0, None, 2, ('double', 0.0), ('int', 0))),
                              ('mfx_plan_status', ('plan', None)),
                              ('mfx_wpost',
                               ('plan', ('double', 100.0), ('double', 200.0), 8, ('double', 500.0), 1, 0, None,
                                ('double', 0.5), ('double', 0.0), 2, ('double', 0.0), ('double', 0.0), ('int', 0))),
                              ('mfx_wfit_batch',
                               ('plan', ('double', 116.0), ('double', 216.0), 8, ('int', 2), ('ubyte', 0), ('double', 512.0),
                                2, 0, None, 1, ('double', 0.0), ('int', 0))),
                              ('mfx_plan_status', ('plan', None)),
                              ('mfx_wpost',
                               ('plan', ('double', 116.0), ('double', 216.0), 8, ('double', 512.0), 2, 0, None,
                                ('double', 0.5), ('double', 0.0), 1, ('double', 0.0), ('double', 0.0), ('int', 0))),
                              ('mfx_wfit_batch',
                               ('plan', ('double', 108.0), ('double', 208.0), 8, ('int', 2), ('ubyte', 1), ('double', 506.0),
                                2, 1, ('double', 600.0), 1, ('double', 0.0), ('int', 0))),
                              ('mfx_plan_status', ('plan', None)),
                              ('mfx_wpost',
                               ('plan', ('double', 108.0), ('double', 208.0), 8, ('double', 506.0), 2, 1, ('double', 600.0),
                                ('double', 0.5), ('double', 0.0), 1, ('double', 0.0), ('double', 0.0), ('int', 0)))],
 'posterior2d/W-VM': [('mfx_wpost2d',
                       ('tables', ('double', 100.0), ('double', 200.0), 8, ('double', 500.0), 1, ('double', 2.0),
                        ('double', 900.0), 2, ('double', 0.0), ('double', 0.0), ('int', 0), ('int', 0))),
                      ('mfx_wpost2d',
                       ('tables', ('double', 108.0), ('double', 208.0), 8, ('double', 506.0), 2, ('double', 8.0),
                        ('double', 901.0), 2, ('double', 0.0), ('double', 0.0), ('int', 0), ('int', 0)))],
 'posterior2d/own-shift/W-VM': [('mfx_wfit2d_batch',
                                 ('tables', ('double', 100.0), ('double', 200.0), 8, ('int', 1), None, ('double', 500.0), 1,
                                  0, None, 2, ('double', 0.0), ('int', 0), ('int', 0))),
                                ('mfx_wpost2d',
                                 ('tables', ('double', 100.0), ('double', 200.0), 8, ('double', 500.0), 1, ('double', 0.5),
                                  ('double', 0.0), 2, ('double', 0.0), ('double', 0.0), ('int', 0), ('int', 0))),
                                ('mfx_wfit2d_batch',
                                 ('tables', ('double', 116.0), ('double', 216.0), 8, ('int', 2), None, ('double', 512.0), 2,
                                  0, None, 1, ('double', 0.0), ('int', 0), ('int', 0))),
                                ('mfx_wpost2d',
                                 ('tables', ('double', 116.0), ('double', 216.0), 8, ('double', 512.0), 2, ('double', 0.5),
                                  ('double', 0.0), 1, ('double', 0.0), ('double', 0.0), ('int', 0), ('int', 0)))],
 'profile2d/W-VM': [('mfx_wprofile2d',
                     ('tables', ('double', 100.0), ('double', 200.0), 8, ('double', 500.0), 1, 2, ('double', 0.0), None,
                      ('int', 0))),
                    ('mfx_wprofile2d',
                     ('tables', ('double', 108.0), ('double', 208.0), 8, ('double', 506.0), 2, 2, ('double', 0.0), None,
                      ('int', 0)))],
 'profile2d/partner/W-VM': [('mfx_wprofile2d',
                             ('tables', ('double', 100.0), ('double', 200.0), 8, ('double', 500.0), 1, 2, ('double', 0.0),
                              ('int', 0), ('int', 0))),
                            ('mfx_wprofile2d',
                             ('tables', ('double', 116.0), ('double', 216.0), 8, ('double', 512.0), 2, 1, ('double', 0.0),
                              ('int', 0), ('int', 0)))],
 'fit_robust/W-VM': [('mfx_rfit_batch',
                      ('plan', ('double', 100.0), ('double', 200.0), 8, ('int', 1), ('ubyte', 0), ('double', 500.0), 2, 1,
                       ('double', 600.0), 1, 2.0, 2, 4, ('double', 0.0), ('double', 0.0), ('double', 0.0), ('int', 0),
                       ('int', 0), ('long', 0), ('int', 0))),
                     ('mfx_plan_status', ('plan', None))],
 'fit2d_robust/W-VM': [('mfx_rfit2d_batch',
                        ('tables', ('double', 100.0), ('double', 200.0), 8, ('int', 1), ('ubyte', 0), ('double', 500.0), 2,
                         1, ('double', 600.0), 2, 3.0, 0, 4, ('double', 0.0), ('double', 0.0), ('double', 0.0), ('int', 0),
                         ('int', 0), ('int', 0), ('long', 0), ('int', 0)))],
 'fit2d_weighted/W-VM': [('mfx_wfit2d_batch',
                          ('tables', ('double', 100.0), ('double', 200.0), 8, ('int', 1), ('ubyte', 0), ('double', 500.0), 2,
                           1, ('double', 600.0), 4, ('double', 0.0), ('int', 0), ('int', 0)))],
 'fit_weighted/W-VM': [('mfx_wfit_batch',
                        ('plan', ('double', 100.0), ('double', 200.0), 8, ('int', 1), ('ubyte', 0), ('double', 500.0), 2, 1,
                         ('double', 600.0), 4, ('double', 0.0), ('int', 0))),
                       ('mfx_plan_status', ('plan', None))],
 'profile/W-M': [('mfx_wprofile',
                  ('plan', ('double', 100.0), ('double', 300.0), 0, ('double', 500.0), 1, 0, None, 2, ('double', 0.0),
                   None)),
                 ('mfx_wprofile',
                  ('plan', ('double', 116.0), ('double', 300.0), 0, ('double', 512.0), 2, 0, None, 1, ('double', 0.0),
                   None)),
                 ('mfx_wprofile',
                  ('plan', ('double', 108.0), ('double', 300.0), 0, ('double', 506.0), 2, 1, ('double', 600.0), 1,
                   ('double', 0.0), None))],
 'profile/partner/W-M': [('mfx_wprofile',
                          ('plan', ('double', 100.0), ('double', 300.0), 0, ('double', 500.0), 1, 0, None, 2,
                           ('double', 0.0), ('int', 0))),
                         ('mfx_wprofile',
                          ('plan', ('double', 116.0), ('double', 300.0), 0, ('double', 512.0), 2, 0, None, 1,
                           ('double', 0.0), ('int', 0))),
                         ('mfx_wprofile',
                          ('plan', ('double', 108.0), ('double', 300.0), 0, ('double', 506.0), 2, 1, ('double', 600.0), 1,
                           ('double', 0.0), ('int', 0)))],
 'pair_objectives/W-M': [('mfx_wpair_objectives',
                          ('plan', ('double', 100.0), ('double', 300.0), 0, ('double', 500.0), 0, None, 4,
                           ('double', 0.0)))],
 'pair_objectives/csf/W-M': [('mfx_wpair_objectives',
                              ('plan', ('double', 100.0), ('double', 300.0), 0, ('double', 500.0), 1, ('double', 600.0), 4,
                               ('double', 0.0)))],
 'posterior/W-M': [('mfx_wpost',
                    ('plan', ('double', 100.0), ('double', 300.0), 0, ('double', 500.0), 1, 0, None, ('double', 2.0),
                     ('double', 900.0), 2, ('double', 0.0), ('double', 0.0), ('int', 0))),
                   ('mfx_wpost',
                    ('plan', ('double', 116.0), ('double', 300.0), 0, ('double', 512.0), 2, 0, None, ('double', 18.0),
                     ('double', 902.0), 1, ('double', 0.0), ('double', 0.0), ('int', 0))),
                   ('mfx_wpost',
                    ('plan', ('double', 108.0), ('double', 300.0), 0, ('double', 506.0), 2, 1, ('double', 600.0),
                     ('double', 8.0), ('double', 901.0), 1, ('double', 0.0), ('double', 0.0), ('int', 0)))],
 'posterior/own-shift/W-M': [('mfx_wfit_batch',
                              ('plan', ('double', 100.0), ('double', 300.0), 0, ('int', 1), ('ubyte', 0), ('double', 500.0),
                               1, 0, None, 2, ('double', 0.0), ('int', 0))),
                             ('mfx_plan_status', ('plan', None)),
                             ('mfx_wpost',
                              ('plan', ('double', 100.0), ('double', 300.0), 0, ('double', 500.0), 1, 0, None,
                               ('double', 0.5), ('double', 0.0), 2, ('double', 0.0), ('double', 0.0), ('int', 0))),
                             ('mfx_wfit_batch',
                              ('plan', ('double', 116.0), ('double', 300.0), 0, ('int', 2), ('ubyte', 0), ('double', 512.0),
                               2, 0, None, 1, ('double', 0.0), ('int', 0))),
                             ('mfx_plan_status', ('plan', None)),
                             ('mfx_wpost',
                              ('plan', ('double', 116.0), ('double', 300.0), 0, ('double', 512.0), 2, 0, None,
                               ('double', 0.5), ('double', 0.0), 1, ('double', 0.0), ('double', 0.0), ('int', 0))),
                             ('mfx_wfit_batch',
                              ('plan', ('double', 108.0), ('double', 300.0), 0, ('int', 2), ('ubyte', 1), ('double', 506.0),
                               2, 1, ('double', 600.0), 1, ('double', 0.0), ('int', 0))),
                             ('mfx_plan_status', ('plan', None)),
                             ('mfx_wpost',
                              ('plan', ('double', 108.0), ('double', 300.0), 0, ('double', 506.0), 2, 1, ('double', 600.0),
                               ('double', 0.5), ('double', 0.0), 1, ('double', 0.0), ('double', 0.0), ('int', 0)))],
 'posterior2d/W-M': [('mfx_wpost2d',
                      ('tables', ('double', 100.0), ('double', 300.0), 0, ('double', 500.0), 1, ('double', 2.0),
                       ('double', 900.0), 2, ('double', 0.0), ('double', 0.0), ('int', 0), ('int', 0))),
                     ('mfx_wpost2d',
                      ('tables', ('double', 108.0), ('double', 300.0), 0, ('double', 506.0), 2, ('double', 8.0),
                       ('double', 901.0), 2, ('double', 0.0), ('double', 0.0), ('int', 0), ('int', 0)))],
 'posterior2d/own-shift/W-M': [('mfx_wfit2d_batch',
                                ('tables', ('double', 100.0), ('double', 300.0), 0, ('int', 1), None, ('double', 500.0), 1,
                                 0, None, 2, ('double', 0.0), ('int', 0), ('int', 0))),
                               ('mfx_wpost2d',
                                ('tables', ('double', 100.0), ('double', 300.0), 0, ('double', 500.0), 1, ('double', 0.5),
                                 ('double', 0.0), 2, ('double', 0.0), ('double', 0.0), ('int', 0), ('int', 0))),
                               ('mfx_wfit2d_batch',
                                ('tables', ('double', 116.0), ('double', 300.0), 0, ('int', 2), None, ('double', 512.0), 2,
                                 0, None, 1, ('double', 0.0), ('int', 0), ('int', 0))),
                               ('mfx_wpost2d',
                                ('tables', ('double', 116.0), ('double', 300.0), 0, ('double', 512.0), 2, ('double', 0.5),
                                 ('double', 0.0), 1, ('double', 0.0), ('double', 0.0), ('int', 0), ('int', 0)))],
 'profile2d/W-M': [('mfx_wprofile2d',
                    ('tables', ('double', 100.0), ('double', 300.0), 0, ('double', 500.0), 1, 2, ('double', 0.0), None,
                     ('int', 0))),
                   ('mfx_wprofile2d',
                    ('tables', ('double', 108.0), ('double', 300.0), 0, ('double', 506.0), 2, 2, ('double', 0.0), None,
                     ('int', 0)))],
 'profile2d/partner/W-M': [('mfx_wprofile2d',
                            ('tables', ('double', 100.0), ('double', 300.0), 0, ('double', 500.0), 1, 2, ('double', 0.0),
                             ('int', 0), ('int', 0))),
                           ('mfx_wprofile2d',
                            ('tables', ('double', 116.0), ('double', 300.0), 0, ('double', 512.0), 2, 1, ('double', 0.0),
                             ('int', 0), ('int', 0)))],
 'fit_robust/W-M': [('mfx_rfit_batch',
                     ('plan', ('double', 100.0), ('double', 300.0), 0, ('int', 1), ('ubyte', 0), ('double', 500.0), 2, 1,
                      ('double', 600.0), 1, 2.0, 2, 4, ('double', 0.0), ('double', 0.0), ('double', 0.0), ('int', 0),
                      ('int', 0), ('long', 0), ('int', 0))),
                    ('mfx_plan_status', ('plan', None))],
 'fit2d_robust/W-M': [('mfx_rfit2d_batch',
                       ('tables', ('double', 100.0), ('double', 300.0), 0, ('int', 1), ('ubyte', 0), ('double', 500.0), 2, 1,
                        ('double', 600.0), 2, 3.0, 0, 4, ('double', 0.0), ('double', 0.0), ('double', 0.0), ('int', 0),
                        ('int', 0), ('int', 0), ('long', 0), ('int', 0)))],
 'fit2d_weighted/W-M': [('mfx_wfit2d_batch',
                         ('tables', ('double', 100.0), ('double', 300.0), 0, ('int', 1), ('ubyte', 0), ('double', 500.0), 2,
                          1, ('double', 600.0), 4, ('double', 0.0), ('int', 0), ('int', 0)))],
 'fit_weighted/W-M': [('mfx_wfit_batch',
                       ('plan', ('double', 100.0), ('double', 300.0), 0, ('int', 1), ('ubyte', 0), ('double', 500.0), 2, 1,
                        ('double', 600.0), 4, ('double', 0.0), ('int', 0))),
                      ('mfx_plan_status', ('plan', None))],
 'fit2d': [('mfx_fit2d_batch',
            ('tables', ('double', 100.0), ('int', 1), ('ubyte', 0), ('double', 500.0), 2, 1, ('double', 600.0), 4,
             ('double', 0.0), ('int', 0)))],
 'fit2d/bare': [('mfx_fit2d_batch',
                 ('tables', ('double', 100.0), ('int', 0), None, None, 0, 0, None, 4, ('double', 0.0), ('int', 0)))],
 'fit2d_weighted/bare': [('mfx_wfit2d_batch',
                          ('tables', ('double', 100.0), ('double', 300.0), 0, ('int', 0), None, None, 0, 0, None, 4,
                           ('double', 0.0), ('int', 0), ('int', 0)))],
 'fit_weighted/bare': [('mfx_wfit_batch',
                        ('plan', ('double', 100.0), ('double', 300.0), 0, ('int', 0), None, None, 0, 0, None, 4,
                         ('double', 0.0), ('int', 0))),
                       ('mfx_plan_status', ('plan', None))],
 'fit_robust/bare': [('mfx_rfit_batch',
                      ('plan', ('double', 100.0), None, 0, ('int', 0), None, None, 0, 0, None, 0, 4.45, 0, 4,
                       ('double', 0.0), ('double', 0.0), ('double', 0.0), ('int', 0), ('int', 0), ('long', 0), ('int', 0))),
                     ('mfx_plan_status', ('plan', None))],
 'fit2d_robust/bare': [('mfx_rfit2d_batch',
                        ('tables', ('double', 100.0), None, 0, ('int', 0), None, None, 0, 0, None, 0, 4.45, 3, 4,
                         ('double', 0.0), ('double', 0.0), ('double', 0.0), ('int', 0), ('int', 0), ('int', 0), ('long', 0),
                         ('int', 0)))],
 'predict2d': [('mfx_predict2d',
                ('tables', ('double', 800.0), ('double', 500.0), 2, 1, ('double', 600.0), 4, ('double', 100.0),
                 ('double', 1.0), 1, 3, 18446744073709551615, 5, ('double', 0.0), ('double', 0.0), ('int', 0)))],
 'predict2d/bare': [('mfx_predict2d',
                     ('tables', ('double', 800.0), None, 0, 0, None, 4, None, None, 0, 0, 0, 0, ('double', 0.0), None,
                      ('int', 0)))],
 'fit_bootstrap': [('mfx_boot_fit',
                    ('plan', ('double', 100.0), ('int', 1), ('ubyte', 0), ('ubyte', 0), ('double', 500.0), 2, 1, 1,
                     ('double', 600.0), ('double', 700.0), 2, ('double', 800.0), ('int', 7), ('long', 40), 4, 4, 1, 0,
                     18446744073709551613, 11, ('double', 1000.0), 2, ('double', 0.1), 2, 1048576, ('double', 0.0),
                     ('int', 0), ('int', 0), ('double', 0.0))),
                   ('mfx_plan_status', ('plan', None))],
 'fit_bootstrap/bare': [('mfx_boot_fit',
                         ('plan', ('double', 100.0), ('int', 0), None, None, None, 0, 0, 0, None, None, 0, None, None, None,
                          4, 3, 0, 1, 0, 0, None, 0, None, 0, 268435456, ('double', 0.0), None, ('int', 0), None)),
                        ('mfx_plan_status', ('plan', None))],
 'fit_bootstrap/flags-unused': [('mfx_boot_fit',
                                 ('plan', ('double', 100.0), ('int', 2), None, None, ('double', 500.0), 2, 0, 0, None, None,
                                  2, None, None, None, 4, 2, 0, 1, 0, 0, None, 0, ('double', 0.025), 2, 268435456,
                                  ('double', 0.0), ('int', 0), ('int', 0), None)),
                                ('mfx_plan_status', ('plan', None))],
 'cleanup_select': [('mfx_cleanup_2fascicles',
                     (('double', 100.0), ('double', 200.0), ('double', 400.0), ('double', 500.0), 4, 0.9, 2.0, 0.25, 0.125,
                      ('double', 0.0), ('double', 0.0), 3))]}

"""examples/TriangulationLOSTExample.cpp re-hosted: 500 random cameras looking at one landmark, 1000 noisy trials
triangulated by LOST, DLT and DLT followed by the nonlinear refinement; prints the covariance of each estimator's error
and the time per trial.  Here the trials of one estimator are ONE batched call (a track per trial) on the device.

usage: python examples/TriangulationLOSTExample.py [--trials N] [--cameras N] [--seed S]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gtsam_petercdev_amd as gt  # noqa: E402


def PrintCovarianceStats(mat, method):
    centered = mat - mat.mean(axis=0)
    cov = centered.T @ centered / (mat.shape[0] - 1)
    print(f"{method} covariance: ")
    print(cov)
    print(f"Trace sqrt: {np.sqrt(np.trace(cov))}\n")


def PrintDuration(seconds, num_samples, method):
    print(f"Time taken by {method}: {seconds / num_samples * 1e6}")


def GetLargeCamerasDataset(rng, nrCameras=500):
    point = np.array([0.0, 0.0, 10.0])
    poses = [gt.Pose3(gt.Rot3(), np.array([rng.uniform(-10, 10), rng.uniform(-10, 10), rng.uniform(-20, 0)]))
             for _ in range(nrCameras)]
    cameras = [gt.PinholeCameraCal3_S2(p, gt.Cal3_S2()) for p in poses]
    return cameras, poses, point, np.array([c.project(point) for c in cameras])


def dataset(trials, n_cameras, seed, measurementSigma=1e-2):
    rng = np.random.default_rng(seed)
    cameras, poses, landmark, measurements = GetLargeCamerasDataset(rng, n_cameras)
    noisy = measurements[None, :, :] + rng.normal(scale=measurementSigma, size=(trials,) + measurements.shape)
    return cameras, poses, landmark, noisy


def estimate(cameras, noisy, rank_tol, optimize, model, useLOST):
    """triangulatePoint3<Cal3_S2>(cameras, noisyMeasurements, rank_tol, optimize, model, useLOST) for every trial at once"""
    t0 = time.perf_counter()
    pts, status = gt.triangulatePoint3Batch(cameras, noisy, rank_tol, optimize, model, useLOST)
    dt = time.perf_counter() - t0
    failed = int(np.count_nonzero(status != gt.TriangulationResult.VALID))
    if failed:
        raise RuntimeError(f"{failed} trials failed to triangulate")
    return pts, dt


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=1000)
    ap.add_argument("--cameras", type=int, default=500)
    ap.add_argument("--seed", type=int, default=42)
    a = ap.parse_args(argv)
    measurementSigma = 1e-2
    cameras, poses, landmark, noisy = dataset(a.trials, a.cameras, a.seed, measurementSigma)
    measurementNoise = gt.noiseModel.Isotropic.Sigma(2, measurementSigma)
    rank_tol = 1e-9
    estimateLOST, durationLOST = estimate(cameras, noisy, rank_tol, False, measurementNoise, True)
    estimateDLT, durationDLT = estimate(cameras, noisy, rank_tol, False, measurementNoise, False)
    estimateDLTOpt, durationDLTOpt = estimate(cameras, noisy, rank_tol, True, measurementNoise, False)
    PrintCovarianceStats(estimateLOST - landmark, "LOST")
    PrintCovarianceStats(estimateDLT - landmark, "DLT")
    PrintCovarianceStats(estimateDLTOpt - landmark, "DLT_OPT")
    PrintDuration(durationLOST, a.trials, "LOST")
    PrintDuration(durationDLT, a.trials, "DLT")
    PrintDuration(durationDLTOpt, a.trials, "DLT_OPT")
    return estimateLOST, estimateDLT, estimateDLTOpt


if __name__ == "__main__":
    main()

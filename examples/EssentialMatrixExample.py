#!/usr/bin/env python3
"""The two-view minimisations of the reference's gtsam/slam/tests/testEssentialMatrixFactor.cpp on the MI355X backend.

    python examples/EssentialMatrixExample.py

1. Five-point (:607-646 on 5pointExample2.txt): one EssentialMatrix, five EssentialMatrixFactor built from pixel
   measurements with the calibration f = 500, Isotropic sigma 0.01, from trueE.retract((0.1, -0.1, 0.1, 0.1, -0.1)).
2. Depth (:229-261, on every track of 18pointExample1.txt): one EssentialMatrix and an inverse depth per track under
   EssentialMatrixFactor2 with unit noise, E from the same perturbation and the depths from baseline / z.
Both by Levenberg-Marquardt with the reference's default parameters."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gtsam_petercdev_amd import datasets  # noqa: E402
from gtsam_petercdev_amd.graph import (Cal3_S2, EssentialMatrix, EssentialMatrixFactor, EssentialMatrixFactor2,  # noqa: E402
                                       LevenbergMarquardtOptimizer, LevenbergMarquardtParams, NonlinearFactorGraph, Pose3, Rot3,
                                       Values, noiseModel)

DATA = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
PERTURBATION = np.array([0.1, -0.1, 0.1, 0.1, -0.1])


def two_views(name):
    """(trueE, pA, pB, points): camera 1's pose in the frame of camera 0 as an EssentialMatrix, each track's measurement in
    the two cameras, and the points."""
    sfm = datasets.read_bal(os.path.join(DATA, name))
    assert sfm.numberCameras() == 2
    pose = Pose3.from_state(sfm.cameras[1][:12])
    n = sfm.numberTracks()
    pA, pB = np.zeros((n, 2)), np.zeros((n, 2))
    for c, j, uv in zip(sfm.cam_idx, sfm.pt_idx, sfm.uv):
        (pA if c == 0 else pB)[j] = uv
    return EssentialMatrix.FromPose3(pose), pA, pB, sfm.points


def five_point():
    trueE, pA, pB, _ = two_views("5pointExample2.txt")
    K = Cal3_S2(500.0, 500.0, 0.0, 0.0, 0.0)
    model = noiseModel.Isotropic.Sigma(1, 0.01)
    graph, initial = NonlinearFactorGraph(), Values()
    for i in range(5):
        graph.add(EssentialMatrixFactor(1, pA[i], pB[i], model, K))
    initial.insert(1, trueE.retract(PERTURBATION))
    return graph, initial, trueE


def depth():
    trueE, pA, pB, points = two_views("18pointExample1.txt")
    model = noiseModel.Unit.Create(2)
    graph, initial = NonlinearFactorGraph(), Values()
    for i in range(len(points)):
        graph.add(EssentialMatrixFactor2(100, i, pA[i], pB[i], model))
        initial.insert(i, np.array([0.1 / points[i][2]]))     # baseline / z
    initial.insert(100, trueE.retract(PERTURBATION))
    return graph, initial, trueE, 0.1 / points[:, 2]


def report(title, key, graph, initial, trueE):
    optimizer = LevenbergMarquardtOptimizer(graph, initial, LevenbergMarquardtParams())
    before = optimizer.error()
    result = optimizer.optimize()
    E = result.at(key)
    print(title)
    print(f"  initial error {before:.6g}, final error {optimizer.error():.3e}")
    print("  direction: " + " ".join(f"{x:.6f}" for x in E.direction().point3()))
    print(f"  distance to the true E: {float(np.max(np.abs(E.state() - trueE.state()))):.3e}")
    return result


def main():
    graph, initial, trueE = five_point()
    report("Five-point minimisation (5pointExample2.txt):", 1, graph, initial, trueE)
    graph, initial, trueE, depths = depth()
    result = report("Depth minimisation (18pointExample1.txt):", 100, graph, initial, trueE)
    worst = max(abs(float(result.at(i)[0]) - depths[i]) for i in range(len(depths)))
    print(f"  largest inverse-depth error: {worst:.3e}")


if __name__ == "__main__":
    main()

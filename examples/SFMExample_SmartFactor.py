"""examples/SFMExample_SmartFactor.cpp re-hosted: structure from motion with one SmartProjectionPose3Factor per landmark —
no landmark variables; each factor triangulates its point at every linearization and hands the optimizer a factor on the
camera poses alone.  The data is the reference's (examples/SFMdata.h): 8 points on a cube seen from 8 poses on a circle,
which is exactly the backend's limit of 8 views per smart factor.

usage: python examples/SFMExample_SmartFactor.py"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gtsam_petercdev_amd as gt  # noqa: E402


def createPoints():
    return [np.array(p, float) for p in ((10, 10, 10), (-10, 10, 10), (-10, -10, 10), (10, -10, 10), (10, 10, -10),
                                         (-10, 10, -10), (-10, -10, -10), (10, -10, -10))]


def createPoses(steps=8):
    init = gt.Pose3(gt.Rot3.Ypr(math.pi / 2, 0, -math.pi / 2), [30, 0, 0])
    delta = gt.Pose3(gt.Rot3.Ypr(0, -math.pi / 4, 0), [math.sin(math.pi / 4) * 30, 0, 30 * (1 - math.sin(math.pi / 4))])
    poses = [init]
    for _ in range(1, steps):
        poses.append(poses[-1].compose(delta))
    return poses


def project(pose, K, point):
    q = pose.transformTo(point)
    k = K.vector()
    u, v = q[0] / q[2], q[1] / q[2]
    return gt.Point2(k[0] * u + k[2] * v + k[3], k[1] * v + k[4])


def main():
    K = gt.Cal3_S2(50.0, 50.0, 0.0, 50.0, 50.0)
    measurementNoise = gt.noiseModel.Isotropic.Sigma(2, 1.0)   # one pixel in u and v
    points, poses = createPoints(), createPoses()

    # The reference's program runs with the default IGNORE_DEGENERACY; the backend takes ZERO_ON_DEGENERACY only, so it is
    # set explicitly.  The two modes differ only for a track without a valid triangulation, and no track degenerates on
    # this data.
    params = gt.SmartProjectionParams()
    params.setDegeneracyMode(gt.ZERO_ON_DEGENERACY)

    graph = gt.NonlinearFactorGraph()
    for j, point in enumerate(points):
        smartfactor = gt.SmartProjectionPose3Factor(measurementNoise, K, None, params)
        for i, pose in enumerate(poses):
            smartfactor.add(project(pose, K, point), i)
        graph.push_back(smartfactor)

    # priors on x0 and x1: 0.1 rad on roll, pitch, yaw, 30 cm on x, y, z; the second fixes the scale
    noise = gt.noiseModel.Diagonal.Sigmas(np.array([0.1, 0.1, 0.1, 0.3, 0.3, 0.3]))
    graph.addPrior(0, poses[0], noise)
    graph.addPrior(1, poses[1], noise)
    print(f"Factor Graph:\nsize: {graph.size()}\n")

    initialEstimate = gt.Values()
    delta = gt.Pose3(gt.Rot3.Rodrigues(-0.1, 0.2, 0.25), [0.05, -0.10, 0.20])
    for i, pose in enumerate(poses):
        initialEstimate.insert(i, pose.compose(delta))
    print(f"Initial Estimates:\nValues with {initialEstimate.size()} values\n")

    optimizer = gt.LevenbergMarquardtOptimizer(graph, initialEstimate)
    result = optimizer.optimize()
    print("Final results:")
    for k in result.keys():
        p = result.at(k)
        print(f"Value {k}: (gtsam::Pose3)\nR: {np.array2string(p.rotation().matrix(), precision=6)}\nt: {p.translation()}\n")

    # the landmarks are not variables: they come out of the factors (SmartProjectionFactor::point)
    print("Landmark results:")
    for j in range(len(points)):
        point = graph.factors[j].point()
        if point.valid():
            print(f"Value {j}: (Eigen::Matrix<double, 3, 1>) {np.array2string(point.get(), precision=6)}")
    print(f"final error: {optimizer.error()}")
    print(f"number of iterations: {optimizer.iterations()}")


if __name__ == "__main__":
    main()

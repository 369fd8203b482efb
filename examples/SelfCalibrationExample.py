#!/usr/bin/env python3
"""examples/SelfCalibrationExample.cpp of the reference on the MI355X backend: same graph, same start, same optimizer,
same print.

    python examples/SelfCalibrationExample.py

Structure from motion with the calibration as a variable: eight cameras on a circle of radius 30 look at the eight
corners of a cube (examples/SFMdata.h), every camera sees every corner through GeneralSFMFactor2<Cal3_S2> — the factor
with three keys (pose, landmark, the one shared calibration K0) — with priors on the first pose, the first landmark and K.
The measurements are exact for K = (50, 50, 0, 50, 50); the start has K = (60, 60, 0, 45, 45) and every pose and landmark
displaced.  DoglegOptimizer, as there."""
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gtsam_petercdev_amd.graph import (Cal3_S2, DoglegOptimizer, GeneralSFMFactor2, NonlinearFactorGraph, Point3,  # noqa: E402
                                       Pose3, Rot3, Values, noiseModel, symbol)
from StereoVOExample import print_values as print_poses_and_points  # noqa: E402


def create_points():
    """createPoints (examples/SFMdata.h): the corners of a cube of side 20."""
    return [Point3(x, y, z) for z in (10.0, -10.0) for x, y in ((10.0, 10.0), (-10.0, 10.0), (-10.0, -10.0), (10.0, -10.0))]


def create_poses(steps=8):
    """createPoses (examples/SFMdata.h): a circular trajectory of radius 30 at pi/4 intervals, always facing the centre."""
    poses = [Pose3(Rot3.Ypr(math.pi / 2, 0, -math.pi / 2), [30.0, 0.0, 0.0])]
    delta = Pose3(Rot3.Ypr(0, -math.pi / 4, 0), [math.sin(math.pi / 4) * 30, 0.0, 30 * (1 - math.sin(math.pi / 4))])
    for _ in range(1, steps):
        poses.append(poses[-1].compose(delta))
    return poses


def project(pose, K, point):
    """PinholeCamera<Cal3_S2>(pose, K).project(point): the simulated measurement (host-side set-up only)."""
    q = pose.transformTo(point)
    x, y = q[0] / q[2], q[1] / q[2]
    fx, fy, s, u0, v0 = K.vector()
    return [fx * x + s * y + u0, fy * y + v0]


def build():
    points, poses = create_points(), create_poses()
    graph = NonlinearFactorGraph()
    # Add a prior on pose x0: 30cm std on x,y,z 0.1 rad on roll,pitch,yaw
    graph.addPrior(symbol("x", 0), poses[0], noiseModel.Diagonal.Sigmas([0.1] * 3 + [0.3] * 3))
    # Simulated measurements from each camera pose, through the factor that also differentiates by the calibration
    K = Cal3_S2(50.0, 50.0, 0.0, 50.0, 50.0)
    measurement_noise = noiseModel.Isotropic.Sigma(2, 1.0)
    for i, pose in enumerate(poses):
        for j, point in enumerate(points):
            graph.add(GeneralSFMFactor2(project(pose, K, point), measurement_noise, symbol("x", i), symbol("l", j),
                                        symbol("K", 0)))
    # Add a prior on the position of the first landmark, and one on the calibration
    graph.addPrior(symbol("l", 0), points[0], noiseModel.Isotropic.Sigma(3, 0.1))
    graph.addPrior(symbol("K", 0), K, noiseModel.Diagonal.Sigmas([500, 500, 0.1, 100, 100]))
    # Create the initial estimate to the solution, now including an estimate on the camera calibration parameters
    initial = Values()
    initial.insert(symbol("K", 0), Cal3_S2(60.0, 60.0, 0.0, 45.0, 45.0))
    for i, pose in enumerate(poses):
        initial.insert(symbol("x", i), pose.compose(Pose3(Rot3.Rodrigues(-0.1, 0.2, 0.25), Point3(0.05, -0.10, 0.20))))
    for j, point in enumerate(points):
        initial.insert(symbol("l", j), point + Point3(-0.25, 0.20, 0.15))
    return graph, initial


def print_values(result, title):
    """Values::print, the calibration as Cal3_S2::print writes its matrix."""
    print(title, end="")
    print(f"Values with {result.size()} values:")
    rest = Values()
    for k in result.keys():
        v = result.at(k)
        if chr(k >> 56) == "K":
            fx, fy, s, u0, v0 = v
            print(f"Value K{k & ((1 << 56) - 1)}: (gtsam::Cal3_S2)")
            print(f"Cal3_S2[\n\t{fx:.6g}, {s:.6g}, {u0:.6g};\n\t0, {fy:.6g}, {v0:.6g};\n\t0, 0, 1\n]\n")
        else:
            rest.insert(k, v)
    import contextlib
    import io
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        print_poses_and_points(rest, "")
    print(buf.getvalue().split("\n", 1)[1], end="")   # (without the second header line)


def main(argv):
    graph, initial = build()
    # Optimize the graph and print results
    optimizer = DoglegOptimizer(graph, initial)
    result = optimizer.optimize()
    print_values(result, "Final results:\n")
    return optimizer, result


if __name__ == "__main__":
    main(sys.argv)

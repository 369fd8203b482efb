#!/usr/bin/env python3
"""examples/StereoVOExample.cpp of the reference on the MI355X backend: same graph, same steps, same print.

    python examples/StereoVOExample.py

A 3D stereo visual odometry example: the robot starts at the origin, moves forward 1 meter and takes stereo readings on
three landmarks from both poses.  The reference fixes the first pose with NonlinearEquality<Pose3>; here it is a
PriorFactor with noiseModel.Constrained.All(6) — six hard-constraint rows, eliminated exactly."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gtsam_petercdev_amd.graph import (Cal3_S2Stereo, GenericStereoFactor, LevenbergMarquardtOptimizer,  # noqa: E402
                                       NonlinearFactorGraph, Point3, Pose3, PriorFactor, Rot3, StereoPoint2, Values,
                                       noiseModel)


def print_values(result, title):
    """Values::print: a Pose3 as its rotation rows and translation, a Point3 as a vector."""
    print(title, end="")
    print(f"Values with {result.size()} values:")
    for k in result.keys():
        v = result.at(k)
        name = chr(k >> 56) + str(k & ((1 << 56) - 1)) if k >> 56 else str(k)
        if isinstance(v, Pose3):
            R, t = v.rotation().matrix(), v.translation()
            print(f"Value {name}: (gtsam::Pose3)")
            print("R: [\n" + ";\n".join("\t" + ", ".join(f"{x:.6g}" for x in row) for row in R) + "\n]")
            print("t: " + " ".join(f"{x:.6g}" for x in t) + "\n")
        else:
            print(f"Value {name}: (Eigen::Matrix<double, 3, 1>)")
            print("[\n" + ";\n".join(f"\t{x:.6g}" for x in v) + "\n]\n")


def build():
    # create graph object, add first pose at origin with key '1'
    graph = NonlinearFactorGraph()
    first_pose = Pose3()
    graph.add(PriorFactor(1, first_pose, noiseModel.Constrained.All(6)))
    # create factor noise model with 3 sigmas of value 1
    model = noiseModel.Isotropic.Sigma(3, 1)
    # create stereo camera calibration object with .2m between cameras
    K = Cal3_S2Stereo(1000, 1000, 0, 320, 240, 0.2)
    # create and add stereo factors between first pose (key value 1) and the three landmarks
    graph.add(GenericStereoFactor(StereoPoint2(520, 480, 440), model, 1, 3, K))
    graph.add(GenericStereoFactor(StereoPoint2(120, 80, 440), model, 1, 4, K))
    graph.add(GenericStereoFactor(StereoPoint2(320, 280, 140), model, 1, 5, K))
    # create and add stereo factors between second pose and the three landmarks
    graph.add(GenericStereoFactor(StereoPoint2(570, 520, 490), model, 2, 3, K))
    graph.add(GenericStereoFactor(StereoPoint2(70, 20, 490), model, 2, 4, K))
    graph.add(GenericStereoFactor(StereoPoint2(320, 270, 115), model, 2, 5, K))
    # create and add initial estimates of camera poses and landmark locations
    initial_estimate = Values()
    initial_estimate.insert(1, first_pose)
    initial_estimate.insert(2, Pose3(Rot3(), Point3(0.1, -0.1, 1.1)))
    initial_estimate.insert(3, Point3(1, 1, 5))
    initial_estimate.insert(4, Point3(-1, 1, 5))
    initial_estimate.insert(5, Point3(0, -0.5, 5))
    return graph, initial_estimate


def main(argv):
    graph, initial_estimate = build()
    # create Levenberg-Marquardt optimizer for resulting factor graph, optimize
    optimizer = LevenbergMarquardtOptimizer(graph, initial_estimate)
    result = optimizer.optimize()
    print_values(result, "Final result:\n")
    return optimizer, result


if __name__ == "__main__":
    main(sys.argv)

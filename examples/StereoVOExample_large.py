#!/usr/bin/env python3
"""examples/StereoVOExample_large.cpp of the reference on the MI355X backend: same data, same steps, same prints.

    python examples/StereoVOExample_large.py

A 3D stereo visual odometry example: the robot starts at the origin and moves forward, taking periodic stereo readings
of many landmarks (VO_calibration.txt, VO_camera_poses_large.txt and the gzip-compressed VO_stereo_factors_large.txt.gz
under tests/golden: 26 poses, 8 189 stereo factors).  The reference fixes the first pose with NonlinearEquality<Pose3>; here it is a PriorFactor
with noiseModel.Constrained.All(6), the hard-constraint path.  params.orderingType = METIS is kept: the
mirror maps it to the library's own nested dissection (GSX_ORDER_ND)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from gtsam_petercdev_amd.graph import (L, X, Cal3_S2Stereo, GenericStereoFactor, LevenbergMarquardtOptimizer,  # noqa: E402
                                       LevenbergMarquardtParams, NonlinearFactorGraph, Pose3, PriorFactor, Rot3,
                                       StereoPoint2, Values, noiseModel)
from StereoVOExample import print_values  # noqa: E402

DATA = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")


def build(data_dir=DATA, first_pose_model=None, verbose=True):
    """The graph and the initial estimate of the example; first_pose_model replaces the hard constraint on x1."""
    say = print if verbose else (lambda *a: None)
    initial_estimate = Values()
    graph = NonlinearFactorGraph()
    model = noiseModel.Isotropic.Sigma(3, 1)
    # read camera calibration info from file: focal lengths fx, fy, skew s, principal point u0, v0, baseline b
    say("Reading calibration info")
    fx, fy, s, u0, v0, b = np.loadtxt(os.path.join(data_dir, "VO_calibration.txt")).reshape(-1)[:6]
    K = Cal3_S2Stereo(fx, fy, s, u0, v0, b)
    # read camera pose parameters and use to make initial estimates of camera poses
    say("Reading camera poses")
    for row in np.loadtxt(os.path.join(data_dir, "VO_camera_poses_large.txt")).reshape(-1, 17):
        m = row[1:].reshape(4, 4)
        initial_estimate.insert(X(int(row[0])), Pose3(Rot3(m[:3, :3]), m[:3, 3]))
    # pixel coordinates uL, uR, v (same for left/right images due to rectification), landmark coordinates X, Y, Z in
    # camera frame, resulting from triangulation
    say("Reading stereo factors")
    for x, l, uL, uR, v, Xc, Yc, Zc in np.loadtxt(os.path.join(data_dir, "VO_stereo_factors_large.txt.gz")).reshape(-1, 8):
        x, l = int(x), int(l)
        graph.add(GenericStereoFactor(StereoPoint2(uL, uR, v), model, X(x), L(l), K))
        # if the landmark of this factor has no initial estimate yet, add it: the triangulated point, moved from the
        # camera pose space to the global space
        if not initial_estimate.exists(L(l)):
            initial_estimate.insert(L(l), initial_estimate.at(X(x)).transformFrom([Xc, Yc, Zc]))
    first_pose = initial_estimate.at(X(1))
    # constrain the first pose such that it cannot change from its original value during optimization
    graph.add(PriorFactor(X(1), first_pose, first_pose_model if first_pose_model is not None
                          else noiseModel.Constrained.All(6)))
    return graph, initial_estimate


def main(argv):
    graph, initial_estimate = build()
    print("Optimizing")
    # create Levenberg-Marquardt optimizer to optimize the factor graph
    params = LevenbergMarquardtParams()
    params.orderingType = "METIS"
    optimizer = LevenbergMarquardtOptimizer(graph, initial_estimate, params)
    result = optimizer.optimize()
    print(f"initial error={optimizer.result['initial_error']:.6g}")
    print(f"final error={optimizer.result['final_error']:.6g}")
    print("Final result sample:")
    pose_values = Values()
    for k in result.keys():
        if isinstance(result.at(k), Pose3):
            pose_values.insert(k, result.at(k))
    print_values(pose_values, "Final camera poses:\n")
    return optimizer, result


if __name__ == "__main__":
    main(sys.argv)

#!/usr/bin/env python3
"""python/gtsam/examples/GPSFactorExample.py of the reference on the MI355X backend: same graph, same prints.

    python examples/GPSFactorExample.py

Simple robot motion example with a prior and one GPS measurement: one Pose3, a prior at the origin and a GPSFactor whose
"fix" is the ENU origin of the reference's flight data (latitude, longitude, height, used as plain numbers as there),
optimized by Levenberg-Marquardt."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gtsam_petercdev_amd.graph import (GPSFactor, LevenbergMarquardtOptimizer, LevenbergMarquardtParams,  # noqa: E402
                                       NonlinearFactorGraph, Point3, Pose3, PriorFactorPose3, Values, noiseModel)

# ENU origin: where the plane was in hold next to the runway
lat0 = 33.86998
lon0 = -84.30626
h0 = 274

GPS_SIGMA, PRIOR_SIGMA = 0.1, 0.25


def eigen_row(v):
    """A row vector as Eigen's stream operator writes it: every entry at six significant digits, padded to the widest."""
    cells = [f"{x:.6g}" for x in v]
    width = max(len(c) for c in cells)
    return " ".join(c.rjust(width) for c in cells)


def print_pose(pose):
    R, t = pose.rotation().matrix(), pose.translation()
    print("R: [\n" + ";\n".join("\t" + ", ".join(f"{x:.6g}" for x in row) for row in R) + "\n]")
    print("t: " + " ".join(f"{x:.6g}" for x in t))


def print_graph(title, prior_mean, gps):
    """NonlinearFactorGraph::print with PriorFactor::print and GPSFactor::print."""
    print(title)
    print("NonlinearFactorGraph: size: 2\n")
    print("Factor 0: PriorFactor on 1")
    print("  prior mean: ", end="")
    print_pose(prior_mean)
    print(f"isotropic dim=6 sigma={PRIOR_SIGMA:g}\n")
    print("Factor 1: GPSFactor on 1")
    print("  GPS measurement: " + eigen_row(gps))
    print(f"  noise model: isotropic dim=3 sigma={GPS_SIGMA:g}\n\n")


def print_values(title, values):
    print(title)
    print(f"Values with {values.size()} values:")
    for k in values.keys():
        print(f"Value {k}: (gtsam::Pose3)")
        print_pose(values.atPose3(k))
        print()
    print()


def build():
    graph = NonlinearFactorGraph()
    # a prior on the first pose, setting it to the origin
    graph.add(PriorFactorPose3(1, Pose3(), noiseModel.Isotropic.Sigma(6, PRIOR_SIGMA)))
    # the GPS factor
    graph.add(GPSFactor(1, Point3(lat0, lon0, h0), noiseModel.Isotropic.Sigma(3, GPS_SIGMA)))
    # the initial estimate, deliberately wrong
    initial = Values()
    initial.insert(1, Pose3())
    return graph, initial


def main():
    graph, initial = build()
    print_graph("\nFactor Graph:", Pose3(), Point3(lat0, lon0, h0))
    print_values("\nInitial Estimate:", initial)
    optimizer = LevenbergMarquardtOptimizer(graph, initial, LevenbergMarquardtParams())
    result = optimizer.optimize()
    print_values("\nFinal Result:", result)
    return result


if __name__ == "__main__":
    main()

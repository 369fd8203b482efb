#!/usr/bin/env python3
"""examples/Pose2SLAMExample_lago.cpp of the reference on the MI355X backend.

    python examples/Pose2SLAMExample_lago.py [g2oFile] [outputFile]

readG2o (2-D; diagonal information matrices become Diagonal models, as the reference's smart constructors make them), a
prior Diagonal::Variances(1e-6, 1e-6, 1e-8) at Pose2() on key 0, the graph printed, lago::initialize, then the estimate is
printed or, with an output file, written by writeG2o with the factors of the file."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gtsam_petercdev_amd import _abi as A, _lib  # noqa: E402

DATA = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")


def _g(x, digits):
    return f"{float(x):.{digits}g}"


def print_graph(arr):
    """NonlinearFactorGraph::print (NonlinearFactorGraph.cpp:55-68) for between and prior factors on Pose2.  The stream
    precision is 6 until a vector is printed, which leaves it at 9 (gtsam/base/Vector.cpp:80-88)."""
    digits = 6
    print(f"size: {arr.n_factors}\n")
    for f in range(arr.n_factors):
        keys = [int(arr.var_keys[v]) for v in arr.f_vars[arr.f_key_ptr[f]:arr.f_key_ptr[f + 1]]]
        z = arr.meas[arr.f_meas_ptr[f]:arr.f_meas_ptr[f + 1]]
        nz = arr.noise[arr.f_noise_ptr[f]:arr.f_noise_ptr[f + 1]]
        pose = "(" + ", ".join(_g(x, digits) for x in z) + ")"
        if arr.f_type[f] == A.F_BETWEEN:
            print(f"Factor {f}: BetweenFactor({keys[0]},{keys[1]})\n  measured:  {pose}")
        else:
            print(f"Factor {f}: PriorFactor on {keys[0]}\n  prior mean:  {pose}")
        kind = int(arr.f_noise_kind[f])
        if kind == A.NOISE_UNIT:
            print(f"  noise model: unit ({int(arr.f_rows[f])}) ")
        elif kind == A.NOISE_ISOTROPIC:
            print(f"isotropic dim={int(arr.f_rows[f])} sigma={_g(nz[0], digits)}")
        elif kind == A.NOISE_DIAGONAL:
            digits = 9
            print("  noise model: diagonal sigmas [" + "; ".join(_g(x, digits) for x in nz) + "];")
        else:
            print("  noise model: (full)")
        print()
    return digits


def main(argv):
    g2o_file = argv[1] if len(argv) > 1 else os.path.join(DATA, "noisyToyGraph.txt")
    graph = _lib.load2d(g2o_file, noise_format=A.NOISE_FORMAT_G2O)     # readG2o: no prior, smart noise models
    # Add prior on the pose having index (key) = 0
    var0 = int(np.searchsorted(graph.var_keys, np.uint64(0)))
    if var0 >= graph.n_vars or int(graph.var_keys[var0]) != 0:
        raise SystemExit("the graph has no pose with key 0")
    with_prior = graph.with_factor(A.F_PRIOR, [var0], 3, [0.0, 0.0, 0.0], A.NOISE_DIAGONAL, np.sqrt([1e-6, 1e-6, 1e-8]))
    digits = print_graph(with_prior)
    print("Computing LAGO estimate")
    estimate = _lib.lago_initialize(with_prior, True, with_prior.values)
    print("done!")
    if len(argv) < 3:
        so = with_prior.state_offsets()
        print("estimateLago\nValues with %d values:" % with_prior.n_vars)
        for i, k in enumerate(with_prior.var_keys):
            s = estimate[so[i]:so[i + 1]]
            print(f"Value {int(k)}: (gtsam::Pose2)\n(" + ", ".join(_g(x, digits) for x in s) + ")\n")
    else:
        print(f"Writing results to file: {argv[2]}")
        _lib.write_g2o(argv[2], graph, estimate)
        print("done! ")
    return estimate


if __name__ == "__main__":
    main(sys.argv)

#!/usr/bin/env python3
"""examples/Pose3SLAMExample_initializePose3Gradient.cpp of the reference on the MI355X backend.

    python examples/Pose3SLAMExample_initializePose3Gradient.py [g2oFile] [outputFile]

readG2o (3-D), prior Diagonal::Variances(1e-6 x3, 1e-4 x3) at Pose3() on the first pose, InitializePose3::initialize
(Riemannian gradient iterations on the rotations from the file's values, one Gauss-Newton iteration
for the poses), then the initialized values are printed or, with an output file, written by writeG2o."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gtsam_petercdev_amd import _lib  # noqa: E402

DATA = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")


def main(argv):
    g2o_file = argv[1] if len(argv) > 1 else os.path.join(DATA, "pose3example.txt")
    arr = _lib.read_g2o(g2o_file, is3D=True)          # (the reader appends the example's prior on the first pose)
    print("Adding prior to g2o file ")
    print("Initializing Pose3 - Riemannian gradient")
    p = _lib.init_pose3_params_default()
    p.use_gradient = 1
    initialization, _ = _lib.initialize_pose3(arr, arr.values, p)
    print("done!")
    be = _lib.ProductBackend(arr)
    print(f"initial error={be.error():.6g}")
    be.set_values(initialization)
    print(f"initialization error={be.error():.6g}")
    be.close()
    if len(argv) < 3:
        print("initialization")
        so = arr.state_offsets()
        for i, k in enumerate(arr.var_keys):
            s = initialization[so[i]:so[i + 1]]
            print(f"Value {int(k)}: (gtsam::Pose3)")
            for row in s[:9].reshape(3, 3):
                print("R: " + " ".join(repr(float(x)) for x in row))
            print("t: " + " ".join(repr(float(x)) for x in s[9:12]))
    else:
        print(f"Writing results to file: {argv[2]}")
        _lib.write_g2o(argv[2], arr, initialization)
        print("done! ")
    return initialization


if __name__ == "__main__":
    main(sys.argv)

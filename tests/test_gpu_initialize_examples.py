"""The two InitializePose3 example programs run as programs (examples/Pose3SLAMExample_initializePose3Chordal.py and
...Gradient.py) and give the poses of tests/_init_pose3_restatement.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from gtsam_petercdev_amd import _lib
from tests import _init_pose3_restatement as IR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(name, *args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", name)] + list(args), capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout


@pytest.fixture(scope="module")
def example_arrays(golden_dir):
    return _lib.read_g2o(os.path.join(golden_dir, "pose3example.txt"), is3D=True)


def test_chordal_example_writes_the_restatements_poses(example_arrays, golden_dir, tmp_path):
    out_file = tmp_path / "chordal.g2o"
    stdout = _run("Pose3SLAMExample_initializePose3Chordal.py", os.path.join(golden_dir, "pose3example.txt"), str(out_file))
    assert "Initializing Pose3 - chordal relaxation" in stdout and "Writing results to file" in stdout
    back = _lib.read_g2o(str(out_file), is3D=True)
    ref = IR.initialize(example_arrays)
    assert np.array_equal(back.var_keys, example_arrays.var_keys)
    assert np.abs(back.values - ref).max() < 1e-6


def test_gradient_example_prints_the_restatements_poses(example_arrays, golden_dir):
    stdout = _run("Pose3SLAMExample_initializePose3Gradient.py", os.path.join(golden_dir, "pose3example.txt"))
    assert "Initializing Pose3 - Riemannian gradient" in stdout and "initialization error=" in stdout
    ref = IR.initialize(example_arrays, example_arrays.values, use_gradient=True)
    ts = np.array([[float(x) for x in line[2:].split()] for line in stdout.splitlines() if line.startswith("t: ")])
    so = example_arrays.state_offsets()
    assert ts.shape == (example_arrays.n_vars, 3)
    for i in range(example_arrays.n_vars):
        assert np.abs(ts[i] - ref[so[i] + 9:so[i] + 12]).max() < 1e-6
    Rs = np.array([[float(x) for x in line[2:].split()] for line in stdout.splitlines() if line.startswith("R: ")])
    assert np.abs(Rs.reshape(-1, 9) - np.stack([ref[so[i]:so[i] + 9] for i in range(example_arrays.n_vars)])).max() < 1e-6


def test_chordal_example_on_sphere2500_lowers_the_error(golden_dir, tmp_path):
    """error(initialized values) < error(values of the file reader) on the full graph.  The float64 restatement shows the
    inequality on the CPU (sparse normal equations of the decoupled 7 503-unknown system and of the 15 006-unknown
    Gauss-Newton step): 1.228e7 for the reader's odometry-chained values, 4.727e3 after the initialization."""
    src = os.path.join(golden_dir, "sphere2500.txt")
    out_file = tmp_path / "sphere.g2o"
    _run("Pose3SLAMExample_initializePose3Chordal.py", src, str(out_file))
    arr = _lib.read_g2o(src, is3D=True)
    back = _lib.read_g2o(str(out_file), is3D=True)
    assert back.n_vars == 2500 and np.array_equal(back.var_keys, arr.var_keys) and np.all(np.isfinite(back.values))
    be = _lib.ProductBackend(arr)
    e_reader = be.error()
    be.set_values(back.values)
    e_init = be.error()
    be.close()
    print(f"sphere2500: error {e_reader:.6g} -> {e_init:.6g}")
    assert e_init < e_reader

"""Translation averaging (1dSfM): camera positions from pairwise translation directions, the steps and prints of the
reference's python/gtsam/examples/TranslationAveragingExample.py on this package: 8 cameras on a circle, directions to the
next two cameras in the camera frame, rotation into the world frame, the MFAS outlier filter over up to 48 sampled projection
directions (one batched launch), TranslationRecovery.  As in the reference's example the last camera is measured from one
camera only: its direction from that camera is recovered, its distance is not determined by the data."""
import argparse
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gtsam_petercdev_amd import graph as gtsam  # noqa: E402

MAX_1DSFM_PROJECTION_DIRECTIONS = 48
OUTLIER_WEIGHT_THRESHOLD = 0.1


def create_poses(n=8, radius=30.0, height=10.0):
    """Cameras on a circle that look at its centre (the layout of the reference's SFMdata.createPoses)."""
    poses = []
    for i in range(n):
        theta = 2 * math.pi * i / n
        position = np.array([radius * math.cos(theta), radius * math.sin(theta), height])
        z = -position / np.linalg.norm(position)                 # optical axis: towards the origin
        x = np.cross(np.array([0.0, 0.0, 1.0]), z)
        x /= np.linalg.norm(x)
        y = np.cross(z, x)
        poses.append(gtsam.Pose3(gtsam.Rot3(np.column_stack([x, y, z])), position))
    return poses


def get_data():
    """Global rotations, and the unit translation directions from camera i to the next two cameras in the frame of camera i."""
    wTc_list = create_poses()
    wRc_values, i_iZj_list = {}, []
    for i in range(len(wTc_list) - 2):
        wRi = wTc_list[i].rotation()
        wRc_values[i] = wRi
        for j in range(i + 1, i + 3):
            w_itj = wTc_list[j].translation() - wTc_list[i].translation()
            i_itj = wRi.matrix().T @ w_itj
            i_iZj_list.append(gtsam.BinaryMeasurementUnit3(i, j, gtsam.Unit3(i_itj), gtsam.noiseModel.Isotropic.Sigma(3, 0.01)))
    for i in (len(wTc_list) - 1, len(wTc_list) - 2):
        wRc_values[i] = wTc_list[i].rotation()
    return wRc_values, i_iZj_list


def filter_outliers(w_iZj_list, rng):
    """Removes the measurements whose mean MFAS outlier weight over the sampled projection directions reaches the threshold."""
    num_directions_to_sample = min(MAX_1DSFM_PROJECTION_DIRECTIONS, len(w_iZj_list))
    sampled_indices = rng.choice(len(w_iZj_list), num_directions_to_sample, replace=False)
    projection_directions = [w_iZj_list[idx].measured() for idx in sampled_indices]
    avg_outlier_weights = gtsam.MFAS.outlierWeightsBatch(w_iZj_list, projection_directions)["mean"]
    return [m for m, w in zip(w_iZj_list, avg_outlier_weights) if w < OUTLIER_WEIGHT_THRESHOLD]


def estimate_poses(i_iZj_list, wRc_values, rng):
    w_iZj_list = []
    for i_iZj in i_iZj_list:
        w_iZj = gtsam.Unit3(wRc_values[i_iZj.key1()].matrix() @ i_iZj.measured().point3())
        w_iZj_list.append(gtsam.BinaryMeasurementUnit3(i_iZj.key1(), i_iZj.key2(), w_iZj, i_iZj.noiseModel()))
    w_iZj_inliers = filter_outliers(w_iZj_list, rng)
    wtc_values = gtsam.TranslationRecovery().run(w_iZj_inliers)
    return {key: gtsam.Pose3(wRc_values[key], wtc_values.at(key)) for key in sorted(wRc_values)}, len(w_iZj_inliers)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=0, help="seed of the sampling of the projection directions")
    args = ap.parse_args()
    wRc_values, i_iZj_list = get_data()
    wTc_values, n_inliers = estimate_poses(i_iZj_list, wRc_values, np.random.default_rng(args.seed))
    print(f"{n_inliers} of {len(i_iZj_list)} measurements kept")
    print("**** Translation averaging output ****")
    print(f"Values with {len(wTc_values)} values:")
    for key, pose in wTc_values.items():
        t = pose.translation()
        print(f"Value {key}: (gtsam::Pose3)")
        print(f"t: {t[0]:.9g} {t[1]:.9g} {t[2]:.9g}")
    print("**************************************")


if __name__ == "__main__":
    main()

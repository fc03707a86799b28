#!/usr/bin/env python
"""Golden vectors for the camera paths of smpl_nerf_amd.create_dataset from the reference itself (camera.py:113-206:
get_sphere_poses, get_circle_poses, get_circle_on_sphere_poses - numpy and scipy only).

    SNERF_REFERENCE=/path/to/reference python tests/golden/make_golden_camera.py

writes tests/golden/g25_camera_paths.npz: the poses and angles of a 3 x 3 sphere, a circle of 5 and a circle on the sphere of 7
around an off-centre point, float64.  Nothing of the reference is copied: the file holds arrays and the call arguments only."""
import contextlib
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden as MG          # noqa: E402  (MG.REF: where the reference lies)

CONFIG = dict(sphere=dict(start_angle=-90, end_angle=90, number_steps=3, r=2.4),
              circle=dict(start_angle=-60, end_angle=45, number_steps=5, r=2.4),
              circle_on_sphere=dict(number_steps=7, circle_radius=10.0, sphere_radius=2.4, center_theta=25.0, center_phi=-15.0))


def main():
    sys.path.insert(0, MG.REF)
    import camera
    out = {"config": json.dumps(CONFIG)}
    with contextlib.redirect_stdout(io.StringIO()):            # (the reference prints its step size)
        for name, fn in (("sphere", camera.get_sphere_poses), ("circle", camera.get_circle_poses),
                         ("circle_on_sphere", camera.get_circle_on_sphere_poses)):
            poses, angles = fn(**CONFIG[name])
            out[name + "_poses"], out[name + "_angles"] = np.asarray(poses, np.float64), np.asarray(angles, np.float64)
    np.savez(os.path.join(HERE, "g25_camera_paths.npz"), **out)
    print({k: np.shape(v) for k, v in out.items()})


if __name__ == "__main__":
    main()

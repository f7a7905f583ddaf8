"""ros_adapters.map_to_odom_transform: the map -> odom transform a localisation node publishes, composed with
the odometry pose, gives back the matched pose; equal poses give the identity."""
import math

import numpy as np
import pytest

from flow_field_based_motion_planner_amd import ros_adapters as A


def _row(x, y, yaw):
    return np.array([x, y, math.cos(yaw), math.sin(yaw)], np.float32)


def _apply(tf, row):
    """The transform (translation + quaternion) applied to a pose row, float64."""
    t, q = tf["transform"]["translation"], tf["transform"]["rotation"]
    yaw = A.quaternion_to_yaw(q["x"], q["y"], q["z"], q["w"])
    c, s = math.cos(yaw), math.sin(yaw)
    x, y, pc, psn = (float(v) for v in row)
    return np.array([c * x - s * y + t["x"], s * x + c * y + t["y"], c * pc - s * psn, s * pc + c * psn])


@pytest.mark.parametrize("odom,matched", [((0.5, -1.0, 0.3), (0.55, -0.9, 0.35)), ((2.0, 1.0, 3.1), (1.9, 1.2, -3.1)),
                                          ((-1.5, 0.2, -2.0), (-1.5, 0.2, -1.0)), ((0.0, 0.0, 0.0), (0.3, 0.4, math.pi / 2))])
def test_composed_with_the_odometry_it_gives_the_matched_pose(odom, matched):
    o, m = _row(*odom), _row(*matched)
    tf = A.map_to_odom_transform(o, m, 12.25)
    assert set(tf) == {"header", "child_frame_id", "transform"}
    assert tf["header"]["frame_id"] == "map" and tf["child_frame_id"] == "odom"
    assert tf["header"]["stamp"] == {"secs": 12, "nsecs": 250000000}
    assert np.abs(_apply(tf, o) - m.astype(np.float64)).max() < 1e-6
    q = tf["transform"]["rotation"]
    yaw = A.quaternion_to_yaw(q["x"], q["y"], q["z"], q["w"])
    assert -math.pi < yaw <= math.pi and tf["transform"]["translation"]["z"] == 0.0
    assert (q["x"], q["y"], q["z"], q["w"]) == A.yaw_to_quaternion(A._wrap_pi(math.atan2(float(m[3]), float(m[2])) - math.atan2(float(o[3]), float(o[2]))))


def test_identity_and_refusals():
    o = _row(1.25, -0.5, 0.7)
    tf = A.map_to_odom_transform(o, o.copy(), 3.0)
    assert tf["transform"]["translation"] == {"x": 0.0, "y": 0.0, "z": 0.0}
    assert tf["transform"]["rotation"] == {"x": 0.0, "y": 0.0, "z": 0.0, "w": 1.0}
    with pytest.raises(ValueError):
        A.map_to_odom_transform(o[:3], o, 0.0)

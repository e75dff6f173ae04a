"""Cameras of the lens-distortion tests (test_track_distortion_abi.py, test_gpu_track_distortion.py): the three distorted
configurations the reference ships (configs/TUM1.yaml, TUM2.yaml, EuRoC.yaml: intrinsics, (k1, k2, p1, p2, k3), image size) and the
KITTI intrinsics at 1241 x 376 with a synthetic k1 = +0.3 - the one camera under which keypoints leave the 64 x 48 grid."""
import numpy as np

F32 = np.float32


def _cam(w, h, K4, dist5):
    return dict(w=w, h=h, K4=np.array(K4, F32), dist=np.array(dist5, F32))


CAMERAS = {
    "TUM1": _cam(640, 480, [517.306408, 516.469215, 318.643040, 255.313989], [0.262383, -0.953104, -0.005358, 0.002628, 1.163314]),
    "TUM2": _cam(640, 480, [520.908620, 521.007327, 325.141442, 249.701764], [0.231222, -0.784899, -0.003257, -0.000105, 0.917205]),
    "EuRoC": _cam(752, 480, [458.654, 457.296, 367.215, 248.375], [-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0]),
    "KITTI_k1": _cam(1241, 376, [718.856, 718.856, 607.1928, 185.2157], [0.3, 0.0, 0.0, 0.0, 0.0]),
}


def oracle_bounds(oracle, cam):
    """Frame::ComputeImageBounds (src/Frame.cc:357-385) from the oracle's undistortion of the four corners, paired as :374-377 pair them"""
    w, h = F32(cam["w"]), F32(cam["h"])
    if cam["dist"][0] == 0:
        return np.array([0, w, 0, h], F32)
    c = oracle.undistort_keypoints(np.array([[0, 0], [w, 0], [0, h], [w, h]], F32), cam["K4"], cam["dist"])
    return np.array([min(c[0, 0], c[2, 0]), max(c[1, 0], c[3, 0]), min(c[0, 1], c[1, 1]), max(c[2, 1], c[3, 1])], F32)


def outside_grid(oracle, kps4, bounds):
    """True where Frame::PosInGrid (src/Frame.cc:309-320) is false: the keypoints the oracle's AssignFeaturesToGrid put into no cell"""
    _, idx = oracle.assign_features_to_grid(kps4, bounds)
    out = np.ones(len(kps4), bool)
    out[idx] = False
    return out

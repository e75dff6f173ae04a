"""GPU parity of orbt_relocalization_refine (csrc/orb_relocrefine.inc; reference src/Tracking.cc:1056-1126) - Relocalization's
refinement behind a PnP pose for every candidate of a round in one call on the resident frame - against
  (a) tests/nprelocrefine.py on the CPU oracle: the literal restatement, the narrow search literally inside the `ip` loop: stage, every
      count, narrow_passes <= N_, the slots, the outlier flags and first_match identical, the pose within 1e-7 (the bar
      tests/test_gpu_track*.py use against the oracle's composition);
  (b) the chain of the per-call host entries it replaces (ba_pose_optimization + orbm_search_by_projection, nprelocrefine.ChainBackend):
      the same results bit for bit, the pose included;
and at its seams: 1 and 8 candidates with the match first, in the middle and nowhere; a keyframe without features; no slot filled;
exactly 2 and 3 correspondences; the periodic-texture frame at 1241 x 376; the same texture at 320 x 240 (windows with more acceptable
candidates than the short lists hold) with the candidate-list regrow path on a fresh thread; a point id at two keyframe features; lens distortion; output buffers left
alone behind n_candidates x n_kp entries; two calls in a row; no resident frame / the wrong extractor."""
import threading

import numpy as np
import pytest

from tests import nprelocrefine as R
from tests import relocrefinecases as RC

pytestmark = pytest.mark.gpu
F32 = np.float32
EINVAL = -1
_expected = {}


def _extractor(n=1000):
    from ceres_mono_orb_slam2_amd import ORBextractor
    return ORBextractor(n, 1.2, 8, 20, 7)


def _make_resident(ex, F):
    """the frame on the device for this thread: an extracting Tracking call without last-frame features"""
    from ceres_mono_orb_slam2_amd import tracking
    z = np.zeros
    got = tracking.track_with_motion_model(ex, F["img"], F["K4"], F["bounds"], np.eye(4), z((0, 3)), z((0, 32), np.uint8), z(0, np.int32), z(0, F32), z(0, np.uint8))
    assert len(got["kps"]) == len(F["kps4"]) and np.array_equal(got["desc"], F["desc"])
    return got


def _refine(ex, F, cands, **kw):
    from ceres_mono_orb_slam2_amd import tracking
    return tracking.relocalization_refine(ex, F["K4"], F["bounds"], cands, F["log_scale"], n_kp=len(F["kps4"]), **kw)


def _want(oracle, F, key, cand, flag, check_ori=True):
    """the literal restatement's result, computed once per (case, flag)"""
    k = (key, flag, check_ori)
    if k not in _expected:
        _expected[k] = R.refine(oracle, F, cand, check_ori, flag)
    return _expected[k]


def _same(got, want, n_kp, exact_pose=False, what=""):
    for key in ("stage", "matched", "n_good", "n_additional", "n_correspondences"):
        assert got[key] == want[key], (what, key, got[key], want[key])
    assert got["narrow_passes"] <= n_kp and (got["narrow_passes"] > 0) == (want["narrow_passes"] > 0), (what, got["narrow_passes"])
    assert np.array_equal(got["slot_kf"], want["slot_kf"]), what
    assert np.array_equal(got["outlier"], want["outlier"]), what
    if exact_pose:
        assert np.array_equal(got["pose7"], want["pose7"]), (what, got["pose7"], want["pose7"])
    else:
        assert np.abs(got["pose7"] - want["pose7"]).max() < 1e-7, (what, got["pose7"], want["pose7"])


def _cases(oracle):
    return {name: RC.candidate(oracle, **kw) for name, kw in RC.CASES.items()}


@pytest.mark.parametrize("flag", [True, False])
def test_every_case_vs_literal_restatement(oracle, flag):
    _, F, _, _ = RC.two_frames(oracle)
    C = _cases(oracle)
    ex = _extractor()
    _make_resident(ex, F)
    got = _refine(ex, F, list(C.values()), narrow_in_loop=flag)
    want = [_want(oracle, F, name, c, flag) for name, c in C.items()]
    for name, g, w in zip(C, got["results"], want):
        print("%-22s flag %d: %-12s nGood %s nadditional %s correspondences %s, %d passes (literal loop %d)" %
              (name, flag, R.STAGE_NAMES[g["stage"]], g["n_good"], g["n_additional"], g["n_correspondences"], g["narrow_passes"], w["narrow_passes"]))
        _same(g, w, len(F["kps4"]), what=name)
    assert got["first_match"] == next(i for i, w in enumerate(want) if w["matched"])
    stages = set(g["stage"] for g in got["results"])
    assert stages >= ({R.NO_POSE, R.FEW_INLIERS, R.MATCH_FIRST, R.MATCH_SECOND, R.FAIL_WIDE, R.FAIL_SECOND} | ({R.FAIL_NARROW} if flag else {R.MATCH_THIRD, R.FAIL_THIRD}))
    # the orientation check off: the same gates, no histogram
    sub = ["fail_wide", "match_second", "narrow"]
    got = _refine(ex, F, [C[k] for k in sub], narrow_in_loop=flag, check_ori=False)
    for name, g in zip(sub, got["results"]):
        _same(g, _want(oracle, F, name, C[name], flag, False), len(F["kps4"]), what=name + " without orientation check")


@pytest.mark.parametrize("flag", [True, False])
def test_every_case_vs_chain_of_host_entries_bit_for_bit(oracle, flag):
    _, F, _, _ = RC.two_frames(oracle)
    C = _cases(oracle)
    ex = _extractor()
    _make_resident(ex, F)
    got = _refine(ex, F, list(C.values()), narrow_in_loop=flag)
    chain = R.ChainBackend()
    want = R.refine_round(chain, F, list(C.values()), True, flag, early_exit=True)
    print("flag %d: the chain made %d host round trips for %d candidates" % (flag, chain.calls, len(C)))
    for name, g, w in zip(C, got["results"], want["results"]):
        _same(g, w, len(F["kps4"]), exact_pose=True, what=name)
    assert got["first_match"] == want["first_match"]


def test_candidate_counts_and_where_the_match_is(oracle):
    _, F, _, _ = RC.two_frames(oracle)
    C = _cases(oracle)
    C["empty_keyframe"] = RC.empty_keyframe_candidate(oracle)
    C["empty_slots"] = RC.empty_slots_candidate(oracle)
    ex = _extractor()
    _make_resident(ex, F)
    fails = ["fail_wide", "few_inliers", "no_pose", "empty_keyframe", "fail_second", "narrow", "empty_slots", "two_correspondences"]
    rounds = {"one, matched": (["match_second"], 0), "one, not matched": (["narrow"], -1), "one without features": (["empty_keyframe"], -1),
              "one without slots": (["empty_slots"], -1), "eight, first": (["match_first"] + fails[:7], 0),
              "eight, middle": (fails[:4] + ["match_second"] + fails[4:6] + ["match_first"], 4), "eight, none": (fails, -1)}
    for what, (names, first) in rounds.items():
        got = _refine(ex, F, [C[k] for k in names])
        assert got["first_match"] == first, what
        for name, g in zip(names, got["results"]):
            _same(g, _want(oracle, F, name, C[name], True), len(F["kps4"]), what="%s: %s" % (what, name))
    for name in ("empty_keyframe", "empty_slots"):
        w = _want(oracle, F, name, C[name], True)
        assert w["stage"] == R.NO_POSE and w["n_correspondences"] == [0, -1, -1] and (w["slot_kf"] == -1).all()
    assert _want(oracle, F, "two_correspondences", C["two_correspondences"], True)["n_correspondences"][0] == 2
    assert _want(oracle, F, "three_correspondences", C["three_correspondences"], True)["n_correspondences"][0] == 3
    # a point id at two keyframe features: the second feature is skipped once the first one's point is found
    c = C["match_second"]
    ids, cnt = np.unique(c["pt"][c["pt"] >= 0], return_counts=True)
    assert (cnt == 2).sum() == 3
    # two calls in a row on one thread; output buffers that are larger than n_candidates x n_kp stay as they were behind it
    names = ["narrow", "match_second", "fail_wide"]
    n_kp = len(F["kps4"])
    slot = np.full(3 * n_kp + 64, 0x5A5A5A5A, np.int32); outl = np.full(3 * n_kp + 64, 0x5A, np.uint8)
    a = _refine(ex, F, [C[k] for k in names])
    b = _refine(ex, F, [C[k] for k in names], out=(slot, outl))
    for name, x, y in zip(names, a["results"], b["results"]):
        _same(y, x, n_kp, exact_pose=True, what="second call: " + name)
    assert (slot[3 * n_kp:] == 0x5A5A5A5A).all() and (outl[3 * n_kp:] == 0x5A).all() and a["first_match"] == b["first_match"] == 1


def _full_list_entries(F, cand, T, th, dmax):
    """What k_trk_windows adds up in its list counter for one search: over the keyframe points that are projected (a point, inside the
    image and the distance range) with more than 16 in-window, in-level candidates at a Hamming distance <= dmax, the number of their
    in-window, in-level candidates (window: |dx| < r and |dy| < r in float32)."""
    kf = dict(Xw=cand["Xw"], min_dist=cand["min_dist"], max_dist=cand["max_dist"])
    uv, rad, lvl, ok = R.project(F, kf, T, th)
    kp = F["kps4"]
    x, y, oc = kp[:, 0], kp[:, 1], kp[:, 2].astype(np.int32)
    total = 0
    for q in np.nonzero(ok & (cand["pt"] >= 0))[0]:
        j = np.nonzero((oc >= lvl[q] - 1) & (oc <= lvl[q] + 1) & (np.abs(x - uv[q, 0]) < rad[q]) & (np.abs(y - uv[q, 1]) < rad[q]))[0]
        if (RC._POP[F["desc"][j] ^ cand["desc"][q]].sum(1) <= dmax).sum() > 16:
            total += len(j)
    return total


def test_periodic_texture_frame(oracle):
    """The periodic frame at 1241 x 376: a point's window holds bit-identical look-alikes, so the first-minimum rule and chains of
    contested features decide the wide search.  (Its windows of 10 scale pixels hold at most a handful of features of three levels: the
    short candidate lists suffice here, the full lists are the next test's.)"""
    F, c = RC.periodic(oracle)
    n_kp = len(F["kps4"])
    assert n_kp > 500
    ex = _extractor(2000)
    _make_resident(ex, F)
    for flag in (True, False):
        w = R.refine(oracle, F, c, True, flag)
        g = _refine(ex, F, [c], narrow_in_loop=flag)["results"][0]
        print("periodic frame, flag %d: %d keypoints, %s nGood %s nadditional %s" % (flag, n_kp, R.STAGE_NAMES[g["stage"]], g["n_good"], g["n_additional"]))
        _same(g, w, n_kp, what="periodic")
        assert w["n_additional"][0] > 500


def test_full_window_lists_regrow_on_a_fresh_thread(oracle):
    """The same texture at 320 x 240 with 3500 features asked for: points of the wide search have more than 16 acceptable candidates, so
    k_trk_windows writes full lists - counted here from the oracle's data before anything runs - and the call, which reserves nothing for
    them on a thread that has not seen such a frame, takes the regrow path and runs twice; the next call there has room.  All equal the
    restatement, and the regrown call equals the warm one bit for bit."""
    F, c = RC.dense_periodic(oracle)
    n_kp = len(F["kps4"])
    trace = {}
    want = [R.refine(oracle, F, c, True, flag, trace=trace) for flag in (True, False)]
    entries = _full_list_entries(F, c, trace["T_wide"], 10.0, 100)
    print("dense periodic frame: %d keypoints, wide search: %d full-list entries; stages %s / %s" %
          (n_kp, entries, R.STAGE_NAMES[want[0]["stage"]], R.STAGE_NAMES[want[1]["stage"]]))
    assert entries > 0
    ex = _extractor(3500)
    got = []

    def fresh_thread():
        try:
            _make_resident(ex, F)
            for flag in (True, False, True):
                got.append(_refine(ex, F, [c], narrow_in_loop=flag))
        except BaseException as e:
            got.append(e)
    t = threading.Thread(target=fresh_thread); t.start(); t.join()
    for g in got:
        if isinstance(g, BaseException):
            raise g
    for g, w in zip(got, (want[0], want[1], want[0])):
        _same(g["results"][0], w, n_kp, what="dense periodic")
    _same(got[2]["results"][0], got[0]["results"][0], n_kp, exact_pose=True, what="dense periodic, regrown against warm")


def test_under_lens_distortion(oracle):
    """orbt_set_distortion: the resident frame's records and grid are the undistorted keypoints, the bounds the undistorted corners'."""
    from ceres_mono_orb_slam2_amd import tracking
    from tests.trackdist_cases import CAMERAS, oracle_bounds
    cam = CAMERAS["TUM1"]
    KF, F0, pairs, T = RC.two_frames(oracle)
    kp = F0["kps4"]
    und = oracle.undistort_keypoints(np.ascontiguousarray(kp[:, :2], F32), cam["K4"], cam["dist"])
    F = dict(F0, kps4=np.concatenate([und, kp[:, 2:]], 1).astype(F32), K4=cam["K4"], bounds=oracle_bounds(oracle, cam))
    ex = _extractor()
    tracking.set_distortion(ex, cam["dist"])
    try:
        got = _make_resident(ex, F)
        assert np.array_equal(got["kps_undistorted"], F["kps4"][:, :2])
        C = _cases(oracle)
        names = ["match_second", "narrow", "fail_wide", "match_first"]
        res = _refine(ex, F, [C[k] for k in names])
        for name, g in zip(names, res["results"]):
            w = R.refine(oracle, F, C[name], True, True)
            print("TUM1 %-14s %-12s nGood %s nadditional %s" % (name, R.STAGE_NAMES[g["stage"]], g["n_good"], g["n_additional"]))
            _same(g, w, len(kp), what="distorted " + name)
        # coefficients changed behind the resident frame: refused
        tracking.set_distortion(ex, None)
        with pytest.raises(Exception, match="orbt_set_distortion changed"):
            _refine(ex, F, [C["fail_wide"]])
    finally:
        tracking.set_distortion(ex, None)


def test_errors(oracle):
    from ceres_mono_orb_slam2_amd import _lib
    _, F, _, _ = RC.two_frames(oracle)
    c = RC.candidate(oracle, **RC.CASES["fail_wide"])
    ex = _extractor()
    seen = []

    def fresh_thread():                                                         # a thread without a resident frame
        try:
            _refine(ex, F, [c])
        except _lib.OrbHipError as e:
            seen.append(str(e))
    t = threading.Thread(target=fresh_thread); t.start(); t.join()
    assert len(seen) == 1 and "code -1" in seen[0] and "no frame resident" in seen[0]
    _make_resident(ex, F)
    other = _extractor()
    with pytest.raises(_lib.OrbHipError, match="not the extractor that produced the resident frame"):
        _refine(other, F, [c])
    bad = dict(c, slot_kf=c["slot_kf"][:-1])
    with pytest.raises(_lib.OrbHipError, match="n_kp differs"):
        from ceres_mono_orb_slam2_amd import tracking
        tracking.relocalization_refine(ex, F["K4"], F["bounds"], [bad], F["log_scale"])
    assert _refine(ex, F, [c])["results"][0]["stage"] == R.FAIL_WIDE              # the frame is still there

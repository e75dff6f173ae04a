"""CPU checks of the batched MapPoint update (orbl_update_map_points, include/orbslam_hip.h): the numpy restatement
tests/npmappoint.py on hand-worked cases of src/MapPoint.cc:256-315 / :335-378, the C ABI's argument checks (they fail before any
device work) and the exported symbols."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import npmappoint as npm  # noqa: E402


def _desc(bits):
    """32-byte descriptor with the given bit positions set"""
    b = np.zeros(256, np.uint8)
    b[list(bits)] = 1
    return np.packbits(b)


def _pick(descs, good=None):
    return npm.distinctive_descriptor(np.stack(descs), np.ones(len(descs), bool) if good is None else np.asarray(good, bool))


def test_n1_picks_the_only_descriptor():
    assert _pick([_desc([3, 9])]) == 0


def test_n2_always_picks_index_0():
    rng = np.random.default_rng(1)
    for _ in range(20):
        a, b = rng.integers(0, 256, (2, 32), dtype=np.uint8)
        assert _pick([a, b]) == 0                                  # both rows {0, d}: median sorted[0] = 0, a tie


def test_n3_picks_the_smallest_nearer_neighbour_distance():
    a = _desc([])                       # d(a, b) = 10, d(a, c) = 8, d(b, c) = 2
    b = _desc(range(10))
    c = _desc(range(8))
    # medians (sorted[1]): a -> 8, b -> 2, c -> 2: the first of the tie is b
    assert _pick([a, b, c]) == 1
    assert _pick([a, c, b]) == 1
    assert _pick([b, a, c]) == 0
    d = _desc(range(20, 40))            # far from everything: a 3-set {a, c, d} - c's nearer neighbour is a (8), a's is c (8)
    assert _pick([d, c, a]) == 1


def test_n4_median_is_the_second_smallest_of_the_row():
    a = _desc([]); b = _desc(range(5)); c = _desc(range(100, 103)); d = _desc(range(100, 104))
    # rows (own zero included), sorted[1]: a -> 3 (c), b -> 5 (a), c -> 1 (d), d -> 1 (c)
    assert _pick([a, b, c, d]) == 2
    assert _pick([a, b, d, c]) == 2


def test_all_equal_descriptors_pick_index_0():
    x = _desc([1, 50, 200])
    for n in (1, 2, 5, 9, 70):
        assert _pick([x] * n) == 0


def test_tied_medians_go_to_the_lowest_index():
    # four descriptors, each pair 2 bits apart in the same pattern: every row sorted = [0, 2, 2, 2]
    ds = [_desc([0, 1]), _desc([2, 3]), _desc([4, 5]), _desc([6, 7])]
    m = npm.hamming_matrix(np.stack(ds))
    assert (m[~np.eye(4, dtype=bool)] == 4).all()
    assert _pick(ds) == 0
    assert _pick(ds[::-1]) == 0


def test_bad_keyframe_counts_for_the_normal_but_not_for_the_descriptor():
    a = _desc([]); b = _desc(range(10)); c = _desc(range(8))
    # without the bad entry: {a, b, c} -> b; with a bad keyframe's descriptor equal to c in front, the good rows are unchanged and
    # the answer is b's LIST position
    assert _pick([c, a, b, c], good=[0, 1, 1, 1]) == 2
    assert _pick([c, a, b, c], good=[1, 1, 1, 1]) == 0       # (counted: c twice -> c's row median 0)
    assert _pick([a, b], good=[0, 0]) == -1                  # no good keyframe: descriptor unchanged
    # the normal uses both observations whatever their keyframe's flag
    b2 = dict(obs_off=np.array([0, 2]), obs_desc=np.stack([a, b]), obs_kf_good=np.array([0, 1], np.uint8), X=np.array([[0.0, 0.0, 10.0]]),
              ref_kf=np.array([1]), ref_level=np.array([0]), obs_kf=np.array([0, 1]), kf_center=np.array([[0.0, 0.0, 0.0], [3.0, 0.0, 6.0]]),
              scale_factors=npm.SCALE_FACTORS, pt_good=None)
    o = npm.update_map_points(b2, npm.DESC | npm.NORMAL_DEPTH)
    assert o["best_obs"][0] == 1 and (o["desc"][0] == b).all()
    n_exp = (np.array([0.0, 0.0, 1.0]) + np.array([-3.0, 0.0, 4.0]) / 5.0) / 2
    assert np.array_equal(o["normal"][0], n_exp) and o["nd_written"][0] == 1
    assert o["min_max"][0][1] == np.float32(5.0)


def test_normal_and_depth_hand_worked():
    n, mn, mx = npm.normal_and_depth([0.0, 0.0, 10.0], [[0.0, 0.0, 0.0], [0.0, 0.0, 5.0]], [0.0, 0.0, 0.0], 2, npm.SCALE_FACTORS)
    assert np.array_equal(n, [0.0, 0.0, 1.0])
    assert mx == np.float32(np.float32(10.0) * npm.SCALE_FACTORS[2])
    assert mn == np.float32(mx / npm.SCALE_FACTORS[7])
    assert mn.dtype == np.float32 and mx.dtype == np.float32


def test_operator_brackets_quirk_uses_keypoint_0():
    octaves = {("k1", 0): 1, ("k1", 5): 3, ("k2", 0): 6, ("k2", 7): 2}
    oct_of = lambda k, i: octaves[(k, i)]                      # noqa: E731
    assert npm.reference_level(["k1", "k2"], [5, 7], "k2", oct_of) == 2
    assert npm.reference_level(["k1"], [5], "k2", oct_of) == 6     # reference keyframe not in the list: observations[ref] = 0


def test_unchanged_points_and_parts():
    b = npm.make_batch(3, [0, 3, 4, 2], bad_pt_frac=0.0)
    b["pt_good"][2] = 0
    out = npm.fresh_outputs(4, poison=True)
    o = npm.update_map_points(b, npm.DESC, out)
    assert o["best_obs"][0] == -1 and o["best_obs"][2] == -1 and (o["desc"][0] == 0xA5).all() and (o["desc"][2] == 0xA5).all()
    assert (o["nd_written"] == 0xA5).all() and (o["normal"] == -12345.5).all()           # NORMAL_DEPTH not selected: untouched
    o = npm.update_map_points(b, npm.NORMAL_DEPTH, out)
    assert list(o["nd_written"]) == [0, 1, 0, 1] and (o["best_obs"] == -7).all() and (o["normal"][2] == -12345.5).all()


def test_hamming_matrix_paths_agree():
    rng = np.random.default_rng(5)
    D = rng.integers(0, 256, (80, 32), dtype=np.uint8)
    big = npm.hamming_matrix(D)
    small = np.stack([npm.hamming_matrix(np.stack([D[i], D[j]]))[0, 1] for i in range(80) for j in range(80)]).reshape(80, 80)
    assert np.array_equal(big, small)


# ------------------------------------------------------------------------------------------------------------ the C ABI
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_hip()
    from ceres_mono_orb_slam2_amd import _lib
    _lib.load()
    return _lib


def _call(lib, b, what, **over):
    a = dict(b)
    a.update(over)
    P = lambda x: None if x is None else C.c_void_p(np.ascontiguousarray(x).ctypes.data)      # noqa: E731
    keep = {k: (None if v is None or np.isscalar(v) else np.ascontiguousarray(v)) for k, v in a.items()}
    n_of = lambda k, arr: a[k] if k in a else len(keep[arr])                                   # noqa: E731
    npts = a["npts"] if "npts" in a else len(keep["obs_off"]) - 1
    o = npm.fresh_outputs(max(npts, 1), poison=True)
    rc = lib.load().orbl_update_map_points(npts, P(keep["obs_off"]), P(keep["X"]), P(keep["ref_kf"]), P(keep["ref_level"]), P(keep["pt_good"]),
                                           n_of("nobs", "obs_kf"), P(keep["obs_kf"]), P(keep["obs_desc"]), P(keep["obs_kf_good"]),
                                           n_of("nkf", "kf_center"), P(keep["kf_center"]), P(keep["scale_factors"]),
                                           n_of("n_levels", "scale_factors"), what, P(o["best_obs"]), P(o["desc"]), P(o["normal"]),
                                           P(o["min_max"]), P(o["nd_written"]))
    return rc, o


def _good_batch():
    b = npm.make_batch(11, [3, 1, 5, 0, 2], nkf=6)
    return {k: (np.ascontiguousarray(v, np.int32) if k in ("obs_off", "obs_kf", "ref_kf", "ref_level") else v) for k, v in b.items()}


@pytest.mark.parametrize("case", ["neg_npts", "neg_nobs", "neg_nkf", "what0", "what4", "off_start", "off_end", "off_decrease",
                                  "kf_index", "kf_negative", "ref_index", "level_high", "level_negative", "null_off", "null_desc",
                                  "null_normal_out", "n_levels0"])
def test_abi_rejects_bad_arguments_before_device_work(lib, case):
    b = _good_batch()
    what = npm.DESC | npm.NORMAL_DEPTH
    over = {}
    if case == "neg_npts": over["npts"] = -1
    elif case == "neg_nobs": over["nobs"] = -1
    elif case == "neg_nkf": over["nkf"] = -1
    elif case == "what0": what = 0
    elif case == "what4": what = 4
    elif case == "off_start": o = b["obs_off"].copy(); o[0] = 1; over["obs_off"] = o
    elif case == "off_end": over["nobs"] = int(b["obs_off"][-1]) + 1; over["obs_kf"] = np.zeros(int(b["obs_off"][-1]) + 1, np.int32)
    elif case == "off_decrease": o = b["obs_off"].copy(); o[2] = o[1] - 1; over["obs_off"] = o
    elif case == "kf_index": k = b["obs_kf"].copy(); k[-1] = 6; over["obs_kf"] = k
    elif case == "kf_negative": k = b["obs_kf"].copy(); k[0] = -1; over["obs_kf"] = k
    elif case == "ref_index": r = b["ref_kf"].copy(); r[0] = 6; over["ref_kf"] = r
    elif case == "level_high": r = b["ref_level"].copy(); r[2] = 8; over["ref_level"] = r
    elif case == "level_negative": r = b["ref_level"].copy(); r[0] = -1; over["ref_level"] = r
    elif case == "null_off": over["obs_off"] = None; over["npts"] = 5
    elif case == "null_desc": over["obs_desc"] = None
    elif case == "null_normal_out": pass
    elif case == "n_levels0": over["n_levels"] = 0
    if case == "null_normal_out":
        L = lib.load()
        P = lambda x: C.c_void_p(x.ctypes.data)                  # noqa: E731
        o = npm.fresh_outputs(5, poison=True)
        rc = L.orbl_update_map_points(5, P(b["obs_off"]), P(b["X"]), P(b["ref_kf"]), P(b["ref_level"]), None, len(b["obs_kf"]), P(b["obs_kf"]),
                                      P(b["obs_desc"]), None, 6, P(b["kf_center"]), P(b["scale_factors"]), 8, what, P(o["best_obs"]), P(o["desc"]),
                                      None, P(o["min_max"]), P(o["nd_written"]))
    else:
        rc, o = _call(lib, b, what, **over)
    assert rc == -1, case                                          # ORBHIP_EINVAL
    assert b"orbl_update_map_points" in lib.load().orbhip_last_error()
    assert (o["best_obs"] == -7).all() and (o["nd_written"] == 0xA5).all()          # nothing written


def test_abi_ignores_indices_of_points_it_leaves_alone(lib):
    """A bad point's or an empty list's reference keyframe is not read (the drop-in passes -1 there), and the descriptor part alone
    does not read the normal's inputs: none of that is an argument error."""
    b = _good_batch()
    r = b["ref_kf"].copy(); r[3] = -1; b["ref_kf"] = r                 # point 3 has no observations
    b["pt_good"] = np.ones(5, np.uint8); b["pt_good"][0] = 0
    r = b["ref_kf"].copy(); r[0] = 99; b["ref_kf"] = r
    rc, _ = _call(lib, b, npm.DESC | npm.NORMAL_DEPTH)
    if os.path.exists("/dev/kfd"):
        assert rc == 0
    else:
        assert rc == -2 and b"no HIP device" in lib.load().orbhip_last_error()       # valid arguments, no device: ENODEV, no fallback
    rc, _ = _call(lib, b, npm.DESC, X=None, ref_kf=None, ref_level=None, obs_kf=None, kf_center=None, scale_factors=None, nkf=0, n_levels=0,
                  nobs=int(b["obs_off"][-1]))
    assert rc in (0, -2)


def test_device_entry_checks_counts_pointers_and_alignment(lib):
    L = lib.load()
    nb = C.c_size_t(0)
    assert L.orbl_update_map_points_workspace(-1, C.byref(nb)) == -1
    assert L.orbl_update_map_points_workspace(1000, None) == -1
    assert L.orbl_update_map_points_workspace(1000, C.byref(nb)) == 0 and nb.value >= 5 * 4 * 1000
    assert L.orbl_update_map_points_device(0, None, None, None, None, None, 0, None, None, None, 0, None, None, 0, 1, None, None, None, None, None,
                                           None, None) == 0
    fake = C.c_void_p(0x100000)                                    # never dereferenced: every case fails on the host first
    odd = C.c_void_p(0x100001)
    args = lambda **k: [k.get("npts", 4), fake, fake, fake, fake, None, k.get("nobs", 10), fake, k.get("desc", fake), None, 3, fake, fake,  # noqa: E731
                        k.get("nl", 8), k.get("what", 3), fake, k.get("dout", fake), fake, fake, fake, k.get("ws", fake), None]
    for bad in (dict(npts=-1), dict(nobs=-1), dict(what=0), dict(what=7), dict(ws=None), dict(desc=None), dict(desc=odd), dict(dout=odd), dict(nl=0),
                dict(nl=65)):
        assert L.orbl_update_map_points_device(*args(**bad)) == -1, bad


def test_new_header_symbols_are_exported(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH]).decode()
    exported = set(l.split()[-1] for l in out.splitlines() if " T " in l)
    for name in ("orbl_update_map_points", "orbl_update_map_points_device", "orbl_update_map_points_workspace"):
        assert name in exported and name in lib.SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "orbslam_hip.h")).read()
    assert "#define ORBL_MP_DESC 1" in hdr and "#define ORBL_MP_NORMAL_DEPTH 2" in hdr

"""CPU checks of the restatement tests/npmapcorrect.py (the literal loops of src/LoopClosing.cc:446-523 and :681-739) that the GPU tests
compare orbl_correct_loop / orbl_propagate_global_ba against: the hand cases against the values written in tests/mapcorrectcases.py,
its Sim3 arithmetic against the existing oracle, and guards that the seeded problems are not weak - conditions, not measurements."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import mapcorrectcases as mc  # noqa: E402
from tests import npmapcorrect as npm  # noqa: E402

RTOL = 1e-12                       # the bar tests/test_gpu_essential_graph.py holds this arithmetic to


def _close(a, b, rtol=RTOL):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return a.shape == b.shape and np.abs(a - b).max() <= rtol * max(1.0, np.abs(b).max())


@pytest.mark.parametrize("name", sorted(mc.hand_loop_cases()))
def test_correct_loop_hand_cases(name):
    pr, exp = mc.hand_loop_cases()[name]
    npts = pr["npts"]
    poison = dict(normal=np.full((npts, 3), mc.POISON), min_max=np.full((npts, 2), mc.POISON, np.float32), nd_written=np.full(npts, 77, np.uint8))
    r = npm.correct_loop(pr, **poison)
    assert r["pt_owner"].tolist() == exp["pt_owner"].tolist() and r["counts"].tolist() == exp["counts"]
    exact = "scale" not in exp                                       # (sqrt(1.04) is not a binary fraction: 1e-12 there, == elsewhere)
    for k in ("kf_Tcw", "X"):
        assert np.array_equal(r[k], exp[k]) if exact else _close(r[k], exp[k]), k
    s = exp.get("scale", 1.0)
    group = pr["conn_kf"].tolist()
    cur = group[-1]
    for k in range(pr["nkf"]):
        if k not in group:
            assert np.array_equal(r["kf_center"][k], pr["kf_center"][k])
        else:                                                        # t / s, and the centre -(R^T t / s) with R = I
            t = (np.array(mc.T_HAND[k]) - np.array(mc.T_HAND[cur]) + np.array(mc.TS)) / s
            assert _close(r["kf_Tcw"][k].reshape(3, 4)[:, 3], t) and _close(r["kf_center"][k], -t)
    # the two Sim3 maps: q = sqrt(s) [0 0 0 1] / [0 0 0 1], the translations of the note in mapcorrectcases
    for c, k in enumerate(group):
        assert _close(r["non_corrected"][c], [0, 0, 0, 1] + list(mc.T_HAND[k]))
        assert _close(r["corrected"][c], [0, 0, 0, np.sqrt(s)] + (np.array(mc.T_HAND[k]) - np.array(mc.T_HAND[cur]) + np.array(mc.TS)).tolist())
    if "new_centre_for" in exp:
        old_c, new_c = pr["kf_center"], r["kf_center"]
        for p, use_new in enumerate(exp["new_centre_for"]):
            obs = pr["obs_kf"][pr["obs_off"][p]:pr["obs_off"][p + 1]].tolist()
            if not obs:
                assert r["nd_written"][p] == 0 and np.all(r["normal"][p] == mc.POISON) and np.all(r["min_max"][p] == np.float32(mc.POISON))
                continue
            ctr = {k: (new_c[k] if k in use_new else old_c[k]) for k in set(obs) | {int(pr["ref_kf"][p])}}
            v = np.array([(r["X"][p] - ctr[k]) / np.linalg.norm(r["X"][p] - ctr[k]) for k in obs])
            assert r["nd_written"][p] == 1 and _close(r["normal"][p], v.mean(0))
            mx = np.linalg.norm(r["X"][p] - ctr[int(pr["ref_kf"][p])]) * mc.SF[pr["ref_level"][p]]
            assert _close(r["min_max"][p], [mx / mc.SF[-1], mx], 1e-6)
        if name.startswith("f_"):
            o, n = npm.correct_loop(pr, "old"), npm.correct_loop(pr, "new")
            assert np.any(r["normal"][0] != o["normal"][0]) and np.any(r["normal"][0] != n["normal"][0])
    else:
        assert r["normal"] is None and r["nd_written"] is None


@pytest.mark.parametrize("name", sorted(mc.hand_gba_cases()))
def test_propagate_global_ba_hand_cases(name):
    pr, exp = mc.hand_gba_cases()[name]
    bef0 = np.full((pr["nkf"], 12), mc.POISON)
    r = npm.propagate_global_ba(pr, kf_bef_Tcw=bef0)
    assert r["kf_reached"].tolist() == exp["kf_reached"] and r["counts"].tolist() == exp["counts"] and r["pt_moved"].tolist() == exp["pt_moved"]
    assert np.array_equal(r["X"], np.array(exp["X"]))
    if "kf_Tcw" in exp:
        assert np.array_equal(r["kf_Tcw"], exp["kf_Tcw"]) and np.array_equal(r["kf_gba_Tcw"], exp["kf_Tcw"])
    if "kf_in_gba" in exp:
        assert r["kf_in_gba"].tolist() == exp["kf_in_gba"]
    if "depth" in exp:
        assert r["depth"] == exp["depth"]
    for k in range(pr["nkf"]):
        if r["kf_reached"][k]:
            assert np.array_equal(r["kf_bef_Tcw"][k], pr["kf_Tcw"][k]) and np.array_equal(r["kf_Tcw"][k], r["kf_gba_Tcw"][k])
            assert np.array_equal(r["kf_center"][k], -r["kf_Tcw"][k].reshape(3, 4)[:, 3])         # (R = I in every hand case)
        else:
            assert np.all(r["kf_bef_Tcw"][k] == mc.POISON) and np.array_equal(r["kf_Tcw"][k], pr["kf_Tcw"][k]) and np.array_equal(r["kf_center"][k], pr["kf_center"][k])


def test_sim3_arithmetic_against_the_oracle(oracle):
    rng = np.random.RandomState(5)
    for _ in range(50):
        A = oracle.sim3_exp(np.concatenate([rng.uniform(-3, 3, 3), rng.uniform(-1.5, 1.5, 3), rng.uniform(-0.1, 0.1, 1)]))
        B = oracle.sim3_exp(np.concatenate([rng.uniform(-3, 3, 3), rng.uniform(-1.5, 1.5, 3), rng.uniform(-0.1, 0.1, 1)]))
        p = rng.uniform(-10, 10, 3)
        assert _close(npm.s3_mul(list(A), list(B)), oracle.sim3_mul(A, B))
        assert _close(npm.s3_inverse(list(A)), oracle.sim3_inverse(A))
        assert _close(npm.s3_act(list(A), list(p)), oracle.sim3_act(A, p))


def test_pose_from_sim3_against_the_oracle_write_back(oracle):
    rng = np.random.RandomState(6)
    lie = np.array([np.concatenate([rng.uniform(-3, 3, 3), rng.uniform(-1.5, 1.5, 3), rng.uniform(-0.1, 0.1, 1)]) for _ in range(40)])
    T, _ = oracle.essential_graph_correct(lie, lie, np.zeros(1, np.int32), np.zeros((1, 3)))
    for v in range(40):
        assert _close(npm.s3_to_pose34(list(oracle.sim3_exp(lie[v]))), T[v])


def test_se3_as_sim3_is_the_pose_codec_and_round_trips():
    rng = np.random.RandomState(7)
    for i in range(60):
        T = mc._rand_pose(rng)
        if i % 3 == 0:                                               # (a half turn: the trace is not positive, the other branches run)
            T = T.reshape(3, 4); T[:, :3] = T[:, :3] @ np.diag([[1, -1, -1], [-1, 1, -1], [-1, -1, 1]][i % 9 // 3]); T = T.reshape(12)
        S = npm.se3_as_sim3(list(T))
        assert abs(sum(q * q for q in S[:4]) - 1.0) < 1e-12
        back = npm.s3_to_pose34(S)
        assert _close(back, T)
        Twc = npm.pose_inverse(list(T))
        assert _close(npm.affine_mul(list(T), Twc), mc._pose((0, 0, 0)))


def test_seeded_correct_loop_problems_are_not_weak():
    seen = 0
    for name, pr in mc.seeded_loop():
        nconn = len(pr["conn_kf"])
        assert np.diff(pr["slot_off"]).max() <= 300
        if nconn < 3:
            continue
        seen += 1
        r, o, n = npm.correct_loop(pr), npm.correct_loop(pr, "old"), npm.correct_loop(pr, "new")
        moved = r["pt_owner"] >= 0
        first = np.full(pr["npts"], -1)
        listed = np.zeros(pr["npts"], int)
        for c in range(nconn):
            pts = np.unique([p for p in pr["slot_pt"][pr["slot_off"][c]:pr["slot_off"][c + 1]] if p >= 0]).astype(int)
            listed[pts] += 1
            first[pts[first[pts] < 0]] = pr["conn_kf"][c]
        contested = moved & (listed >= 2)
        assert contested.sum() == r["counts"][1] and contested.sum() >= 0.10 * moved.sum(), name
        assert (r["pt_owner"][contested] != first[contested]).sum() >= contested.sum() / 3.0, name
        differs = moved & (r["nd_written"] == 1) & np.any(r["normal"] != o["normal"], 1) & np.any(r["normal"] != n["normal"], 1)
        assert differs.sum() >= 0.05 * moved.sum(), name
        assert (~moved).sum() > 0 and (moved & (r["nd_written"] == 0)).sum() >= 0
    assert seen >= 4
    assert any(np.diff(pr["obs_off"]).max() == 600 for _, pr in mc.seeded_loop())


def test_seeded_propagation_problems_are_not_weak():
    seen = 0
    for name, pr in mc.seeded_gba():
        if pr["nkf"] < 64:
            continue
        seen += 1
        r = npm.propagate_global_ba(pr)
        assert (pr["kf_in_gba"] == 0).sum() >= 0.10 * pr["nkf"], name
        assert r["depth"] >= 3, name
        for kind in (0, 1, 2):
            assert (r["pt_moved"] == kind).sum() >= 0.05 * pr["npts"], (name, kind)
        assert r["counts"][3] > 0 and r["counts"][0] < pr["nkf"], name
    assert seen == 3

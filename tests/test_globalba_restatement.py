"""tests/npglobalba.py against the hand-worked cases of tests/globalbacases.py, and the seeded maps against what they are meant to contain.
No GPU and no library."""
import numpy as np
import pytest

from tests import globalbacases as gc
from tests import npglobalba as npg

HAND = gc.hand_assemble_cases()
SEEDED = gc.seeded_maps()


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_assemble(name):
    m, rob, hand = HAND[name]
    r = npg.assemble(m, is_robust=rob)
    for k, v in hand.items():
        assert np.array_equal(r[k], np.asarray(v, r[k].dtype).reshape(r[k].shape)), (k, r[k], v)
    assert r["gobs_weight"].dtype == np.float64 and r["gobs_uv"].dtype == np.float64


@pytest.mark.parametrize("stage", [0, 1])
def test_hand_apply(stage):
    m, (ck, gp, p7, p3), s0, s1 = gc.hand_apply_case()
    poison = dict(normal=np.full((7, 3), gc.POISON), min_max=np.full((7, 2), gc.POISON, np.float32))
    r = npg.apply(m, ck, gp, p7, p3, stage=stage, **(poison if stage == 0 else {}))
    hand = s1 if stage else s0
    for k, v in hand.items():
        if k not in ("normal6", "min_max6"):
            assert np.array_equal(r[k], np.asarray(v, r[k].dtype).reshape(r[k].shape)), (k, r[k], v)
    if stage == 0:
        assert np.array_equal(r["normal"][6], hand["normal6"]) and np.array_equal(r["min_max"][6], np.array(hand["min_max6"], np.float32))
        untouched = [p for p in range(7) if not r["nd_written"][p]]
        assert np.all(r["normal"][untouched] == gc.POISON) and np.all(r["min_max"][untouched] == gc.POISON)
        n = npg.apply(m, ck, gp, p7, p3, stage=0, normals=False)
        assert n["normal"] is None and n["counts"].tolist() == [3, 2, 0] and np.array_equal(n["X"], r["X"]) and np.array_equal(n["kf_Tcw"], r["kf_Tcw"])


@pytest.mark.parametrize("name,m", SEEDED, ids=[n for n, _ in SEEDED])
def test_seeded_structure(name, m):
    """the restatement's problem, solved by nothing here, compared structurally: every row joins a camera that is not bad and listed with
    a point that is not bad and listed; cameras ascend by (id, first position); each problem point has a row; rows keep list order"""
    r = npg.assemble(m)
    ncam, npb, nob = r["counts"]
    ba_kf = m["ba_kf"].tolist(); ba_pt = m["ba_pt"].tolist()
    assert ncam > 0 and npb > 0 and nob >= npb
    first_k = {k: i for i, k in reversed(list(enumerate(ba_kf)))}; at_p = {p: i for i, p in enumerate(ba_pt)}
    keys = [(int(m["kf_id"][k]), first_k[k]) for k in r["cam_kf"]]
    assert keys == sorted(keys) and len(set(r["cam_kf"].tolist())) == ncam
    assert set(r["cam_kf"].tolist()) == {k for k in ba_kf if not m["kf_bad"][k]}
    assert all(not m["pt_bad"][p] and p in at_p for p in r["gpt_pt"])
    assert np.all(np.diff([at_p[p] for p in r["gpt_pt"]]) > 0)
    assert np.array_equal(np.unique(r["gobs_pt"]), np.arange(npb)) and np.all(np.diff(r["gobs_pt"]) >= 0)
    assert np.array_equal(r["cam_kf"][r["gobs_cam"]], m["obs_kf"][r["gobs_src"]])
    p_of_row = r["gpt_pt"][r["gobs_pt"]]
    assert np.all(r["gobs_src"] >= m["obs_off"][p_of_row]) and np.all(r["gobs_src"] < m["obs_off"][p_of_row + 1])
    same = np.diff(r["gobs_pt"]) == 0
    assert np.all(np.diff(r["gobs_src"])[same] > 0)
    assert np.array_equal(r["kf_cam"][r["cam_kf"]], np.arange(ncam)) and np.array_equal(r["pt_idx"][r["gpt_pt"]], np.arange(npb))
    assert (r["kf_cam"] >= 0).sum() == ncam and (r["pt_idx"] >= 0).sum() == npb
    assert r["cam_fixed"].sum() == sum(1 for k in r["cam_kf"] if m["kf_id"][k] == 0)
    # what the maps are meant to contain
    if m["nkf"] == 300:
        assert ncam > 256 and len(ba_kf) < m["nkf"], "the cameras do not cross a tile of the all-pairs count, or no keyframe is outside the list"
        at = np.array([at_p[p] for p in r["gpt_pt"]])
        assert np.any(at < 256) and np.any(at >= 256), "the point scan carries no sum into its second workgroup"
    if m["npts"] == 70000:
        assert len(ba_pt) > 256 * 256 and set(np.diff(m["obs_off"]).tolist()) <= {0, 1, 2}, "the scan does not see more than 256 workgroup sums"
    listed = [p for p in ba_pt if not m["pt_bad"][p]]
    assert len(listed) > npb, "no point without rows"
    assert any(m["kf_bad"][k] for k in ba_kf) and len(set(ba_kf)) < len(ba_kf) and len(set(ba_kf)) <= m["nkf"]


@pytest.mark.parametrize("name,m", SEEDED, ids=[n for n, _ in SEEDED])
def test_order_blind_variant_differs(name, m):
    r, b = npg.assemble(m), npg.assemble(m, blind=True)
    assert not np.array_equal(r["cam_kf"], b["cam_kf"]), "the cameras do not tell the id order from the list order"
    assert not np.array_equal(r["gpt_pt"], b["gpt_pt"]), "the points do not tell the list order from the index order"
    assert b["counts"][1] > r["counts"][1], "no point without rows"


def test_apply_seeded_flags_and_skips():
    name, m = SEEDED[0]
    asm = npg.assemble(m)
    p7, p3 = gc.solver_result(7, asm)
    w = gc.turned_bad(8, m, asm)
    r1 = npg.apply(w, asm["cam_kf"], asm["gpt_pt"], p7, p3, stage=1)
    assert r1["counts"][0] < asm["counts"][0] and r1["counts"][1] < asm["counts"][1]
    assert r1["kf_in_gba"].sum() == r1["counts"][0] and r1["pt_in_gba"].sum() == r1["counts"][1]
    assert not np.any(r1["kf_in_gba"][w["kf_bad"] != 0]) and not np.any(r1["pt_in_gba"][w["pt_bad"] != 0])
    r0 = npg.apply(w, asm["cam_kf"], asm["gpt_pt"], p7, p3, stage=0)
    assert np.array_equal(r0["X"][r1["pt_in_gba"] == 0], m["X"][r1["pt_in_gba"] == 0]) and 0 < r0["counts"][2] <= r0["counts"][1]
    assert np.array_equal(r0["kf_Tcw"][r1["kf_in_gba"] != 0], r1["kf_gba_Tcw"][r1["kf_in_gba"] != 0])

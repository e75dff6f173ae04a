"""CPU checks of the test infrastructure of orbl_local_ba_assemble / orbl_local_ba_apply: the restatement tests/nplocalba.py reproduces the
hand-worked cases of tests/localbacases.py, an ORDER-BLIND variant (index order for the ranks, erases scored against the state at entry, the
centres at entry for the normals) gives different outputs on every seeded map, and no seeded map is vacuous.  These are checks of the
test infrastructure alone: they call nothing of the library and pass without it (tests/test_localba_abi.py and tests/test_gpu_localba*.py
are the ones that need the feature)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import localbacases as lc  # noqa: E402
from tests import nplocalba as npl  # noqa: E402

HAND = lc.hand_assemble_cases()
_SEEDED = []


def seeded():
    """every seeded map with its restated outputs (assembled, solver result, applied), computed once and shared"""
    if not _SEEDED:
        for i, (name, m) in enumerate(lc.seeded_maps()):
            asm = npl.assemble(m)
            res = lc.solver_result(900 + i, m, asm)
            _SEEDED.append((name, m, asm, res, npl.apply(m, asm, *res)))
    return _SEEDED


@pytest.mark.parametrize("name", sorted(HAND))
def test_restatement_reproduces_the_hand_assemble_cases(name):
    m, hand = HAND[name]
    got = npl.assemble(m)
    for k, v in hand.items():
        assert got[k].tolist() == v, (name, k)
    ncam = hand["counts"][0]
    assert got["K4"].shape == (ncam, 4) and got["poses7"].shape == (ncam, 7)
    for c, k in enumerate(hand["cam_kf"]):                             # [I | t]: t, then the identity quaternion
        assert got["poses7"][c].tolist() == [float(k), 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]
    for i, e in enumerate(hand["lobs_src"]):
        assert got["lobs_uv"][i].tolist() == [100.0 + e, 50.0 + 2 * e] and got["lobs_inv_sigma2"][i] == lc.ISG[e % 8]
    for j, p in enumerate(hand["lpt_pt"]):
        assert got["pts3"][j].tolist() == [float(p), 1.0, 2.0]


def test_restatement_reproduces_the_hand_apply_case():
    m, res, hand = lc.hand_apply_case()
    asm = npl.assemble(m)
    assert asm["lobs_src"].tolist() == list(range(15)) and asm["cam_kf"].tolist() == [0, 1, 2, 3, 4] and asm["cam_fixed"].tolist() == [1, 0, 0, 0, 1]
    got = npl.apply(m, asm, *res, normal=np.full((5, 3), lc.POISON), min_max=np.full((5, 2), lc.POISON, np.float32))
    for k in ("kf_slot_pt", "pt_bad", "pt_nobs", "pt_ref_kf", "obs_erased", "counts", "nd_written"):
        assert got[k].tolist() == hand[k], k
    assert got["diag"] == hand["diag"]
    assert [tuple(c) for c in got["kf_center"].tolist()] == hand["kf_center"] and [tuple(x) for x in got["X"].tolist()] == hand["X"]
    assert got["kf_Tcw"][0].tolist() == [1.0, 0.0, 0.0, -10.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]               # (id 0: fixed in the solve, still SetPose'd)
    assert got["normal"][4].tolist() == hand["normal4"] and got["min_max"][4].tolist() == hand["min_max4"] and got["min_max"][3].tolist() == hand["min_max3"]
    assert np.all(got["normal"][[1, 2]] == lc.POISON) and np.all(got["min_max"][[1, 2]] == lc.POISON)              # (rows of bad points are untouched)


def test_no_seeded_map_is_vacuous_and_sizes_cross_the_scan_units():
    big = False
    for name, m, asm, res, out in seeded():
        assert np.any(asm["cam_local"] == 0), name                     # a fixed camera
        assert np.any(asm["kf_role"] == 3), name                       # a bad neighbour
        assert out["diag"]["turned_bad"] >= 1 and out["diag"]["ref_moved"] >= 1 and out["diag"]["dead_rows"] >= 1, (name, out["diag"])
        assert 0.1 * len(res[2]) <= res[2].sum() <= 0.3 * len(res[2]), name
        assert np.any(asm["cam_fixed"][asm["cam_local"] == 1]), name   # keyframe id 0 is local
        assert np.any(out["nd_written"]) and np.any(asm["pt_local"] == 0), name
        # the scan positions (kf_rank, pt_rank) of the fixed keyframes and of the local points lie on both sides of 256: both workgroup scans
        # carry a sum into their second workgroup
        rk, rp = m["kf_rank"][asm["kf_role"] == 2], m["pt_rank"][asm["pt_local"] != 0]
        carry = np.any(rk < 256) and np.any(rk >= 256) and np.any(rp < 256) and np.any(rp >= 256)
        big = big or (asm["counts"][0] > 64 and asm["counts"][2] > 4096 and int(np.max(np.diff(m["obs_off"]))) > 256 and carry)
    assert big


def test_an_order_blind_variant_differs_on_every_seeded_map():
    for name, m, asm, res, out in seeded():
        blind = npl.assemble(m, order="index")
        assert blind["counts"].tolist() == asm["counts"].tolist(), name
        assert not np.array_equal(blind["cam_kf"], asm["cam_kf"]) and not np.array_equal(blind["lpt_pt"], asm["lpt_pt"]), name
        assert not np.array_equal(blind["lobs_src"], asm["lobs_src"]), name
        b = npl.apply(m, asm, *res, blind=True)
        assert b["counts"].tolist() != out["counts"].tolist(), name     # (erase rows on dead observations are counted by the blind one)
        assert not np.array_equal(b["pt_nobs"], out["pt_nobs"]), name
        assert not np.array_equal(b["normal"], out["normal"]), name     # (old centres)
        assert np.array_equal(b["X"], out["X"]) and np.array_equal(b["kf_Tcw"], out["kf_Tcw"]), name

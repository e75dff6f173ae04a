"""GPU: k_pose_lm (csrc/ba_small_lm.inc) on the case table of tests/posecases.py - both of its data paths (observations in registers
up to 2048, streamed from global memory above), sizes at the minimum / a wave / a workgroup / the switch, rejected steps and
retries, and every termination the table reaches (1, 2, 3, 5).

Each case is compared twice:
  * with the CPU oracle at the bars tests/test_gpu_ba.py states - iterations, accepted steps, termination, inlier count and every
    outlier flag identical, costs within 1e-9, the pose within 1e-7;
  * with the references of tests/nppose.py, no oracle in the loop - the initial cost against the mp cost at pose0, the final cost
    against the mp cost AT THE DEVICE'S OWN POSE, within 100 x the oracle's largest deviation from mp (posecases.MP_BAR_*, measured by
    tests/test_pose_reference.py), the flags against mp chi2 > 5.991 at that pose with nothing left out, and the optimality gap
    against an independent float64 minimiser no worse than the oracle's plus 2e-9.
Costs that are rounding residue (posecases.is_residue: the final cost of size_3 / exact_near / exact_at_truth, the initial cost of
exact_at_truth) get the absolute bar posecases.residue_atol instead of a relative one, as on the CPU side.

Measured on MI355X: deviation from mp at most 4.2e-13 (initial cost, exact_near) and 5.0e-14 (final cost, size_4) - the oracle's own
figures; against the oracle the costs differ by at most 2.7e-15 relative and the poses by 8e-15; every optimality gap equals the
oracle's to three digits (at most 9.2e-7); each case takes 0.02 - 0.35 s."""
import ctypes as C

import numpy as np
import pytest

from tests import nppose
from tests import posecases as P

pytestmark = pytest.mark.gpu
RTOL_COST, RTOL_X = P.RTOL_COST, P.RTOL_X


def _close(a, b, rtol):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return np.abs(a - b).max() <= rtol * max(1.0, np.abs(b).max())


@pytest.mark.parametrize("name", P.ALL_CASES)
def test_pose_lm_case(oracle, name):
    from ceres_mono_orb_slam2_amd import optimizer
    p = P.make_case(name)
    ni, pose, out, s = optimizer.pose_optimization(*P.args(p))
    oni, opose, oout, os_ = P.oracle_run(name)
    print("%s n = %d (%s)  device %s  oracle %s" % (name, len(out), "streamed" if P.is_streaming(name) else "registers", s, os_))
    # ---- against the oracle
    assert (os_["iterations"], os_["successful_steps"], os_["termination"]) == P.ORACLE_TABLE[name]
    assert (s["iterations"], s["successful_steps"], s["termination"]) == (os_["iterations"], os_["successful_steps"], os_["termination"])
    assert ni == oni and np.array_equal(out, oout)
    # the trust-region radius the solve ends with (tests/test_gpu_sim3.py's bar for it)
    assert abs(s["final_radius"] - os_["final_radius"]) <= 1e-9 * os_["final_radius"]
    if name in P.INF_CASES:
        # five invalid steps: the radius is halved, quartered, ... four times and NOT after the fifth, which ends the solve - 1e4 / 1024
        assert pose.tobytes() == p["pose0"].tobytes() and s["termination"] == 5 and s["final_radius"] == os_["final_radius"] == 1e4 / 1024
        return
    mp_i = P.mp_initial_cost(name)
    atol = P.residue_atol(name, mp_i)
    print("    cost vs oracle: initial %.3g final %.3g (absolute); pose %.3g" % (abs(s["initial_cost"] - os_["initial_cost"]), abs(s["final_cost"] - os_["final_cost"]),
                                                                                np.abs(pose - opose).max()))
    if name in P.RESIDUE_AT_START:
        assert abs(s["initial_cost"] - os_["initial_cost"]) <= atol
    else:
        assert abs(s["initial_cost"] - os_["initial_cost"]) <= RTOL_COST * os_["initial_cost"]
    if name in P.RESIDUE_CASES:
        assert abs(s["final_cost"] - os_["final_cost"]) <= atol
    else:
        assert abs(s["final_cost"] - os_["final_cost"]) <= RTOL_COST * os_["final_cost"]
    assert _close(pose, opose, RTOL_X)
    if name in P.EXACT_CASES:
        assert np.abs(pose - p["pose_gt"]).max() <= RTOL_X
    # ---- against mp, at the device's own pose
    depth, chi2, sq = nppose.mp_terms(p["K4"], pose, p["Xw"], p["uv"], p["inv_sigma2"])
    mp_f = nppose.mp_cost(sq)
    for key, cost, ref, bar in (("initial", s["initial_cost"], mp_i, P.MP_BAR_INITIAL), ("final", s["final_cost"], mp_f, P.MP_BAR_FINAL)):
        residue = ref != 0 and P.is_residue(name, ref, mp_i)
        assert residue == (name in (P.RESIDUE_AT_START if key == "initial" else P.RESIDUE_CASES))
        if ref == 0:
            print("    %s cost %.17g, mp 0" % (key, cost))
            assert cost == 0.0
        elif residue:
            print("    %s cost %.17g, mp %.17g: residue, bar %.3g" % (key, cost, float(ref), atol))
            assert 0.0 <= cost <= atol
        else:
            dev = nppose.rel_dev(cost, ref)
            print("    %s cost deviation from mp %.3g (bar %.3g)" % (key, dev, bar))
            assert dev <= bar
    flags, band = nppose.mp_flags(chi2)
    print("    nearest observation to the gate %.3g" % band)
    assert band > P.GATE_BAND
    assert np.array_equal(out, flags)
    # ---- optimality against the independent minimum
    gap, ogap = P.gap(name, pose), P.gap(name, opose)
    print("    optimality gap %.3g (oracle %.3g)" % (gap, ogap))
    assert gap <= ogap + 2.0 * RTOL_COST


def test_pose_optimization_batch_spans_both_paths():
    """One launch over problems on both data paths, at the switch and below the minimum: the same kernel as the single call, so the
    pose bytes, the flags, the inlier count and the summary record are identical; fewer than 3 observations leave the pose alone."""
    import torch
    from ceres_mono_orb_slam2_amd import optimizer, synth, _lib
    sizes = [2049, 2, 4100, 3, 256, 2048, 0, 257]
    probs = []
    for n in sizes:
        if n >= 3:
            probs.append(P.make_case("size_%d" % n))
        else:
            q = synth.make_pose_problem(100 + n, n=10)
            probs.append({k: q[k][:n] if k in ("Xw", "uv", "inv_sigma2") else q[k] for k in ("K4", "pose0", "Xw", "uv", "inv_sigma2")})
    assert [len(q["Xw"]) for q in probs] == sizes
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    K4 = torch.from_numpy(np.stack([q["K4"] for q in probs])).cuda()
    poses = torch.from_numpy(np.stack([q["pose0"] for q in probs])).cuda()
    Xw = torch.from_numpy(np.concatenate([q["Xw"] for q in probs])).cuda()
    uv = torch.from_numpy(np.concatenate([q["uv"] for q in probs])).cuda()
    isg = torch.from_numpy(np.concatenate([q["inv_sigma2"] for q in probs])).cuda()
    outl, ninl, summ = optimizer.pose_optimization_batch(K4, poses, Xw, uv, isg, torch.from_numpy(offs).cuda())
    torch.cuda.synchronize()
    poses = poses.cpu().numpy(); outl = outl.cpu().numpy(); ninl = ninl.cpu().numpy(); summ = summ.cpu().numpy()
    assert len(outl) == offs[-1]
    for i, q in enumerate(probs):
        rec = _lib.BaSummary.from_buffer_copy(summ[i].tobytes()).as_dict()
        if sizes[i] < 3:
            assert poses[i].tobytes() == q["pose0"].tobytes() and ninl[i] == 0
            assert rec == _lib.BaSummary().as_dict()
            continue
        n1, pose1, out1, s1 = optimizer.pose_optimization(*P.args(q))
        assert poses[i].tobytes() == pose1.tobytes(), sizes[i]
        assert np.array_equal(outl[offs[i]:offs[i + 1]], out1) and ninl[i] == n1, sizes[i]
        assert rec == s1, (sizes[i], rec, s1)
        assert s1["iterations"] >= 3
    assert C.sizeof(_lib.BaSummary) == summ.shape[1]

"""orbl_update_connections(_device) on the MI355X against the restatement tests/npconnections.py (the literal loop of
src/KeyFrame.cc:314-398 with AddConnection's re-sorts, and the links of src/LoopClosing.cc:551-573): every output is an integer array and
is compared with ==.  tests/test_connections_restatement.py shows that the problems take every path of the loop and tell it from an
order-blind implementation."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import connectioncases as cc  # noqa: E402
from tests import npconnections as npc  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ("tgt_status", "tgt_parent", "counts", "aff_kf", "conn_off", "conn_kf", "conn_w", "ord_off", "ord_kf", "ord_w", "link_off", "link_kf")
LISTS = dict(aff_kf=0, conn_kf=1, conn_w=1, ord_kf=2, ord_w=2, link_kf=3)       # output -> the entry of counts[] that is its length
HAND = cc.hand_cases()
POISON = -7777
ECAP = -4
_SEEDED = None


def _seeded():
    """every seeded problem with its restated outputs, computed once and shared"""
    global _SEEDED
    if _SEEDED is None:
        _SEEDED = [(name, pr, npc.connections(pr)) for name, pr in cc.seeded(20)]
        for _, pr, exp in _SEEDED:
            for v in list(pr.values()) + list(exp.values()):
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
    return _SEEDED


def _args(pr, conv=lambda a: a):
    a = [conv(pr[k]) for k in ("tgt_kf", "slot_off", "slot_pt")] + [pr["nkf"]] + [conv(pr[k]) for k in ("obs_off", "obs_kf", "conn_off", "conn_kf", "conn_w")]
    kw = dict(tgt_flags=conv(pr["tgt_flags"]), pt_bad=conv(pr["pt_bad"]), kf_rank=conv(pr["kf_rank"]), prev_off=conv(pr["prev_off"]), prev_kf=conv(pr["prev_kf"]),
              th=pr["th"])
    return a, kw


def _host(pr, **kw):
    from ceres_mono_orb_slam2_amd import localmapping
    a, k = _args(pr)
    k.update(kw)
    return localmapping.update_connections(*a, **k)


def _device_raw(pr, **kw):
    import torch
    from ceres_mono_orb_slam2_amd import localmapping

    def t(a):
        return None if a is None else torch.as_tensor(np.array(a)).cuda()          # (a copy: the shared problems are read-only)
    a, k = _args(pr, t)
    k.update(kw)
    r = localmapping.update_connections_device(*a, **k)
    torch.cuda.synchronize()
    return r


def _trim(r):
    """the device form's full-capacity tensors cut to the written counts, as the host form returns them"""
    c = r["counts"].cpu().numpy()
    o = dict(counts=c, status=int(r["status"].item()) & 0xFFFFFFFF, tgt_status=r["tgt_status"].cpu().numpy(), tgt_parent=r["tgt_parent"].cpu().numpy())
    for k, i in LISTS.items():
        o[k] = None if r.get(k) is None else r[k].cpu().numpy()[:c[i]]
    o["conn_off"] = r["conn_off"].cpu().numpy()[:c[0] + 1]; o["ord_off"] = r["ord_off"].cpu().numpy()[:c[0] + 1]
    o["link_off"] = None if r.get("link_off") is None else r["link_off"].cpu().numpy()
    return o


def _device(pr, **kw):
    return _trim(_device_raw(pr, **kw))


def _same(got, exp, what="", keys=KEYS):
    for k in keys:
        if exp[k] is None:
            assert got[k] is None, (what, k)
        else:
            assert got[k] is not None and got[k].dtype == exp[k].dtype and np.array_equal(got[k], exp[k]), (what, k, got[k], exp[k])


def _both(pr, what, exp=None):
    exp = npc.connections(pr) if exp is None else exp
    h, d = _host(pr), _device(pr)
    _same(h, exp, what + " host")
    _same(d, exp, what + " device")
    assert d["status"] == 0, what
    return exp


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_worked_cases_host_and_device(name):
    pr, exp = HAND[name]
    _both(pr, name, exp)


def test_seeded_maps_host_and_device_equal_the_restatement_and_each_other():
    for name, pr, exp in _seeded():
        h, d = _host(pr), _device(pr)
        _same(h, exp, name + " host")
        _same(d, h, name + " device against host")
        _same(d, exp, name + " device")
        assert d["status"] == 0, name


@pytest.mark.parametrize("nkf", [1, 2, 63, 64, 65, 257])
def test_keyframe_counts_at_the_seams_one_target_and_all_targets(nkf):
    for ntgt in sorted({1, nkf}):
        pr = cc.make(nkf, nkf=nkf, ntgt=ntgt, dup=True, per_kf=40 if nkf < 100 else 24)
        exp = _both(pr, "nkf %d ntgt %d" % (nkf, ntgt))
        assert len(pr["tgt_kf"]) == ntgt and (nkf < 8 or exp["counts"][0] >= 1)


def test_empty_null_and_long_slot_lists():
    # target 0 has no slot at all, target 1 only null slots and a bad point, target 2 has 2 100 slots (more than one pass of its workgroup,
    # more than eight workgroups of the slot kernel), target 3 a few
    obs = [[1, 5]] + [[2, 3 + p % 3] for p in range(2100)] + [[3, 4]] * 20
    slots = [[], [-1, 0, -1], list(range(1, 2101)), list(range(2101, 2121)) + [5, 6]]
    pt_bad = [1] + [0] * 2120
    pr = cc.flatten(6, obs, [0, 1, 2, 3], slots, conn=[{1: 3}, {}, {3: 700, 4: 1}, {}, {}, {}], prev=[[1], [], [4], []], flags=[1, 1, 1, 1], pt_bad=pt_bad)
    exp = _both(pr, "slot lists")
    assert exp["tgt_status"].tolist() == [1, 1, 0, 0] and exp["tgt_parent"].tolist() == [-1, -1, 5, 4] and np.diff(pr["slot_off"]).max() == 2100
    assert sorted(exp["conn_w"].tolist())[-3:] == [700, 700, 700]


def _tile_problem(rank, equal):
    """rows at entry one shorter than, equal to and one longer than the 256-entry sort tile, and one naming every other keyframe; target 0
    reaches keyframes 1-4 with th = 1, which re-sorts their whole rows (1 and 4 held target 0 already, with another weight)"""
    nkf = 300
    rng = np.random.RandomState(7)
    conn = [{} for _ in range(nkf)]
    for k, n, has0 in ((1, 255, True), (2, 256, False), (3, 257, False), (4, 299, True)):
        others = [b for b in rng.permutation(nkf).tolist() if b not in (0, k)][:n - has0] + ([0] if has0 else [])
        rng.shuffle(others)
        conn[k] = {b: (7 if equal else int(rng.randint(1, 6))) for b in others}
        if has0:
            conn[k][0] = 9                                           # (not the weight the target sends: the send changes it)
        assert len(conn[k]) == n
    return cc.flatten(nkf, [[0, 1, 2, 3, 4]], [0], [[0]], conn=conn, prev=[[]], flags=[1], rank=rank, th=1)


@pytest.mark.parametrize("rank", [None, "reversed"])
@pytest.mark.parametrize("equal", [False, True], ids=["weights1to5", "weightsEqual"])
def test_rows_around_the_sort_tile_and_a_full_row(rank, equal):
    pr = _tile_problem(None if rank is None else np.arange(300)[::-1], equal)
    exp = _both(pr, "tile rows")
    assert np.diff(exp["ord_off"]).tolist() == [4, 255, 257, 258, 299]
    if equal:                                                        # rank alone orders the old entries of a row: descending rank
        row = exp["ord_kf"][exp["ord_off"][2]:exp["ord_off"][3]]
        r = (lambda k: k) if rank is None else (lambda k: 299 - k)
        old = [r(int(k)) for k in row if k != 0]
        assert old == sorted(old, reverse=True) and len(old) == 256


@pytest.mark.parametrize("th", [1, 15])
def test_counts_just_below_at_and_above_the_threshold(th):
    # target 0 shares th - 1, th and th + 1 points with keyframes 1, 2, 3; target 4 shares th - 1 with keyframe 1 and nothing else
    obs = [[0, 1]] * (th - 1) + [[0, 2]] * th + [[0, 3]] * (th + 1) + [[4, 1]] * (th - 1)
    held = lambda k: [p for p, ks in enumerate(obs) if k in ks]
    pr = cc.flatten(5, obs, [0, 4], [held(0), held(4)], prev=[[], []], flags=[1, 1], th=th)
    exp = _both(pr, "threshold %d" % th)
    assert exp["ord_kf"][:2].tolist() == [3, 2] and exp["ord_w"][:2].tolist() == [th + 1, th]
    assert exp["tgt_status"].tolist() == ([0, 1] if th == 1 else [0, 0]) and exp["tgt_parent"].tolist() == ([3, -1] if th == 1 else [3, 1])


def test_outputs_are_untouched_beyond_the_written_counts():
    import torch
    name, pr, exp = _seeded()[5]
    ntgt, nkf = len(pr["tgt_kf"]), pr["nkf"]
    caps = (nkf + 3, int(exp["counts"][1]) + 5, int(exp["counts"][2]) + 5, int(exp["counts"][3]) + 5)
    sizes = dict(aff_kf=caps[0], conn_off=caps[0] + 1, conn_kf=caps[1], conn_w=caps[1], ord_off=caps[0] + 1, ord_kf=caps[2], ord_w=caps[2], link_kf=caps[3])
    written = dict(aff_kf=exp["counts"][0], conn_off=exp["counts"][0] + 1, conn_kf=exp["counts"][1], conn_w=exp["counts"][1], ord_off=exp["counts"][0] + 1,
                   ord_kf=exp["counts"][2], ord_w=exp["counts"][2], link_kf=exp["counts"][3])
    out = {k: np.full(n, POISON, np.int32) for k, n in sizes.items()}
    h = _host(pr, caps=caps, out=out)
    _same(h, exp, name)
    for k, n in written.items():
        assert (out[k][n:] == POISON).all() and (out[k][:n] != POISON).all(), k
    dout = {k: torch.full((n,), POISON, dtype=torch.int32).cuda() for k, n in sizes.items()}
    d = _device_raw(pr, caps=caps, out=dout)
    _same(_trim(d), exp, name)
    for k, n in written.items():
        v = dout[k].cpu().numpy()
        assert (v[n:] == POISON).all() and (v[:n] != POISON).all(), k


@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_each_capacity_one_too_small(which):
    import torch
    name, pr, exp = _seeded()[3]
    assert all(int(c) >= 2 for c in exp["counts"])
    caps = [int(c) for c in exp["counts"]]
    caps[which] -= 1
    sizes = dict(aff_kf=caps[0], conn_off=caps[0] + 1, conn_kf=caps[1], conn_w=caps[1], ord_off=caps[0] + 1, ord_kf=caps[2], ord_w=caps[2], link_kf=caps[3],
                 tgt_status=len(pr["tgt_kf"]), tgt_parent=len(pr["tgt_kf"]), link_off=len(pr["tgt_kf"]) + 1)
    out = {k: np.full(n, POISON, np.int32) for k, n in sizes.items()}
    h = _host(pr, caps=tuple(caps), out=out, check=False)
    assert h["rc"] == ECAP and np.array_equal(h["counts"], exp["counts"])
    for k in sizes:                                                  # only the wanted counts are written
        assert (out[k] == POISON).all(), k
    from ceres_mono_orb_slam2_amd._lib import OrbHipError
    with pytest.raises(OrbHipError, match="capacit"):
        _host(pr, caps=tuple(caps))
    # the device form: the capacity's bit, the wanted counts, and nothing beyond the capacity (each output is the front of a longer tensor)
    base = {k: torch.full((n + 8,), POISON, dtype=torch.int32).cuda() for k, n in sizes.items()}
    d = _device_raw(pr, caps=tuple(caps), out={k: base[k][:n] for k, n in sizes.items()})
    assert int(d["status"].item()) == 4 << which and np.array_equal(d["counts"].cpu().numpy(), exp["counts"])
    for k, n in sizes.items():
        assert (base[k].cpu().numpy()[n:] == POISON).all(), k
    # what fits below the capacity is what the full call gives
    full = dict(aff_kf=exp["aff_kf"], conn_kf=exp["conn_kf"], conn_w=exp["conn_w"], ord_kf=exp["ord_kf"], ord_w=exp["ord_w"], link_kf=exp["link_kf"])
    for k, v in full.items():
        assert np.array_equal(base[k].cpu().numpy()[:sizes[k]], v[:sizes[k]]), k


def test_nullable_arguments():
    name, pr, exp = _seeded()[1]
    # no link outputs although the previous lists are given; no previous lists at all
    for q in (dict(pr), dict(pr, prev_off=None, prev_kf=None)):
        e = dict(exp, link_off=None, link_kf=None, counts=np.array(list(exp["counts"][:3]) + [0], np.int32))
        _same(_host(q, links=False), e, "no links host")
        _same(_device(q, links=False), e, "no links device")
    # no flags, no bad points, no rank: as zeros, zeros and the index order
    q = dict(pr, tgt_flags=None, pt_bad=None, kf_rank=None)
    z = dict(pr, tgt_flags=np.zeros_like(pr["tgt_flags"]), pt_bad=np.zeros_like(pr["pt_bad"]), kf_rank=np.arange(pr["nkf"], dtype=np.int32))
    e = npc.connections(z)
    assert (e["tgt_parent"] == -1).all() and not np.array_equal(e["ord_kf"], exp["ord_kf"])
    _same(_host(q), e, "nullable inputs host")
    _same(_device(q), e, "nullable inputs device")
    _same(_device(z), e, "explicit defaults device")
    # no targets: nothing is written but the counts and the closing offsets
    q = dict(pr, tgt_kf=pr["tgt_kf"][:0], tgt_flags=None, slot_off=np.zeros(1, np.int32), slot_pt=pr["slot_pt"][:0], prev_off=np.zeros(1, np.int32), prev_kf=pr["prev_kf"][:0])
    _both(q, "no targets")


def test_device_form_out_of_range_entries_set_status_and_the_call_completes():
    name, pr, exp = _seeded()[2]
    nkf, mid = pr["nkf"], lambda k: len(pr[k]) // 2
    for key, value, bit in (("slot_pt", 10 ** 6, 2), ("slot_pt", -5, 2), ("obs_kf", nkf, 2), ("obs_kf", -1, 2), ("tgt_kf", nkf + 3, 2), ("tgt_kf", -2, 2),
                            ("conn_kf", nkf, 2), ("conn_kf", -9, 2), ("prev_kf", 10 ** 5, 2), ("kf_rank", nkf, 2), ("kf_rank", -1, 2),
                            ("slot_off", 10 ** 7, 1), ("obs_off", -9, 1), ("conn_off", 10 ** 8, 1), ("prev_off", -3, 1)):
        q = dict(pr); q[key] = pr[key].copy(); q[key][mid(key)] = value
        d = _device(q)
        assert d["status"] & bit, (key, value)
        assert 0 <= d["counts"][0] <= nkf and set(d["tgt_status"].tolist()) <= {0, 1}
    q = dict(pr); q["tgt_kf"] = pr["tgt_kf"].copy(); q["tgt_kf"][0] = pr["tgt_kf"][1]                # a duplicate target
    assert _device(q)["status"] & 2
    q = dict(pr); q["kf_rank"] = pr["kf_rank"].copy(); q["kf_rank"][0] = pr["kf_rank"][1]            # not a permutation
    assert _device(q)["status"] & 2
    # an absent slot is a slot that is not there: the same answer as with a null slot in its place; an absent table entry likewise
    q = dict(pr); q["slot_pt"] = pr["slot_pt"].copy()
    s = int(np.nonzero(pr["slot_pt"] >= 0)[0][3]); q["slot_pt"][s] = pr["npts"]
    w = dict(pr); w["slot_pt"] = pr["slot_pt"].copy(); w["slot_pt"][s] = -1
    _same(_device(q), npc.connections(w), "absent slot")
    e = 0                                                            # (the first entry of the first row that is not empty)
    q = dict(pr); q["conn_kf"] = pr["conn_kf"].copy(); q["conn_kf"][e] = nkf
    row = int(np.searchsorted(pr["conn_off"], e, side="right") - 1)
    w = dict(pr); w["conn_kf"] = np.delete(pr["conn_kf"], e); w["conn_w"] = np.delete(pr["conn_w"], e); w["conn_off"] = pr["conn_off"].copy(); w["conn_off"][row + 1:] -= 1
    _same(_device(q), npc.connections(w), "absent table entry")
    d = _device(pr)
    _same(d, exp, "a clean call afterwards")
    assert d["status"] == 0


def test_links_with_and_without_the_previous_lists():
    name, pr, exp = _seeded()[6]
    assert exp["counts"][3] >= 5
    # empty previous lists: every non-target key of a target's map is a new link, unless an earlier target's send re-sorted its list first
    q = dict(pr, prev_off=np.zeros(len(pr["tgt_kf"]) + 1, np.int32), prev_kf=np.zeros(0, np.int32))
    e = _both(q, "empty previous lists")
    assert e["counts"][3] > exp["counts"][3]
    _same(e, exp, "the tables do not depend on prev", [k for k in KEYS[:10] if k != "counts"])


def test_two_calls_on_one_workspace_give_identical_results():
    import torch
    (_, pa, ea), (_, pb, eb) = _seeded()[7], _seeded()[8]
    big = max(_device_raw(p)["_workspace"].numel() for p in (pa, pb))
    ws = torch.full((big,), 0x5A, dtype=torch.uint8).cuda()          # (a dirty workspace: every call clears what it reads)
    for pr, exp in ((pa, ea), (pb, eb), (pa, ea), (pa, ea)):
        _same(_trim(_device_raw(pr, workspace=ws)), exp, "shared workspace")

"""Problems for orbl_keyframe_culling: the hand-worked cases (a)-(i) with their expected outputs written out, and the seeded
generator with its configurations.  TEST INFRASTRUCTURE (the problem layout is that of tests/npculling.py)."""
import numpy as np


def flatten(nkf, obs, slots, cand, flags, pt_bad=None, pt_nobs=None):
    """obs[p] = [(keyframe, level), ...], slots[k] = [(point, level), ...] -> the flattened problem"""
    npts = len(obs)
    obs_off = np.zeros(npts + 1, np.int32)
    for p in range(npts):
        obs_off[p + 1] = obs_off[p] + len(obs[p])
    flat = [o for l in obs for o in l]
    slot_off = np.zeros(len(cand) + 1, np.int32)
    sl = []
    for c, k in enumerate(cand):
        sl += slots[k]
        slot_off[c + 1] = len(sl)
    return dict(nkf=nkf, npts=npts, cand_kf=np.array(cand, np.int32).reshape(-1), cand_flags=np.array(flags, np.uint8).reshape(-1),
                slot_off=slot_off, slot_pt=np.array([s[0] for s in sl], np.int32), slot_level=np.array([s[1] for s in sl], np.int32),
                obs_off=obs_off, obs_kf=np.array([o[0] for o in flat], np.int32), obs_level=np.array([o[1] for o in flat], np.int32),
                pt_bad=None if pt_bad is None else np.array(pt_bad, np.uint8), pt_nobs=None if pt_nobs is None else np.array(pt_nobs, np.int32))


def make(seed, nkf, npts, span, q, ncand=None, lvl_jit=2, long_pt=0):
    r = np.random.default_rng(seed)
    obs = [[] for _ in range(npts)]; slots = [[] for _ in range(nkf)]
    for p in range(npts):
        c = r.integers(0, nkf); w = r.integers(1, span + 1); base = r.integers(0, 7)
        lo, hi, qq = (0, nkf, 1.0) if p < long_pt else (max(0, c - w), min(nkf, c + w + 1), q)
        for k in range(lo, hi):
            if r.random() < qq:
                l = int(np.clip(base + r.integers(-lvl_jit, lvl_jit + 1), 0, 7))
                obs[p].append((k, l)); slots[k].append((p, l))
    for k in range(nkf):
        perm = r.permutation(len(slots[k])); slots[k] = [slots[k][i] for i in perm]
    cand = list(r.permutation(nkf - 1))[: (ncand or nkf - 1)]
    # flags: 1 if k == 0 else (2 if r.random() < 0.1 else 0), drawn in cand order
    flags = [1 if k == 0 else (2 if r.random() < 0.1 else 0) for k in cand]
    return flatten(nkf, obs, slots, [int(k) for k in cand], flags)


CONFIGS = {
    "tiny": (dict(nkf=8, npts=60, span=8, q=1.0, lvl_jit=1), (1, 2, 3, 5)),
    "small": (dict(nkf=24, npts=600, span=12, q=0.95, lvl_jit=1), (0, 1, 2, 3, 4, 5)),
    "mid": (dict(nkf=64, npts=1500, span=10, q=0.9, lvl_jit=1), (0, 1, 2, 3, 4, 5)),
    "wide": (dict(nkf=140, npts=3000, span=8, q=0.8, lvl_jit=2, long_pt=2), (0, 1, 2, 3)),
}
FAT = dict(nkf=6, npts=5000, span=6, q=1.0)                      # keyframes with more slots than one workgroup pass (1024); seed 0 culls nothing
FAT_CULL = dict(nkf=7, npts=5000, span=6, q=1.0, lvl_jit=0)      # the same with one level per point: seed 0 culls one keyframe, 370 points turn bad


def seeded():
    """[(name, problem)] for every configuration and seed"""
    return [("%s-%d" % (name, s), make(s, **kw)) for name, (kw, seeds) in CONFIGS.items() for s in seeds]


# ------------------------------------------------------------------------------------------------ hand-worked cases
# A map is given by the keyframe -> level dict of every point; the slots of a keyframe are its points in point order (a consistent
# map) unless a case lists them itself.  th_obs = 3, ratio = 0.9 throughout.  `expect`: culled, n_redundant, n_map_points per
# candidate; the points that end bad; the (point, keyframe) observations that end erased; nobs of every point at the end.

def _case(nkf, points, cand, flags, expect, slots=None, pt_nobs=None):
    obs = [sorted(d.items()) for d in points]
    sl = [[(p, d[k]) for p, d in enumerate(points) if k in d] for k in range(nkf)]
    for k, v in (slots or {}).items():
        sl[k] = v
    pr = flatten(nkf, obs, sl, cand, flags, pt_nobs=pt_nobs)
    erased = np.zeros(len(pr["obs_kf"]), np.uint8)
    for p, k in expect["erased"]:
        e = [e for e in range(pr["obs_off"][p], pr["obs_off"][p + 1]) if pr["obs_kf"][e] == k]
        assert len(e) == 1
        erased[e[0]] = 1
    bad = np.zeros(len(points), np.uint8); bad[list(expect["bad"])] = 1
    exp = dict(culled=np.array(expect["culled"], np.uint8).reshape(-1), n_redundant=np.array(expect["n_redundant"], np.int32).reshape(-1),
               n_map_points=np.array(expect["n_map_points"], np.int32).reshape(-1), pt_bad=bad, pt_nobs=np.array(expect["nobs"], np.int32).reshape(-1),
               obs_erased=erased)
    return pr, exp


def _seen(kfs, level=0):
    return {k: level for k in kfs}


def hand_cases():
    """{name: (problem, expected outputs)}"""
    C = {}
    # (a) nothing culled: 4 keyframes, 6 points; keyframe 3 is the current one.  p0-p3 have 3 observations (not > 3), p4 and p5 have 4
    #     with 3 other observers: every candidate sees 5 points of which 2 are redundant, 2 > 4.5 is false.
    pts = [_seen([0, 1, 2]), _seen([1, 2, 3]), _seen([0, 2, 3]), _seen([0, 1, 3]), _seen([0, 1, 2, 3]), _seen([0, 1, 2, 3])]
    C["a_nothing_culled"] = _case(4, pts, [0, 1, 2], [0, 0, 0], dict(culled=[0, 0, 0], n_redundant=[2, 2, 2], n_map_points=[5, 5, 5], bad=[], erased=[],
                                                                 nobs=[3, 3, 3, 3, 4, 4]))
    # (b) the 0.9 boundary: keyframe 0 with R redundant points (seen by 0, 1, 2, 3) and one that is not (seen by 0, 1, 2)
    #     9 of 10: 9 > 9.0 is false.  19 of 20: 19 > 18.0, culled - every redundant point drops to 3 observations, the other one to 2: bad.
    pts = [_seen([0, 1, 2, 3])] * 9 + [_seen([0, 1, 2])]
    C["b_9_of_10"] = _case(4, pts, [0], [0], dict(culled=[0], n_redundant=[9], n_map_points=[10], bad=[], erased=[], nobs=[4] * 9 + [3]))
    pts = [_seen([0, 1, 2, 3])] * 10
    C["b_10_of_10"] = _case(4, pts, [0], [0], dict(culled=[1], n_redundant=[10], n_map_points=[10], bad=[], erased=[(p, 0) for p in range(10)], nobs=[3] * 10))
    pts = [_seen([0, 1, 2, 3])] * 19 + [_seen([0, 1, 2])]
    C["b_19_of_20"] = _case(4, pts, [0], [0], dict(culled=[1], n_redundant=[19], n_map_points=[20], bad=[19],
                                                   erased=[(p, 0) for p in range(20)] + [(19, 1), (19, 2)], nobs=[3] * 19 + [2]))
    # (c) the level rule: keyframe 0 sees both points at level 2.  p0: observers at 3, 3, 3 (= level + 1: all count) - redundant.
    #     p1: observers at 3, 3, 4 (level + 2 does not count): 2 < 3.
    pts = [{0: 2, 1: 3, 2: 3, 3: 3}, {0: 2, 1: 3, 2: 3, 3: 4}]
    C["c_level_rule"] = _case(4, pts, [0], [0], dict(culled=[0], n_redundant=[1], n_map_points=[2], bad=[], erased=[], nobs=[4, 4]))
    # (d) Observations() == th_obs is not `>`: both points have three other observers, p0 reports 3 observations, p1 reports 4
    pts = [_seen([0, 1, 2, 3]), _seen([0, 1, 2, 3])]
    C["d_observation_count"] = _case(4, pts, [0], [0], dict(culled=[0], n_redundant=[1], n_map_points=[2], bad=[], erased=[], nobs=[3, 4]), pt_nobs=[3, 4])
    # (e) order dependence: 4 points seen by A = 0, B = 1 and by 2, 3 (keyframe 4 is the current one).  Whoever comes first has 3 other
    #     observers on every point and goes; the points are left with 3 observations (not > 3) and the second one stays.
    pts = [_seen([0, 1, 2, 3])] * 4
    C["e_order_AB"] = _case(5, pts, [0, 1], [0, 0], dict(culled=[1, 0], n_redundant=[4, 0], n_map_points=[4, 4], bad=[], erased=[(p, 0) for p in range(4)], nobs=[3] * 4))
    C["e_order_BA"] = _case(5, pts, [1, 0], [0, 0], dict(culled=[1, 0], n_redundant=[4, 0], n_map_points=[4, 4], bad=[], erased=[(p, 1) for p in range(4)], nobs=[3] * 4))
    # (f) cascade: A = 0 sees p0-p9 (with 2, 3, 4: redundant) and p10 (with 1, 2): 10 > 9.9, culled.  p10 drops to 2 observations and turns
    #     bad.  C = 1 sees p10 and p11-p19 (with 2, 3, 4, 5: redundant): 9 of 10 before (kept), 9 of 9 after p10 is gone: culled.
    pts = [_seen([0, 2, 3, 4])] * 10 + [_seen([0, 1, 2])] + [_seen([1, 2, 3, 4, 5])] * 9
    C["f_cascade"] = _case(6, pts, [0, 1], [0, 0], dict(culled=[1, 1], n_redundant=[10, 9], n_map_points=[11, 9], bad=[10],
                                                      erased=[(p, 0) for p in range(11)] + [(10, 1), (10, 2)] + [(p, 1) for p in range(11, 20)],
                                                      nobs=[3] * 10 + [2] + [4] * 9))
    # (g) do_not_erase_: the map of (e) with A flagged.  A is reported culled and stays; B still sees A's observations and goes.
    pts = [_seen([0, 1, 2, 3])] * 4
    C["g_do_not_erase"] = _case(5, pts, [0, 1], [2, 0], dict(culled=[1, 1], n_redundant=[4, 4], n_map_points=[4, 4], bad=[], erased=[(p, 1) for p in range(4)], nobs=[3] * 4))
    # (h) id_ == 0: the map of (e) with A the first keyframe of the map - skipped with zeros, B goes
    C["h_id_zero"] = _case(5, pts, [0, 1], [1, 0], dict(culled=[0, 1], n_redundant=[0, 4], n_map_points=[0, 4], bad=[], erased=[(p, 1) for p in range(4)], nobs=[3] * 4))
    # (i) degenerate inputs: no candidate; a candidate without slots (keyframe 4 observes nothing) between two others; p0 twice in A's slots
    #     (5 slots, 5 redundant; p0 loses ONE observation)
    C["i_no_candidate"] = _case(5, pts, [], [], dict(culled=[], n_redundant=[], n_map_points=[], bad=[], erased=[], nobs=[4] * 4))
    C["i_no_slots"] = _case(5, pts, [4, 0, 1], [0, 0, 0], dict(culled=[0, 1, 0], n_redundant=[0, 4, 0], n_map_points=[0, 4, 4], bad=[], erased=[(p, 0) for p in range(4)], nobs=[3] * 4))
    C["i_point_twice"] = _case(5, pts, [0, 1], [0, 0], dict(culled=[1, 0], n_redundant=[5, 0], n_map_points=[5, 4], bad=[], erased=[(p, 0) for p in range(4)], nobs=[3] * 4),
                               slots={0: [(0, 0), (1, 0), (0, 0), (2, 0), (3, 0)]})
    return C

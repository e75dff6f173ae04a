"""Restatement of LocalMapping::KeyFrameCulling (src/LocalMapping.cc:576-637) with the state changes of KeyFrame::SetBadFlag
(src/KeyFrame.cc:460-480), MapPoint::EraseObservation (src/MapPoint.cc:140-162) and MapPoint::SetBadFlag (:174-191), monocular
case, over the flattened arrays of orbl_keyframe_culling.  Written from the reference text with the reference's containers
(a dict per point for std::map<KeyFrame*, size_t>, a list per keyframe for map_points_), one candidate after the other: TEST
INFRASTRUCTURE, no relation to how the kernels are organised.

A problem is a dict: nkf, npts, cand_kf[ncand], cand_flags[ncand] (bit 0: id_ == 0, bit 1: do_not_erase_), slot_off[ncand + 1],
slot_pt[nslots], slot_level[nslots], obs_off[npts + 1], obs_kf[nobs], obs_level[nobs], pt_bad (None: all good), pt_nobs (None: the
list lengths)."""
import numpy as np


def culling(pr, th_obs=3, ratio=0.9, sequential=True):
    """-> dict(culled uint8[ncand], n_redundant int32[ncand], n_map_points int32[ncand], pt_bad uint8[npts], pt_nobs int32[npts],
    obs_erased uint8[nobs]).  sequential=False skips SetBadFlag (every candidate sees the initial state): used ONLY to show that the
    test problems tell the two apart."""
    npts = int(pr["npts"])
    obs_off = np.asarray(pr["obs_off"], np.int64)
    nobs_total = int(obs_off[-1])
    bad = [False] * npts if pr.get("pt_bad") is None else [bool(b) for b in pr["pt_bad"]]
    nobs = [int(obs_off[p + 1] - obs_off[p]) for p in range(npts)] if pr.get("pt_nobs") is None else [int(n) for n in pr["pt_nobs"]]
    # observations_ of every point: keyframe -> (octave of that keyframe's keypoint, entry); bad points keep no list
    observations = []
    for p in range(npts):
        d = {}
        if not bad[p]:
            for e in range(int(obs_off[p]), int(obs_off[p + 1])):
                d[int(pr["obs_kf"][e])] = (int(pr["obs_level"][e]), e)
        observations.append(d)
    erased = np.zeros(nobs_total, np.uint8)
    ncand = len(pr["cand_kf"])
    culled = np.zeros(ncand, np.uint8); n_red = np.zeros(ncand, np.int32); n_mp = np.zeros(ncand, np.int32)

    def set_bad_flag_point(p):                                       # MapPoint::SetBadFlag (:174-191)
        bad[p] = True
        for _, e in observations[p].values():
            erased[e] = 1
        observations[p] = {}                                         # (EraseMapPointMatch in every observer: `bad` hides the slots)

    def erase_observation(p, k):                                     # MapPoint::EraseObservation (:140-162), mvuRight < 0
        if k in observations[p]:
            erased[observations[p][k][1]] = 1
            del observations[p][k]
            nobs[p] -= 1
            if nobs[p] <= 2:
                set_bad_flag_point(p)

    for c in range(ncand):
        k = int(pr["cand_kf"][c]); flags = int(pr["cand_flags"][c])
        if flags & 1:                                                # (:588) id_ == 0
            continue
        slots = range(int(pr["slot_off"][c]), int(pr["slot_off"][c + 1]))
        redundant = 0; points = 0
        for s in slots:                                              # (:595-631)
            p = int(pr["slot_pt"][s])
            if bad[p]:
                continue
            points += 1
            if nobs[p] > th_obs:
                level = int(pr["slot_level"][s])
                n = 0
                for kf, (lvl, _) in observations[p].items():
                    if kf == k:
                        continue
                    if lvl <= level + 1:
                        n += 1
                        if n >= th_obs:
                            break
                if n >= th_obs:
                    redundant += 1
        n_red[c] = redundant; n_mp[c] = points
        if float(redundant) > ratio * float(points):                # (:633) int > double
            culled[c] = 1
            if sequential and not flags & 2:                         # KeyFrame::SetBadFlag (:460-480); do_not_erase_: nothing changes
                for s in slots:
                    p = int(pr["slot_pt"][s])
                    if not bad[p]:
                        erase_observation(p, k)
    return dict(culled=culled, n_redundant=n_red, n_map_points=n_mp, pt_bad=np.array(bad, np.uint8).reshape(npts),
                pt_nobs=np.array(nobs, np.int32).reshape(npts), obs_erased=erased)

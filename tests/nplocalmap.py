"""Restatement of Tracking::UpdateLocalMap (reference src/Tracking.cc:838-977: UpdateLocalKeyFrames :874-977, UpdateLocalPoints
:847-872) and of what SearchLocalPoints (:793-826) fixes from that state, with Python dicts and lists, one statement per reference
statement.  It keeps its own track_reference_for_frame_ marks; the reference's pointer order (std::map<KeyFrame*, int>) is emulated
by iterating in kf_rank; the children come in the order the problem lists them (std::set<KeyFrame*> order).  TEST INFRASTRUCTURE: it
shares no code with the library or with ceres_mono_orb_slam2_amd/tracking.py.

A problem is a dict of the tables include/orbslam_hip.h names (numpy arrays): frame_pt, seen_pt, prev_local_kf, pt_bad, pt_nobs, obs_off,
obs_kf, pt_Xw, pt_normal, pt_min_dist, pt_max_dist, pt_desc, kf_bad, kf_rank (or None), kf_parent, cov_off, cov_kf, child_off, child_kf,
kf_slot_off, kf_slot_pt."""
import numpy as np

OK, NO_VOTES = 0, 1
FRAME_ID = 7                      # current_frame_.id_: any value no mark carries at entry


def _row(off, val, i):
    return [int(v) for v in val[off[i]:off[i + 1]]]


def update_local_map(pr, cap_pt=None):
    """Returns dict(frame_pt_out, local_kf, n_local_kf, ref_kf, status, votes, local_pt, n_local_pt, mp_Xw, mp_normal, mp_min_dist,
    mp_max_dist, mp_desc (n_local_pt rows each), mp_state[cap_pt or n_local_pt], slot_Xw, slot_state, kf_mark, pt_mark (the
    track_reference_for_frame_ == current id flags), paths = dict(no_votes, stop80, parent_break))."""
    nkf, npts = len(pr["kf_bad"]), len(pr["pt_bad"])
    rank = list(range(nkf)) if pr.get("kf_rank") is None else [int(r) for r in pr["kf_rank"]]
    kf_track_ref = [0] * nkf                                        # KeyFrame::track_reference_for_frame_
    pt_track_ref = [0] * npts                                       # MapPoint::track_reference_for_frame_
    frame = [int(p) for p in pr["frame_pt"]]                        # current_frame_.map_points_
    local_keyframes = [int(k) for k in pr["prev_local_kf"]]         # local_keyframes_ as the frame before left it
    paths = dict(no_votes=False, stop80=False, parent_break=False)

    # ---- UpdateLocalKeyFrames (:874-977)
    counter = {}                                                    # keyframeCounter
    for i in range(len(frame)):
        if frame[i] >= 0:
            mp = frame[i]
            if not pr["pt_bad"][mp]:
                for kf in _row(pr["obs_off"], pr["obs_kf"], mp):
                    counter[kf] = counter.get(kf, 0) + 1
            else:
                frame[i] = -1
    ref_kf = -1                                                     # -1: reference_keyframe_ is left alone
    status = OK
    if not counter:                                                 # (:894-896) return
        status = NO_VOTES
        paths["no_votes"] = True
    else:
        mx = 0
        keyframe_max = None
        local_keyframes = []
        for kf in sorted(counter, key=lambda k: rank[k]):           # the map iterates in pointer order
            if pr["kf_bad"][kf]:
                continue
            if counter[kf] > mx:
                mx = counter[kf]
                keyframe_max = kf
            local_keyframes.append(kf)
            kf_track_ref[kf] = FRAME_ID
        it, it_end = 0, len(local_keyframes)                        # itKF, itEndKF: the end is taken before the appends (:924-925)
        while it != it_end:
            if len(local_keyframes) > 80:
                paths["stop80"] = True
                break
            kf = local_keyframes[it]
            for nb in _row(pr["cov_off"], pr["cov_kf"], kf):        # GetBestCovisibilityKeyFrames(10)
                if not pr["kf_bad"][nb]:
                    if kf_track_ref[nb] != FRAME_ID:
                        local_keyframes.append(nb)
                        kf_track_ref[nb] = FRAME_ID
                        break
            for ch in _row(pr["child_off"], pr["child_kf"], kf):    # GetChilds()
                if not pr["kf_bad"][ch]:
                    if kf_track_ref[ch] != FRAME_ID:
                        local_keyframes.append(ch)
                        kf_track_ref[ch] = FRAME_ID
                        break
            parent = int(pr["kf_parent"][kf])
            if parent >= 0:
                if kf_track_ref[parent] != FRAME_ID:
                    local_keyframes.append(parent)
                    kf_track_ref[parent] = FRAME_ID
                    paths["parent_break"] = True
                    break
            it += 1
        if keyframe_max is not None:
            ref_kf = keyframe_max

    # ---- UpdateLocalPoints (:847-872)
    local_map_points = []
    for kf in local_keyframes:
        for mp in _row(pr["kf_slot_off"], pr["kf_slot_pt"], kf):
            if mp < 0:
                continue
            if pt_track_ref[mp] == FRAME_ID:
                continue
            if not pr["pt_bad"][mp]:
                local_map_points.append(mp)
                pt_track_ref[mp] = FRAME_ID

    # ---- SearchLocalPoints (:793-826): which points are searched, and what the frame's slots hold
    last_seen = [False] * npts                                      # last_seen_frame_id_ == current_frame_.id_
    for mp in pr["seen_pt"]:
        last_seen[int(mp)] = True
    for i in range(len(frame)):
        if frame[i] >= 0:
            if pr["pt_bad"][frame[i]]:
                frame[i] = -1
            else:
                last_seen[frame[i]] = True
    n = len(local_map_points)
    mp_state = np.zeros(n if cap_pt is None else cap_pt, np.uint8)
    for j, mp in enumerate(local_map_points[:len(mp_state)]):
        if last_seen[mp]:
            continue
        if pr["pt_bad"][mp]:
            continue
        mp_state[j] = 1 if pr["pt_nobs"][mp] > 0 else 3
    slot_state = np.zeros(len(frame), np.uint8)
    slot_Xw = np.zeros((len(frame), 3), np.float64)
    for i, mp in enumerate(frame):
        if mp >= 0:
            slot_state[i] = 1 if pr["pt_nobs"][mp] > 0 else 3
            slot_Xw[i] = pr["pt_Xw"][mp]
    votes = np.zeros(nkf, np.int32)
    for kf, c in counter.items():
        votes[kf] = c
    lp = np.array(local_map_points, np.int32).reshape(-1)
    return dict(frame_pt_out=np.array(frame, np.int32).reshape(-1), local_kf=np.array(local_keyframes, np.int32).reshape(-1), n_local_kf=len(local_keyframes),
                ref_kf=ref_kf, status=status, votes=votes, local_pt=lp, n_local_pt=n,
                mp_Xw=np.asarray(pr["pt_Xw"], np.float64).reshape(-1, 3)[lp], mp_normal=np.asarray(pr["pt_normal"], np.float64).reshape(-1, 3)[lp],
                mp_min_dist=np.asarray(pr["pt_min_dist"], np.float32)[lp], mp_max_dist=np.asarray(pr["pt_max_dist"], np.float32)[lp],
                mp_desc=np.asarray(pr["pt_desc"], np.uint8).reshape(-1, 32)[lp], mp_state=mp_state, slot_Xw=slot_Xw, slot_state=slot_state,
                kf_mark=np.array([t == FRAME_ID for t in kf_track_ref], bool), pt_mark=np.array([t == FRAME_ID for t in pt_track_ref], bool), paths=paths)

"""KeyFrameDatabase on the device (csrc/orb_kfdb.inc, orbv_db_*) against the independent restatement tests/npkfdb.py: candidate lists with
their order, the whole trace (scores as float bit patterns) and the relocalisation state, identical for every query - no tolerance, no
case left out of any comparison."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import npkfdb  # noqa: E402

pytestmark = pytest.mark.gpu

ECAP, EINVAL = -4, -1


def _mods():
    from ceres_mono_orb_slam2_amd import KeyFrameDatabase, _lib, synth          # (the library is built by __graft_entry__.build())
    return KeyFrameDatabase, _lib, synth


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _same_trace(tr, ref, what):
    for k in ("n_sharing", "max_common", "min_common", "n_scored", "n_kept", "n_cand"):
        assert tr[k] == ref[k], (what, k, tr[k], ref[k])
    assert _bits(tr["best_acc"]) == _bits(ref["best_acc"]), (what, "best_acc", tr["best_acc"], ref["best_acc"])
    for k in ("kept_slot", "kept_best"):
        assert list(tr[k]) == list(ref[k]), (what, k)
    for k in ("kept_score", "kept_acc"):
        assert np.array_equal(_bits(tr[k]), _bits(ref[k])), (what, k)


def _replay_loop(seed, first_query=10, **kw):
    """The sequence replayed as LoopClosing does: min_score, query, add (and the covisibility rows the new keyframe changes)."""
    KeyFrameDatabase, _, synth = _mods()
    seq = synth.make_place_sequence(seed, **kw)
    db = KeyFrameDatabase(seq["n_words"]); ref = npkfdb.NpKeyFrameDatabase(seq["n_words"])
    nonempty = 0
    for i in range(seq["n_kf"]):
        bow = seq["bows"][i]
        con = synth.place_connected(seq, i, upto=i - 1)
        if i >= first_query:
            ms = db.min_score(bow, con); rms = ref.min_score(bow, con)
            assert _bits(ms) == _bits(rms), (i, ms, rms)
            cand, tr = db.detect_loop_candidates(bow, con, ms, i + 1, trace=True)
            rcand, rtr = ref.detect_loop_candidates(bow, con, rms, i + 1)
            assert list(cand) == rcand, (i, list(cand), rcand)
            _same_trace(tr, rtr, i)
            nonempty += len(rcand) > 0
        db.add(i, bow); ref.add(i, bow)
        for j in range(max(0, i - 10), i + 1):
            nb = synth.place_best_covisibles(seq, j, upto=i)
            db.set_best_covisibles(j, nb); ref.set_best_covisibles(j, nb)
    assert len(db) == seq["n_kf"]
    return nonempty


def test_loop_replay_300_keyframes():
    assert _replay_loop(3) >= 100


def test_loop_replay_5000_keyframes():
    assert _replay_loop(5, n_kf=5000, n_words=20000, n_feat=300, step=8, revisit=600) >= 1000


def _fixed_database(seed=11, n_kf=200, **kw):
    KeyFrameDatabase, _, synth = _mods()
    seq = synth.make_place_sequence(seed, n_kf=n_kf, revisit=0, **kw)
    db = KeyFrameDatabase(seq["n_words"]); ref = npkfdb.NpKeyFrameDatabase(seq["n_words"])
    for i in range(n_kf):
        db.add(i, seq["bows"][i]); ref.add(i, seq["bows"][i])
        nb = synth.place_best_covisibles(seq, i)
        db.set_best_covisibles(i, nb); ref.set_best_covisibles(i, nb)
    return seq, db, ref


def _reloc_queries(seq, n, seed):
    """Views of places of the sequence: a keyframe's BowVector with a share of its words dropped and a few foreign words mixed in; consecutive
    queries stay near each other, so neighbours of one query's kept keyframes carry the scores of the query before."""
    rng = np.random.default_rng(seed)
    out = []
    place = int(rng.integers(0, seq["n_kf"]))
    for _ in range(n):
        place = int(np.clip(place + rng.integers(-9, 10), 0, seq["n_kf"] - 1)) if rng.random() < 0.8 else int(rng.integers(0, seq["n_kf"]))
        w, v = seq["bows"][place]
        keep = rng.random(len(w)) < rng.uniform(0.5, 0.95)
        w2 = np.union1d(w[keep], rng.integers(0, seq["n_words"], 40).astype(np.uint32))
        v2 = np.where(np.isin(w2, w), 0.0, 1e-3); v2[np.isin(w2, w)] = v[np.isin(w, w2)]
        out.append((w2.astype(np.uint32), v2 / np.abs(v2).sum()))
    return out


def _to_device(queries):
    import torch
    off = np.zeros(len(queries) + 1, np.int32); off[1:] = np.cumsum([len(w) for w, _ in queries])
    w = np.concatenate([q[0] for q in queries]).astype(np.uint32).view(np.int32); v = np.concatenate([q[1] for q in queries])
    return torch.from_numpy(off).cuda(), torch.from_numpy(w).cuda(), torch.from_numpy(v).cuda()


def test_relocalisation_single_and_batched_with_stale_scores():
    import torch
    seq, db, ref = _fixed_database()
    _, db2, _ = _fixed_database()                                     # the same database, queried singly where `db` is queried in batches
    queries = _reloc_queries(seq, 8 + 1 + 7 + 64, 5)
    slots = np.arange(seq["n_kf"])
    qid = 1

    def check_state(d):
        q, s = d.get_state(slots); rq, rs = ref.get_state(slots)
        assert np.array_equal(q, rq) and np.array_equal(_bits(s), _bits(rs))

    for bow in queries[:8]:                                           # singly, with the trace
        cand, tr = db.detect_relocalization_candidates(bow, qid, trace=True)
        assert list(db2.detect_relocalization_candidates(bow, qid)) == list(cand)
        rcand, rtr = ref.detect_relocalization_candidates(bow, qid)
        assert list(cand) == rcand and len(rcand) > 0
        _same_trace(tr, rtr, qid)
        check_state(db)
        qid += 1
    pos = 8
    for Q in (1, 7, 64):
        batch = queries[pos:pos + Q]; pos += Q
        info, cand = db.detect_relocalization_candidates_batch_device(*_to_device(batch), qid)
        torch.cuda.synchronize()
        res = db.batch_results(info, cand)
        for k, bow in enumerate(batch):
            single, str_ = db2.detect_relocalization_candidates(bow, qid + k, trace=True)
            rcand, rtr = ref.detect_relocalization_candidates(bow, qid + k)
            assert list(res[k][0]) == rcand == list(single), (Q, k)
            for f in ("n_sharing", "max_common", "min_common", "n_scored", "n_kept", "n_cand"):
                assert res[k][1][f] == rtr[f] == str_[f], (Q, k, f)
            assert _bits(res[k][1]["best_acc"]) == _bits(rtr["best_acc"]) == _bits(str_["best_acc"])
        qid += Q
        check_state(db); check_state(db2)                             # the state a batch leaves = the state the single calls leave
    assert ref.stale_reads > 0, "the stale-score path was never taken"


def test_interleaved_program():
    """add / erase / set_best_covisibles / loop and relocalisation queries from a seeded random program, compared after every step."""
    KeyFrameDatabase, _, synth = _mods()
    seq = synth.make_place_sequence(21, n_kf=120, n_words=3000, n_feat=200, step=10, revisit=30)
    db = KeyFrameDatabase(seq["n_words"]); ref = npkfdb.NpKeyFrameDatabase(seq["n_words"])
    rng = np.random.default_rng(7)
    live = set(); lq = rq = 0; nq = 0
    for step in range(700):
        op = rng.random()
        s = int(rng.integers(0, seq["n_kf"]))
        if op < 0.35:
            if s not in live:
                db.add(s, seq["bows"][s]); ref.add(s, seq["bows"][s]); live.add(s)
        elif op < 0.45:
            db.erase(s); ref.erase(s); live.discard(s)
        elif op < 0.6:
            nb = [int(x) for x in rng.choice(seq["n_kf"], int(rng.integers(0, 11)), replace=False)]
            db.set_best_covisibles(s, nb); ref.set_best_covisibles(s, nb)
        elif op < 0.8:
            lq += int(rng.integers(1, 4))
            con = [j for j in synth.place_connected(seq, s) if rng.random() < 0.7]
            ms = np.float32(rng.uniform(0.0, 0.08))
            cand, tr = db.detect_loop_candidates(seq["bows"][s], con, ms, lq, trace=True)
            rcand, rtr = ref.detect_loop_candidates(seq["bows"][s], con, ms, lq)
            assert list(cand) == rcand, step
            _same_trace(tr, rtr, step); nq += len(rcand) > 0
        else:
            rq += int(rng.integers(1, 4))
            cand, tr = db.detect_relocalization_candidates(seq["bows"][s], rq, trace=True)
            rcand, rtr = ref.detect_relocalization_candidates(seq["bows"][s], rq)
            assert list(cand) == rcand, step
            _same_trace(tr, rtr, step); nq += len(rcand) > 0
        assert len(db) == len(ref) == len(live)
        q, sc = db.get_state(np.arange(seq["n_kf"])) if step > 0 and db._hi >= seq["n_kf"] else (None, None)
        if q is not None:
            r_q, r_s = ref.get_state(np.arange(seq["n_kf"]))
            assert np.array_equal(q, r_q) and np.array_equal(_bits(sc), _bits(r_s)), step
    assert nq > 50
    db.clear(); ref.clear()
    assert len(db) == 0 and len(db.detect_relocalization_candidates(seq["bows"][0], 1)) == 0


def test_empty_outcomes():
    KeyFrameDatabase, _, synth = _mods()
    seq = synth.make_place_sequence(2, n_kf=40, n_words=2000, n_feat=100, step=10, revisit=0)
    db = KeyFrameDatabase(seq["n_words"])
    bow = seq["bows"][0]
    c, tr = db.detect_loop_candidates(bow, [], 0.0, 1, trace=True)                       # an empty database
    assert len(c) == 0 and tr["n_sharing"] == 0
    assert len(db.detect_relocalization_candidates(bow, 1)) == 0
    for i in range(20):
        db.add(i, seq["bows"][i])
    unused = np.setdiff1d(np.arange(seq["n_words"]), np.concatenate([seq["bows"][i][0] for i in range(20)]))
    foreign = (unused[-3:].astype(np.uint32), np.full(3, 1.0 / 3))                        # words no stored keyframe has
    c, tr = db.detect_loop_candidates(foreign, [], 0.0, 2, trace=True)                    # shares no word
    assert len(c) == 0 and tr["n_sharing"] == 0
    c, tr = db.detect_relocalization_candidates(foreign, 2, trace=True)
    assert len(c) == 0 and tr["n_sharing"] == 0
    c, tr = db.detect_loop_candidates(bow, list(range(20)), 0.0, 3, trace=True)           # every sharing keyframe is connected
    assert len(c) == 0 and tr["n_sharing"] == 0 and tr["n_scored"] == 0
    c, tr = db.detect_loop_candidates(bow, [], 1.5, 4, trace=True)                        # nothing reaches minScore
    assert len(c) == 0 and tr["n_sharing"] > 0 and tr["n_scored"] > 0 and tr["n_kept"] == 0
    with pytest.raises(Exception, match="query_id"):                                      # a stale id
        db.detect_loop_candidates(bow, [], 0.0, 4)
    with pytest.raises(Exception, match="already in the database"):
        db.add(3, bow)


def test_one_word_and_more_words_than_the_lds_tile():
    """BowVectors of 1 word and of more words than k_kfdb_scan's LDS tile (4096 query words): past the tile the query is searched in global
    memory, and the result is the same list."""
    KeyFrameDatabase, _, _ = _mods()
    from ceres_mono_orb_slam2_amd.keyframe_database import LDS_WORDS
    rng = np.random.default_rng(4)
    n_words = 30000
    db = KeyFrameDatabase(n_words); ref = npkfdb.NpKeyFrameDatabase(n_words)

    def bow(n):
        w = np.sort(rng.choice(n_words, n, replace=False)).astype(np.uint32); v = rng.uniform(0.1, 1.0, n)
        return w, v / v.sum()
    sizes = [1, 1, 2, 63, 64, 65, LDS_WORDS - 1, LDS_WORDS, LDS_WORDS + 1, 6000, 9000, 500, 700, 900, 1200]
    bows = [bow(n) for n in sizes]
    bows[1] = (bows[8][0][:1].copy(), np.array([1.0]))                 # a one-word keyframe that shares its word with the big ones' first
    for i, b in enumerate(bows):
        db.add(i, b); ref.add(i, b)
        nb = [j for j in range(len(bows)) if j != i][:10]
        db.set_best_covisibles(i, nb); ref.set_best_covisibles(i, nb)
    qid = 0
    for b in bows + [bow(LDS_WORDS + 777), bow(1)]:
        qid += 1
        c, tr = db.detect_relocalization_candidates(b, qid, trace=True); rc, rtr = ref.detect_relocalization_candidates(b, qid)
        assert list(c) == rc
        _same_trace(tr, rtr, ("reloc", qid))
        c, tr = db.detect_loop_candidates(b, [2], 0.0, qid, trace=True); rc, rtr = ref.detect_loop_candidates(b, [2], 0.0, qid)
        assert list(c) == rc
        _same_trace(tr, rtr, ("loop", qid))
        assert _bits(db.min_score(b, range(len(bows)))) == _bits(ref.min_score(b, range(len(bows))))
    # erase / add cycles of a large keyframe until the arena has been compacted (erased BowVectors are more than half of it): the keyframe
    # goes to the back of every list each time, and nothing else moves
    for r in range(140):
        db.erase(10); ref.erase(10); db.add(10, bows[10]); ref.add(10, bows[10])
        if r % 20 == 19:
            db.erase(6); ref.erase(6); db.add(6, bows[6]); ref.add(6, bows[6])
    for b in bows:
        qid += 1
        c, tr = db.detect_relocalization_candidates(b, qid, trace=True); rc, rtr = ref.detect_relocalization_candidates(b, qid)
        assert list(c) == rc
        _same_trace(tr, rtr, ("after compaction", qid))


def test_capacity_errors_leave_the_outputs_untouched():
    import torch
    KeyFrameDatabase, lib, synth = _mods()
    seq = synth.make_place_sequence(13, n_kf=80, revisit=0, n_words=3000, n_feat=200, step=10)
    db = KeyFrameDatabase(seq["n_words"])
    for i in range(80):                                              # no neighbour table: every kept keyframe stands for itself
        db.add(i, seq["bows"][i])
    L = lib.load()
    w, ia, _ = np.intersect1d(seq["bows"][39][0], seq["bows"][41][0], return_indices=True)       # what keyframes 39 and 41 both see: 39, 40, 41 come back
    bow = (w, seq["bows"][39][1][ia] / seq["bows"][39][1][ia].sum())
    w = np.ascontiguousarray(bow[0], np.uint32); v = np.ascontiguousarray(bow[1])
    full, trf = db.detect_relocalization_candidates(bow, 1, trace=True)
    assert len(full) >= 2 and trf["n_kept"] >= 2
    cand = np.full(64, -77, np.int32); n = C.c_int(-5)
    rc = L.orbv_db_detect_relocalization_candidates(db._h, lib.ptr(w), lib.ptr(v), len(w), 2, lib.ptr(cand), len(full) - 1, C.byref(n), None)
    assert rc == ECAP and n.value == -5 and (cand == -77).all()
    # trace capacity
    info = lib.DbQueryInfo(); info.n_kept = -9
    ks = np.full(256, -77, np.int32)
    t = lib.DbTrace(C.pointer(info), lib.ptr(ks), None, None, None, trf["n_kept"] - 1, 0)
    rc = L.orbv_db_detect_relocalization_candidates(db._h, lib.ptr(w), lib.ptr(v), len(w), 3, lib.ptr(cand), 64, C.byref(n), C.byref(t))
    assert rc == ECAP and n.value == -5 and (cand == -77).all() and (ks == -77).all() and info.n_kept == -9
    # begin: kept capacity
    rc = L.orbv_db_detect_relocalization_candidates_begin(db._h, lib.ptr(w), lib.ptr(v), len(w), 4, lib.ptr(ks), trf["n_kept"] - 1, C.byref(n))
    assert rc == ECAP and n.value == -5 and (ks == -77).all()
    # exact capacity is enough
    rc = L.orbv_db_detect_relocalization_candidates(db._h, lib.ptr(w), lib.ptr(v), len(w), 5, lib.ptr(cand), len(full), C.byref(n), None)
    assert rc == 0 and list(cand[:n.value]) == list(full)
    # the batched entry: the query that does not fit gets the status and none of its candidates; the others are complete
    unused = np.setdiff1d(np.arange(seq["n_words"]), np.concatenate([b[0] for b in seq["bows"]]))
    qs = [bow, (unused[-1:].astype(np.uint32), np.array([1.0])), seq["bows"][10]]      # (the second one shares no word with the database)
    off, dw, dv = _to_device(qs)
    d_info = torch.empty((3, 8), dtype=torch.int32, device="cuda"); d_cand = torch.full((3, 1), -77, dtype=torch.int32, device="cuda")
    ws = torch.empty((db.workspace_bytes(3),), dtype=torch.uint8, device="cuda")
    rc = L.orbv_db_detect_relocalization_candidates_batch_device(db._h, 3, lib.ptr(off), lib.ptr(dw), lib.ptr(dv), 6, lib.ptr(d_info), lib.ptr(d_cand), 1,
                                                                 lib.ptr(ws), ws.numel(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    hi = d_info.cpu().numpy(); hc = d_cand.cpu().numpy()
    assert hi[0, 5] == ECAP and hi[0, 4] == len(full) and hc[0, 0] == -77
    assert hi[1, 5] == 0 and hi[1, 4] == 0 and hc[1, 0] == -77
    # a workspace that is too small is refused before anything is enqueued
    rc = L.orbv_db_detect_relocalization_candidates_batch_device(db._h, 3, lib.ptr(off), lib.ptr(dw), lib.ptr(dv), 20, lib.ptr(d_info), lib.ptr(d_cand), 1,
                                                                 lib.ptr(ws), ws.numel() - 1, None)
    assert rc == EINVAL


def test_host_entry_device_entry_and_begin_finish_agree():
    import torch
    KeyFrameDatabase, lib, synth = _mods()
    seq, db, ref = _fixed_database(seed=17, n_kf=150, n_words=5000, n_feat=400, step=12)
    dbs = [db, _fixed_database(seed=17, n_kf=150, n_words=5000, n_feat=400, step=12)[1], _fixed_database(seed=17, n_kf=150, n_words=5000, n_feat=400, step=12)[1]]
    queries = _reloc_queries(seq, 12, 3)
    rng = np.random.default_rng(1)
    n_nonempty = 0
    for k, bow in enumerate(queries):
        qid = k + 1
        con = [int(x) for x in rng.choice(150, 20, replace=False)]
        ms = np.float32(0.02)
        for kind in ("reloc", "loop"):
            if kind == "reloc":
                a, atr = dbs[0].detect_relocalization_candidates(bow, qid, trace=True)
                info, cand = dbs[1].detect_relocalization_candidates_batch_device(*_to_device([bow]), qid)
                kept = dbs[2].detect_relocalization_candidates_begin(bow, qid)
                rc_, rtr = ref.detect_relocalization_candidates(bow, qid)
            else:
                a, atr = dbs[0].detect_loop_candidates(bow, con, ms, qid, trace=True)
                d_con = torch.tensor(con, dtype=torch.int32, device="cuda"); d_coff = torch.tensor([0, len(con)], dtype=torch.int32, device="cuda")
                info, cand = dbs[1].detect_loop_candidates_batch_device(*_to_device([bow]), d_coff, d_con, torch.tensor([ms], dtype=torch.float32, device="cuda"), qid)
                kept = dbs[2].detect_loop_candidates_begin(bow, con, ms, qid)
                rc_, rtr = ref.detect_loop_candidates(bow, con, ms, qid)
            torch.cuda.synchronize()
            b = dbs[1].batch_results(info, cand)[0][0]
            assert list(kept) == list(atr["kept_slot"])
            rows = [synth.place_best_covisibles(seq, int(s)) for s in kept]      # the same rows as the resident table
            c, ctr = dbs[2].detect_candidates_finish(rows, trace=True)
            assert list(a) == list(b) == list(c) == rc_, (k, kind)
            _same_trace(atr, rtr, (k, kind)); _same_trace(ctr, rtr, (k, kind))
            n_nonempty += len(a) > 0
    assert n_nonempty >= 12
    # rows that differ from the resident table are honoured by finish
    bow = queries[0]
    kept = dbs[2].detect_relocalization_candidates_begin(bow, 100)
    rows = [[int(s) + 1] if int(s) + 1 < 150 else [] for s in kept]
    c, ctr = dbs[2].detect_candidates_finish(rows, trace=True)
    rc_, rtr = ref.detect_relocalization_candidates(bow, 100, rows=rows)
    # (ref's reloc ids ran 1..12; dbs[2] saw the same queries, so the states agree)
    assert list(c) == rc_
    _same_trace(ctr, rtr, "rows")
    with pytest.raises(Exception, match="no query pending"):
        dbs[2].detect_candidates_finish(rows)


def test_hand_worked_database():
    """tests/kfdbcases.py: first-touch order with a tie broken by add order, a keyframe that went to the back after erase and add, the boundary of
    int(5 * 0.8f), >= at minScore, strict > at 0.75f * bestAccScore, the duplicate removal - expected values worked out by hand."""
    import kfdbcases
    KeyFrameDatabase, _, _ = _mods()
    db = KeyFrameDatabase(64)
    kfdbcases.build(db)
    assert len(db) == 7
    cand, tr = db.detect_loop_candidates(kfdbcases.QUERY, kfdbcases.CONNECTED, kfdbcases.MIN_SCORE, 7, trace=True)
    kfdbcases.check(cand, tr, kfdbcases.LOOP_EXPECTED)
    cand, tr = db.detect_relocalization_candidates(kfdbcases.QUERY, 3, trace=True)
    kfdbcases.check(cand, tr, kfdbcases.RELOC_EXPECTED)
    q, s = db.get_state(range(7))
    assert list(q) == [3] * 7 and list(s) == [0, 1, 0, 0, 0, 0, 0]

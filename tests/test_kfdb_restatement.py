"""CPU checks of the KeyFrameDatabase restatement (tests/npkfdb.py) itself: its score against orbv_score_l1 and a hand-worked value, a hand-worked
database that pins the order and every gate, the generator's inputs (every gate does something), and the stale relocalisation score."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kfdbcases  # noqa: E402
import npkfdb  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build_hip()
    from ceres_mono_orb_slam2_amd import _lib
    return _lib


def _host_score(lib, a, b):
    w1 = np.ascontiguousarray(a[0], np.uint32); v1 = np.ascontiguousarray(a[1], np.float64)
    w2 = np.ascontiguousarray(b[0], np.uint32); v2 = np.ascontiguousarray(b[1], np.float64)
    return float(lib.load().orbv_score_l1(lib.ptr(w1), lib.ptr(v1), len(w1), lib.ptr(w2), lib.ptr(v2), len(w2)))


def test_score_is_the_library_host_score_bit_for_bit(lib):
    rng = np.random.default_rng(0)

    def bow(n, n_words=5000):
        w = np.sort(rng.choice(n_words, n, replace=False)).astype(np.uint32); v = rng.uniform(0.01, 1, n)
        return w, v / v.sum()
    pairs = [(bow(int(rng.integers(1, 1500))), bow(int(rng.integers(1, 1500)))) for _ in range(40)]
    big = bow(1200)
    for n in (1, 5, 400, 1200):                                   # nested: one BowVector's words are a subset of the other's
        idx = np.sort(rng.choice(1200, n, replace=False))
        sub = (big[0][idx], rng.uniform(0.01, 1, n))
        pairs += [(big, sub), (sub, big)]
    pairs.append((big, big))
    pairs.append((bow(10), (np.zeros(0, np.uint32), np.zeros(0))))
    for a, b in pairs:
        s = npkfdb.score_l1(a, b)
        assert s == _host_score(lib, a, b) == npkfdb.score_l1_merge(a, b)            # the same double, hence the same float


def test_score_three_word_example():
    # common words 1 and 3: (|.5 - .25| - .5 - .25) + (|.25 - .25| - .25 - .25) = -.5 + -.5 = -1  ->  -(-1) / 2 = 0.5
    q = (np.array([1, 3, 7], np.uint32), np.array([0.5, 0.25, 0.25])); k = (np.array([1, 3, 5], np.uint32), np.array([0.25, 0.25, 0.5]))
    assert npkfdb.score_l1(q, k) == 0.5 and npkfdb.score_l1_merge(q, k) == 0.5


def test_float_truncation_of_min_common_words():
    """int(maxCommonWords * 0.8f): the float product, truncated.  At 5 it sits on the boundary (0.8f is a little above 0.8, and 5 * 0.8f rounds to
    4.0f exactly: 4 common words are not enough, as the hand-worked database below shows).  For every count a map can reach the float and the
    double product truncate to the same integer; the restatement and the device still form it as the reference does."""
    F = np.float32
    assert int(F(5) * F(0.8)) == 4 and int(F(8) * F(0.8)) == 6 and int(F(10) * F(0.8)) == 8 and int(F(1) * F(0.8)) == 0
    assert F(5) * F(0.8) == F(4) and float(F(0.8)) > 0.8
    assert all(int(F(m) * F(0.8)) == int(m * 0.8) for m in range(1, 20000))


def test_hand_worked_database():
    db = npkfdb.NpKeyFrameDatabase(64)
    kfdbcases.build(db)
    assert len(db) == 7
    assert db.inv[10] == [2, 1, 3] and db.inv[12] == [5, 4, 0, 1, 3]              # the erased and re-added keyframe 3 is at the back
    cand, tr = db.detect_loop_candidates(kfdbcases.QUERY, kfdbcases.CONNECTED, kfdbcases.MIN_SCORE, 7)
    kfdbcases.check(cand, tr, kfdbcases.LOOP_EXPECTED)
    assert db.n_loop_words[1] == 1 and db.n_loop_query[1] == 0                      # the connected keyframe: reset at every touch, never stamped
    cand, tr = db.detect_relocalization_candidates(kfdbcases.QUERY, 3)
    kfdbcases.check(cand, tr, kfdbcases.RELOC_EXPECTED)
    q, s = db.get_state(range(7))
    assert list(q) == [3] * 7 and list(s) == [0, 1, 0, 0, 0, 0, 0]


def _replay(seq, synth, first_query=10):
    db = npkfdb.NpKeyFrameDatabase(seq["n_words"])
    out = []
    for i in range(seq["n_kf"]):
        con = synth.place_connected(seq, i, upto=i - 1)
        if i >= first_query:
            ms = db.min_score(seq["bows"][i], con)
            cand, tr = db.detect_loop_candidates(seq["bows"][i], con, ms, i + 1)
            out.append((i, cand, tr))
        db.add(i, seq["bows"][i])
        for j in range(max(0, i - 10), i + 1):
            db.set_best_covisibles(j, synth.place_best_covisibles(seq, j, upto=i))
    return out


def test_generator_exercises_every_gate():
    from ceres_mono_orb_slam2_amd import synth
    seq = synth.make_place_sequence(3, n_kf=300, n_words=10000, n_feat=1000, step=25, flip=0.25, revisit=60)
    for w, v in seq["bows"]:
        assert (np.diff(w.astype(np.int64)) > 0).all() and w.max() < seq["n_words"] and abs(np.abs(v).sum() - 1) < 1e-12
    res = _replay(seq, synth)
    n = len(res)
    assert n == 290
    for i, cand, tr in res:
        tp = seq["true_place"][i]
        if tp >= 0:
            assert any(abs(c - tp) <= 10 for c in cand), (i, cand)               # every revisit query returns a true place
            assert not set(cand) & set(synth.place_connected(seq, i))            # ... through keyframes that are not connected to it
    assert sum(seq["true_place"] >= 0) == 60
    assert sum(tr["n_scored"] < tr["n_sharing"] for _, _, tr in res) >= n / 4
    assert sum(tr["n_kept"] < tr["n_scored"] for _, _, tr in res) >= n / 4
    assert sum(len(c) < tr["n_kept"] for _, c, tr in res) >= n / 4
    assert sum(len(c) > 0 for _, c, _ in res) >= n / 2


def test_stale_relocalisation_score_is_reached_and_matters():
    """A neighbour that the query stamped but did not score adds the reloc_score_ an earlier query left on it (:282-288).  The sequence reaches
    that path, and reading the stale value as 0 instead changes at least one returned list."""
    from ceres_mono_orb_slam2_amd import synth
    seq = synth.make_place_sequence(11, n_kf=200, revisit=0)
    dbs = [npkfdb.NpKeyFrameDatabase(seq["n_words"]), npkfdb.NpKeyFrameDatabase(seq["n_words"], stale_as_zero=True)]
    for db in dbs:
        for i in range(seq["n_kf"]):
            db.add(i, seq["bows"][i]); db.set_best_covisibles(i, synth.place_best_covisibles(seq, i))
    rng = np.random.default_rng(5)
    differ = 0; place = 100
    for q in range(1, 81):
        place = int(np.clip(place + rng.integers(-9, 10), 0, 199))
        w, v = seq["bows"][place]
        keep = rng.random(len(w)) < 0.7
        bow = (w[keep], v[keep] / v[keep].sum())
        a, _ = dbs[0].detect_relocalization_candidates(bow, q); b, _ = dbs[1].detect_relocalization_candidates(bow, q)
        differ += a != b
    assert dbs[0].stale_reads > 0
    assert differ > 0

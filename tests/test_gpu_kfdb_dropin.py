"""KeyFrameDatabaseT (csrc/compat/orbslam_keyframedatabase.h) over the mock data model: tests/cpp/test_keyframedatabase_dropin.cpp runs a
program of add / erase / clear and loop / relocalisation queries through the reference's interface; the KeyFrame* vectors it returns and
the query fields it writes back to the keyframes equal the restatement's (tests/npkfdb.py), scores as float bit patterns."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import npkfdb  # noqa: E402

pytestmark = pytest.mark.gpu


def _bow_text(bow):
    return "%d %s" % (len(bow[0]), " ".join("%d %s" % (int(w), float(v).hex()) for w, v in zip(*bow)))


def _bits(x):
    return int(np.float32(x).view(np.uint32))


def test_dropin_matches_restatement(tmp_path):
    from ceres_mono_orb_slam2_amd import _lib, synth
    exe = tmp_path / "test_keyframedatabase_dropin"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "test_keyframedatabase_dropin.cpp"), "-o", str(exe), _lib.LIB_PATH, "-lpthread",
                           "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH), "-Wl,-rpath,/opt/rocm/lib"])
    seq = synth.make_place_sequence(8, n_kf=160, n_words=4000, n_feat=300, step=10, revisit=40)
    n = seq["n_kf"]
    rng = np.random.default_rng(3)
    ref = npkfdb.NpKeyFrameDatabase(seq["n_words"])
    lines = ["V %d" % seq["n_words"]] + ["K %d %s" % (i, _bow_text(seq["bows"][i])) for i in range(n)]
    expected = []                                    # per query: (kind, id, candidates, snapshot of the fields)
    frame_id = 0
    in_db = set()

    def snapshot(kind, qid, cand):
        ref._reserve(n)
        expected.append((kind, qid, list(cand), ref.n_loop_query[:n].copy(), ref.n_loop_words[:n].copy(), ref.loop_score[:n].copy(), ref.reloc_query[:n].copy(),
                         ref.n_reloc_words[:n].copy(), ref.reloc_score[:n].copy()))

    def reloc(place):
        nonlocal frame_id
        frame_id += int(rng.integers(1, 5))
        w, v = seq["bows"][place]
        keep = rng.random(len(w)) < 0.7
        bow = (w[keep], v[keep] / v[keep].sum())
        lines.append("R %d %s" % (frame_id, _bow_text(bow)))
        cand, _ = ref.detect_relocalization_candidates(bow, frame_id)
        snapshot("R", frame_id, cand)

    for i in range(n):                               # the LoopClosing order: (min score from the library), query, add
        con = synth.place_connected(seq, i, upto=i - 1)
        for j in range(max(0, i - 45), i + 1):       # the covisibility graph as of keyframe i (ordered, best first)
            lst = synth.place_connected(seq, j, upto=i)
            lines.append("C %d %d %s" % (j, len(lst), " ".join(map(str, lst))))
            ref.set_best_covisibles(j, lst[:10])
        if i >= 10:
            ms = ref.min_score(seq["bows"][i], [j for j in con if j in in_db])
            lines.append("L %d %s" % (i, float(ms).hex()))
            cand, _ = ref.detect_loop_candidates(seq["bows"][i], con, ms, i)
            snapshot("L", i, cand)
        lines.append("A %d" % i); ref.add(i, seq["bows"][i]); in_db.add(i)
        if i % 7 == 3 and i > 20:                    # culling: a recent keyframe leaves (KeyFrame::SetBadFlag), now and then it comes back
            j = i - int(rng.integers(2, 9))
            lines.append("E %d" % j); ref.erase(j); in_db.discard(j)
            if rng.random() < 0.3:
                lines.append("A %d" % j); ref.add(j, seq["bows"][j]); in_db.add(j)
        if i > 30 and i % 3 == 0:                    # a lost frame near a place seen before; consecutive ones stay close (stale scores)
            reloc(int(np.clip(i - 20 + rng.integers(-6, 7), 0, i)))
    assert ref.stale_reads > 0
    path = tmp_path / "program.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.split()[-1] == "OK", r.stdout[-2000:] + r.stderr[-1000:]
    out = r.stdout.splitlines()
    pos = 0
    nonempty = 0
    for kind, qid, cand, lq, lw, ls, rq, rw, rs in expected:
        q = out[pos].split(); pos += 1
        assert q[0] == "Q" and [int(x) for x in q[2:]] == cand, (kind, qid, q, cand)
        nonempty += len(cand) > 0
        for k in range(n):
            f = out[pos].split(); pos += 1
            assert f[0] == "F" and int(f[1]) == k
            got = [int(x) for x in f[2:8]]
            assert got[0] == lq[k] and got[2] == _bits(ls[k]), (kind, qid, k, "loop fields")
            if kind == "L" and lq[k] == qid:         # (a connected keyframe's n_loop_words_ is left alone: see the header)
                assert got[1] == lw[k], (kind, qid, k, "n_loop_words_")
            assert got[3] == rq[k] and got[4] == rw[k] and got[5] == _bits(rs[k]), (kind, qid, k, "reloc fields")
    assert out[pos] == "OK" and nonempty > len(expected) // 3
    # GetBestCovisibilityKeyFrames was asked of kept keyframes only: far fewer calls than keyframes x queries
    calls = sum(int(out[pos - n + k].split()[8]) for k in range(n))
    assert 0 < calls < len(expected) * n // 4

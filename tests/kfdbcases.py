"""A hand-worked KeyFrameDatabase of seven keyframes (all values dyadic, so every score and every float sum below is exact and was worked out
by hand), shared by the CPU test of the restatement and the GPU test of the device code.

The query has the words 10 .. 17 with value 1/8 each.  A keyframe that shares k of them with value v scores k * (1/8 + v - |1/8 - v|) / 2:
5 words at 1/8 -> 0.625, 5 at 1/16 -> 0.3125, 5 at 1/32 -> 0.15625.

  name slot  words                     value  common  first shared word
  F    3     10 11 12 13 14            1/8    5       10   added FIRST, then erased and added again LAST: it goes to the back of every list
  A    5     12 13 14 15 16            1/16   5       12   added before C: the tie on word 12 is broken by add order, not by slot number
  B    2     10 13 14 15 16            1/16   5       10
  C    4     12 13 14 15 17            1/16   5       12
  D    0     11 12 13 14 30            1/8    4       11   4 > int(5 * 0.8f) = 4 is false: in the sharing list, not scored
  E    1     10 .. 17                  1/8    8       -    connected to the query: neither listed nor counted into maxCommonWords (8 would give
                                                           minCommonWords 6 and nothing would be scored)
  G    6     13 14 15 16 17            1/32   5       13   scored (0.15625) but below minScore = 0.3125; B, A, C sit ON minScore and are kept (>=)

Sharing list (first touch): word 10: B, F; word 11: D; word 12: A, C; word 13: G  ->  [2, 3, 0, 5, 4, 6].
Kept: [2, 3, 5, 4] with scores [.3125, .625, .3125, .3125].
Neighbours and accumulation (bestAccScore starts at minScore):
  B: [F, D, E]   D was not scored, E was not stamped          acc .3125 + .625 = .9375          best F
  F: [A, C]                                                    acc .625 + .3125 + .3125 = 1.25   best F (no neighbour is strictly better)
  A: [F, B]                                                    acc .3125 + .625 + .3125 = 1.25   best F
  C: [A, B, G]   G contributes: stamped and above minCommon    acc .3125 * 3 + .15625 = 1.09375  best C (ties do not replace)
bestAccScore 1.25, minScoreToRetain .9375: B sits ON it and is dropped (strict >); F kept; A names F again: dropped as a duplicate; C kept.
Candidates [3, 4]."""
import numpy as np

QUERY = (np.arange(10, 18, dtype=np.uint32), np.full(8, 0.125))
MIN_SCORE = np.float32(0.3125)
CONNECTED = [1]


def _kf(words, value):
    return np.array(words, np.uint32), np.full(len(words), value)


KEYFRAMES = {3: _kf([10, 11, 12, 13, 14], 1 / 8), 5: _kf([12, 13, 14, 15, 16], 1 / 16), 2: _kf([10, 13, 14, 15, 16], 1 / 16), 4: _kf([12, 13, 14, 15, 17], 1 / 16),
             0: _kf([11, 12, 13, 14, 30], 1 / 8), 1: _kf(list(range(10, 18)), 1 / 8), 6: _kf([13, 14, 15, 16, 17], 1 / 32)}
NEIGHBOURS = {2: [3, 0, 1], 3: [5, 4], 5: [3, 2], 4: [5, 2, 6]}


def build(db):
    """The program on any object with add / erase / set_best_covisibles."""
    db.add(3, KEYFRAMES[3])
    for s in (5, 2, 4, 0, 1):
        db.add(s, KEYFRAMES[s])
    db.erase(3); db.erase(9)                      # (9 is not in the database: nothing happens)
    db.add(3, KEYFRAMES[3])
    db.add(6, KEYFRAMES[6])
    for s, nb in NEIGHBOURS.items():
        db.set_best_covisibles(s, nb)


LOOP_EXPECTED = dict(cand=[3, 4], n_sharing=6, max_common=5, min_common=4, n_scored=5, n_kept=4, n_cand=2, best_acc=np.float32(1.25), kept_slot=[2, 3, 5, 4],
                     kept_score=[0.3125, 0.625, 0.3125, 0.3125], kept_acc=[0.9375, 1.25, 1.25, 1.09375], kept_best=[3, 3, 3, 4])
# The same database asked as a relocalisation query: E counts (8 common words), minCommonWords = int(8 * 0.8f) = 6, only E is scored (1.0); E has
# no neighbours: candidates [1].  All seven keyframes are stamped with the query id; only E's reloc_score changes.
RELOC_EXPECTED = dict(cand=[1], n_sharing=7, max_common=8, min_common=6, n_scored=1, n_kept=1, n_cand=1, best_acc=np.float32(1.0), kept_slot=[1], kept_score=[1.0],
                      kept_acc=[1.0], kept_best=[1])


def check(cand, tr, exp):
    assert list(cand) == exp["cand"], (list(cand), exp["cand"])
    for k in ("n_sharing", "max_common", "min_common", "n_scored", "n_kept", "n_cand"):
        assert tr[k] == exp[k], (k, tr[k], exp[k])
    assert np.float32(tr["best_acc"]) == exp["best_acc"]
    assert list(tr["kept_slot"]) == exp["kept_slot"] and list(tr["kept_best"]) == exp["kept_best"]
    assert [float(x) for x in tr["kept_score"]] == exp["kept_score"] and [float(x) for x in tr["kept_acc"]] == exp["kept_acc"]

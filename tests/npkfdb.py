"""Independent restatement of the reference's KeyFrameDatabase (src/KeyFrameDatabase.cc) and of LoopClosing::DetectLoop's minScore
(src/LoopClosing.cc:127-139), written as the reference writes it: one list per word, walked word by word, with the reference's
per-keyframe fields (n_loop_query_, n_loop_words_, loop_score_, reloc_query_, n_reloc_words_, reloc_score_) held explicitly.  It is
NOT a scan over keyframes like the device code: the two must be able to disagree.  `float` of the reference is np.float32 here.

A keyframe is a slot index.  The fields live in arrays indexed by slot and survive erase / add, as the fields of a KeyFrame object do;
clear() forgets everything (the reference's Reset deletes the keyframes).  reloc_score_ starts at 0.0f (the reference leaves it
uninitialised).  A word's list is a Python list in push_back order; the walk over one list is done with array operations on that list
(a keyframe occurs at most once in it, so the per-element updates of the reference do not interact inside one list)."""
import numpy as np

F = np.float32


def score_l1(bow1, bow2):
    """L1Scoring::score (lib/DBoW2/DBoW2/ScoringObject.cpp:23-68): double sum over the common words in ascending id, -s/2."""
    w1, v1 = bow1; w2, v2 = bow2
    _, i1, i2 = np.intersect1d(np.asarray(w1), np.asarray(w2), assume_unique=True, return_indices=True)      # ascending word id
    vi = np.asarray(v1, np.float64)[i1]; wi = np.asarray(v2, np.float64)[i2]
    terms = (np.abs(vi - wi) - np.abs(vi)) - np.abs(wi)          # element-wise IEEE doubles, as the reference's expression
    s = 0.0
    for t in terms.tolist():                                     # score += ..., in word order
        s += t
    return -s / 2.0


def score_l1_merge(bow1, bow2):
    """The same as the reference's two-iterator merge, literally (slow; the tests pin score_l1 to it)."""
    w1, v1 = bow1; w2, v2 = bow2
    a = b = 0; s = 0.0
    while a < len(w1) and b < len(w2):
        if w1[a] == w2[b]:
            vi = float(v1[a]); wi = float(v2[b])
            s += abs(vi - wi) - abs(vi) - abs(wi); a += 1; b += 1
        elif w1[a] < w2[b]:
            a += 1
        else:
            b += 1
    return -s / 2.0


class NpKeyFrameDatabase:
    def __init__(self, n_words, stale_as_zero=False):
        self.n_words = n_words
        self.stale_as_zero = stale_as_zero          # test switch: read a stale reloc_score_ as 0 (to show that the quirk matters)
        self.clear()

    def clear(self):
        self.inv = {}                                # word -> list of slots, push_back order
        self.bow = {}                                # slot -> (words, values) of the keyframes in the database
        self.best_covis = {}                         # slot -> list of at most 10 slots
        self.stale_reads = 0                         # neighbours read with a score of an earlier query that was not 0
        self._cap = 0
        self.n_loop_query = np.zeros(0, np.int64); self.n_loop_words = np.zeros(0, np.int64); self.loop_score = np.zeros(0, F)
        self.reloc_query = np.zeros(0, np.int64); self.n_reloc_words = np.zeros(0, np.int64); self.reloc_score = np.zeros(0, F)
        self.reloc_scored_in = np.zeros(0, np.int64)     # bookkeeping of the restatement only: the query that wrote reloc_score

    def _reserve(self, n):
        if n <= self._cap:
            return
        cap = max(n, 2 * self._cap, 64)
        for name in ("n_loop_query", "n_loop_words", "loop_score", "reloc_query", "n_reloc_words", "reloc_score", "reloc_scored_in"):
            a = getattr(self, name); b = np.zeros(cap, a.dtype); b[:len(a)] = a; setattr(self, name, b)
        self._cap = cap

    def __len__(self):
        return len(self.bow)

    def add(self, slot, bow):
        assert slot not in self.bow
        self._reserve(slot + 1)
        w = np.asarray(bow[0]).astype(np.int64); v = np.asarray(bow[1], np.float64)
        self.bow[slot] = (w, v)
        for x in w.tolist():
            self.inv.setdefault(x, []).append(slot)

    def erase(self, slot):
        if slot not in self.bow:
            return
        for x in self.bow[slot][0].tolist():
            self.inv[x].remove(slot)
        del self.bow[slot]

    def set_best_covisibles(self, slot, neigh):
        self._reserve(slot + 1)
        self.best_covis[slot] = [int(x) for x in neigh]

    def get_state(self, slots):
        self._reserve(max(list(slots) + [0]) + 1)
        s = np.asarray(slots, np.int64)
        return self.reloc_query[s].copy(), self.reloc_score[s].copy()

    def min_score(self, bow, slots):
        m = F(1.0)
        for s in slots:
            sc = F(score_l1(bow, self.bow[s]))
            if sc < m:
                m = sc
        return m

    def _neighbours(self, slot, rows, i):
        return rows[i] if rows is not None else self.best_covis.get(slot, [])

    def detect_loop_candidates(self, bow, connected, min_score, qid, rows=None):
        """-> (candidates, trace).  rows: optional neighbour lists of the kept keyframes (else the stored best covisibles)."""
        min_score = F(min_score)
        connected = set(int(x) for x in connected)
        tr = dict(n_sharing=0, max_common=0, min_common=0, n_scored=0, n_kept=0, n_cand=0, best_acc=F(0), kept_slot=[], kept_score=[], kept_acc=[], kept_best=[])
        sharing = []
        for w in np.asarray(bow[0]).tolist():
            lst = self.inv.get(w)
            if not lst:
                continue
            lst = np.asarray(lst, np.int64)
            fresh = lst[self.n_loop_query[lst] != qid]                # if (n_loop_query_ != id) {
            if len(fresh):
                self.n_loop_words[fresh] = 0                          #   n_loop_words_ = 0;
                ok = fresh[[int(x) not in connected for x in fresh]] if connected else fresh
                self.n_loop_query[ok] = qid                           #   if (!connected.count(kf)) { n_loop_query_ = id; push_back }
                sharing.extend(ok.tolist())
            self.n_loop_words[lst] += 1                               # n_loop_words_++
        tr["n_sharing"] = len(sharing)
        if not sharing:
            return [], tr
        max_common = 0
        for s in sharing:
            if self.n_loop_words[s] > max_common:
                max_common = int(self.n_loop_words[s])
        min_common = int(F(max_common) * F(0.8))                      # int minCommonWords = maxCommonWords * 0.8f
        tr["max_common"] = max_common; tr["min_common"] = min_common
        sam = []
        for s in sharing:
            if self.n_loop_words[s] > min_common:
                tr["n_scored"] += 1
                sc = F(score_l1(bow, self.bow[s]))
                self.loop_score[s] = sc
                if sc >= min_score:
                    sam.append((sc, s))
        tr["n_kept"] = len(sam)
        if not sam:
            return [], tr
        acc_list = []
        best_acc = min_score
        for i, (sc, s) in enumerate(sam):
            best_score = sc; acc = sc; best = s
            for j in self._neighbours(s, rows, i):
                if j not in self.bow:                                 # (a neighbour that is not in the database contributes nothing)
                    continue
                if self.n_loop_query[j] == qid and self.n_loop_words[j] > min_common:
                    acc = F(acc + self.loop_score[j])
                    if self.loop_score[j] > best_score:
                        best = j; best_score = self.loop_score[j]
            acc_list.append((acc, best))
            if acc > best_acc:
                best_acc = acc
        return self._select(sam, acc_list, best_acc, tr)

    def detect_relocalization_candidates(self, bow, qid, rows=None):
        tr = dict(n_sharing=0, max_common=0, min_common=0, n_scored=0, n_kept=0, n_cand=0, best_acc=F(0), kept_slot=[], kept_score=[], kept_acc=[], kept_best=[])
        sharing = []
        for w in np.asarray(bow[0]).tolist():
            lst = self.inv.get(w)
            if not lst:
                continue
            lst = np.asarray(lst, np.int64)
            fresh = lst[self.reloc_query[lst] != qid]
            if len(fresh):
                self.n_reloc_words[fresh] = 0
                self.reloc_query[fresh] = qid
                sharing.extend(fresh.tolist())
            self.n_reloc_words[lst] += 1
        tr["n_sharing"] = len(sharing)
        if not sharing:
            return [], tr
        max_common = 0
        for s in sharing:
            if self.n_reloc_words[s] > max_common:
                max_common = int(self.n_reloc_words[s])
        min_common = int(F(max_common) * F(0.8))
        tr["max_common"] = max_common; tr["min_common"] = min_common
        sam = []
        for s in sharing:
            if self.n_reloc_words[s] > min_common:
                tr["n_scored"] += 1
                sc = F(score_l1(bow, self.bow[s]))
                self.reloc_score[s] = sc; self.reloc_scored_in[s] = qid
                sam.append((sc, s))
        tr["n_kept"] = len(sam)
        if not sam:
            return [], tr
        acc_list = []
        best_acc = F(0)
        for i, (sc, s) in enumerate(sam):
            best_score = sc; acc = sc; best = s
            for j in self._neighbours(s, rows, i):
                if j not in self.bow:
                    continue
                if self.reloc_query[j] != qid:
                    continue
                sj = self.reloc_score[j]                              # whatever the last query that scored j left there
                if self.reloc_scored_in[j] != qid:
                    if sj != 0:
                        self.stale_reads += 1
                    if self.stale_as_zero:
                        sj = F(0)
                acc = F(acc + sj)
                if sj > best_score:
                    best = j; best_score = sj
            acc_list.append((acc, best))
            if acc > best_acc:
                best_acc = acc
        return self._select(sam, acc_list, best_acc, tr)

    @staticmethod
    def _select(sam, acc_list, best_acc, tr):
        keep = F(F(0.75) * best_acc)                                  # minScoreToRetain
        added = set(); out = []
        for acc, best in acc_list:
            if acc > keep:
                if best not in added:
                    out.append(best); added.add(best)
        tr["best_acc"] = F(best_acc); tr["n_cand"] = len(out)
        tr["kept_slot"] = [s for _, s in sam]; tr["kept_score"] = [sc for sc, _ in sam]
        tr["kept_acc"] = [a for a, _ in acc_list]; tr["kept_best"] = [b for _, b in acc_list]
        return out, tr

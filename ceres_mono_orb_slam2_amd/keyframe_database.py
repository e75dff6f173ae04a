"""Host mirror of KeyFrameDatabase (reference src/KeyFrameDatabase.cc) over the HIP C ABI (include/orbslam_hip.h, orbv_db_*): the
loop and relocalisation candidates by a device scan of every stored BowVector.  A keyframe is a slot index; a BowVector is a pair
(ascending uint32 words, float64 values) as ORBVocabulary.transform returns it.  There is no CPU fallback."""
import ctypes as C

import numpy as np

from . import _lib

LDS_WORDS = 4096          # a query of more words is searched in global memory (slower, same result)


def _bow(bow):
    return np.ascontiguousarray(bow[0], np.uint32), np.ascontiguousarray(bow[1], np.float64)


def _info_dict(i):
    return {k: getattr(i, k) for k, _ in _lib.DbQueryInfo._fields_}


class KeyFrameDatabase:
    def __init__(self, vocabulary_or_n_words, device=0):
        self._L = _lib.load()
        n_words = getattr(vocabulary_or_n_words, "n_words", None)
        if n_words is None:
            n_words = int(vocabulary_or_n_words)
        self.n_words = int(n_words)
        self._h = C.c_void_p()
        _lib.check(self._L.orbv_db_create(self.n_words, int(device), C.byref(self._h)), "orbv_db_create")
        self._hi = 0          # highest slot touched + 1: the most any list can hold

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.orbv_db_destroy(self._h); self._h = None

    def __len__(self):
        return int(self._L.orbv_db_size(self._h))

    def add(self, slot, bow):
        w, v = _bow(bow)
        _lib.check(self._L.orbv_db_add(self._h, int(slot), _lib.ptr(w), _lib.ptr(v), len(w)), "orbv_db_add")
        self._hi = max(self._hi, int(slot) + 1)

    def erase(self, slot):
        _lib.check(self._L.orbv_db_erase(self._h, int(slot)), "orbv_db_erase")

    def clear(self):
        _lib.check(self._L.orbv_db_clear(self._h), "orbv_db_clear")
        self._hi = 0

    def set_best_covisibles(self, slot, neighbours):
        nb = np.ascontiguousarray(neighbours, np.int32)
        _lib.check(self._L.orbv_db_set_best_covisibles(self._h, int(slot), _lib.ptr(nb), len(nb)), "orbv_db_set_best_covisibles")
        self._hi = max(self._hi, int(slot) + 1)

    def get_state(self, slots):
        """-> (reloc_query int64[n], reloc_score float32[n]) of the listed slots."""
        s = np.ascontiguousarray(slots, np.int32)
        q = np.zeros(len(s), np.int64); sc = np.zeros(len(s), np.float32)
        _lib.check(self._L.orbv_db_get_state(self._h, _lib.ptr(s), len(s), _lib.ptr(q), _lib.ptr(sc)), "orbv_db_get_state")
        return q, sc

    def min_score(self, bow, slots):
        """LoopClosing::DetectLoop's minScore: the lowest float score of `bow` against the listed slots, from 1.0f."""
        w, v = _bow(bow); s = np.ascontiguousarray(slots, np.int32)
        out = C.c_float(0)
        _lib.check(self._L.orbv_db_min_score(self._h, _lib.ptr(w), _lib.ptr(v), len(w), _lib.ptr(s), len(s), C.byref(out)), "orbv_db_min_score")
        return np.float32(out.value)

    # ---- host queries -------------------------------------------------------------------------------------------------------------
    def _trace(self, on):
        if not on:
            return None, None
        n = max(self._hi, 1)
        a = dict(info=_lib.DbQueryInfo(), kept_slot=np.zeros(n, np.int32), kept_score=np.zeros(n, np.float32), kept_acc=np.zeros(n, np.float32),
                 kept_best=np.zeros(n, np.int32))
        t = _lib.DbTrace(C.pointer(a["info"]), _lib.ptr(a["kept_slot"]), _lib.ptr(a["kept_score"]), _lib.ptr(a["kept_acc"]), _lib.ptr(a["kept_best"]), n, 0)
        return t, a

    @staticmethod
    def _trace_out(a):
        d = _info_dict(a["info"]); k = d["n_kept"]
        d["best_acc"] = np.float32(d["best_acc"])
        for key in ("kept_slot", "kept_score", "kept_acc", "kept_best"):
            d[key] = a[key][:k].copy()
        return d

    def _cap(self, cap):
        return max(self._hi, 1) if cap is None else int(cap)

    def detect_loop_candidates(self, bow, connected, min_score, query_id, trace=False, cap=None):
        """DetectLoopCandidates: the candidate slots in the reference's order (int32), with trace=True also the trace dict."""
        w, v = _bow(bow); cn = np.ascontiguousarray(connected, np.int32)
        cap = self._cap(cap); cand = np.zeros(max(cap, 1), np.int32); n = C.c_int(0)
        t, a = self._trace(trace)
        _lib.check(self._L.orbv_db_detect_loop_candidates(self._h, _lib.ptr(w), _lib.ptr(v), len(w), _lib.ptr(cn), len(cn), C.c_float(min_score), int(query_id),
                                                          _lib.ptr(cand), cap, C.byref(n), C.byref(t) if t else None), "orbv_db_detect_loop_candidates")
        return (cand[:n.value], self._trace_out(a)) if trace else cand[:n.value]

    def detect_relocalization_candidates(self, bow, query_id, trace=False, cap=None):
        w, v = _bow(bow)
        cap = self._cap(cap); cand = np.zeros(max(cap, 1), np.int32); n = C.c_int(0)
        t, a = self._trace(trace)
        _lib.check(self._L.orbv_db_detect_relocalization_candidates(self._h, _lib.ptr(w), _lib.ptr(v), len(w), int(query_id), _lib.ptr(cand), cap, C.byref(n),
                                                                    C.byref(t) if t else None), "orbv_db_detect_relocalization_candidates")
        return (cand[:n.value], self._trace_out(a)) if trace else cand[:n.value]

    def detect_loop_candidates_begin(self, bow, connected, min_score, query_id):
        """First half: the kept keyframes (score_and_matches) in order; hand their GetBestCovisibilityKeyFrames(10) to detect_candidates_finish."""
        w, v = _bow(bow); cn = np.ascontiguousarray(connected, np.int32)
        kept = np.zeros(max(self._hi, 1), np.int32); n = C.c_int(0)
        _lib.check(self._L.orbv_db_detect_loop_candidates_begin(self._h, _lib.ptr(w), _lib.ptr(v), len(w), _lib.ptr(cn), len(cn), C.c_float(min_score), int(query_id),
                                                                _lib.ptr(kept), len(kept), C.byref(n)), "orbv_db_detect_loop_candidates_begin")
        return kept[:n.value]

    def detect_relocalization_candidates_begin(self, bow, query_id):
        w, v = _bow(bow)
        kept = np.zeros(max(self._hi, 1), np.int32); n = C.c_int(0)
        _lib.check(self._L.orbv_db_detect_relocalization_candidates_begin(self._h, _lib.ptr(w), _lib.ptr(v), len(w), int(query_id), _lib.ptr(kept), len(kept),
                                                                          C.byref(n)), "orbv_db_detect_relocalization_candidates_begin")
        return kept[:n.value]

    def detect_candidates_finish(self, neighbour_rows, trace=False, cap=None):
        """Second half: neighbour_rows[i] = the best covisible slots (at most 10, in order) of the i-th kept keyframe."""
        k = len(neighbour_rows)
        rows = np.zeros((max(k, 1), 10), np.int32); rn = np.zeros(max(k, 1), np.int32)
        for i, r in enumerate(neighbour_rows):
            r = np.asarray(r, np.int32)
            if len(r) > 10:
                raise ValueError("a neighbour row has at most 10 slots")
            rows[i, :len(r)] = r; rn[i] = len(r)
        cap = self._cap(cap); cand = np.zeros(max(cap, 1), np.int32); n = C.c_int(0)
        t, a = self._trace(trace)
        _lib.check(self._L.orbv_db_detect_candidates_finish(self._h, _lib.ptr(rows), _lib.ptr(rn), _lib.ptr(cand), cap, C.byref(n), C.byref(t) if t else None),
                   "orbv_db_detect_candidates_finish")
        return (cand[:n.value], self._trace_out(a)) if trace else cand[:n.value]

    # ---- batched queries on torch device buffers ---------------------------------------------------------------------------------
    def workspace_bytes(self, n_queries):
        b = C.c_size_t(0)
        _lib.check(self._L.orbv_db_detect_workspace(self._h, int(n_queries), C.byref(b)), "orbv_db_detect_workspace")
        return int(b.value)

    def _batch(self, kind, q_off, q_words, q_values, first_query_id, cap, conn_off=None, conn=None, min_score=None, workspace=None, stream=None):
        import torch
        dev = q_words.device
        Q = int(q_off.shape[0]) - 1
        cap = self._cap(cap)
        need = self.workspace_bytes(Q)
        if workspace is None:
            workspace = torch.empty((need,), dtype=torch.uint8, device=dev)
        info = torch.empty((Q, 8), dtype=torch.int32, device=dev)
        cand = torch.empty((Q, max(cap, 1)), dtype=torch.int32, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
        if kind == "loop":
            rc = self._L.orbv_db_detect_loop_candidates_batch_device(self._h, Q, _lib.ptr(q_off), _lib.ptr(q_words), _lib.ptr(q_values), _lib.ptr(conn_off),
                                                                     _lib.ptr(conn), _lib.ptr(min_score), int(first_query_id), _lib.ptr(info), _lib.ptr(cand), cap,
                                                                     _lib.ptr(workspace), workspace.numel(), C.c_void_p(st))
        else:
            rc = self._L.orbv_db_detect_relocalization_candidates_batch_device(self._h, Q, _lib.ptr(q_off), _lib.ptr(q_words), _lib.ptr(q_values),
                                                                               int(first_query_id), _lib.ptr(info), _lib.ptr(cand), cap, _lib.ptr(workspace),
                                                                               workspace.numel(), C.c_void_p(st))
        _lib.check(rc, "orbv_db_detect_%s_candidates_batch_device" % ("loop" if kind == "loop" else "relocalization"))
        return info, cand

    def detect_loop_candidates_batch_device(self, q_off, q_words, q_values, conn_off, conn, min_score, first_query_id, cap=None, workspace=None, stream=None):
        """Enqueue only.  Device tensors: q_off int32[Q+1], q_words int32/uint32 bits [n], q_values float64[n], conn_off int32[Q+1], conn int32[m],
        min_score float32[Q].  -> (info int32[Q, 8] = orbv_db_query_info rows, best_acc as float bits in column 6; cand int32[Q, cap])."""
        return self._batch("loop", q_off, q_words, q_values, first_query_id, cap, conn_off, conn, min_score, workspace, stream)

    def detect_relocalization_candidates_batch_device(self, q_off, q_words, q_values, first_query_id, cap=None, workspace=None, stream=None):
        return self._batch("reloc", q_off, q_words, q_values, first_query_id, cap, None, None, None, workspace, stream)

    @staticmethod
    def batch_results(info, cand):
        """(info, cand) of a batched call, after the stream has been synchronised -> list of (candidates int32[], info dict)."""
        hi = info.cpu().numpy(); hc = cand.cpu().numpy()
        names = [k for k, _ in _lib.DbQueryInfo._fields_]
        out = []
        for q in range(hi.shape[0]):
            d = dict(zip(names, (int(x) for x in hi[q])))
            d["best_acc"] = hi[q, 6:7].view(np.float32)[0]
            out.append((hc[q, :d["n_cand"]].copy() if d["status"] == 0 else None, d))
        return out

"""Initializer::Initialize (reference src/Initializer.cc:54-889, monocular map initialisation) on the GPU (include/orbslam_hip.h:
orbt_initialize*).  Thin ctypes layer: arrays in, arrays out."""
import ctypes as C

import numpy as np

from . import _lib

# report->reason (ORBT_INIT_*)
OK, BAD_INPUT, NO_MODEL = 0, 1, 2
H_DEGENERATE, H_AMBIGUOUS, H_PARALLAX, H_FEW = 3, 4, 5, 6
F_FEW, F_AMBIGUOUS, F_PARALLAX = 7, 8, 9
REASONS = {OK: "ok", BAD_INPUT: "bad input", NO_MODEL: "no model", H_DEGENERATE: "H degenerate", H_AMBIGUOUS: "H ambiguous",
           H_PARALLAX: "H parallax", H_FEW: "H too few", F_FEW: "F too few", F_AMBIGUOUS: "F ambiguous", F_PARALLAX: "F parallax"}
REPORT_FIELDS = ("model", "reason", "score_h", "score_f", "rh", "best_h", "best_f", "n_matches", "n_inliers", "motion")


def draw_ransac_sets(n_matches, iterations, randint=None):
    """The minimal sets of src/Initializer.cc:90-101: for every iteration, 8 draws by swap-remove from the full list of match
    positions (randint(0, len - 1) picks a slot, the slot takes the back entry, the back is popped).  randint(lo, hi) is inclusive
    on both ends, as DUtils::Random::RandomInt.  The reference's own sequence comes from the process-global rand(), seeded once per
    process (:88); this library cannot see it, so the default is numpy's generator (seed 0)."""
    if randint is None:
        rng = np.random.default_rng(0)

        def randint(lo, hi):
            return int(rng.integers(lo, hi + 1))
    sets = np.zeros((iterations, 8), np.int32)
    for it in range(iterations):
        avail = list(range(n_matches))
        for j in range(8):
            r = randint(0, len(avail) - 1)
            sets[it, j] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return sets


def _report_dict(rep):
    d = {k: getattr(rep, k) for k in REPORT_FIELDS}
    d["n_good"] = np.array(rep.n_good[:], np.int32)
    d["parallax"] = np.array(rep.parallax[:], np.float32)
    return d


def initialize(kps1, kps2, matches12, K4, sigma=1.0, iterations=200, ransac_sets=None, trace=False, out=None):
    """orbt_initialize for one pair.  kps1[n1, 2], kps2[n2, 2] undistorted keypoints; matches12[n1] frame-2 index or -1;
    K4 = (fx, fy, cx, cy); ransac_sets[iterations, 8] positions in the ascending match list (None = draw_ransac_sets with its
    default generator).  out: optional dict of preset R21 (3, 3), t21 (3,), P3D (n1, 3), triangulated (n1,) arrays; the call
    writes them only on success.  Returns a dict: success, R21, t21, P3D, triangulated, the report fields and, with trace=True,
    H21 / H12 / F21 [iterations, 3, 3], scores_h / scores_f [iterations], motion_R [8, 3, 3], motion_t [8, 3], inliers_h /
    inliers_f [n_matches] (bool)."""
    L = _lib.load()
    k1 = np.ascontiguousarray(kps1, np.float32).reshape(-1, 2)
    k2 = np.ascontiguousarray(kps2, np.float32).reshape(-1, 2)
    m12 = np.ascontiguousarray(matches12, np.int32).reshape(-1)
    K = np.ascontiguousarray(K4, np.float32).reshape(4)
    n1, n2 = len(k1), len(k2)
    nm = int((m12 >= 0).sum())
    if ransac_sets is None:
        ransac_sets = draw_ransac_sets(nm, iterations)
    sets = np.ascontiguousarray(ransac_sets, np.int32)
    if sets.ndim != 2 or sets.shape != (iterations, 8):
        raise ValueError("initialize: ransac_sets has shape %s, expected (iterations = %d, 8)" % (sets.shape, iterations))
    o = {} if out is None else out
    o.setdefault("R21", np.zeros((3, 3))); o.setdefault("t21", np.zeros(3))
    o.setdefault("P3D", np.zeros((n1, 3))); o.setdefault("triangulated", np.zeros(n1, np.uint8))
    for k, dt in (("R21", np.float64), ("t21", np.float64), ("P3D", np.float64), ("triangulated", np.uint8)):
        assert o[k].dtype == dt and o[k].flags.c_contiguous, k
    rep = _lib.InitReport()
    tr = None
    if trace:
        it = iterations
        o.update(H21=np.zeros((it, 3, 3)), H12=np.zeros((it, 3, 3)), F21=np.zeros((it, 3, 3)), scores_h=np.zeros(it, np.float32),
                 scores_f=np.zeros(it, np.float32), motion_R=np.zeros((8, 3, 3)), motion_t=np.zeros((8, 3)),
                 inliers_h=np.zeros(max(nm, 1), np.uint8), inliers_f=np.zeros(max(nm, 1), np.uint8))
        tr = _lib.InitTrace(*[_lib.ptr(o[k]) for k in ("H21", "H12", "F21", "scores_h", "scores_f", "motion_R", "motion_t", "inliers_h", "inliers_f")])
    _lib.check(L.orbt_initialize(_lib.ptr(k1), n1, _lib.ptr(k2), n2, _lib.ptr(m12), _lib.ptr(K), float(sigma), iterations, _lib.ptr(sets),
                                 _lib.ptr(o["R21"]), _lib.ptr(o["t21"]), _lib.ptr(o["P3D"]), _lib.ptr(o["triangulated"]), C.byref(rep),
                                 C.byref(tr) if tr is not None else None), "orbt_initialize")
    o.update(_report_dict(rep))
    o["success"] = rep.reason == OK
    if trace:
        o["inliers_h"] = o["inliers_h"][:nm].astype(bool)
        o["inliers_f"] = o["inliers_f"][:nm].astype(bool)
    return o


def initialize_batch_device(kps1, off1, kps2, off2, matches12, K4, sigma, iterations, ransac_sets, out):
    """orbt_initialize_batch_device on torch CUDA tensors: kps1[n1_total, 2] float32, off1[npairs + 1] int32 (CSR over pairs),
    kps2 / off2 likewise, matches12[n1_total] int32 (frame-2 index within the pair or -1), K4[npairs, 4] float32,
    ransac_sets[npairs, iterations, 8] int32.  out = dict of device tensors R21[npairs, 3, 3] float64, t21[npairs, 3] float64,
    P3D[n1_total, 3] float64, triangulated[n1_total] uint8, report[npairs * sizeof(orbt_init_report)] uint8, written on the
    current stream (the rows of pairs that fail stay as they were).  decode_reports() turns the report bytes into dicts."""
    L = _lib.load()
    npairs = off1.numel() - 1
    ws = _lib.workspace("orbt_initialize_workspace", npairs, kps1.shape[0], kps2.shape[0], int(iterations), device=kps1.device, min_bytes=16)
    p = _lib.ptr
    _lib.check(L.orbt_initialize_batch_device(npairs, p(kps1), p(off1), kps1.shape[0], p(kps2), p(off2), kps2.shape[0], p(matches12), p(K4),
                                              float(sigma), int(iterations), p(ransac_sets), p(out["R21"]), p(out["t21"]), p(out["P3D"]),
                                              p(out["triangulated"]), p(out["report"]), p(ws), _lib.stream()),
               "orbt_initialize_batch_device")
    out["_workspace"] = ws                                       # (kept alive until the caller synchronises)
    return out


def report_bytes(npairs):
    """Size in bytes of npairs orbt_init_report records (for initialize_batch_device's out["report"])."""
    return npairs * C.sizeof(_lib.InitReport)


def decode_reports(buf):
    """bytes of orbt_init_report records (a host numpy uint8 array) -> list of report dicts."""
    b = np.ascontiguousarray(buf, np.uint8)
    sz = C.sizeof(_lib.InitReport)
    return [_report_dict(_lib.InitReport.from_buffer_copy(b[i * sz:(i + 1) * sz].tobytes())) for i in range(len(b) // sz)]

"""The seeded two-view cases of the initializer tests (tests/test_gpu_initializer.py, tests/test_initializer_restatement.py)."""
import numpy as np

from ceres_mono_orb_slam2_amd import synth
from ceres_mono_orb_slam2_amd.initializer import draw_ransac_sets

# the cases that reach each branch of the decision (checked on the restatement by the CPU tests and on the device by the GPU tests)
WITNESS = {"H success": (0, "planar", 500, 0.0, 0.2, 200, None), "F success": (0, "general", 500, 0.0, 0.2, 200, None),
           "parallax": (1, "rotation", 500, 0.0, 0.5, 200, None), "count": (0, "sparse", 200, 0.1, 0.5, 200, None)}

# (seed, kind, n_kps, outlier_frac, noise px, iterations, degenerate sets: None | "collinear" | "repeated")
CASES = list(WITNESS.values()) + [
    (1, "general", 10, 0.0, 0.0, 1, None), (2, "general", 12, 0.0, 0.3, 200, None), (3, "planar", 16, 0.2, 0.3, 200, None),
    (4, "sparse", 60, 0.0, 0.3, 200, None), (5, "general", 120, 0.1, 0.3, 200, None), (6, "planar", 120, 0.3, 0.3, 200, None),
    (7, "rotation", 150, 0.0, 0.3, 200, None), (8, "general", 300, 0.6, 0.3, 200, None), (9, "planar", 300, 0.0, 0.0, 1, None),
    (10, "general", 300, 0.0, 0.0, 200, None), (11, "planar", 400, 0.0, 0.0, 200, None), (12, "rotation", 400, 0.2, 0.3, 1000, None),
    (13, "sparse", 400, 0.3, 0.5, 200, None), (14, "general", 600, 0.2, 0.2, 1000, None), (15, "planar", 600, 0.2, 0.2, 200, None),
    (16, "rotation", 800, 0.0, 0.3, 200, None), (17, "general", 1000, 0.1, 0.2, 200, None), (18, "planar", 1000, 0.4, 0.2, 200, None),
    (19, "general", 1000, 0.0, 0.5, 1, None), (20, "sparse", 1000, 0.2, 0.3, 200, None), (21, "general", 2000, 0.3, 0.2, 200, None),
    (22, "planar", 2000, 0.1, 0.2, 200, None), (23, "rotation", 2000, 0.1, 0.5, 200, None), (24, "general", 4400, 0.2, 0.2, 200, None),
    (25, "planar", 4400, 0.5, 0.3, 200, None), (26, "general", 200, 0.0, 0.2, 200, "collinear"), (27, "planar", 200, 0.0, 0.2, 200, "repeated"),
    (28, "general", 500, 0.1, 0.2, 200, "collinear"), (29, "rotation", 500, 0.0, 0.2, 200, "repeated"), (30, "general", 800, 0.0, 0.2, 1000, None),
    (31, "planar", 800, 0.0, 0.2, 1000, None), (32, "general", 1500, 0.0, 0.1, 200, None), (33, "planar", 1500, 0.3, 0.1, 200, None),
    (34, "rotation", 1200, 0.0, 0.5, 200, None), (35, "sparse", 2000, 0.0, 0.3, 200, None), (36, "general", 250, 0.0, 0.2, 200, None),
    (37, "planar", 250, 0.0, 0.2, 200, None), (38, "general", 700, 0.05, 0.2, 200, None), (39, "planar", 700, 0.05, 0.2, 200, None),
]


def make_case(case):
    """-> (kps1, kps2, matches12, K4, ransac_sets)."""
    seed, kind, n, of, noise, iters, degen = case
    s = synth.make_two_view(seed, kind, n, of, noise)
    kps1, kps2, m12 = s["kps1"].copy(), s["kps2"].copy(), s["matches12"]
    nm = int((m12 >= 0).sum())
    if nm < 8:                                                  # (a tiny scene: match what there is)
        free = np.nonzero(m12 < 0)[0][:8 - nm]
        m12 = m12.copy(); m12[free] = np.arange(len(free)) % len(kps2)
        nm = int((m12 >= 0).sum())
    sets = draw_ransac_sets(nm, iters, None)
    if degen == "collinear":                                    # the first 12 matches on one line in both frames; every set from them
        i1 = np.nonzero(m12 >= 0)[0][:12]
        tt = np.linspace(0.1, 0.9, 12).astype(np.float32)
        kps1[i1, 0] = 100 + 900 * tt; kps1[i1, 1] = 50 + 250 * tt
        kps2[m12[i1], 0] = 120 + 880 * tt; kps2[m12[i1], 1] = 60 + 240 * tt
        rng = np.random.default_rng(seed)
        sets = np.stack([rng.permutation(12)[:8] for _ in range(iters)]).astype(np.int32)
    elif degen == "repeated":                                   # sets that repeat positions (rank-deficient systems) beside drawn ones
        sets = sets.copy()
        sets[::2, 4:] = sets[::2, :4]
        sets[1::4] = sets[1::4, :1]
    return kps1, kps2, m12, s["K4"], sets

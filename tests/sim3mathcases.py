"""One deterministic case table for csrc/sim3_math.h at its branch points, the mp truths of every case (tests/npsim3.py, computed once
per process), the flat binary file tools/ubench/sim3_math_probe.hip reads and the parser of what it writes, and the acceptance rule of
tests/test_sim3_math_reference.py and tests/test_gpu_sim3_math.py.

Every case carries a bucket name: the function and the regime of the branch it exercises.  theta and |sigma| run over
    0, 1e-12, 9.9e-11 | 1.01e-10 | 1e-9 | 1e-8 | 1e-7 | 1e-6 | 9.9e-6, 1.01e-5 | 1e-3, 0.1, 1       (| separates the bucket classes)
theta further over pi - 1e-9, pi, pi + 1e-9 | 2 pi - 1e-9, 6.5 and sigma over both signs and +-5: the thresholds of s3_exp (|theta|,
|sigma| against 1e-10), of s3_log (theta^2, sigma^2 against 1e-10; |v|^2 against 1e-20; w < 0) and of s3_plus' clamp.

The rule: per bucket, max e <= max(64 * 2.2e-16, 8 * E_oracle[bucket]) with e = max|out - truth| / max(1, max|truth|) per function and
case, and E_oracle the CPU oracle's maximum over the bucket, measured against mp and committed in tests/golden/sim3_math_oracle_err.npz
(tests/test_sim3_math_reference.py checks that the oracle built there reproduces it within a factor of 2)."""
import functools
import os

import numpy as np
from mpmath import mp, mpf

from tests import npsim3 as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_SRC = os.path.join(ROOT, "tools", "ubench", "sim3_math_probe.hip")
PROBE_FLAGS = ["-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "--offload-arch=gfx950"]       # the library's own (__graft_entry__.HIPFLAGS)
GOLDEN = os.path.join(ROOT, "tests", "golden", "sim3_math_oracle_err.npz")
FLOOR = 64 * 2.2e-16
FACTOR = 8.0
MAX_CASES = 1500
PI = float(np.pi)

FID = dict(exp=0, log=1, plus=2, inverse=3, mul=4, adj=5, edge=6, term=7, outlier=8, act=9, pose34=10)
NIN = dict(exp=7, log=7, plus=14, inverse=7, mul=14, adj=7, edge=21, term=18, outlier=18, act=10, pose34=7)
NOUT = dict(exp=7, log=7, plus=7, inverse=7, mul=7, adj=49, edge=56, term=17, outlier=1, act=3, pose34=12)
SPLIT = dict(edge=(7, 49), term=(2, 14, 1))                      # the parts of an output row that are measured on their own

TINY = [(0.0, "<1e-10"), (1e-12, "<1e-10"), (9.9e-11, "<1e-10"), (1.01e-10, "1.01e-10"), (1e-9, "1e-9"), (1e-8, "1e-8"), (1e-7, "1e-7"), (1e-6, "1e-6"),
        (9.9e-6, "~1e-5"), (1.01e-5, "~1e-5")]
THETAS = TINY + [(1e-3, "1e-3..1"), (0.1, "1e-3..1"), (1.0, "1e-3..1"), (PI - 1e-9, "~pi"), (PI, "~pi"), (PI + 1e-9, "~pi"), (2 * PI - 1e-9, "~2pi"), (6.5, "~2pi")]
SIG_MAG = TINY + [(1e-3, "1e-3..1"), (0.1, "1e-3..1"), (1.0, "1e-3..1"), (5.0, "5")]
SIGMAS = [(0.0, "<1e-10")] + [(s * m, lab) for m, lab in SIG_MAG[1:] for s in (1.0, -1.0)]
UPS = [0.0, 1e-8, 1.0, 1e3]
K4 = np.array([500.0, 480.0, 320.0, 240.0])
HUBER = float(np.sqrt(10.0))
TH2 = 10.0
EDGE_SIZES = [(0.0, "0"), (1e-9, "1e-9"), (1e-5, "1e-5"), (1e-2, "1e-2"), (0.3, "0.3")]
OUTLIER_ROT = [0.7, 2.2, 3.0, PI - 1e-6]                         # 0.7: the trace > 0 arm; the others, past 120 degrees, the three other arms
OUTLIER_SCALES = [0.5, 1.0, 2.0]
OUTLIER_RATIOS = [0.3, 0.9, 1.1, 3.0, 1 - 1e-5, 1 + 1e-5]
KEEP_BAND = 1e-6


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


_rng0 = np.random.default_rng(20240521)
AXES = [np.array([1.0, 0, 0]), np.array([0, 1.0, 0]), np.array([0, 0, 1.0]), _unit(_rng0.normal(0, 1, 3)), _unit(_rng0.normal(0, 1, 3))]
DIRS = [_unit(_rng0.normal(0, 1, 3)) for _ in range(4)]
DIR7 = [_unit(_rng0.normal(0, 1, 7)) for _ in range(8)]


def _f(a):
    return N.to_f64(a)


def _quat(theta, axis, scale_log):
    """sqrt(e^sigma) (sin(theta / 2) axis, cos(theta / 2)), each component rounded once from mp"""
    with mp.workdps(N.DPS):
        r = mp.exp(mpf(scale_log) / 2); h = mpf(theta) / 2
        return np.array([float(r * mp.sin(h) * mpf(float(a))) for a in axis] + [float(r * mp.cos(h))])


def _exp_cases():
    rows, b = [], []
    for ti, (th, tl) in enumerate(THETAS):
        for si, (sg, sl) in enumerate(SIGMAS):
            ax = AXES[(ti + 2 * si) % 5]; um = UPS[(3 * ti + si) % 4]
            rows.append(np.concatenate([um * DIRS[(ti + si) % 4], th * ax, [sg]]))
            b.append("exp/th=%s/sg=%s" % (tl, sl))
    return np.array(rows), b


def _log_cases():
    rows, b = [], []
    for ti, (th, tl) in enumerate(THETAS):
        for mi, (m, sl) in enumerate(SIG_MAG):
            sg = m if (ti + mi) % 2 == 0 else -m
            ax = AXES[(2 * ti + mi) % 5]; tm = UPS[(ti + 3 * mi) % 4]
            rows.append(np.concatenate([_quat(th, ax, sg), tm * DIRS[(ti + mi) % 4]]))
            b.append("log/th=%s/sg=%s" % (tl, sl))
    k = 0
    for ax in AXES:                                               # w == 0 exactly: a half turn
        for sl in (0.0, 5.0, -5.0):
            rows.append(np.concatenate([float(np.exp(sl / 2)) * ax, [0.0], UPS[k % 4] * DIRS[k % 4]])); b.append("log/w=0"); k += 1
    for n, lab in ((0.99e-10, "log/v2<1e-20"), (1.01e-10, "log/v2>1e-20")):      # |v|^2 on either side of the quaternion branch, w of both signs
        for w in (1.0, -1.0):
            for sl in (0.0, 5.0, -5.0, 1e-7):
                r = float(np.exp(sl / 2))
                rows.append(np.concatenate([r * n * AXES[k % 5], [r * w], UPS[k % 4] * DIRS[k % 4]])); b.append(lab); k += 1
    return np.array(rows), b


GEN_X = [np.array([1.5, -0.7, 2.0, 0.5, -0.4, 0.45, 0.2]), np.array([-3.0, 0.2, 0.9, -0.1, 1.1, 0.3, -0.3]), np.array([0.4, 2.5, -1.0, 2.0, 1.5, -1.2, 0.05])]


def _plus_cases():
    rows, b = [], []
    um = [0.0, 1e-8, 1e-10, 1e-6]
    for ti, (th, tl) in enumerate(TINY):
        for si, (m, sl) in enumerate(TINY):
            sg = m if (ti + si) % 2 == 0 else -m
            d = np.concatenate([um[(ti + si) % 4] * DIRS[(ti + 2 * si) % 4], th * AXES[(ti + si) % 5], [sg]])
            rows.append(np.concatenate([GEN_X[(ti * 10 + si) % 3], d])); b.append("plus/d: th=%s/sg=%s" % ("<1e-10" if th < 1e-10 else ">=1e-10", sl))
    for x in GEN_X:                                               # the clamp of d[6] at -20
        for d6 in (-19.9, -20.0, -25.0):
            rows.append(np.concatenate([x, 0.01 * DIRS[1], 0.02 * AXES[3], [d6]])); b.append("plus/clamp")
    return np.array(rows), b


@functools.lru_cache(maxsize=None)
def _generic_elements():
    """40 group elements over large and small rotations and scales, as float64 qt7, with the sigma label of each"""
    S, lab = [], []
    k = 0
    for th in (0.0, 1e-7, 0.1, 1.0, 3.0, PI, 6.5, 2 * PI - 1e-9):
        for sg, sl in ((-5.0, "5"), (-0.1, "0.1"), (0.0, "<=1e-8"), (1e-8, "<=1e-8"), (5.0, "5")):
            a = np.concatenate([UPS[k % 4] * DIRS[k % 4], th * AXES[k % 5], [sg]])
            S.append(_f(N.mp_exp_qt(a))); lab.append(sl); k += 1
    return S, lab


def _group_cases(name):
    S, lab = _generic_elements()
    rng = np.random.default_rng(77)
    rows = []
    for i in range(len(S)):
        if name == "mul":
            rows.append(np.concatenate([S[i], S[(7 * i + 3) % len(S)]]))
        elif name == "act":
            rows.append(np.concatenate([S[i], rng.uniform(-10, 10, 3)]))
        else:
            rows.append(S[i])
    return np.array(rows), ["%s/sg=%s" % (name, l) for l in lab]


def _edge_cases():
    rng = np.random.default_rng(4242)
    rows, b = [], []
    near_pi = [PI - 1e-6, 3.0, PI - 1e-3, 3.1]
    for c in range(8):
        li = np.concatenate([rng.uniform(-5, 5, 3), rng.uniform(0.2, 1.2) * _unit(rng.normal(0, 1, 3)), [rng.uniform(-0.1, 0.1)]])
        th = rng.uniform(0.2, 1.2) if c < 4 else near_pi[c - 4]
        lj = np.concatenate([rng.uniform(-5, 5, 3), th * _unit(rng.normal(0, 1, 3)), [rng.uniform(-0.1, 0.1)]])
        for size, sl in EDGE_SIZES:
            with mp.workdps(N.DPS):
                Sji = _f(N.qt_of(N.mp_exp(size * DIR7[c]) * N.mp_exp(lj) * N.mp_inverse(N.mp_exp(li))))
            rows.append(np.concatenate([lj, li, Sji])); b.append("edge/r=%s/%s" % (sl, "generic" if c < 4 else "lie_j near pi"))
    return np.array(rows), b


TERM_LIE = np.array([0.3, -0.2, 0.5, 0.4, -0.5, 0.28, float(np.log(1.3))])


def _term_cases():
    """inputs [K4, S, P, uv, w, huber]; meta rows (inverse flag) for the oracle, which takes the tangent and the flag"""
    rows, b, inv = [], [], []
    with mp.workdps(N.DPS):
        Sf = N.mp_exp(TERM_LIE); Si = N.mp_inverse(Sf)
        Sf64, Si64 = _f(N.mp_exp_qt(TERM_LIE)), _f(N.qt_of(Si))
    ratios = [1e-4, 0.5, 1 - 1e-5, 1 + 1e-5, 4.0, 1e4]
    k = 0
    for depth in (0.1, 0.5, 2.0, 10.0, 50.0):
        for inverse in (0, 1):
            S64 = Si64 if inverse else Sf64
            pc = np.array([0.1 * depth * (1 + (0.3 * k) % 3), -0.07 * depth * (1 + k % 2), depth])
            P = _f(N.mp_act(Sf if inverse else Si, pc))                          # so that S P lies at pc (up to P's rounding)
            with mp.workdps(N.DPS):
                p = N.mp_act(S64, P)
                proj = np.array([float(K4[0] * p[0] / p[2] + K4[2]), float(K4[1] * p[1] / p[2] + K4[3])])
            for ri, ratio in enumerate(ratios):
                w = (1.0, 0.8)[(k + ri) % 2]
                e = np.sqrt(ratio) * HUBER / w * _unit(DIRS[(k + ri) % 4][:2])
                rows.append(np.concatenate([K4, S64, P, proj + e, [w, HUBER]])); inv.append(inverse)
                b.append("term/%s/%s" % ("inverse" if inverse else "forward", "linear" if ratio > 1 else "quadratic"))
            k += 1
    return np.array(rows), b, np.array(inv)




def _outlier_cases():
    """inputs [K4, S, P, uv, inv_sigma, thres]: every rotation about x, y, z and a random axis at three scales, three points each whose
    pixel sits at a chosen chi2 / thres from the projection of the reference's own camera point"""
    rng = np.random.default_rng(99)
    rows, k = [], 0
    t = np.array([0.2, -0.1, 0.3])
    for th in OUTLIER_ROT:
        for ax in AXES[:4]:
            for sc in OUTLIER_SCALES:
                S = np.concatenate([_quat(th, ax, float(np.log(sc))), t])
                for j in range(3):
                    inv_sigma = float(np.float32((1.0, 1 / 1.44)[(k + j) % 2]))
                    while True:                                   # a point in front of the camera under the reference's arithmetic
                        P = rng.uniform(-3, 3, 3)
                        c = _f(N.mp_outlier_camera_point(S, P)[0])
                        if c[2] > 0.5:
                            break
                    proj = np.array([K4[0] * c[0] / c[2] + K4[2], K4[1] * c[1] / c[2] + K4[3]])
                    ratio = OUTLIER_RATIOS[(k + j) % len(OUTLIER_RATIOS)]
                    e = np.sqrt(ratio * TH2 / inv_sigma) * _unit(DIRS[(k + j) % 4][:2])
                    rows.append(np.concatenate([K4, S, P, proj + e, [inv_sigma, TH2]]))
                k += 1
    return np.array(rows)


# ---------------------------------------------------------------- the mp truth of one case: a list of parts (lists of mp values)
def _truth_one(name, row, extra=None):
    with mp.workdps(N.DPS):
        if name == "exp":
            return [N.mp_exp_qt(row)]
        if name == "log":
            return [N.mp_log(row)]
        if name == "plus":
            return [N.mp_plus(row[:7], row[7:])]
        if name == "inverse":
            return [_mat_list(N.mp_inverse(row))]
        if name == "mul":
            return [_mat_list(N.mp_mul(row[:7], row[7:]))]
        if name == "adj":
            A = N.mp_adj(row)
            return [[A[i, j] for i in range(7) for j in range(7)]]
        if name == "edge":
            r, J = N.mp_graph_edge(row[:7], row[7:14], row[14:])
            return [r, [J[i, j] for i in range(7) for j in range(7)]]
        if name == "term":
            t = N.mp_term(row[:4], row[4:11], row[11:14], row[14:16], row[16], row[17])
            return [t["r"], t["J"][0] + t["J"][1], [t["rho0"]]], t
        if name == "outlier":
            return N.mp_check_outlier(row[:4], row[4:11], row[11:14], row[14:16], row[16], row[17])
        if name == "act":
            return [N.mp_act(row[:7], row[7:])]
        if name == "pose34":
            return [N.mp_to_pose34(row)]
    raise KeyError(name)


def _mat_list(M):
    return [M[i, j] for i in range(3) for j in range(4)]


def as_mat12(qt7):
    """float64 qt7 rows -> the 12 entries [s R | t] the group-valued truths are stated in (a quaternion's sign is not part of the element)"""
    q = np.asarray(qt7, np.float64).reshape(-1, 7)
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    M = np.stack([w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y), q[:, 4],
                  2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x), q[:, 5],
                  2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z, q[:, 6]], axis=1)
    return M


GROUP_VALUED = ("inverse", "mul")                                 # compared as matrices: 12 values per case


@functools.lru_cache(maxsize=None)
def table():
    """name -> dict(inputs [n, NIN], buckets [n], truth [n] (lists of parts), and per function: inverse [n] (term), flag / ratio / arm
    (outlier), linear / ratio (term)).  Terms and outlier cases within KEEP_BAND of their threshold are left out; nothing else is."""
    T = {}
    for name, (rows, b) in (("exp", _exp_cases()), ("log", _log_cases()), ("plus", _plus_cases()), ("inverse", _group_cases("inverse")), ("mul", _group_cases("mul")),
                            ("adj", _group_cases("adj")), ("edge", _edge_cases()), ("act", _group_cases("act")), ("pose34", _group_cases("pose34"))):
        T[name] = dict(inputs=rows, buckets=list(b), truth=[_truth_one(name, r) for r in rows])
    rows, b, inv = _term_cases()
    tr = [_truth_one("term", r) for r in rows]
    keep = [i for i, (_, t) in enumerate(tr) if abs(t["ratio"] - 1) >= KEEP_BAND]
    T["term"] = dict(inputs=rows[keep], buckets=[b[i] for i in keep], truth=[tr[i][0] for i in keep], inverse=inv[keep], linear=np.array([tr[i][1]["linear"] for i in keep]),
                     ratio=np.array([float(tr[i][1]["ratio"]) for i in keep]), n_built=len(rows))
    rows = _outlier_cases()
    tr = [_truth_one("outlier", r) for r in rows]
    keep = [i for i, t in enumerate(tr) if abs(t[1] - 1) >= KEEP_BAND]
    T["outlier"] = dict(inputs=rows[keep], buckets=["outlier/arm=%s" % ("trace", "x", "y", "z")[(tr[i][2] + 1) % 4] for i in keep], truth=[None] * len(keep),
                        flag=np.array([tr[i][0] for i in keep]), ratio=np.array([float(tr[i][1]) for i in keep]), arm=np.array([tr[i][2] for i in keep]), n_built=len(rows))
    for name, t in T.items():
        assert t["inputs"].shape == (len(t["buckets"]), NIN[name]), name
        t["inputs"].setflags(write=False)
    return T


ORDER = ("exp", "log", "plus", "inverse", "mul", "adj", "edge", "term", "outlier", "act", "pose34")


def n_cases():
    return sum(len(t["buckets"]) for t in table().values())


# ---------------------------------------------------------------- the probe's files
def pack():
    T = table()
    out = []
    for name in ORDER:
        out += [np.array([FID[name], len(T[name]["inputs"])], np.float64), T[name]["inputs"].reshape(-1)]
    return np.concatenate(out).astype("<f8").tobytes()


def unpack(blob):
    """results.bin -> (device, host): name -> [n, NOUT]; device is None for a --host-only run"""
    a = np.frombuffer(blob, "<f8")
    has_dev = bool(a[0]); pos = 1
    dev, host = ({} if has_dev else None), {}
    T = table()
    for name in ORDER:
        f, n, no = int(a[pos]), int(a[pos + 1]), int(a[pos + 2]); pos += 3
        assert (f, n, no) == (FID[name], len(T[name]["inputs"]), NOUT[name]), (name, f, n, no)
        if has_dev:
            dev[name] = a[pos:pos + n * no].reshape(n, no); pos += n * no
        host[name] = a[pos:pos + n * no].reshape(n, no); pos += n * no
    assert pos == len(a)
    return dev, host


def build_probe(workdir, src=PROBE_SRC):
    import subprocess
    exe = os.path.join(str(workdir), os.path.splitext(os.path.basename(src))[0])
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + PROBE_FLAGS + ["-o", exe, src])
    return exe


def run_probe(exe, workdir, host_only):
    import subprocess
    cin, cout = os.path.join(str(workdir), "cases.bin"), os.path.join(str(workdir), "results.bin")
    with open(cin, "wb") as f:
        f.write(pack())
    r = subprocess.run([exe] + (["--host-only"] if host_only else []) + [cin, cout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    with open(cout, "rb") as f:
        return unpack(f.read())


# ---------------------------------------------------------------- measuring
def case_error(name, out_row, truth):
    """e of one case: the largest e over the parts of the output row"""
    o = np.asarray(out_row, np.float64).reshape(-1)
    if name in GROUP_VALUED:
        o = as_mat12(o)[0]
    parts = SPLIT.get(name, (len(o),))
    e, pos = 0.0, 0
    for n, t in zip(parts, truth):
        e = max(e, N.err(o[pos:pos + n], t)); pos += n
    return e


def bucket_maxima(name, outs):
    """bucket -> max e of the function's output rows [n, NOUT]"""
    t = table()[name]
    m = {}
    for row, b, tr in zip(outs, t["buckets"], t["truth"]):
        m[b] = max(m.get(b, 0.0), case_error(name, row, tr))
    return m


def fold(m, buckets, errors):
    for b, e in zip(buckets, errors):
        m[b] = max(m.get(b, 0.0), float(e))
    return m


def load_golden():
    z = np.load(GOLDEN)
    return {str(k): float(v) for k, v in zip(z["bucket"], z["max_err"])}


def bound(E, bucket):
    return max(FLOOR, FACTOR * E[bucket])


def check(measured, E, what, other=None):
    """the acceptance rule on a dict bucket -> max e; other: bucket -> a figure printed beside it in the message (not asserted)"""
    bad = ["%s: %.3g > %.3g%s" % (b, e, bound(E, b), "" if other is None else " (device to host %.3g)" % other.get(b, float("nan")))
           for b, e in sorted(measured.items()) if not e <= bound(E, b)]
    assert not bad, "%s breaks max(64 * 2.2e-16, 8 * E_oracle) in %d of %d buckets:\n  " % (what, len(bad), len(measured)) + "\n  ".join(bad)


# ---------------------------------------------------------------- problems for the library's own entry points, from the same tables
N_VTX, N_PTS = 129, 257                                           # a ragged tail for the 128- and 256-thread blocks of k_pg_poses / k_pg_points
CORRECT_STARTS = (0, 129, 258, 357)                               # four windows of 129 over the 486 exp cases


@functools.lru_cache(maxsize=None)
def correct_problems():
    """essential_graph_correct(x0, x, ref, pts) with x over the exp table: a list of dict(idx [129] exp cases, x0, x, ref, pts, T_truth
    [129] lists of 12, pts_truth [257] lists of 3)"""
    T = table()["exp"]
    out = []
    for w, s in enumerate(CORRECT_STARTS):
        rng = np.random.default_rng(500 + w)
        idx = np.arange(s, s + N_VTX)
        x = T["inputs"][idx]
        x0 = np.stack([GEN_X[v % 3] for v in range(N_VTX)]) + rng.normal(0, 0.05, (N_VTX, 7))
        ref = rng.permutation(N_PTS).astype(np.int32) % N_VTX
        pts = rng.uniform(-20, 20, (N_PTS, 3))
        with mp.workdps(N.DPS):
            E = [N.mp_exp(a) for a in x]
            Tt = [N.mp_to_pose34(M) for M in E]
            Ei = [mp.inverse(M) for M in E]
            E0 = [N.mp_exp(a) for a in x0]
            Pt = [N.mp_act(Ei[r], N.mp_act(E0[r], p)) for r, p in zip(ref, pts)]
        out.append(dict(idx=idx, x0=x0, x=x, ref=ref, pts=pts, T_truth=Tt, pts_truth=Pt))
    return out


def correct_errors(results):
    """results: per problem (T [129, 3, 4], pts [257, 3]) -> bucket -> max e, under correct_T/<exp bucket> and correct_pts/<exp bucket>"""
    B = table()["exp"]["buckets"]
    m = {}
    for pr, (Tg, Pg) in zip(correct_problems(), results):
        Tg = np.asarray(Tg).reshape(N_VTX, 12); Pg = np.asarray(Pg).reshape(N_PTS, 3)
        fold(m, ["correct_T/" + B[i][4:] for i in pr["idx"]], [N.err(Tg[v], pr["T_truth"][v]) for v in range(N_VTX)])
        fold(m, ["correct_pts/" + B[pr["idx"][r]][4:] for r in pr["ref"]], [N.err(Pg[p], pr["pts_truth"][p]) for p in range(N_PTS)])
    return m


def explog_errors(S_out):
    """exp(log(S)) of every log case, [n, 7] -> bucket explog/<log bucket> -> max e, as matrices against the input element itself"""
    t = table()["log"]
    with mp.workdps(N.DPS):
        truth = [_mat_list(N.mat_of(r)) for r in t["inputs"]]
    return fold({}, ["explog/" + b[4:] for b in t["buckets"]], [N.err(as_mat12(o)[0], tr) for o, tr in zip(np.asarray(S_out).reshape(-1, 7), truth)])


@functools.lru_cache(maxsize=None)
def graph_problems():
    """one two-vertex graph per edge case: vertex 0 = i, fixed; vertex 1 = j, free; the edge (1, 0, Sji).  dict(lie [2, 7], fixed, ej, ei,
    Sji [1, 7], cost_truth = |r|^2 / 2 in mp, consistent, answer = the 12 entries of Sji exp(x_i), bucket)"""
    t = table()["edge"]
    out = []
    for row, b, tr in zip(t["inputs"], t["buckets"], t["truth"]):
        with mp.workdps(N.DPS):
            cost = sum(c * c for c in tr[0]) / 2
            ans = _mat_list(N.mp_mul(row[14:], N.mp_exp(row[7:14])))
        out.append(dict(lie=np.stack([row[7:14], row[:7]]), fixed=np.array([1, 0], np.uint8), ej=np.array([1], np.int32), ei=np.array([0], np.int32), Sji=row[14:].reshape(1, 7),
                        cost_truth=cost, consistent=b.startswith("edge/r=0/"), answer=ans, bucket=b[5:]))
    return out


def graph_errors(results, exp_of):
    """results: per graph (lie7 [2, 7], summary) -> (bucket -> max e) under cost/<edge bucket> and, for the consistent cases, solve/<edge
    bucket>: exp of the free vertex (exp_of: tangent -> float64 qt7; the mp exp of the float64 tangent is used when it is None) against
    Sji exp(x_i)"""
    m = {}
    for g, (x, s) in zip(graph_problems(), results):
        fold(m, ["cost/" + g["bucket"]], [N.err([s["initial_cost"]], [g["cost_truth"]])])
        if g["consistent"]:
            with mp.workdps(N.DPS):
                got = _f(_mat_list(N.mp_exp(x[1])))
            fold(m, ["solve/" + g["bucket"]], [N.err(got, g["answer"])])
    return m


N_KF = 130


@functools.lru_cache(maxsize=None)
def assemble_map():
    """a map of 130 keyframes, every one a member of the corrected group, whose corrected Sim(3)s are 130 cases of the log table: every
    special case (w == 0, |v|^2 about 1e-20) and a stride through the grid that meets every theta and sigma class.  Returns (map, idx)."""
    from tests import essgraphcases as ec
    t = table()["log"]
    n = len(t["buckets"])
    grid = len(THETAS) * len(SIG_MAG)
    special = list(range(grid, n))
    rest = N_KF - len(special)
    pick = sorted(set(int(round(v)) for v in np.linspace(0, grid - 1, rest)))
    extra = [i for i in range(grid) if i not in pick]
    idx = np.array((pick + extra[:rest - len(pick)] + special)[:N_KF])
    assert len(set(idx.tolist())) == N_KF
    rng = np.random.default_rng(31)
    Tcw = np.stack([ec.pose12(ec.rot(rng.normal(0, 1, 3), rng.uniform(0.2, 1.2)), rng.uniform(-10, 10, 3)) for _ in range(N_KF)])
    m = dict(nkf=N_KF, kf_id=np.arange(N_KF, dtype=np.int32), kf_bad=np.zeros(N_KF, np.uint8), kf_rank=rng.permutation(N_KF).astype(np.int32), kf_Tcw=Tcw, loop=0, cur=N_KF - 1)
    parents = [-1] + list(range(N_KF - 1)); children = [[k + 1] for k in range(N_KF - 1)] + [[]]
    empty = [[] for _ in range(N_KF)]
    grp = [(k, t["inputs"][idx[k]], ec.se3_as_sim3(Tcw[k])) for k in range(N_KF)]
    pts = dict(X=[], bad=[], done=[], corr_ref=[], ref=[], obs=[], level=[])
    return ec._finish(m, parents, children, empty, empty, empty, grp, [], pts), idx


def assemble_errors(vtx_kf, lie7):
    t = table()["log"]
    _, idx = assemble_map()
    return fold({}, [t["buckets"][idx[k]] for k in vtx_kf], [N.err(l, t["truth"][idx[k]][0]) for k, l in zip(vtx_kf, np.asarray(lie7).reshape(-1, 7))])


# ---------------------------------------------------------------- the CPU oracle against mp: E_oracle
def measure_oracle():
    """bucket -> max e of oracle/sim3_oracle.cpp (g++) over the whole table and over the oracle's own forms of the library-level problems"""
    from oracle import pyoracle as O
    T = table()
    E = {}
    f1 = dict(exp=O.sim3_exp, log=O.sim3_log, inverse=O.sim3_inverse, adj=lambda S: O.sim3_adj(S).reshape(-1))
    for name, f in f1.items():
        E.update(bucket_maxima(name, [f(r) for r in T[name]["inputs"]]))
    E.update(bucket_maxima("plus", [O.sim3_plus(r[:7], r[7:]) for r in T["plus"]["inputs"]]))
    E.update(bucket_maxima("mul", [O.sim3_mul(r[:7], r[7:]) for r in T["mul"]["inputs"]]))
    E.update(bucket_maxima("act", [O.sim3_act(r[:7], r[7:]) for r in T["act"]["inputs"]]))
    E.update(bucket_maxima("edge", [np.concatenate([a.reshape(-1) for a in O.eg_eval_edge(r[:7], r[7:14], r[14:])]) for r in T["edge"]["inputs"]]))
    # the oracle evaluates a term from the tangent, without the loss: measured against mp_term of the same term without it
    t = T["term"]
    errs = []
    for row, inv in zip(t["inputs"], t["inverse"]):
        r, J = O.sim3_eval_term(K4, TERM_LIE, row[11:14], row[14:16], row[16], int(inv))
        tr = N.mp_term(row[:4], row[4:11], row[11:14], row[14:16], row[16], 1e300)
        errs.append(max(N.err(r, tr["r"]), N.err(J, tr["J"][0] + tr["J"][1])))
    fold(E, t["buckets"], errs)
    # the write-backs ride on exp, inverse, act and to_pose34
    res = [O.essential_graph_correct(p["x0"], p["x"], p["ref"], p["pts"]) for p in correct_problems()]
    E.update(correct_errors(res))
    # s3_to_pose34 alone has no counterpart in the oracle, and no transcendental function in it: a square root, two divisions and the
    # products of quat_to_R, each rounded once.  Its buckets get no oracle figure: the floor of the rule, 64 * 2.2e-16, is their bound
    for b in set(T["pose34"]["buckets"]):
        E[b] = 0.0
    E.update(explog_errors(np.stack([O.sim3_exp(O.sim3_log(S)) for S in T["log"]["inputs"]])))
    E.update(graph_errors([O.optimize_essential_graph(g["lie"], g["fixed"], g["ej"], g["ei"], g["Sji"]) for g in graph_problems()], None))
    return E


def write_golden():
    E = measure_oracle()
    k = sorted(E)
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    np.savez(GOLDEN, bucket=np.array(k), max_err=np.array([E[b] for b in k]))
    return E


if __name__ == "__main__":
    for b, e in sorted(write_golden().items()):
        print("%-44s %.3g" % (b, e))


def huber_side(term_out):
    """which side of the corrector each s3_term_eval output row [r 2, J 14, rho0] took, from the outputs alone: rho0 = |r|^2 on the
    quadratic side, 2 |r|^2 - huber^2 on the linear one (|r|^2 = huber sqrt(s) there); the two differ by |s - huber^2| >= 1e-6 huber^2"""
    o = np.asarray(term_out, np.float64).reshape(-1, 17)
    n2 = o[:, 0] ** 2 + o[:, 1] ** 2
    return np.abs(o[:, 16] - (2 * n2 - HUBER * HUBER)) < np.abs(o[:, 16] - n2)


def probe_report(outs):
    """everything asserted of one half of the probe's results: (bucket -> max e over all measured functions, outlier flags, Huber sides)"""
    m = {}
    for name in ORDER:
        if name != "outlier":
            m.update(bucket_maxima(name, outs[name]))
    return m, outs["outlier"][:, 0].astype(np.int64), huber_side(outs["term"])

"""CPU checks of the orbv_db_* entry points (KeyFrameDatabase): the symbols exist, every argument error is ORBHIP_EINVAL before any device work,
a zero or stale query_id is ORBHIP_EINVAL, valid calls fail loudly (ORBHIP_ENODEV) without a GPU, the structs match the header, and the drop-in
header with its test program compiles."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENODEV = -1, -2
NO_GPU = not os.path.exists("/dev/kfd")

NAMES = ("orbv_db_create", "orbv_db_destroy", "orbv_db_clear", "orbv_db_add", "orbv_db_erase", "orbv_db_size", "orbv_db_set_best_covisibles", "orbv_db_get_state",
         "orbv_db_min_score", "orbv_db_detect_loop_candidates", "orbv_db_detect_relocalization_candidates", "orbv_db_detect_loop_candidates_begin",
         "orbv_db_detect_relocalization_candidates_begin", "orbv_db_detect_candidates_finish", "orbv_db_pending_fields", "orbv_db_detect_loop_candidates_batch_device",
         "orbv_db_detect_relocalization_candidates_batch_device", "orbv_db_detect_workspace")


@pytest.fixture(scope="module")
def lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build_hip()
    from ceres_mono_orb_slam2_amd import _lib
    return _lib


@pytest.fixture()
def db(lib):
    h = C.c_void_p()
    assert lib.load().orbv_db_create(100, 0, C.byref(h)) == 0
    yield h
    assert lib.load().orbv_db_destroy(h) == 0


def test_symbols_are_exported(lib):
    L = lib.load()
    for name in NAMES:
        assert name in lib.SYMBOLS and getattr(L, name)
    from ceres_mono_orb_slam2_amd import KeyFrameDatabase
    assert KeyFrameDatabase.__module__ == "ceres_mono_orb_slam2_amd.keyframe_database"


def test_struct_layouts(lib, tmp_path):
    structs = (("orbv_db_query_info", lib.DbQueryInfo), ("orbv_db_trace", lib.DbTrace))
    body = ""
    for name, cls in structs:
        body += '  printf("%%zu ", sizeof(%s));\n' % name
        body += "".join('  printf("%%zu ", offsetof(%s, %s));\n' % (name, f) for f, _ in cls._fields_) + '  printf("\\n");\n'
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "orbslam_hip.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)]).decode().splitlines()
    for (name, cls), line in zip(structs, lines):
        got = [int(x) for x in line.split()]
        assert got[0] == C.sizeof(cls), name
        assert got[1:] == [getattr(cls, f).offset for f, _ in cls._fields_], name
    assert C.sizeof(lib.DbQueryInfo) == 32                 # the batched entries write rows of 8 x 4 bytes


def test_create_and_host_state_without_a_device(lib):
    L = lib.load()
    h = C.c_void_p()
    assert L.orbv_db_create(0, 0, C.byref(h)) == EINVAL
    assert L.orbv_db_create(100, -1, C.byref(h)) == EINVAL
    assert L.orbv_db_create(100, 0, None) == EINVAL
    assert L.orbv_db_create(100, 0, C.byref(h)) == 0
    assert L.orbv_db_size(h) == 0 and L.orbv_db_size(None) == EINVAL
    assert L.orbv_db_clear(h) == 0 and L.orbv_db_clear(None) == EINVAL
    assert L.orbv_db_erase(h, 5) == 0                       # not in the database: nothing to do, as the reference
    assert L.orbv_db_erase(h, -1) == EINVAL
    assert L.orbv_db_destroy(h) == 0 and L.orbv_db_destroy(None) == 0


def test_argument_errors(lib, db):
    L = lib.load()
    p = lib.ptr
    w = np.array([1, 5, 9], np.uint32); v = np.array([0.5, 0.25, 0.25])
    desc = np.array([5, 1, 9], np.uint32); same = np.array([1, 5, 5], np.uint32); big = np.array([1, 5, 100], np.uint32)
    cand = np.zeros(8, np.int32); n = C.c_int(0); ms = C.c_float(0)
    # add
    assert L.orbv_db_add(None, 0, p(w), p(v), 3) == EINVAL
    assert L.orbv_db_add(db, -1, p(w), p(v), 3) == EINVAL
    assert L.orbv_db_add(db, 0, None, p(v), 3) == EINVAL and L.orbv_db_add(db, 0, p(w), None, 3) == EINVAL
    assert L.orbv_db_add(db, 0, p(w), p(v), -1) == EINVAL
    assert L.orbv_db_add(db, 0, p(desc), p(v), 3) == EINVAL and b"ascend" in L.orbhip_last_error()
    assert L.orbv_db_add(db, 0, p(same), p(v), 3) == EINVAL
    assert L.orbv_db_add(db, 0, p(big), p(v), 3) == EINVAL and b"n_words" in L.orbhip_last_error()
    # neighbours
    nb = np.arange(11, dtype=np.int32)
    assert L.orbv_db_set_best_covisibles(db, 0, p(nb), 11) == EINVAL
    assert L.orbv_db_set_best_covisibles(db, -1, p(nb), 3) == EINVAL
    assert L.orbv_db_set_best_covisibles(db, 0, None, 3) == EINVAL
    assert L.orbv_db_set_best_covisibles(db, 0, p(np.array([1, -2], np.int32)), 2) == EINVAL
    # state / min_score
    q = np.zeros(2, np.int64); s = np.zeros(2, np.float32)
    assert L.orbv_db_get_state(db, p(np.array([0, 1], np.int32)), 2, p(q), p(s)) == EINVAL           # slots the database has never seen
    assert L.orbv_db_get_state(db, None, 2, p(q), p(s)) == EINVAL
    assert L.orbv_db_min_score(db, p(w), p(v), 3, p(np.array([0], np.int32)), 1, C.byref(ms)) == EINVAL and b"not in the database" in L.orbhip_last_error()
    assert L.orbv_db_min_score(db, p(w), p(v), 3, None, 0, None) == EINVAL
    assert L.orbv_db_min_score(db, p(desc), p(v), 3, None, 0, C.byref(ms)) == EINVAL
    assert L.orbv_db_min_score(db, p(w), p(v), 3, None, 0, C.byref(ms)) == 0 and ms.value == 1.0     # no covisible keyframe: minScore stays 1
    # queries
    assert L.orbv_db_detect_loop_candidates(None, p(w), p(v), 3, None, 0, 0.0, 1, p(cand), 8, C.byref(n), None) == EINVAL
    assert L.orbv_db_detect_loop_candidates(db, p(w), p(v), 3, None, 2, 0.0, 1, p(cand), 8, C.byref(n), None) == EINVAL
    assert L.orbv_db_detect_loop_candidates(db, p(w), p(v), 3, None, 0, 0.0, 1, None, 8, C.byref(n), None) == EINVAL
    assert L.orbv_db_detect_loop_candidates(db, p(w), p(v), 3, None, 0, 0.0, 1, p(cand), 8, None, None) == EINVAL
    assert L.orbv_db_detect_loop_candidates(db, p(w), p(v), 3, None, 0, 0.0, 1, p(cand), -1, C.byref(n), None) == EINVAL
    assert L.orbv_db_detect_loop_candidates(db, p(desc), p(v), 3, None, 0, 0.0, 1, p(cand), 8, C.byref(n), None) == EINVAL
    assert L.orbv_db_detect_relocalization_candidates(db, p(big), p(v), 3, 1, p(cand), 8, C.byref(n), None) == EINVAL
    t = lib.DbTrace(None, None, None, None, None, -1, 0)
    assert L.orbv_db_detect_relocalization_candidates(db, p(w), p(v), 3, 1, p(cand), 8, C.byref(n), C.byref(t)) == EINVAL
    assert L.orbv_db_detect_relocalization_candidates_begin(db, p(w), p(v), 3, 1, None, 8, C.byref(n)) == EINVAL
    assert L.orbv_db_detect_loop_candidates_begin(db, p(w), p(v), 3, None, 0, 0.0, 1, p(cand), 8, None) == EINVAL
    assert L.orbv_db_detect_candidates_finish(db, None, None, p(cand), 8, C.byref(n), None) == EINVAL and b"no query pending" in L.orbhip_last_error()
    info = lib.DbQueryInfo()
    assert L.orbv_db_pending_fields(db, C.byref(info), p(cand), p(s), 8) == EINVAL and b"no query pending" in L.orbhip_last_error()
    assert L.orbv_db_pending_fields(db, None, p(cand), p(s), 8) == EINVAL
    # batched
    sz = C.c_size_t(0)
    assert L.orbv_db_detect_workspace(db, 0, C.byref(sz)) == EINVAL and L.orbv_db_detect_workspace(db, 70000, C.byref(sz)) == EINVAL
    assert L.orbv_db_detect_workspace(db, 4, None) == EINVAL
    assert L.orbv_db_detect_workspace(db, 4, C.byref(sz)) == 0 and sz.value > 0
    x = C.c_void_p(256)                                                                  # (never dereferenced: the checks come first)
    assert L.orbv_db_detect_relocalization_candidates_batch_device(db, 0, x, x, x, 1, x, x, 4, x, sz.value, None) == EINVAL
    assert L.orbv_db_detect_relocalization_candidates_batch_device(db, 4, None, x, x, 1, x, x, 4, x, sz.value, None) == EINVAL
    assert L.orbv_db_detect_relocalization_candidates_batch_device(db, 4, x, x, x, 1, x, x, 4, None, sz.value, None) == EINVAL
    assert L.orbv_db_detect_relocalization_candidates_batch_device(db, 4, x, x, x, 1, x, x, 4, x, sz.value - 1, None) == EINVAL
    assert L.orbv_db_detect_loop_candidates_batch_device(db, 4, x, x, x, None, x, x, 1, x, x, 4, x, sz.value, None) == EINVAL
    assert L.orbv_db_detect_loop_candidates_batch_device(db, 4, x, x, x, x, x, None, 1, x, x, 4, x, sz.value, None) == EINVAL
    assert L.orbv_db_detect_relocalization_candidates_batch_device(db, 4, x, x, x, 0, x, x, 4, x, sz.value, None) == EINVAL      # query id 0
    # none of the refused calls used up a query id
    assert L.orbv_db_detect_relocalization_candidates(db, p(w), p(v), 3, 1, p(cand), 8, C.byref(n), None) in (0, ENODEV)


def test_zero_and_stale_query_ids(lib, db):
    """Per kind of query an id of 0, a negative one, or one not greater than the last id used is ORBHIP_EINVAL.  An id is used up once a call's
    arguments have passed - also when the call then finds no device - so the rule can be seen here too."""
    L = lib.load()
    p = lib.ptr
    w = np.array([1, 5, 9], np.uint32); v = np.array([0.5, 0.25, 0.25]); cand = np.zeros(8, np.int32); n = C.c_int(0)
    ok = (0, ENODEV)

    def reloc(qid):
        return L.orbv_db_detect_relocalization_candidates(db, p(w), p(v), 3, qid, p(cand), 8, C.byref(n), None)

    def loop(qid):
        return L.orbv_db_detect_loop_candidates(db, p(w), p(v), 3, None, 0, 0.0, qid, p(cand), 8, C.byref(n), None)
    assert reloc(0) == EINVAL and reloc(-3) == EINVAL and loop(0) == EINVAL
    assert reloc(5) in ok
    assert reloc(5) == EINVAL and b"query_id" in L.orbhip_last_error()
    assert reloc(4) == EINVAL
    assert loop(3) in ok                                       # the two kinds count separately, as the two fields of the reference do
    assert loop(3) == EINVAL and loop(2) == EINVAL
    assert L.orbv_db_detect_relocalization_candidates_begin(db, p(w), p(v), 3, 5, p(cand), 8, C.byref(n)) == EINVAL
    assert reloc(6) in ok and loop(2 ** 40) in ok and loop(2 ** 40) == EINVAL
    assert L.orbv_db_clear(db) == 0                            # clear forgets the ids
    assert reloc(1) in ok


@pytest.mark.skipif(not NO_GPU, reason="GPU present: the no-device error path cannot be exercised")
def test_compute_entries_fail_loudly_without_gpu(lib, db):
    from ceres_mono_orb_slam2_amd import KeyFrameDatabase
    from ceres_mono_orb_slam2_amd._lib import OrbHipError
    L = lib.load()
    p = lib.ptr
    w = np.array([1, 5, 9], np.uint32); v = np.array([0.5, 0.25, 0.25]); cand = np.zeros(8, np.int32); n = C.c_int(0)
    assert L.orbv_db_add(db, 0, p(w), p(v), 3) == ENODEV and b"no HIP device" in L.orbhip_last_error()
    assert L.orbv_db_set_best_covisibles(db, 0, p(np.array([1], np.int32)), 1) == ENODEV
    assert L.orbv_db_detect_loop_candidates(db, p(w), p(v), 3, None, 0, 0.0, 1, p(cand), 8, C.byref(n), None) == ENODEV
    assert L.orbv_db_detect_relocalization_candidates(db, p(w), p(v), 3, 1, p(cand), 8, C.byref(n), None) == ENODEV
    assert L.orbv_db_detect_loop_candidates_begin(db, p(w), p(v), 3, None, 0, 0.0, 2, p(cand), 8, C.byref(n)) == ENODEV
    assert L.orbv_db_detect_relocalization_candidates_begin(db, p(w), p(v), 3, 2, p(cand), 8, C.byref(n)) == ENODEV
    sz = C.c_size_t(0)
    assert L.orbv_db_detect_workspace(db, 2, C.byref(sz)) == 0
    x = C.c_void_p(256)
    assert L.orbv_db_detect_relocalization_candidates_batch_device(db, 2, x, x, x, 3, x, x, 4, x, sz.value, None) == ENODEV
    assert L.orbv_db_detect_loop_candidates_batch_device(db, 2, x, x, x, x, x, x, 3, x, x, 4, x, sz.value, None) == ENODEV
    assert L.orbv_db_size(db) == 0
    kf = KeyFrameDatabase(100)
    with pytest.raises(OrbHipError, match="no HIP device"):
        kf.add(0, (w, v))
    with pytest.raises(OrbHipError, match="no HIP device"):
        kf.detect_relocalization_candidates((w, v), 1)
    with pytest.raises(OrbHipError, match="word ids must ascend"):
        kf.add(0, (w[::-1], v))


def test_dropin_header_compiles(lib, tmp_path):
    """csrc/compat/orbslam_keyframedatabase.h: the test program links against the library (it runs on the GPU box: tests/test_gpu_kfdb_dropin.py), and
    the `#ifdef ORBSLAM_DROPIN_REFERENCE_TYPES` branch compiles with every member instantiated over the mock data model (a spelling / type check
    of our header, not a build of the reference)."""
    inc = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall"] + inc + [os.path.join(ROOT, "tests", "cpp", "test_keyframedatabase_reference_types.cpp")])
    exe = tmp_path / "test_keyframedatabase_dropin"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall"] + inc + [os.path.join(ROOT, "tests", "cpp", "test_keyframedatabase_dropin.cpp"), "-o", str(exe),
                           lib.LIB_PATH, "-lpthread", "-Wl,-rpath," + os.path.dirname(lib.LIB_PATH), "-Wl,-rpath,/opt/rocm/lib"])
    assert exe.exists()

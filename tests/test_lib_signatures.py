"""The ctypes signatures _lib derives from include/orbslam_hip.h, held to what the C++ compiler reads in the same header: a program that
instantiates a template on decltype(&name) for every declared function prints each return and parameter type as a kind (pointer,
floating, integer, void) and a size.  The names come from test_abi's own regex, not from the parser under test.  No GPU, no linking."""
import ctypes as C
import os
import subprocess

import pytest

from ceres_mono_orb_slam2_amd import _lib
from tests.test_abi import ROOT, _declared_functions

PROGRAM = r"""
#include <cstdio>
#include <type_traits>
#include "orbslam_hip.h"
template <class T> void kind() {
  if constexpr (std::is_void_v<T>) std::printf(" v0");
  else std::printf(" %c%zu", std::is_pointer_v<T> ? 'p' : std::is_floating_point_v<T> ? 'f' : std::is_integral_v<T> ? 'i' : '?', sizeof(T));
}
template <class F> struct Sig;
template <class R, class... A> struct Sig<R (*)(A...)> {
  static void print(const char* name) { std::printf("%s", name); kind<R>(); (kind<A>(), ...); std::printf("\n"); }
};
int main() {
@CALLS@
  return 0;
}
"""


def _kind(t):
    if t is None:
        return "v0"
    if issubclass(t, (C.c_void_p, C.c_char_p, C._Pointer)):
        return "p%d" % C.sizeof(t)
    return ("f%d" if t in (C.c_float, C.c_double) else "i%d") % C.sizeof(t)


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """{name: [return kind, parameter kinds...]} as the host compiler sees the header"""
    d = tmp_path_factory.mktemp("signatures")
    src, exe = d / "signatures.cpp", d / "signatures"
    src.write_text(PROGRAM.replace("@CALLS@", "\n".join('  Sig<decltype(&%s)>::print("%s");' % (n, n) for n in _declared_functions())))
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    rows = [line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines()]
    return {r[0]: r[1:] for r in rows}


def test_derived_signatures_match_the_compiler(compiled):
    with open(_lib.HEADER_PATH) as f:
        derived = _lib.parse_header(f.read())
    assert len(compiled) >= 167 and sorted(compiled) == sorted(derived) == _declared_functions()
    for name, (restype, argtypes) in derived.items():
        want = compiled[name]
        assert len(argtypes) == len(want) - 1, "%s: %d parameters derived, the compiler sees %d" % (name, len(argtypes), len(want) - 1)
        assert _kind(restype) == want[0], "%s: return type %s, the compiler sees %s" % (name, _kind(restype), want[0])
        for i, t in enumerate(argtypes):
            assert _kind(t) == want[1 + i], "%s: parameter %d is %s (%s), the compiler sees %s" % (name, i, t.__name__, _kind(t), want[1 + i])


def test_load_binds_every_declared_function():
    import __graft_entry__ as g
    g.build_hip()
    L = _lib.load()
    with open(_lib.HEADER_PATH) as f:
        derived = _lib.parse_header(f.read())
    for name in _lib.SYMBOLS:
        f = getattr(L, name)
        assert f.argtypes is not None, name                                      # (ctypes' default: None = convert whatever comes)
        assert (f.restype, list(f.argtypes)) == (derived[name][0], derived[name][1]), name


def test_symbols_has_no_duplicates():
    assert len(_lib.SYMBOLS) == len(set(_lib.SYMBOLS)) >= 167


def test_parser_reads_the_forms_the_header_uses():
    text = """
    #define ORB_X(a) \\
       int not_a_declaration(int a);
    typedef struct orb_s { int a; float b[4]; } orb_s;   // int neither(void);
    /* int nor_this(int); */
    const char* orb_name(void);
    void orb_free(orb_s* s);
    double orb_f(const volatile float* a /*[n]*/, int64_t n, size_t bytes, float K[4], long long id,
                 uint32_t* const out, orb_s** h, const ba_summary* s, const char* path);
    """
    sig = _lib.parse_header(text)
    assert list(sig) == ["orb_name", "orb_free", "orb_f"]
    assert sig["orb_name"] == (C.c_char_p, []) and sig["orb_free"] == (None, [C.c_void_p])
    ret, args = sig["orb_f"]
    assert ret is C.c_double and args[:7] == [C.c_void_p, C.c_int64, C.c_size_t, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p] and args[8] is C.c_char_p
    s = _lib.BaSummary()
    assert args[7].from_param(s)._obj is s and isinstance(args[7].from_param(None), (type(None), C.c_void_p)) and C.sizeof(args[7]) == C.sizeof(C.c_void_p)


def test_unknown_scalar_type_raises_and_names_the_declaration():
    text = "int orb_a(int n);\nint orb_b(const float* x,\n          unsigned short n);\n"
    with pytest.raises(_lib.OrbHipError, match="orb_b.*unsigned short"):
        _lib.parse_header(text)

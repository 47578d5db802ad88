"""The reference compiled as C (oracle/_ref/libaomref_c.so, built by oracle/ref_build.py) behind ctypes: the second opinion that neither
the oracle's restatement nor the fixture interpreter had a hand in.  A plain helper module, imported by the tests that need it.

    lib()                  the library, rtcd tables and wedge masks initialised once
    fn(name, restype)      a function with argtypes set from the arguments' kinds (see call())
    call(f, *args)         numpy arrays / Ptr go as c_void_p, Python ints as c_int, ctypes values as they are

Pointer arguments are always c_void_p: a bare Python int would be truncated to a 32-bit int by ctypes' default conversion."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_DIR = os.path.join(ROOT, "oracle", "_ref")
LIB_PATH = os.path.join(REF_DIR, "libaomref_c.so")
SHIM_PATH = os.path.join(REF_DIR, "librefshim.so")

_lib = None


def reference_tree():
    return os.environ.get("AOMHIP_REFERENCE_DIR", "/root/reference")


def _open(path):
    """Missing library: a failure where the reference tree exists (build() makes the library there), a skip where neither exists."""
    if not os.path.exists(path):
        what = os.path.relpath(path, ROOT)
        if os.path.isdir(reference_tree()):
            pytest.fail("%s is missing although the reference tree %s exists: run build()" % (what, reference_tree()), pytrace=False)
        pytest.skip("%s is missing and there is no reference tree to build it from" % what)
    return C.CDLL(path, mode=C.RTLD_GLOBAL)


def lib():
    global _lib
    if _lib is None:
        l = _open(LIB_PATH)
        for init in ("aom_dsp_rtcd", "av1_rtcd", "aom_scale_rtcd", "av1_init_wedge_masks"):
            f = getattr(l, init)
            f.restype, f.argtypes = None, []
            f()
        _lib = l
    return _lib


_shim = None


def shim():
    """oracle/_ref/librefshim.so (oracle/refshim/*.c): flat entry points around what is `static` in the reference; it resolves the
    reference's functions from libaomref_c.so, loaded first"""
    global _shim
    if _shim is None:
        lib()
        _shim = _open(SHIM_PATH)
    return _shim


def has(name):
    return hasattr(lib(), name)


class Ptr:
    """A pointer into a numpy array: element offset `at`; hbd = the reference's byte-pointer encoding of 16-bit planes,
    CONVERT_TO_BYTEPTR(x) = (uint8_t *)((uintptr_t)x >> 1) (aom_ports/mem.h:79-80)."""

    def __init__(self, a, at=0, hbd=False):
        self.a, self.at, self.hbd = a, int(at), hbd

    @property
    def value(self):
        addr = self.a.ctypes.data + self.at * self.a.itemsize
        if self.hbd:
            assert self.a.itemsize == 2 and addr % 2 == 0
            addr >>= 1
        return addr


class PtrList:
    """const uint8_t *const ref_array[n]: a C array of pointers, built (and kept alive) when the call is made"""

    def __init__(self, ptrs):
        self.ptrs, self.carr = list(ptrs), None


def byteptr(a, at=0):
    """CONVERT_TO_BYTEPTR of &a.flat[at] for a uint16 array"""
    return Ptr(a, at, hbd=True)


def carg(x):
    """one argument as a ctypes value: every pointer a c_void_p, every Python int a c_int"""
    if x is None:
        return C.c_void_p(None)
    if isinstance(x, np.ndarray):
        return C.c_void_p(x.ctypes.data)
    if isinstance(x, Ptr):
        return C.c_void_p(x.value)
    if isinstance(x, PtrList):
        x.carr = (C.c_void_p * len(x.ptrs))(*[carg(p).value for p in x.ptrs])
        return C.c_void_p(C.addressof(x.carr))
    if isinstance(x, (bool, int, np.integer)):
        return C.c_int(int(x))
    if isinstance(x, (C.Structure, C.Array)):
        return C.c_void_p(C.addressof(x))
    return x   # already a ctypes value (c_ssize_t, c_int64, byref(...), c_void_p)


def fn(name, restype=None, library=None):
    """library[name] is a function object of its own: setting its argtypes leaves the ones other modules set on library.name alone"""
    f = (library if library is not None else lib())[name]
    f.restype = restype
    return f


def call(f, *args):
    """f(*args) with argtypes set for this call from the converted arguments, so nothing goes through ctypes' default int conversion"""
    cargs = [carg(a) for a in args]
    f.argtypes = [type(a) for a in cargs]
    return f(*cargs)


def clone(x, memo):
    """an argument with its numpy buffers copied; memo (id -> copy) keeps two pointers into one buffer in one copy"""
    if isinstance(x, np.ndarray):
        if id(x) not in memo:
            memo[id(x)] = x.copy()
        return memo[id(x)]
    if isinstance(x, Ptr):
        return Ptr(clone(x.a, memo), x.at, x.hbd)
    if isinstance(x, PtrList):
        return PtrList([clone(p, memo) for p in x.ptrs])
    return x


def run_pair(fa, fb, args, what, ignore=None):
    """Calls fa and fb with the same arguments, each on its own copy of every buffer, and requires equal return values and equal
    buffers afterwards, inputs and guard regions included.  ignore = {buffer index: slice of the flattened buffer} names a region
    that the reference leaves as scratch: it is left out of the comparison (and of `wrote`).
    -> (fb's return value, fb's buffers in argument order, whether fb wrote)."""
    res = []
    for f in (fa, fb):
        memo = {}
        a = [clone(x, memo) for x in args]
        r = call(f, *a)
        res.append((r, list(memo.values())))
    assert res[0][0] == res[1][0], (what, "return value", res[0][0], res[1][0])
    before = [x.copy() for x in _arrays(args)]
    for i, sl in (ignore or {}).items():
        for bufs in (res[0][1], res[1][1], before):
            bufs[i].reshape(-1)[sl] = 0
    for i, (g, w) in enumerate(zip(res[0][1], res[1][1])):
        if not np.array_equal(g, w):
            bad = np.flatnonzero(g.ravel() != w.ravel())
            raise AssertionError((what, "buffer %d" % i, "%d of %d differ, first at %d: %r != %r" % (bad.size, g.size, bad[0], g.ravel()[bad[0]], w.ravel()[bad[0]])))
    wrote = any(not np.array_equal(b, a) for b, a in zip(before, res[1][1]))
    return res[1][0], res[1][1], wrote


def _arrays(args):
    seen, out = set(), []

    def walk(x):
        if isinstance(x, np.ndarray):
            if id(x) not in seen:
                seen.add(id(x))
                out.append(x)
        elif isinstance(x, Ptr):
            walk(x.a)
        elif isinstance(x, PtrList):
            for p in x.ptrs:
                walk(p)
    for x in args:
        walk(x)
    return out

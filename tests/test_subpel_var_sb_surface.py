"""aomhip_sub_pixel_variance_sb_batch exists on every layer: declared in include/aomhip.h, exported by libaomhip.so, bound in capi (prototype
table, EXPORTED, a Context method) -- and so does its test-support counter aomhip_debug_subpel_sb_fallbacks.  No GPU needed."""
import ctypes
import os
import re

from conftest import ROOT

NAME = "aomhip_sub_pixel_variance_sb_batch"
DEBUG = "aomhip_debug_subpel_sb_fallbacks"


def _header():
    src = open(os.path.join(ROOT, "include", "aomhip.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_declares_the_entry_point_with_17_arguments():
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % NAME, _header())
    assert m, "include/aomhip.h does not declare " + NAME
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 17, args
    assert args[0].startswith("aomhip_ctx") and "aomhip_var_cand" in args[11] and "int32_t" in args[12] and "int64_t" in args[14]
    assert re.search(r"\bint\s+%s\s*\(\s*aomhip_ctx\s*\*\s*\w+\s*\)\s*;" % DEBUG, _header())


def test_library_exports_the_symbols(hip):
    lib = ctypes.CDLL(hip.capi.LIB_PATH)
    assert hasattr(lib, NAME) and hasattr(lib, DEBUG)


def test_binding_has_prototype_and_method(hip):
    capi = hip.capi
    assert NAME in capi.EXPORTED and DEBUG in capi.EXPORTED
    fn = getattr(capi.lib, NAME)
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 17
    assert fn.argtypes[14] is ctypes.c_int64
    assert callable(getattr(capi.Context, "sub_pixel_variance_sb_batch")) and callable(getattr(capi.Context, "debug_subpel_sb_fallbacks"))


def test_header_points_sub_pixel_lists_at_the_bucketed_call():
    src = open(os.path.join(ROOT, "include", "aomhip.h")).read()
    doc = src[src.index("aom_varianceWxH / aom_highbd_{10,12}_varianceWxH (aom_dsp/variance.c:56-163,383-420) through the SAME strip walk"):]
    doc = doc[:doc.index("int aomhip_variance_sb_batch")]
    assert NAME in doc

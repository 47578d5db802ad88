"""The av1_rtcd transform / quantisation surface (include/aomhip.h "the av1_rtcd transform / quantisation surface"), checked without a GPU:
every member of aomhip_rtcd_av1_table has an exact-signature entry point whose parameter types equal its add_proto line token by token,
the library and the binding export them with the two batched block-error calls, and aomhip_txfm_param has TxfmParam's layout
(aom_dsp/txfm_common.h:89-101) as a C compiler sees it."""
import ctypes
import os
import re
import subprocess

from conftest import ROOT
from test_rtcd_protos import header_protos, reference_protos

TX = ["4x4", "8x8", "16x16", "32x32", "64x64", "4x8", "8x4", "8x16", "16x8", "16x32", "32x16", "32x64", "64x32", "4x16", "16x4", "8x32", "32x8",
      "16x64", "64x16"]
# the 36 members of aomhip_rtcd_av1_table in order -> the entry point installed there and the reference proto it matches (None: no proto)
MEMBERS = ([("inv_txfm_add", "aomhip_inv_txfm_add", "av1_inv_txfm_add"),
            ("highbd_inv_txfm_add", "aomhip_highbd_inv_txfm_add", "av1_highbd_inv_txfm_add")] +
           [("highbd_inv_txfm_add_sz[%d]" % i, "aomhip_highbd_inv_txfm_add_" + s, None if s == "16x16" else "av1_highbd_inv_txfm_add_" + s)
            for i, s in enumerate(TX)] +
           [("highbd_iwht4x4_1_add", "aomhip_highbd_iwht4x4_1_add", "av1_highbd_iwht4x4_1_add"),
            ("highbd_iwht4x4_16_add", "aomhip_highbd_iwht4x4_16_add", "av1_highbd_iwht4x4_16_add"),
            ("lowbd_fwd_txfm", "aomhip_lowbd_fwd_txfm", "av1_lowbd_fwd_txfm"),
            ("fwht4x4", "aomhip_fwht4x4", "av1_fwht4x4"),
            ("round_shift_array", "aomhip_round_shift_array", "av1_round_shift_array"),
            ("block_error", "aomhip_block_error", "av1_block_error"),
            ("block_error_lp", "aomhip_block_error_lp", "av1_block_error_lp"),
            ("highbd_block_error", "aomhip_highbd_block_error", "av1_highbd_block_error"),
            ("quantize_fp", "aomhip_quantize_fp", "av1_quantize_fp"),
            ("quantize_fp_32x32", "aomhip_quantize_fp_32x32", "av1_quantize_fp_32x32"),
            ("quantize_fp_64x64", "aomhip_quantize_fp_64x64", "av1_quantize_fp_64x64"),
            ("highbd_quantize_fp", "aomhip_highbd_quantize_fp", "av1_highbd_quantize_fp"),
            ("quantize_lp", "aomhip_quantize_lp", "av1_quantize_lp"),
            ("cdef_copy_rect8_8bit_to_16bit", "aomhip_cdef_copy_rect8_8bit_to_16bit", "cdef_copy_rect8_8bit_to_16bit"),
            ("cdef_copy_rect8_16bit_to_16bit", "aomhip_cdef_copy_rect8_16bit_to_16bit", "cdef_copy_rect8_16bit_to_16bit")])
# (test_rtcd_protos._param_type keeps the name of a parameter whose type is a library struct: "aomhip_ctx * ctx")
BATCHED = {"aomhip_block_error_batch": ("int", ["aomhip_ctx * ctx", "const int32_t *", "const int32_t *", "int", "int", "int", "int", "int64_t *"]),
           "aomhip_block_error_lp_batch": ("int", ["aomhip_ctx * ctx", "const int16_t *", "const int16_t *", "int", "int", "int64_t *"])}


def test_table_members_are_the_36_exact_signature_entry_points():
    assert len(MEMBERS) == 36
    ref, hdr = reference_protos(), header_protos()
    missing = [name for _, name, _ in MEMBERS if name not in hdr]
    assert not missing, missing
    matched = []
    for _, name, proto in MEMBERS:
        if proto is None:   # the 16x16 highbd form the reference does not declare: the same signature as its 18 siblings
            assert hdr[name] == ref["av1_highbd_inv_txfm_add_8x8"], name
            continue
        assert proto in ref, proto
        assert hdr[name] == ref[proto], (name, hdr[name], proto, ref[proto])
        matched.append(proto)
    assert len(matched) == 35
    # test_rtcd_protos' own walk (aomhip_X -> aom_X / av1_X / X) reaches the same protos: the new names are in its comparison
    walked = set()
    for name in hdr:
        stem = name[len("aomhip_"):]
        for cand in ("aom_" + stem, "av1_" + stem, stem):
            if cand in ref:
                walked.add(cand)
                break
    assert set(matched) <= walked


def test_table_layout_in_the_header():
    src = subprocess.run(["gcc", "-E", "-P", os.path.join(ROOT, "include", "aomhip.h")], check=True, capture_output=True, text=True).stdout
    body = re.search(r"typedef struct aomhip_rtcd_av1_table \{(.*?)\} aomhip_rtcd_av1_table;", src, re.S).group(1)
    members = []
    for decl in [d.strip() for d in body.split(";") if d.strip()]:
        m = re.match(r"(?:aomhip_\w+_fn)\s+(.*)$", decl, re.S)
        if m:   # "aomhip_x_fn a, b, c[19]"
            for part in m.group(1).split(","):
                part = part.strip()
                a = re.match(r"(\w+)\[(\d+)\]$", part)
                members += ["%s[%d]" % (a.group(1), i) for i in range(int(a.group(2)))] if a else [part]
        else:   # "ret (*name)(...)"
            members.append(re.search(r"\(\s*\*\s*(\w+)\s*\)", decl).group(1))
    assert members == [m for m, _, _ in MEMBERS]


def test_batched_block_error_declarations():
    hdr = header_protos()
    for name, sig in BATCHED.items():
        assert hdr.get(name) == sig, (name, hdr.get(name))


def test_library_and_binding_export_the_surface(hip):
    lib = ctypes.CDLL(hip.capi.LIB_PATH)
    names = [n for _, n, _ in MEMBERS] + list(BATCHED) + ["aomhip_rtcd_av1"]
    assert not [n for n in names if not hasattr(lib, n)]
    assert not [n for n in names if n not in hip.capi.EXPORTED]
    assert sorted(hip.capi.RTCD_AV1_STAMPED) == sorted(["aomhip_highbd_inv_txfm_add_" + s for s in TX] +
                                                        ["aomhip_quantize_fp", "aomhip_quantize_fp_32x32", "aomhip_quantize_fp_64x64"])
    assert not set(hip.capi.RTCD_AV1_STAMPED) & set(hip.capi.RTCD_STAMPED)
    # without a device the installer keeps the caller's pointers: an all-NULL table and AOMHIP_ERR_NO_DEVICE
    if hip.capi.lib.aomhip_device_count() <= 0:
        table = (ctypes.c_void_p * 36)(*([1] * 36))
        assert hip.capi.lib.aomhip_rtcd_av1(table) == 1
        assert not any(table)


def test_txfm_param_layout_is_txfmparam(tmp_path):
    prog = tmp_path / "layout.c"
    prog.write_text("""#include <stdio.h>
#include "aomhip.h"
int main(void) {
  printf("%d %d %d %d %d %d %d %d\\n", (int)offsetof(aomhip_txfm_param, tx_type), (int)offsetof(aomhip_txfm_param, tx_size),
         (int)offsetof(aomhip_txfm_param, lossless), (int)offsetof(aomhip_txfm_param, bd), (int)offsetof(aomhip_txfm_param, is_hbd),
         (int)offsetof(aomhip_txfm_param, tx_set_type), (int)offsetof(aomhip_txfm_param, eob), (int)sizeof(aomhip_txfm_param));
  printf("%d %d\\n", (int)sizeof(((aomhip_txfm_param *)0)->tx_type), (int)sizeof(((aomhip_txfm_param *)0)->tx_set_type));
  return 0;
}
""")
    exe = tmp_path / "layout"
    for std in ("-std=c99", "-std=c11"):   # the C99 fallback of the header's static assertion and _Static_assert
        subprocess.run(["gcc", std, "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)],
                       check=True)
        out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
        assert [int(v) for v in out[0].split()] == [0, 1, 4, 8, 12, 16, 20, 24]
        assert [int(v) for v in out[1].split()] == [1, 1]

"""The binding states the C ABI once (_capi.SIGNATURES, _capi.RECORDS and the constants); this file holds each statement
against include/ffl.h itself: every prototype parameter by parameter in its ABI class, every record field by field against
the header compiled as plain C99, every integer macro by value.  No device is needed."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from funscript_flow_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")


def stripped(text):
    """the header without comments"""
    return re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))


HEADER = stripped(open(os.path.join(INCLUDE, "ffl.h")).read())

# ---- (a) prototypes -----------------------------------------------------------------------------------------------------------
# the ABI class of every C type the header may use in a prototype; anything else is reported, not guessed
C_CLASS = {"int": "i32", "int32_t": "i32", "unsigned": "u32", "float": "f32", "double": "f64", "ptrdiff_t": "i64",
           "size_t": "u64", "uint64_t": "u64", "void": "void"}
PROTOTYPE = re.compile(r"((?:const\s+)?\b\w+\b[\s*]+)(ffl_\w+)\s*\(([^()]*)\)\s*;")


def c_class(decl, named):
    """ABI class of a return type, or of a parameter with its name ("const int *slots", "int win[4]", "ptrdiff_t stride")"""
    if "*" in decl or "[" in decl:
        return "ptr"
    words = [w for w in decl.split() if w != "const"]
    ctype = " ".join(words[:-1] if named and len(words) > 1 else words)
    return C_CLASS.get(ctype, f"unknown C type {ctype!r}")


def ctypes_class(t):
    if t is None:
        return "void"
    if t in (C.c_void_p, C.c_char_p) or issubclass(t, (C._Pointer, C.Array)):
        return "ptr"
    if not issubclass(t, C._SimpleCData):
        return f"unknown ctypes type {t!r}"
    bits = 8 * C.sizeof(t)
    return ("f" if t._type_ in "fd" else "i" if t._type_ in "bhilq" else "u") + str(bits)


def prototypes(text):
    """{name: (return class, [parameter classes])} of every `ret ffl_name(params);`, in order.  Every `ffl_name(` of the
    text must have been read as a prototype: one the pattern cannot read fails here and is not skipped."""
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)
    found = PROTOTYPE.findall(text)
    assert len(found) == len(re.findall(r"\bffl_\w+\s*\(", text)), "a declaration of ffl.h was not read as a prototype"
    out = {}
    for ret, name, params in found:
        params = [p.strip() for p in params.split(",")]
        params = [] if params == ["void"] else params
        assert name not in out and all(params), (name, params)
        out[name] = (c_class(ret, False), [c_class(p, True) for p in params])
    return out


def differences(text, table):
    """[(symbol, what differs)] between the prototypes of a header text and a signature table; [] when they agree"""
    protos, diffs = prototypes(text), []
    diffs += [(n, "declared in the header, missing in the table") for n in protos if n not in table]
    diffs += [(n, "in the table, not declared in the header") for n in table if n not in protos]
    for name, (ret, params) in protos.items():
        if name not in table:
            continue
        restype, argtypes = table[name]
        if ctypes_class(restype) != ret:
            diffs.append((name, f"returns {ret}, the table says {ctypes_class(restype)}"))
        if len(argtypes) != len(params):
            diffs.append((name, f"{len(params)} parameters, the table has {len(argtypes)}"))
            continue
        diffs += [(name, f"parameter {k} is {want}, the table says {ctypes_class(t)}")
                  for k, (want, t) in enumerate(zip(params, argtypes)) if ctypes_class(t) != want]
    if not diffs and list(protos) != list(table):
        diffs.append((next(a for a, b in zip(protos, table) if a != b), "the table is not in the header's order"))
    return diffs


def test_every_prototype_matches_the_signature_table():
    assert len(prototypes(HEADER)) >= 74
    assert differences(HEADER, _capi.SIGNATURES) == []
    assert _capi.EXPORTS == list(_capi.SIGNATURES) == list(prototypes(HEADER))


def test_load_applies_the_table_to_every_symbol():
    L = _capi.load()
    for name, (restype, argtypes) in _capi.SIGNATURES.items():
        fn = getattr(L, name)
        assert fn.restype is restype and tuple(fn.argtypes) == tuple(argtypes), name


# ---- (b) the checker is not vacuous -------------------------------------------------------------------------------------------
def mutated(symbol, old, new):
    """the header with `old` replaced by `new` inside the prototype of `symbol` alone"""
    m = re.search(rf"\b{symbol}\s*\([^()]*\)", HEADER)
    assert m and m.group(0).count(old) == 1, (symbol, old)
    return HEADER[:m.start()] + m.group(0).replace(old, new) + HEADER[m.end():]


@pytest.mark.parametrize("symbol, old, new, words", [
    ("ffl_export_flows", "uint64_t stream", "int stream", "parameter 6 is i32, the table says u64"),
    ("ffl_upload_frame", "ptrdiff_t stride_bytes", "int stride_bytes", "parameter 6 is i32, the table says i64"),
    ("ffl_flow_pairs", ", int pov_mode", "", "5 parameters, the table has 6"),
    ("ffl_host_alloc", "size_t bytes", "unsigned bytes", "parameter 1 is u32, the table says u64"),
    ("ffl_radial", "double *out", "double out", "parameter 7 is f64, the table says ptr"),
    ("ffl_radial_window", "int n_seq", "long n_seq", "parameter 1 is unknown C type 'long', the table says i32"),
])
def test_a_changed_prototype_is_reported_for_its_symbol(symbol, old, new, words):
    assert differences(mutated(symbol, old, new), _capi.SIGNATURES) == [(symbol, words)]


def test_a_changed_table_is_reported_for_its_symbol():
    table = dict(_capi.SIGNATURES)
    del table["ffl_sync"]
    assert differences(HEADER, table) == [("ffl_sync", "declared in the header, missing in the table")]
    for name, k, wrong, words in (("ffl_import_flows", 6, C.c_int, "parameter 6 is u64, the table says i32"),
                                  ("ffl_cells_extra_bytes", 3, C.c_size_t, "parameter 3 is ptr, the table says u64")):
        restype, argtypes = _capi.SIGNATURES[name]
        table = {**_capi.SIGNATURES, name: (restype, argtypes[:k] + (wrong,) + argtypes[k + 1:])}
        assert differences(HEADER, table) == [(name, words)]
    table = {**_capi.SIGNATURES, "ffl_destroy": (C.c_int, _capi.SIGNATURES["ffl_destroy"][1])}
    assert differences(HEADER, table) == [("ffl_destroy", "returns void, the table says i32")]
    gone = re.sub(r"int ffl_sync\s*\([^()]*\)\s*;", " ", HEADER)
    assert differences(gone, _capi.SIGNATURES) == [("ffl_sync", "in the table, not declared in the header")]
    with pytest.raises(AssertionError, match="not read as a prototype"):   # a form the pattern cannot read is not skipped
        prototypes(HEADER.replace("int ffl_sync(ffl_ctx *ctx);", "int ffl_sync(ffl_ctx *ctx, void (*done)(int));"))


# ---- (c) records --------------------------------------------------------------------------------------------------------------
UNMIRRORED_RECORDS = {}   # {struct name: why Python has no statement for it}
STRUCT = re.compile(r"typedef\s+struct\s+(ffl_\w+)\s*\{([^{}]*)\}\s*\1\s*;")


def header_records(text):
    """{struct name: [member designator]} of every `typedef struct ffl_x { ... } ffl_x;`, in order; a member that is itself
    such a record is given by its leaves ("base.dot")"""
    out = {}
    for name, body in STRUCT.findall(text):
        members = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            first, *rest = [d.strip() for d in decl.split(",")]
            m = re.fullmatch(r"(.*?)(\w+)\s*(?:\[\d+\])?", first)
            ctype = m.group(1).strip()
            for field in [m.group(2)] + [re.fullmatch(r"\*?\s*(\w+)\s*(?:\[\d+\])?", d).group(1) for d in rest]:
                members += [f"{field}.{leaf}" for leaf in out[ctype]] if ctype in out else [field]
        out[name] = members
    assert len(out) == len(re.findall(r"\btypedef\s+struct\s+ffl_\w+\s*\{", text)), "a record of ffl.h was not read"
    return out


def python_layout(mirror):
    """(size, [(field, offset, size)]) of a ctypes.Structure or a numpy record dtype"""
    if isinstance(mirror, np.dtype):
        return mirror.itemsize, [(k, mirror.fields[k][1], mirror.fields[k][0].itemsize) for k in mirror.names]
    return C.sizeof(mirror), [(k, getattr(mirror, k).offset, getattr(mirror, k).size) for k, _ in mirror._fields_]


def compiled_layouts(tmp_path, records):
    """{struct name: (size, [(leaf field, offset, size)])} as the host C compiler lays the header's records out"""
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "ffl.h"', "int main(void) {"]
    for name, members in records.items():
        lines.append(f'    printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'    printf("{name}.{m.split(".")[-1]} %zu %zu\\n", offsetof({name}, {m}), sizeof((({name} *)0)->{m}));'
                  for m in members]
    (tmp_path / "probe.c").write_text("\n".join(lines + ["    return 0;", "}", ""]))
    subprocess.run(["cc", "-std=c99", "-Wall", "-I", INCLUDE, "-o", str(tmp_path / "probe"), str(tmp_path / "probe.c")],
                   check=True, capture_output=True, text=True)
    out = {}
    for line in subprocess.run([str(tmp_path / "probe")], check=True, capture_output=True, text=True).stdout.splitlines():
        key, *nums = line.split()
        name, _, field = key.partition(".")
        if not field:
            out[name] = (int(nums[0]), [])
        else:
            out[name][1].append((field, int(nums[0]), int(nums[1])))
    return out


@pytest.fixture(scope="module")
def c_layouts(tmp_path_factory):
    if shutil.which("cc") is None:
        pytest.skip("no C compiler (cc) on PATH")
    return compiled_layouts(tmp_path_factory.mktemp("abi"), header_records(HEADER))


def test_every_record_has_the_layout_of_the_compiled_header(c_layouts):
    """also the only place the header is compiled as plain C"""
    assert len(c_layouts) >= 11
    assert not set(_capi.RECORDS) & set(UNMIRRORED_RECORDS)
    assert set(c_layouts) == set(_capi.RECORDS) | set(UNMIRRORED_RECORDS), set(c_layouts) ^ set(_capi.RECORDS)
    for name, mirror in _capi.RECORDS.items():
        assert python_layout(mirror) == c_layouts[name], name


def test_a_changed_record_is_noticed(c_layouts):
    p2 = _capi.PASS2_DTYPE
    offsets = [p2.fields[k][1] for k in p2.names]
    offsets[5] += 4
    moved = np.dtype({"names": list(p2.names), "formats": [p2.fields[k][0] for k in p2.names], "offsets": offsets, "itemsize": 52})
    assert python_layout(moved) != c_layouts["ffl_pass2_record"]

    class Narrow(C.Structure):   # a ptrdiff_t taken for an int
        _fields_ = [("base", C.c_void_p), ("item_stride", C.c_int), ("row_pitch", C.c_ssize_t)]
    assert python_layout(Narrow)[1] != c_layouts["ffl_dev_weights"][1]
    assert python_layout(_capi.DevWeights) == c_layouts["ffl_dev_weights"]


def test_the_record_dtypes_keep_their_statement():
    """what pipeline.py and the GPU tests index by name: names, formats, offsets and itemsize of the four dtypes"""
    want = {"PASS2_DTYPE": ("dot:<f8:0 cx:<f8:8 cy:<f8:16 mean_mag:<f4:24 div_val:<f4:28 x:<i4:32 y:<i4:36 cut:<i4:40 pad:<i4:44", 48),
            "PASS2_AXES_DTYPE": ("dot:<f8:0 cx:<f8:8 cy:<f8:16 mean_mag:<f4:24 div_val:<f4:28 x:<i4:32 y:<i4:36 cut:<i4:40 pad:<i4:44 "
                                 "tangential:<f8:48 shift_x:<f8:56 shift_y:<f8:64 reserved:<f8:72", 80),
            "CELL_DTYPE": ("mean_u:<f8:0 mean_v:<f8:8 mean_mag:<f8:16 var_mag:<f8:24", 32),
            "GRID_CENTRE_DTYPE": ("cx:<f8:0 cy:<f8:8 total_var:<f8:16 cells:<i4:24 empty:<i4:28", 32)}
    for name, (fields, size) in want.items():
        dt = getattr(_capi, name)
        assert " ".join(f"{k}:{dt.fields[k][0].str}:{dt.fields[k][1]}" for k in dt.names) == fields and dt.itemsize == size, name


# ---- (d) constants ------------------------------------------------------------------------------------------------------------
def _k(name):
    return _capi.KERNEL_CLASSES.index(name)


# every integer macro of the header Python mirrors, and where
MACROS = {
    "FFL_OK": _capi.FFL_OK, "FFL_ERR_INVALID": _capi.FFL_ERR_INVALID, "FFL_ERR_STATE": _capi.FFL_ERR_STATE,
    "FFL_MAX_BATCH": _capi.FFL_MAX_BATCH, "FFL_MAX_RADIUS": _capi.FFL_MAX_RADIUS, "FFL_MAX_CELLS": _capi.FFL_MAX_CELLS,
    "FFL_YUV_I420": _capi.YUV_LAYOUTS["i420"], "FFL_YUV_NV12": _capi.YUV_LAYOUTS["nv12"],
    "FFL_DEV_GRAY": _capi.DEV_FORMATS["gray"], "FFL_DEV_BGR": _capi.DEV_FORMATS["bgr"], "FFL_DEV_RGB": _capi.DEV_FORMATS["rgb"],
    "FFL_DEV_I420": _capi.DEV_FORMATS["i420"], "FFL_DEV_NV12": _capi.DEV_FORMATS["nv12"],
    "FFL_FLOW_NHWC": _capi.FLOW_LAYOUTS["nhwc"], "FFL_FLOW_NCHW": _capi.FLOW_LAYOUTS["nchw"],
    "FFL_F32": _capi.FLOW_DTYPES["<f4"], "FFL_F16": _capi.FLOW_DTYPES["<f2"], "FFL_BF16": _capi.FLOW_DTYPES["bfloat16"],
    "FFL_AXIS_RADIAL": _capi.AXES.index("radial"), "FFL_AXIS_TANGENTIAL": _capi.AXES.index("tangential"),
    "FFL_AXIS_SHIFT_X": _capi.AXES.index("shift_x"), "FFL_AXIS_SHIFT_Y": _capi.AXES.index("shift_y"), "FFL_N_AXES": len(_capi.AXES),
    "FFL_FB_USE_INITIAL_FLOW": _capi.FFL_FB_USE_INITIAL_FLOW, "FFL_FB_GAUSSIAN_WINDOW": _capi.FFL_FB_GAUSSIAN_WINDOW,
    "FFL_PROFILE_ALL": _capi.FFL_PROFILE_ALL,
    "FFL_K_GRAY": _k("k_gray"), "FFL_K_PYRAMID": _k("k_pyr_level"), "FFL_K_POLYEXP": _k("k_polyexp"),
    "FFL_K_FRONTEND": _k("k_frontend"), "FFL_K_UPDATE_MATRICES": _k("k_update_matrices"), "FFL_K_BLUR_SOLVE": _k("k_blur_solve"),
    "FFL_K_PASS1": _k("k_pass1"), "FFL_K_RADIAL": _k("k_radial"), "FFL_K_COUNT": len(_capi.KERNEL_CLASSES),
}
UNMIRRORED_MACROS = {"FFL_ERR_HIP": "Python reads a status through FFLError.code and names only the two it branches on",
                     "FFL_ERR_NO_DEVICE": "as FFL_ERR_HIP"}


def header_macros(text):
    """{name: value} of every `#define FFL_X <integer literal>`"""
    found = re.findall(r"^[ \t]*#[ \t]*define[ \t]+(FFL_\w+)[ \t]+(\S.*?)[ \t]*$", text, flags=re.M)
    return {k: int(v.rstrip("uU"), 0) for k, v in found if re.fullmatch(r"(0[xX][0-9a-fA-F]+|\d+)[uU]?", v)}


def test_every_integer_macro_is_mirrored_by_value_or_listed():
    macros = header_macros(HEADER)
    assert len(macros) >= 37 and macros["FFL_PROFILE_ALL"] == 255 and macros["FFL_FB_GAUSSIAN_WINDOW"] == 256
    assert not set(MACROS) & set(UNMIRRORED_MACROS)
    assert set(macros) == set(MACROS) | set(UNMIRRORED_MACROS), set(macros) ^ (set(MACROS) | set(UNMIRRORED_MACROS))
    assert {k: macros[k] for k in MACROS} == MACROS
    assert len(_capi.KERNEL_CLASSES) == macros["FFL_K_COUNT"] and _capi.FFL_PROFILE_ALL == (1 << macros["FFL_K_COUNT"]) - 1
    assert header_macros(HEADER.replace("#define FFL_MAX_CELLS 64", "#define FFL_MAX_CELLS 65"))["FFL_MAX_CELLS"] != MACROS["FFL_MAX_CELLS"]

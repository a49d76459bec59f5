"""What the host tests share about the C boundary (no test lives here): reading a header of ``include/`` and comparing it
with a ctypes table of ``_lib.HEADERS``, the plain-C check of a header, and the fake device addresses the alignment
refusals are provoked with.

An argument set describes one call, parameter by parameter: ``Dev(align)`` a DEVICE pointer and the alignment the entry
point requires of it, ``DevArray`` a HOST array of such, ``Job()`` a HOST ``rgcn_slab_job``, ``Host(make)`` any other
HOST pointer, ``HANDLE`` the fake graph handle, ``STREAM`` / ``None`` NULL, a callable a value made when the set is
built (a ``*_workspace_bytes`` query), anything else the value itself.  The addresses are never dereferenced: every set
is only ever called with ONE pointer moved below its alignment, which the entry point refuses after every other argument
check and before its first HIP runtime call.
"""
import ctypes
import importlib
import os
import re
import shutil
import subprocess

import pytest

from primekg_rgcn_linkprediction_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RGCN_MAX_LEVELS = 8                    # csrc/rgcn_plan.h
FAKE_BASE, FAKE_STEP = 0x7F0000000000, 0x100000        # fake device addresses: multiples of 1 MiB, never dereferenced


# ------------------------------------------------------------------------------------------------ headers
def header_text(header):
    with open(os.path.join(ROOT, "include", header)) as f:
        return f.read()


def header_code(header):
    """the header without its comments"""
    return re.sub(r"/\*.*?\*/", "", header_text(header), flags=re.S)


def declared(header):
    """name -> (return type text, [parameter declarations]) of every function the header declares"""
    found = re.findall(r"^((?:const\s+)?\w+\s*\**)\s*\b([a-z_0-9]+)\s*\(([^;{()]*)\)\s*;", header_code(header), flags=re.M)
    return {name: (" ".join(ret.split()), [] if params.strip() == "void" else [" ".join(p.split()) for p in params.split(",")])
            for ret, name, params in found}


def kind_in_header(param):
    if "*" in param:
        return "pointer"
    return next(k for k in ("float", "double", "size_t", "int64_t", "int") if re.search(rf"\b{k}\b", param))


def is_pointer(ty):
    return ty in (ctypes.c_void_p, ctypes.c_char_p) or (isinstance(ty, type) and issubclass(ty, ctypes._Pointer))


def kind_in_ctypes(ty):
    kinds = {ctypes.c_float: "float", ctypes.c_double: "double", ctypes.c_size_t: "size_t", ctypes.c_int64: "int64_t",
             ctypes.c_int: "int"}
    return "pointer" if is_pointer(ty) else kinds[ty]


def restype_in_header(text):
    """the ctypes restype of a declared return type: ``const char*`` is a string, any other pointer an address"""
    text = text.replace("const", "").replace(" ", "")
    if text.endswith("*"):
        return ctypes.c_char_p if text == "char*" else ctypes.c_void_p
    return {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "void": None}[text]


def plain_c(header, tmp_path, main_body="return RGCN_OK;", before_main=""):
    """the header compiles as C99 and as C++17 under -Wall -Wextra -pedantic; -> the source, for a test that goes on to link"""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / (header[:-2] + ".c")
    src.write_text(f'#include "include/{header}"\n{before_main}int main(void) {{ {main_body} }}\n')
    for cc, std, lang in (("gcc", "-std=c99", "c"), ("g++", "-std=c++17", "c++")):
        subprocess.run([cc, std, "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", "-x", lang, "-I", ROOT, str(src)], check=True)
    return src


# ------------------------------------------------------------------------------------------------ argument sets
class Dev:
    """a DEVICE pointer parameter: ``align`` is what the entry point requires of it; ``half``: an fp16 table"""

    def __init__(self, align, half=False):
        assert align in (4, 8, 16)
        self.align, self.half = align, half

    def shifts(self):
        by = {16: (4, 8, 12), 8: (4,), 4: (2,)}[self.align]
        return by + ((2,) if self.half else ())


class DevArray:
    """a HOST array of DEVICE pointers (``count`` entries, each with the alignment of ``dev``)"""

    def __init__(self, dev, count=1):
        self.dev, self.count = dev, count


class Job:
    """a HOST ``rgcn_slab_job`` whose pointer fields are DEVICE pointers read in 16-byte pieces by the reduction"""
    FIELDS = ("slab", "bias_part", "grad_weight", "grad_root", "grad_bias")


class Host:
    """a HOST pointer (an array of sizes, a struct, an out-parameter): ``make()`` builds the object that is passed"""

    def __init__(self, make=None):
        self.make = make or (lambda: None)


HANDLE, STREAM = "handle", "stream"    # an rgcn_graph handle (owns its device arrays); a hipStream_t: NULL here
T16, T8, T4 = Dev(16), Dev(8), Dev(4)         # tables / index vectors and doubles / words, counters and amax heads


def i64s(*values):
    return Host(lambda: (ctypes.c_int64 * len(values))(*values))


def _q(name, *args):
    """a ``*_workspace_bytes`` query, made when the set is built"""
    return lambda: getattr(_lib.load(), name)(*args)


class _Csr(ctypes.Structure):
    """``rgcn_csr`` (csrc/rgcn_common.h), field by field: only the host-side fields the argument checks read are set"""
    _fields_ = [("rowptr", ctypes.c_void_p), ("col", ctypes.c_void_p), ("perm", ctypes.c_void_p), ("val", ctypes.c_void_p),
                ("weighted", ctypes.c_bool), ("n_key", ctypes.c_int64), ("n_other", ctypes.c_int64),
                ("num_levels", ctypes.c_int), ("items", ctypes.c_void_p * RGCN_MAX_LEVELS),
                ("num_items", ctypes.c_int64 * RGCN_MAX_LEVELS), ("num_partials", ctypes.c_int64),
                ("head_col", ctypes.c_void_p), ("head_w", ctypes.c_void_p), ("tile_mask", ctypes.c_void_p),
                ("num_row_tiles", ctypes.c_int64), ("fin_ptr", ctypes.c_void_p), ("num_fin_tiles", ctypes.c_int64),
                ("weight_bound", ctypes.c_float)]


class _Graph(ctypes.Structure):
    """``rgcn_graph``"""
    _fields_ = [("E", ctypes.c_int64), ("N", ctypes.c_int64), ("R", ctypes.c_int64), ("dir", _Csr * 2)]


def _fake_graph():
    """one node, one relation, one edge; the forward direction has one partial row, so the gather needs a workspace"""
    g = _Graph(E=1, N=1, R=1)
    c = g.dir[0]
    c.rowptr, c.col, c.perm, c.val = (FAKE_BASE - (i + 1) * FAKE_STEP for i in range(4))
    c.n_key, c.n_other, c.num_levels, c.num_partials, c.weight_bound = 1, 1, 2, 1, 1.0
    return g


_GRAPH = _fake_graph()
GRAPH = ctypes.addressof(_GRAPH)


def build(args, shift_at=None, shift=0):
    """-> (ctypes values of an argument set, the host objects they point to); ``shift_at`` = (position, entry or field
    or None) moves ONE pointer by ``shift``"""
    values, keep, fake = [], [], [FAKE_BASE]

    def address(where):
        fake[0] += FAKE_STEP
        return fake[0] + (shift if where == shift_at else 0)

    for pos, a in enumerate(args):
        if isinstance(a, Dev):
            values.append(address((pos, None)))
        elif isinstance(a, DevArray):
            arr = (ctypes.c_void_p * a.count)(*[address((pos, j)) for j in range(a.count)])
            keep.append(arr)
            values.append(ctypes.cast(arr, ctypes.c_void_p))
        elif isinstance(a, Job):
            job = _lib.SlabJob(splits=1, K1=4, Kc=8, N=4, **{f: address((pos, f)) for f in Job.FIELDS})
            keep.append(job)
            values.append(ctypes.pointer(job))
        elif isinstance(a, Host):
            obj = a.make()
            keep.append(obj)
            values.append(obj if obj is None or isinstance(obj, ctypes._Pointer) else ctypes.cast(obj, ctypes.c_void_p))
        elif a == HANDLE:
            values.append(GRAPH)
        elif a == STREAM or a is None:
            values.append(None)
        else:
            values.append(a() if callable(a) else a)
    return values, keep


def targets(name, args):
    """[(position, entry / field / None, Dev)] - every device pointer of the set"""
    out = []
    for pos, a in enumerate(args):
        if isinstance(a, Dev):
            out.append((pos, None, a))
        elif isinstance(a, DevArray):
            out.extend((pos, j, a.dev) for j in range(a.count))
        elif isinstance(a, Job):
            out.extend((pos, f, T16) for f in Job.FIELDS)
    return out


def misaligned_refusals(fn, name, args):
    """every device pointer of the set moved below its alignment, one at a time: -> what did NOT come back as
    RGCN_ERR_ALIGN.  The fully aligned set is never called - that would be a launch."""
    failed = []
    for pos, sub, dev in targets(name, args):
        for shift in dev.shifts():
            values, keep = build(args, (pos, sub), shift)
            code = fn(*values)
            if code != _lib.RGCN_ERR_ALIGN:
                failed.append(f"{name}: parameter {pos}{'' if sub is None else f'[{sub}]'} (alignment {dev.align}) moved by "
                              f"{shift}: code {code} ({_lib.strerror(code)})")
            del keep
    return failed


ALIGNMENT_OWNERS = ("test_alignment_host", "test_resample_host", "test_complex_host", "test_softmax_host")


def alignment_rows():
    """name -> argument sets, from every host test module that keeps some (its ``ALIGNMENT_CASES``)"""
    rows = {}
    for module in ALIGNMENT_OWNERS:
        for name, sets in importlib.import_module(module).ALIGNMENT_CASES.items():
            assert name not in rows, f"{name} has alignment rows in two modules ({module})"
            rows[name] = sets
    return rows

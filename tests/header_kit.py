"""What every extension header's tests repeat, once: the C-prototype and Rust `extern "C"` parsers, the checks that a header's entries are
exported by the built libraries and typed the same in the package's table, the build-and-run of a tests/cpp/*_facade_tests.cpp program,
and the built product library with its kernel resources.  A plain module: what is specific to a header stays in that header's test file."""
import ctypes as C
import functools
import importlib.util
import os
import re
import subprocess

import pytest

import hostsim
from kernel_resources import kernel_resources
import petal_decomposition_amd as petal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_LIBRARY = os.path.join(ROOT, "petal-decomposition_amd", "libpetal_hip.so")


def _strip_c_comments(text):
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def _c_class(t):
    """machine class of a C parameter type"""
    t = t.strip()
    if "*" in t or re.search(r"\bpetal_allreduce_fn\b", t):
        return "ptr"
    t = re.sub(r"\bconst\b", "", t).strip()
    return {"int": "i32", "int32_t": "i32", "int64_t": "i64", "double": "f64", "void": "void", "size_t": "u64"}[t]


def _rust_class(t):
    t = t.strip()
    if t.startswith("*"):
        return "ptr"
    return {"c_int": "i32", "i32": "i32", "i64": "i64", "f64": "f64", "c_double": "f64", "usize": "u64"}[t]


def header_functions(path, prefix="petal_", drop=()):
    """{name: (class of the result, [class of each parameter])} of every prototype in the C header at `path` whose name starts with
    `prefix`.  `drop`: regular expressions of what else the header declares (typedefs), taken out of the text first."""
    text = re.sub(r"^\s*#.*$", "", _strip_c_comments(open(path).read()), flags=re.M).replace('extern "C" {', "")
    for pattern in drop:
        text = re.sub(pattern, "", text, flags=re.S)
    fns = {}
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(%s\w+)\s*\(([^;{}]*?)\)\s*;" % re.escape(prefix), text, flags=re.S):
        args = m.group(3).strip()
        params = [] if args in ("", "void") else [_c_class(re.match(r"(.*?)(\w+)$", a.strip(), flags=re.S).group(1)) for a in args.split(",")]
        fns[m.group(2)] = (_c_class(m.group(1).strip()), params)
    return fns


def rust_functions(path):
    """the same mapping for the `extern "C"` block of the Rust source at `path`"""
    text = re.sub(r"//.*$", "", open(path).read(), flags=re.M)
    block = re.search(r'extern\s+"C"\s*\{(.*)\}', text, flags=re.S).group(1)
    fns = {}
    for m in re.finditer(r"pub\s+fn\s+(\w+)\s*\((.*?)\)\s*(->\s*([^;]+))?;", block, flags=re.S):
        fns[m.group(1)] = ("void" if m.group(4) is None else _rust_class(m.group(4)),
                           [_rust_class(a.split(":", 1)[1]) for a in m.group(2).split(",") if a.strip()])
    return fns


def check_exported(fns, want_hip=False):
    """every name is a symbol of the host-simulation library, and of libpetal_hip.so where that exists (`want_hip`: it has to)"""
    libs = [hostsim.build()]
    if want_hip or os.path.exists(HIP_LIBRARY):
        libs.append(HIP_LIBRARY)
    for path in libs:
        lib = C.CDLL(path)
        for name in fns:
            assert hasattr(lib, name), (path, name)


_CLASS = {C.c_void_p: "ptr", petal._M: "ptr", petal._L: "ptr", petal._D: "ptr", petal._I: "ptr", petal._I32: "ptr", petal._NS: "ptr",
          petal._KS: "ptr", C.POINTER(C.c_void_p): "ptr", C.POINTER(C.c_int32): "ptr", C.c_int: "i32", C.c_int32: "i32", C.c_int64: "i64",
          C.c_double: "f64", None: "void"}


def check_python_table(header_file_name, fns, entries):
    """the header's functions are `entries` and the names of its table in petal.ABI_TABLES, typed the same there; no other table has one"""
    table = petal.ABI_TABLES[header_file_name]
    assert sorted(fns) == entries == sorted(n for n, _, _ in table)
    for name, res, args in table:
        assert (_CLASS[res], [_CLASS[a] for a in args]) == fns[name], name
    for other, rows in petal.ABI_TABLES.items():
        if other != header_file_name:
            assert not {n for n, _, _ in rows} & set(fns), other


def run_cpp_facade(stem, mode, lib_path, tag):
    """build tests/cpp/<stem>_facade_tests.cpp against the library at `lib_path` as tests/_build/<stem>_facade_tests_<tag>, run it with
    `mode` as a fresh child process and expect its closing line"""
    assert os.path.exists(lib_path), f"{os.path.basename(lib_path)} missing: run python __graft_entry__.py build"
    out = os.path.join(ROOT, "tests", "_build", f"{stem}_facade_tests_{tag}")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    libdir, libname = os.path.split(lib_path)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", f"{stem}_facade_tests.cpp"), "-o", out,
                           "-L", libdir, f"-l:{libname}", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"])
    res = subprocess.run([out, mode], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    assert f"{stem.replace('_', ' ')} facade tests passed ({mode})" in res.stdout


@functools.lru_cache(maxsize=None)
def built_library():
    """the product library's path, built if it has to be (petal-decomposition_amd/build.py)"""
    spec = importlib.util.spec_from_file_location("petal_build", os.path.join(ROOT, "petal-decomposition_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.build()


@functools.lru_cache(maxsize=None)
def built_kernel_resources():
    """kernel_resources() of the built product library: one dictionary per process, read and never written"""
    return kernel_resources(built_library())


@pytest.fixture(scope="module")
def resources():
    return built_kernel_resources()

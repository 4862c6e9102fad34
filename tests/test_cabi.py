"""CPU: libclapgpu.so loads and exports exactly what include/clapgpu.h declares, and clap_amd/_lib.py mirrors that header
whole: every struct's layout as gcc makes it, every prototype's argument classes, every constant.
No compute call is made (there is no GPU here)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from clap_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "clapgpu.h")


def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(clapgpu_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def built_lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_header_functions_all_bound_and_exported(built_lib):
    declared = declared_functions()
    assert len(declared) >= 15
    assert sorted(_lib.SYMBOLS) == declared, "clap_amd/_lib.py SYMBOLS must mirror include/clapgpu.h"
    for name in declared:
        assert hasattr(built_lib, name), f"libclapgpu.so does not export {name}"


def test_exports_are_c_abi(built_lib):
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
    exported = {l.split()[-1] for l in out.stdout.splitlines() if " T " in l}
    for name in declared_functions():
        assert name in exported, f"{name} is not an unmangled exported symbol"


def test_abi_version(built_lib):
    assert built_lib.clapgpu_abi_version() == _lib.ABI_VERSION


def constants():
    return {k: v for k, v in vars(_lib).items() if k.isupper() and type(v) is int}


@pytest.fixture(scope="module")
def gcc_says(tmp_path_factory):
    """What gcc makes of the header: sizeof of every struct of _lib.STRUCTS, offsetof and sizeof of every field the binding
    names (a field the header lacks does not compile), the value of CLAPGPU_<NAME> for every constant NAME of the binding."""
    out = []
    for cname, cls in _lib.STRUCTS.items():
        out.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        out += [f'printf("{cname}.{f} %zu %zu\\n", offsetof({cname}, {f}), sizeof((({cname} *)0)->{f}));' for f, _t in cls._fields_]
    out += [f'printf("{k} %lld\\n", (long long)(CLAPGPU_{k}));' for k in constants()]
    d = tmp_path_factory.mktemp("cabi")
    src, exe = d / "abi.c", d / "abi"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "clapgpu.h"\nint main(void)\n{\n    ' + "\n    ".join(out) +
                   "\n    return 0;\n}\n")
    p = subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    return {l.split()[0]: [int(x) for x in l.split()[1:]] for l in lines}


def test_every_struct_of_the_binding_is_laid_out_as_the_header(gcc_says):
    own = [v for v in vars(_lib).values() if isinstance(v, type) and issubclass(v, C.Structure) and v.__module__ == _lib.__name__]
    assert sorted(own, key=id) == sorted(_lib.STRUCTS.values(), key=id), "every Structure of _lib stands in STRUCTS, once"
    for cname, cls in _lib.STRUCTS.items():
        end = 0
        for f, t in cls._fields_:
            d = getattr(cls, f)
            assert gcc_says[f"{cname}.{f}"] == [d.offset, d.size], f"{cname}.{f}"
            # the fields cover the struct: between two of them only what the next one's alignment asks for
            assert d.offset - end == -end % C.alignment(t), f"{cname}: the header has a field in front of {f}"
            end = d.offset + d.size
        assert gcc_says[cname][0] - end == -end % C.alignment(cls), f"{cname}: the header has a field behind {f}"
        assert gcc_says[cname] == [C.sizeof(cls)], cname


def test_constants_and_version_match_the_header(gcc_says):
    assert len(constants()) >= 45 and "ABI_VERSION" in constants()
    for k, v in constants().items():
        assert gcc_says[k] == [v], k


SCALARS = {"int": "int", "int32_t": "int", "uint32_t": "uint32_t", "size_t": "size_t", "double": "double", "float": "float",
           "void": "void"}
CTYPES = {C.c_int32: "int", C.c_uint32: "uint32_t", C.c_size_t: "size_t", C.c_double: "double", C.c_float: "float", None: "void"}


def c_class(decl, named):
    """(class, struct pointed at) of a C parameter (named) or return type: "pointer" (arrays too) or the scalar's class"""
    if "*" in decl or "[" in decl:
        s = re.search(r"\bclapgpu_\w+", decl.split("[")[0].rsplit("*", 1)[0])
        return "pointer", s.group(0) if s else None
    words = [w for w in decl.split() if w != "const"]
    return SCALARS[" ".join(words[:-1] if named else words)], None


def ctypes_class(t):
    if isinstance(t, type) and issubclass(t, C._Pointer):
        return "pointer", t._type_ if issubclass(t._type_, C.Structure) else None
    return ("pointer" if t in (C.c_void_p, C.c_char_p) else CTYPES[t]), None


def prototypes():
    """name -> (return type, [parameter declarations]) of every function the comment-stripped header declares"""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    src = re.sub(r"^\s*#.*$", "", src, flags=re.M)
    src = re.sub(r"\{[^{}]*\}", "", src)                                    # struct bodies
    found = {}
    for stmt in src.split(";"):
        m = re.search(r"([^{}]*?)\b(clapgpu_[a-z0-9_]+)\s*\((.*)\)\s*$", " ".join(stmt.split()))
        if m:
            args = [a.strip() for a in m.group(3).split(",")]
            found[m.group(2)] = (m.group(1).strip(), [] if args == ["void"] else args)
    return found


def test_every_prototype_of_the_header_is_bound_with_its_argument_classes():
    protos = prototypes()
    assert sorted(protos) == declared_functions()
    name_of = {cls: cname for cname, cls in _lib.STRUCTS.items()}
    for name, (ret, args) in protos.items():
        res, argtypes = _lib.SYMBOLS[name]
        assert c_class(ret, False)[0] == ctypes_class(res)[0], f"{name}: the return type"
        assert len(args) == len(argtypes), f"{name}: {len(args)} arguments in the header, {len(argtypes)} in SYMBOLS"
        for i, (a, t) in enumerate(zip(args, argtypes)):
            (want, struct), (got, cls) = c_class(a, True), ctypes_class(t)
            assert want == got, f"{name}: argument {i} ({a}) is bound as {got}"
            assert cls is None or name_of[cls] == struct, f"{name}: argument {i} ({a}) is bound as a {name_of[cls]}"


def test_code_object_is_gfx950_only():
    """The fat binary's bundle ids name the ISAs it carries: gfx950 and nothing else."""
    blob = open(_lib.LIB_PATH, "rb").read()
    targets = set(re.findall(rb"amdgcn-amd-amdhsa--(gfx[0-9a-z]+)", blob))
    assert targets == {b"gfx950"}, targets


def test_error_codes_match_reference_cerr_enum():
    # core/error.h:12-49 of the reference
    assert (_lib.ERR_NOMEM, _lib.ERR_INVALID_ARGUMENTS, _lib.ERR_NOT_SUPPORTED) == (-1, -2, -3)
    assert (_lib.ERR_TOO_LARGE, _lib.ERR_INIT_FAILED, _lib.ERR_OUT_OF_BOUNDS, _lib.ERR_UNKNOWN) == (-11, -14, -26, -32)


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(_lib.ClapGpuError):
        _lib.lib()


def test_experiment_switches_cannot_reach_a_release_build():
    """The A/B and sensitivity macros of the kernels (some compile arithmetic out: wrong results on purpose) need
    -DCLAPGPU_EXPERIMENT, and an experiment build reports an ABI version with the top bit set, which _lib refuses."""
    import subprocess
    src = os.path.join(ROOT, "clap_amd", "csrc", "runtime.hip")
    base = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-E", src,
            "--cuda-host-only", "-o", "-"]
    for macro in ("CLAPGPU_EXP_NO_INVERT", "CLAPGPU_EXP_NO_AABB", "CLAPGPU_PLAIN_STORES", "BP_SEARCH_IN_FLIGHT=2"):
        p = subprocess.run(base + ["-D" + macro], capture_output=True, text=True)
        assert p.returncode != 0 and "experiment switches" in p.stderr, macro
    p = subprocess.run(base + ["-DCLAPGPU_EXPERIMENT", "-DCLAPGPU_EXP_NO_AABB"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-500:]
    line = [l for l in p.stdout.splitlines() if "clapgpu_abi_version(void)" in l and "return" in l][-1]
    assert "0x80000000u" in line
    p = subprocess.run(base, capture_output=True, text=True)
    line = [l for l in p.stdout.splitlines() if "clapgpu_abi_version(void)" in l and "return" in l][-1]
    assert p.returncode == 0 and "0x80000000u" not in line

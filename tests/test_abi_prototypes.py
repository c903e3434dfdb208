"""CPU: the prototype table of mcmc_amd/_abi.py against the two headers, on the loaded function objects, and the struct mirrors against the
compiler's layout; bare addresses and 64-bit results arrive whole; a wrong kind of argument raises in Python (no device)."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import mcmc_amd
from mcmc_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = (os.path.join(ROOT, "include", "mi_mcmc.h"), os.path.join(ROOT, "mcmc_amd", "csrc", "mi_mcmc_probes.h"))
STRUCTS = {c.__name__: c for c in (_abi.mi_target, _abi.mi_settings, _abi.mi_chains, _abi.mi_de_settings, _abi.mi_populations,
                                   _abi.mi_aees_settings, _abi.mi_aees_runs)}
SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "double": C.c_double}
FN_TYPEDEFS = ("mi_log_kernel_cb", "mi_tensor_cb", "mi_small_launch_fn", "mi_tile_launch_fn")
POINTEES = ("void", "double", "uint8_t", "uint32_t", "uint64_t", "mi_collation")       # data pointers: c_void_p, whatever they point to

needs_lib = pytest.mark.skipif(not os.path.exists(mcmc_amd.LIB_PATH), reason="libmi_mcmc.so not built (run __graft_entry__.build())")


def _statements(path):
    """The header without comments, preprocessor lines and the extern "C" braces, cut at the semicolons outside braces."""
    src = open(path).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    src = re.sub(r"^\s*#.*$", " ", src, flags=re.M)
    src = re.sub(r'extern\s+"C"\s*\{', " ", src)
    out, depth, cur = [], 0, ""
    for ch in src:
        if ch == "{":
            depth += 1
        elif ch == "}":
            if depth == 0:                                # the closing brace of extern "C"
                continue
            depth -= 1
        if ch == ";" and depth == 0:
            out.append(" ".join(cur.split()))
            cur = ""
        else:
            cur += ch
    assert not cur.strip(), f"{path}: text after the last statement: {cur.strip()!r}"
    return [s for s in out if s]


def _param_type(text, where):
    toks = re.findall(r"[A-Za-z_][A-Za-z0-9_]*|\*", text)
    toks = [t for t in toks if t != "const"]
    assert "".join(toks) == re.sub(r"\bconst\b|\s", "", text), f"{where}: cannot read {text!r}"
    known = set(SCALARS) | set(STRUCTS) | set(FN_TYPEDEFS) | set(POINTEES)
    if len(toks) > 1 and toks[-1] != "*" and toks[-1] not in known:
        toks = toks[:-1]                                  # the parameter's name
    base, stars = toks[0], toks[1:]
    assert all(t == "*" for t in stars) and len(stars) <= 2, f"{where}: unknown parameter type {text!r}"
    if stars:
        if base in STRUCTS and len(stars) == 1:
            return C.POINTER(STRUCTS[base])
        assert base in POINTEES, f"{where}: unknown pointee in {text!r}"
        return C.c_void_p
    if base in FN_TYPEDEFS:
        return C.c_void_p
    assert base in SCALARS, f"{where}: unknown parameter type {text!r}"
    return SCALARS[base]


def _return_type(text, where):
    text = " ".join(text.split())
    if text == "void":
        return None
    if text == "const char*" or text == "const char *":
        return C.c_char_p
    assert text in SCALARS, f"{where}: unknown return type {text!r}"
    return SCALARS[text]


def header_prototypes():
    """name -> (restype, [argtypes]) of every function the two headers declare, by the fixed mapping; fails on whatever it cannot read."""
    protos = {}
    for path in HEADERS:
        for st in _statements(path):
            if re.match(r"(typedef|enum)\b", st):               # types and constants: no prototype
                continue
            m = re.fullmatch(r"(.*?)\b(mi_[a-z0-9_]+)\s*\((.*)\)", st)
            assert m, f"{path}: not a prototype: {st!r}"
            ret, name, params = m.group(1).strip(), m.group(2), m.group(3).strip()
            assert name not in protos, f"{name} declared twice"
            args = [] if params == "void" else [_param_type(p.strip(), f"{name}, parameter {i}") for i, p in enumerate(params.split(","))]
            protos[name] = (_return_type(ret, name), args)
    return protos


def test_table_matches_the_headers():
    hdr = header_prototypes()
    for name in sorted(set(hdr) | set(_abi.PROTOTYPES)):
        assert name in _abi.PROTOTYPES, f"{name}: declared in a header, missing from the table"
        assert name in hdr, f"{name}: in the table, declared in no header"
        (h_ret, h_args), (t_ret, t_args) = hdr[name], _abi.PROTOTYPES[name]
        assert t_ret is h_ret, f"{name}: restype {t_ret} in the table, {h_ret} by the header"
        assert len(t_args) == len(h_args), f"{name}: {len(t_args)} parameters in the table, {len(h_args)} in the header"
        for i, (t, h) in enumerate(zip(t_args, h_args)):
            assert t is h, f"{name}, parameter {i}: {t} in the table, {h} by the header"
    assert sorted(_abi.EXPORTS + _abi.TEST_HOOKS + _abi.PROBE_EXPORTS) == sorted(hdr)
    assert all(n.startswith("mi_probe_") for n in _abi.PROBE_EXPORTS) and all(n.startswith("mi_mcmc_test_") for n in _abi.TEST_HOOKS)


def test_parser_refuses_what_it_does_not_know():
    for bad in ("float x", "long n", "char* s", "char** p", "double*** p", "struct foo* p"):
        with pytest.raises(AssertionError):
            _param_type(bad, "probe")
    with pytest.raises(AssertionError):
        _return_type("float", "probe")


@needs_lib
def test_table_is_applied_to_the_loaded_libraries():
    for handle, names in ((mcmc_amd.lib(), _abi.EXPORTS + _abi.TEST_HOOKS), (mcmc_amd.probes_lib(), _abi.PROBE_EXPORTS)):
        for name in names:
            fn = getattr(handle, name)
            ret, args = _abi.PROTOTYPES[name]
            assert fn.restype is ret, f"{name}: restype {fn.restype}"
            assert fn.argtypes is not None and len(fn.argtypes) == len(args), f"{name}: argtypes {fn.argtypes}"
            for i, (a, t) in enumerate(zip(fn.argtypes, args)):
                assert a is t, f"{name}, parameter {i}: {a}, table {t}"


def test_struct_layout_matches_the_compiler():
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "mi_mcmc.h"', "int main(void) {"]
    for name, cls in STRUCTS.items():
        lines.append(f'    printf("{name} %zu\\n", sizeof({name}));')
        for field, _ in cls._fields_:
            lines.append(f'    printf("{name}.{field} %zu\\n", offsetof({name}, {field}));')
    lines += ["    return 0;", "}"]
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "layout.cpp"), "w") as f:
            f.write("\n".join(lines) + "\n")
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), "layout.cpp", "-o", "layout"], cwd=tmp)
        got = dict(line.split() for line in subprocess.check_output([os.path.join(tmp, "layout")], text=True).splitlines())
    want = {}
    for name, cls in STRUCTS.items():
        want[name] = str(C.sizeof(cls))
        for field, _ in cls._fields_:
            want[f"{name}.{field}"] = str(getattr(cls, field).offset)
    assert got == want


@needs_lib
def test_bare_addresses_arrive_whole():
    p = np.array([0.5, 0.975, 0.025, 0.8413447460685429])
    z = np.full(p.size, np.nan)
    if min(p.ctypes.data, z.ctypes.data) <= 2 ** 32:
        pytest.skip(f"the allocator returned addresses below 2^32 ({p.ctypes.data:#x}, {z.ctypes.data:#x}): a cut address would go unnoticed")
    assert mcmc_amd.lib().mi_mcmc_norm_ppf(p.ctypes.data, p.size, z.ctypes.data) == mcmc_amd.MI_OK
    # AS 241 PPND16 is good to about 1e-16 relative; the probabilities above are rounded to doubles, which moves z by up to 1e-16 / pdf(z) < 2e-15
    assert z[0] == 0.0
    np.testing.assert_allclose(z[1:], [1.959963984540054, -1.959963984540054, 1.0], rtol=0, atol=1e-14)


@needs_lib
def test_rank_major_index_beyond_32_bits():
    """include/mi_mcmc.h: shard r packed at n_keep * d * chain0(r) with its own row length n_local(r); equal shards: [G][n_keep][d][C / G]."""
    from mcmc_amd.dist import shard_bounds
    for Ct, world in (((1 << 20), 8), ((1 << 20) + 3, 8)):             # equal and ragged shards
        n_keep, d = 64, 128
        i, j, c = n_keep - 1, d - 1, Ct - 1
        c0, nl = shard_bounds(Ct, world, world - 1)
        want = n_keep * d * c0 + (i * d + j) * nl + (c - c0)
        assert want > 2 ** 32
        assert mcmc_amd.lib().mi_mcmc_rank_major_index(Ct, world, n_keep, d, i, j, c) == want
    assert mcmc_amd.lib().mi_mcmc_rank_major_index(16, 4, 2, 2, 0, 0, 16) == 2 ** 64 - 1


@needs_lib
def test_wrong_kinds_raise_in_python():
    lib = mcmc_amd.lib()
    p, z = np.array([0.5]), np.zeros(1)
    with pytest.raises(C.ArgumentError):
        lib.mi_mcmc_norm_ppf(p.ctypes.data, 1.0, z.ctypes.data)          # a float where a uint64_t is declared
    with pytest.raises(C.ArgumentError):
        lib.mi_mcmc_norm_ppf(p, 1, z.ctypes.data)                        # an ndarray where a pointer is declared
    s, c = mcmc_amd.default_settings(), mcmc_amd.make_chains(np.zeros((4, 2)), 2)
    with pytest.raises(C.ArgumentError):
        lib.mi_mcmc_hmc_run(0x1000, C.byref(s), C.byref(c), None)        # an int where a mi_target* is declared
    assert lib.mi_mcmc_norm_ppf(p.ctypes.data, 1, z.ctypes.data) == mcmc_amd.MI_OK and z[0] == 0.0    # ... and the process goes on


@needs_lib
def test_gemm_nuts_last_ticks_returns_three_counts():
    """the one test hook's wrapper that no other test calls: host bookkeeping, no device"""
    got = mcmc_amd.test_gemm_nuts_last_ticks()
    assert len(got) == 3 and all(isinstance(v, int) and v >= 0 for v in got)


def test_ptr_refuses_what_it_cannot_address():
    a = np.zeros(3)

    class Tensor:
        def data_ptr(self):
            return 0x7000_0000_1000

    assert mcmc_amd._ptr(None) is None and mcmc_amd._ptr(5) == 5 and mcmc_amd._ptr(a) == a.ctypes.data
    assert type(mcmc_amd._ptr(np.uint64(2 ** 40))) is int and mcmc_amd._ptr(np.int64(7)) == 7
    assert mcmc_amd._ptr(Tensor()) == 0x7000_0000_1000
    for bad in ([1.0, 2.0], 1.5, "x", (a,)):
        with pytest.raises(TypeError, match=type(bad).__name__):
            mcmc_amd._ptr(bad)

"""CPU: the state of mcmc_amd/csrc/host_linalg.hpp -- what is installed, the staging budget, the counters, the memo -- is ONE per library, not one per
translation unit that includes the header.  Two host units over the header (tests/linalg_state_unit.cpp compiled twice) in one shared library: what
one does, the other sees.  The library's host files (mi_mcmc.hip, mass_adapt.hip) rely on exactly that: the device INV / CHOL_LOWER is installed in
the first and the test hooks live there, the factorisations are asked for in both."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(HERE, "linalg_state_unit.cpp")
_HDR = [os.path.join(HERE, "..", "mcmc_amd", "csrc", f) for f in ("host_linalg.hpp", "linalg_stage.hpp")]
_SO = os.path.join(HERE, "_linalg_state.so")
D = 64                                                     # the smallest d the memo keeps


@pytest.fixture(scope="module")
def units():
    if not os.path.exists(_SO) or any(os.path.getmtime(s) > os.path.getmtime(_SO) for s in [_SRC] + _HDR):
        cxx = os.environ.get("CXX", "g++")
        objs = []
        for u in "ab":
            objs.append(os.path.join(HERE, f"_linalg_state_{u}.o"))
            subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", f"-DUNIT={u}", "-c", "-o", objs[-1], _SRC])
        subprocess.check_call([cxx, "-shared", "-o", _SO] + objs)
    lib = C.CDLL(_SO)
    for u in "ab":
        getattr(lib, f"unit_{u}_accel").restype = C.c_void_p
        getattr(lib, f"unit_{u}_n_computed").restype = C.c_uint64
    return lib


def _chol(lib, unit, A):
    L = np.zeros_like(A)
    dp = C.POINTER(C.c_double)
    assert getattr(lib, f"unit_{unit}_cholesky_lower")(A.ctypes.data_as(dp), C.c_uint32(A.shape[0]), L.ctypes.data_as(dp)) == 0
    return L


def test_both_units_see_one_accel(units):
    assert units.unit_a_accel() == units.unit_b_accel()


def test_a_factorisation_of_one_unit_answers_the_other_from_the_memo(units):
    G = np.random.default_rng(4).standard_normal((D, D))
    A = np.ascontiguousarray(G @ G.T / D + np.eye(D))
    n0 = units.unit_a_n_computed()
    La = _chol(units, "a", A)
    assert units.unit_a_n_computed() - n0 == 1 and units.unit_b_n_computed() - n0 == 1
    Lb = _chol(units, "b", A)                               # the same matrix, the other unit: the memo's copy, nothing computed
    assert units.unit_b_n_computed() - n0 == 1 and units.unit_a_n_computed() - n0 == 1
    assert np.array_equal(La.view(np.uint64), Lb.view(np.uint64))
    assert np.allclose(La @ La.T, A, rtol=1e-12, atol=1e-12)


def test_the_staging_budget_set_in_one_unit_routes_the_other(units):
    units.unit_a_install()                                  # (as mi_mcmc.hip installs the device kernels)
    try:
        assert units.unit_b_on_device(1, D) == 1            # CHOL_LOWER at d = 64 stages 512 bytes
        units.unit_a_set_stage_bytes(256)
        assert units.unit_b_on_device(1, D) == 0 and units.unit_a_on_device(1, D) == 0
        units.unit_b_set_stage_bytes(0)                     # 0: the real budget
        assert units.unit_a_on_device(1, D) == 1 and units.unit_b_on_device(1, D) == 1
    finally:
        units.unit_a_set_stage_bytes(0)
        units.unit_a_uninstall()

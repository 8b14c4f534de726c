"""Partly observed outputs (model.skip_missing) off the device: the new entry points are in the header, the library
and the ctypes table, the step io carries the flag, the attribute is validated, and the skip instantiations of the fused
ELBO kernel that mirror the two headline ones hold the register bars tests/test_cabi.py::test_kernel_resources sets for
those: no scratch, at most 16 VGPR spills, at most 400 SGPR spills (the body differs by one select)."""
import ctypes as C
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["gpsa_count_observed_workspace", "gpsa_count_observed", "gpsa_quadform_elbo_skip_f32",
       "gpsa_quadform_elbo_delta_skip_f32", "gpsa_lmc_loglik_fused_skip_f32", "gpsa_elbo_loss_skip_fwd",
       "gpsa_elbo_loss_skip_bwd"]


def _lib():
    import __graft_entry__ as ge

    ge.build()
    from spatial_alignment_amd import _lib

    return _lib


def test_new_symbols_in_header_table_and_library():
    L = _lib()
    header = open(os.path.join(ROOT, "include", "gpsa_hip.h")).read()
    lib = L.load()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in L.SIGNATURES, name
        assert getattr(lib, name) is not None
        # the table's argument count is the header's
        decl = re.search(r"\b%s\(([^;()]*)\);" % name, header, re.S).group(1)
        n_args = 0 if decl.strip() in ("", "void") else decl.count(",") + 1
        assert len(L.SIGNATURES[name][1]) == n_args, name


def test_step_io_mirror_ends_with_the_flag():
    L = _lib()
    assert L.StepIO._fields_[-1][0] == "skip_missing"
    io = L.StepIO()
    assert io.skip_missing == 0  # a zero-initialised host: today's behaviour
    header = open(os.path.join(ROOT, "include", "gpsa_hip.h")).read()
    body = header[header.index("typedef struct gpsa_step_io {"):header.index("} gpsa_step_io;")]
    assert body.rstrip().endswith("int skip_missing;")


def test_refusals_before_any_launch():
    """argument checks of the new entries run on the host (no device needed)"""
    L = _lib()
    lib = L.load()
    one = (C.c_void_p * 1)(8)
    S, N, P = (C.c_int * 1)(1), (C.c_longlong * 1)(4), (C.c_int * 1)(2)
    out = (C.c_void_p(8), C.c_void_p(8), C.c_void_p(8), 8 * 4100, None)
    head = (1, one, one, one, S, N, P)
    # no counts table
    assert lib.gpsa_elbo_loss_skip_fwd(*head, None, 0, None, None, None, None, None, 0, 1.0, *out) == L.GPSA_EINVAL
    # weights without views
    assert lib.gpsa_elbo_loss_skip_fwd(*head, None, 0, None, None, one, one, None, 0, 1.0, *out) == L.GPSA_EINVAL
    # a workspace below the terms' slots
    small = (C.c_void_p(8), C.c_void_p(8), C.c_void_p(8), 8, None)
    assert lib.gpsa_elbo_loss_skip_fwd(*head, None, 0, None, None, None, one, None, 0, 1.0, *small) == L.GPSA_EWORKSPACE
    assert lib.gpsa_count_observed(1, one, N, P, None, None, one, C.c_void_p(8), 8, None) == L.GPSA_EWORKSPACE
    assert lib.gpsa_count_observed(5, one, N, P, None, None, one, C.c_void_p(8), 1 << 20, None) == L.GPSA_EINVAL
    assert lib.gpsa_lmc_loglik_fused_skip_f32(one, one, one, one, 1, 4, 65, 2, one, 1, one, one, one, 1 << 30,
                                              None) == L.GPSA_EUNSUPPORTED


def test_attribute_is_validated():
    from golden_io import CASES, Golden
    from model_util import build_model

    _lib()
    model, _ = build_model(Golden(CASES[0]))
    assert model.skip_missing is False
    model.skip_missing = True
    assert model.skip_missing is True
    for bad in (1, "yes", None, 0.0):
        with pytest.raises(TypeError):
            model.skip_missing = bad
    assert model.skip_missing is True


def test_skip_kernel_resources():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_meta import demangle, library_kernels

    L = _lib()
    ks = library_kernels(L.LIB_PATH)
    by = dict(zip(demangle([k["name"] for k in ks]), ks))
    heads, fam = 0, 0
    for nm, k in by.items():
        if "panel_elbo_skip_kernel<" in nm:
            fam += 1
            assert k["max_wg"] == 256, (nm, k)  # the launch bounds reached the instantiation
        if "panel_elbo_skip_kernel<13, 2, 2, true, true>" in nm or "panel_elbo_skip_kernel<13, 2, 4, true, true>" in nm:
            heads += 1
            assert k["scratch"] == 0 and k["vgpr_spill"] <= 16 and k["sgpr_spill"] <= 400, (nm, k)
    assert heads == 2 and fam == 12, (heads, fam)
    # the default family is what it was: ten shapes and the two headline instantiations
    assert sum("panel_elbo_kernel<" in nm for nm in by) == 12

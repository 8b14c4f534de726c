"""Count outputs (model.likelihood = "poisson") off the device: the new entry points are in the header, the library and
the ctypes table; the step io still ends with ``skip_missing`` (the likelihood travels through gpsa_step_likelihood); the
attribute and the offsets are validated; every new entry refuses bad arguments on the host, before any launch; and, from
the code object, the Poisson instantiations of the fused ELBO kernel that mirror the two headline ones hold the bars of
the skip kernels (no scratch, at most 16 VGPR spills, at most 400 SGPR spills) while the kernels that share a fragment
or a unit with them keep the figures they had before (tests/golden/poisson_parent_kernel_meta.json)."""
import ctypes as C
import json
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["gpsa_lgamma_sum_workspace", "gpsa_lgamma_sum", "gpsa_elbo_loss_pois_fwd", "gpsa_elbo_loss_pois_bwd",
       "gpsa_quadform_elbo_pois_f32", "gpsa_quadform_elbo_delta_pois_f32", "gpsa_lmc_loglik_fused_pois_f32",
       "gpsa_step_likelihood"]


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
        decl = re.search(r"\b%s\(([^;()]*)\);" % name, header, re.S).group(1)
        n_args = 0 if decl.strip() in ("", "void") else decl.count(",") + 1
        assert len(L.SIGNATURES[name][1]) == n_args, name
    assert "#define GPSA_LIK_GAUSSIAN 0" in header and "#define GPSA_LIK_POISSON 1" in header
    assert L.LIK_KINDS == {"gaussian": 0, "poisson": 1}


def test_step_io_still_ends_with_skip_missing():
    L = _lib()
    assert L.StepIO._fields_[-1][0] == "skip_missing"
    header = open(os.path.join(ROOT, "include", "gpsa_hip.h")).read()
    body = header[header.index("typedef struct gpsa_step_io {"):header.index("} gpsa_step_io;")]
    assert body.rstrip().endswith("int skip_missing;")


def _model():
    from golden_io import Golden
    from model_util import build_model

    g = Golden("c5_two_modalities")
    model, dd = build_model(g)
    return g, model, dd


def test_likelihood_is_validated():
    _lib()
    g, model, _ = _model()
    assert model.likelihood == "gaussian" and model._lik_kinds() is None
    model.likelihood = "poisson"
    assert model._lik_kinds() == [1] * len(g.mods)
    model.likelihood = {g.mods[0]: "poisson"}
    assert model._lik_kinds() == [1] + [0] * (len(g.mods) - 1)
    assert model.likelihood_of(g.mods[0]) == "poisson" and model.likelihood_of(g.mods[1]) == "gaussian"
    for bad in ("negbin", "Poisson", None, 1, ["poisson"], {g.mods[0]: "negbin"}, {g.mods[0]: 1},
                {"no_such_modality": "poisson"}):
        with pytest.raises(ValueError):
            model.likelihood = bad
    assert model.likelihood == {g.mods[0]: "poisson"}  # a refused value leaves the attribute as it was
    model.likelihood = {g.mods[0]: "gaussian"}
    assert model._lik_kinds() is None  # every modality Gaussian: nothing new runs
    model.likelihood = "gaussian"
    assert model._lik_kinds() is None


def test_log_offset_on_a_gaussian_modality_is_refused():
    import torch

    _lib()
    g, model, dd = _model()
    a, b = g.mods[0], g.mods[1]
    model.likelihood = {a: "poisson"}
    dd[a]["log_offset"] = torch.zeros(dd[a]["outputs"].shape[0])
    aux = model._loss_aux(dd)
    assert aux["kinds"] == [1, 0] and aux["log_offset"][0] is dd[a]["log_offset"] and aux["log_offset"][1] is None
    dd[b]["log_offset"] = torch.zeros(dd[b]["outputs"].shape[0])
    with pytest.raises(ValueError, match="Gaussian"):
        model._loss_aux(dd)
    del dd[b]["log_offset"]
    for bad in (torch.zeros(3), torch.zeros(dd[a]["outputs"].shape[0], dtype=torch.float64), [0.0]):
        dd[a]["log_offset"] = bad
        with pytest.raises(ValueError, match="log_offset"):
            model._loss_aux(dd)
    # ... with every modality Gaussian too
    model.likelihood = "gaussian"
    dd[a]["log_offset"] = torch.zeros(dd[a]["outputs"].shape[0])
    with pytest.raises(ValueError, match="Gaussian"):
        model._loss_aux(dd)


def test_predict_refuses_lpd_for_a_poisson_modality():
    _lib()
    g, model, dd = _model()
    model.likelihood = {g.mods[0]: "poisson"}
    X = {m: dd[m]["spatial_coords"] for m in g.mods}
    with pytest.raises(ValueError, match="Poisson"):
        model.predict(X, Y={m: dd[m]["outputs"] for m in g.mods})


def test_refusals_before_any_launch():
    """argument checks of the new entries run on the host (no device needed)"""
    L = _lib()
    lib = L.load()
    one = (C.c_void_p * 1)(8)
    null1 = (C.c_void_p * 1)(None)
    S, N, P = (C.c_int * 1)(1), (C.c_longlong * 1)(4), (C.c_int * 1)(2)
    kind = lambda k: (C.c_int * 1)(k)
    out = (C.c_void_p(8), C.c_void_p(8), C.c_void_p(8), 8 * 4100, None)
    small = (C.c_void_p(8), C.c_void_p(8), C.c_void_p(8), 8, None)
    head = (1, one, one, one, S, N, P)
    fwd = lib.gpsa_elbo_loss_pois_fwd
    tail = (0, None, 0, 1.0)  # skip, kl, n_kl, kl_scale
    # (zpart, nparts, n_views, view_off, w, nobs, kind, lgam, log_offset)
    ok_tabs = (None, 0, None, None, None, None, kind(1), one, None)
    assert fwd(*head, *ok_tabs, *tail, *small) == L.GPSA_EWORKSPACE  # (the tables pass: only the workspace is short)
    assert fwd(*head, None, 0, None, None, None, None, None, one, None, *tail, *out) == L.GPSA_EINVAL  # no kind table
    assert fwd(*head, None, 0, None, None, None, None, kind(1), None, None, *tail, *out) == L.GPSA_EINVAL  # no lgamma table
    assert fwd(*head, None, 0, None, None, None, None, kind(1), null1, None, *tail, *out) == L.GPSA_EINVAL  # ... entry
    for k in (2, -1):  # a kind outside {0, 1}
        assert fwd(*head, None, 0, None, None, None, None, kind(k), one, None, *tail, *out) == L.GPSA_EINVAL
    # weights without views
    assert fwd(*head, None, 0, None, None, one, None, kind(1), one, None, *tail, *out) == L.GPSA_EINVAL
    # a Gaussian term without counts needs views and weights; with counts and draws it needs the skip flag
    assert fwd(*head, None, 0, None, None, None, None, kind(0), one, None, *tail, *out) == L.GPSA_EINVAL
    assert fwd(*head, None, 0, None, None, None, one, kind(0), one, None, *tail, *out) == L.GPSA_EINVAL
    # a fused term without partial sums to read
    assert fwd(*head, one, 0, None, None, None, None, kind(1), one, None, *tail, *out) == L.GPSA_EINVAL
    # no outputs
    assert fwd(*head, *ok_tabs, *tail, None, None, C.c_void_p(8), 8 * 4100, None) == L.GPSA_EINVAL
    bwd = lib.gpsa_elbo_loss_pois_bwd
    btail = (0, C.c_void_p(8), 0, 1.0)  # skip, gloss, n_kl, kl_scale
    grads = (one, one, None, 0, None)  # dF, dnoise, dnoise_all, n_noise, dkl
    assert bwd(*head, *ok_tabs, *btail, *grads, C.c_void_p(8), 8, None) == L.GPSA_EWORKSPACE
    assert bwd(*head, *ok_tabs, 0, None, 0, 1.0, *grads, C.c_void_p(8), 8 * 4100, None) == L.GPSA_EINVAL  # no gloss
    assert bwd(*head, *ok_tabs, *btail, null1, one, None, 0, None, C.c_void_p(8), 8 * 4100, None) == L.GPSA_EINVAL  # no dF
    assert bwd(*head, None, 0, None, None, None, None, kind(3), one, None, *btail, *grads, C.c_void_p(8), 8 * 4100,
               None) == L.GPSA_EINVAL
    # the lgamma table
    lg = lib.gpsa_lgamma_sum
    assert lg(1, one, N, P, None, None, 0, one, C.c_void_p(8), 8, None) == L.GPSA_EWORKSPACE
    assert lg(5, one, N, P, None, None, 0, one, C.c_void_p(8), 1 << 20, None) == L.GPSA_EINVAL
    assert lg(1, null1, N, P, None, None, 0, one, C.c_void_p(8), 1 << 20, None) == L.GPSA_EINVAL
    assert lg(1, one, N, P, (C.c_int * 1)(1), None, 0, one, C.c_void_p(8), 1 << 20, None) == L.GPSA_EINVAL
    # the fused pass: null tables, a workspace below the queried size
    v = C.c_void_p(8)
    M, Cn, Ln = 64, 231, 3
    wsb = lib.gpsa_quadform_elbo_f32_workspace(M, Cn, Ln)
    assert wsb > 0
    qf = lib.gpsa_quadform_elbo_pois_f32
    args = lambda ws, **kw: (1, kw.get("alpha", v), v, M, Cn, Ln, kw.get("mean", v), v, v, v, kw.get("Y", v), 77, 3, None, v,
                             v, v, kw.get("part", v), None, None, 1, v, ws, None)
    assert qf(*args(wsb - 1)) == L.GPSA_EWORKSPACE  # (noise_u and log_offset may be NULL)
    for kw in (dict(alpha=None), dict(mean=None), dict(Y=None), dict(part=None)):
        assert qf(*args(wsb, **kw)) == L.GPSA_EINVAL
    assert lib.gpsa_quadform_elbo_delta_pois_f32(*args(wsb, mean=None)) == L.GPSA_EINVAL
    assert lib.gpsa_quadform_elbo_delta_pois_f32(*args(wsb - 1)) in (L.GPSA_EWORKSPACE, L.GPSA_EUNSUPPORTED)
    # the fused LMC pass
    lm = lib.gpsa_lmc_loglik_fused_pois_f32
    need = lib.gpsa_lmc_loglik_workspace(2 * 77, 3, 5, 512)
    assert lm(v, v, v, None, 0, 2, 77, 3, 5, v, 512, v, v, v, need - 1, None) == L.GPSA_EWORKSPACE
    assert lm(None, v, v, None, 0, 2, 77, 3, 5, v, 512, v, v, v, need, None) == L.GPSA_EINVAL
    assert lm(v, v, v, None, 0, 2, 77, 3, 5, None, 512, v, v, v, need, None) == L.GPSA_EINVAL
    assert lm(v, v, v, None, 0, 2, 77, 65, 5, v, 512, v, v, v, 1 << 30, None) == L.GPSA_EUNSUPPORTED
    # the plan's setter without a plan
    assert lib.gpsa_step_likelihood(None, 0, 1, None) == L.GPSA_EINVAL


def test_poisson_kernel_resources_and_the_default_kernels_figures():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_meta import demangle, library_kernels

    L = _lib()
    ks = library_kernels(L.LIB_PATH)
    by = dict(zip(demangle([k["name"] for k in ks]), ks))
    heads, fam, lmc = 0, 0, 0
    for nm, k in by.items():
        if "panel_elbo_pois_kernel<" in nm:
            fam += 1
            assert k["max_wg"] == 256, (nm, k)  # the launch bounds reached the instantiation
        if "panel_elbo_pois_kernel<13, 2, 2, true, true>" in nm or "panel_elbo_pois_kernel<13, 2, 4, true, true>" in nm:
            heads += 1
            assert k["scratch"] == 0 and k["vgpr_spill"] <= 16 and k["sgpr_spill"] <= 400, (nm, k)
        if "lmc_mfma_pois_kernel<" in nm:
            lmc += 1
            assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["vgpr"] <= 256, (nm, k)  # two workgroups per CU
    assert heads == 2 and fam == 12 and lmc == 3, (heads, fam, lmc)
    # the kernels over the shared fragments, and those of the units the Poisson closing joined, are what they were
    rec = json.load(open(os.path.join(ROOT, "tests", "golden", "poisson_parent_kernel_meta.json")))["kernels"]
    assert len(rec) == 41
    for nm, want in rec.items():
        assert nm in by, nm
        got = {f: by[nm][f] for f in want}
        assert got == want, (nm, got, want)

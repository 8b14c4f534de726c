"""Count outputs (model.likelihood = "negative_binomial") off the device: the new entry points are in the header, the
library and the ctypes table; the attribute is validated and creates / removes model.log_dispersion[m]; every new entry refuses bad arguments on the
host, before any launch; and, from the code object, the new kernels use no scratch and spill no vector register."""
import ctypes as C
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["gpsa_nb_const_workspace", "gpsa_nb_const", "gpsa_elbo_loss_nb_workspace", "gpsa_elbo_loss_nb_fwd",
       "gpsa_elbo_loss_nb_bwd", "gpsa_lmc_loglik_nb_workspace", "gpsa_lmc_loglik_fused_nb_f32",
       "gpsa_quadform_elbo_nb_f32", "gpsa_quadform_elbo_delta_nb_f32", "gpsa_step_dispersion"]


def _lib():
    import __graft_entry__ as ge

    ge.build()
    from spatial_alignment_amd import _lib

    return _lib


def _model():
    from golden_io import Golden
    from model_util import build_model

    g = Golden("c5_two_modalities")
    model, dd = build_model(g)
    return g, model, dd


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
    assert "#define GPSA_LIK_NEGBIN 2" in header
    assert L.LIK_NEGBIN == 2 and L.LIK_KIND_OF == {"gaussian": 0, "poisson": 1, "negative_binomial": 2}


def test_likelihood_accepts_negbin_and_owns_the_dispersion_parameter():
    import torch

    _lib()
    g, model, _ = _model()
    a, b = g.mods
    n0 = len(list(model.parameters()))
    assert not [k for k in model.state_dict() if k.startswith("log_dispersion")]
    model.likelihood = {a: "negative_binomial"}
    assert model._lik_kinds() == [2, 0]
    assert model.likelihood_of(a) == "negative_binomial" and model.likelihood_of(b) == "gaussian"
    rho = model.log_dispersion[a]
    assert isinstance(rho, torch.nn.Parameter) and rho.requires_grad
    assert tuple(rho.shape) == (model.Ps[a],) and rho.dtype == model.noise_variance.dtype and (rho == 0).all()  # r = 1
    assert [k for k in model.state_dict() if k.startswith("log_dispersion")] == [f"log_dispersion.{a}"]
    assert len(list(model.parameters())) == n0 + 1 and any(p is rho for p in model.parameters())
    with torch.no_grad():
        rho.fill_(0.5)
    model.likelihood = "negative_binomial"  # a modality that stays NB keeps its parameter (and its values)
    assert model.log_dispersion[a] is rho and float(rho.detach()[0]) == 0.5
    assert sorted(k for k in model.state_dict() if k.startswith("log_dispersion")) == sorted(
        f"log_dispersion.{m}" for m in g.mods)
    assert model._lik_kinds() == [2, 2]
    for bad in ("nb", "negbin", "NegBin", {a: "nb"}, {"no_such_modality": "negative_binomial"}):
        with pytest.raises(ValueError, match="likelihood"):
            model.likelihood = bad
    assert model.likelihood == "negative_binomial" and len(model.log_dispersion) == 2  # a refused value changes nothing
    model.likelihood = {a: "poisson", b: "negative_binomial"}
    assert a not in model.log_dispersion and b in model.log_dispersion and model._lik_kinds() == [1, 2]
    model.likelihood = "gaussian"
    assert len(model.log_dispersion) == 0 and len(list(model.parameters())) == n0 and model._lik_kinds() is None
    assert not [k for k in model.state_dict() if k.startswith("log_dispersion")]


def test_log_offset_is_accepted_for_a_negbin_modality_only():
    import torch

    _lib()
    g, model, dd = _model()
    a, b = g.mods
    model.likelihood = {a: "negative_binomial"}
    dd[a]["log_offset"] = torch.zeros(dd[a]["outputs"].shape[0])
    aux = model._loss_aux(dd)
    assert aux["kinds"] == [2, 0] and aux["log_offset"][0] is dd[a]["log_offset"] and aux["log_offset"][1] is None
    dd[b]["log_offset"] = torch.zeros(dd[b]["outputs"].shape[0])
    with pytest.raises(ValueError, match="Gaussian"):
        model._loss_aux(dd)


def test_output_sharded_ranks_own_their_columns_dispersion():
    _lib()
    from spatial_alignment_amd import parallel

    g, model, _ = _model()
    model.likelihood = "negative_binomial"
    shared = parallel.shared_parameters(model)
    assert not any(p is model.log_dispersion[m] for p in shared for m in g.mods)
    assert any(p is model.noise_variance for p in shared)


def test_predict_refuses_the_count_scale_for_a_negbin_modality():
    _lib()
    g, model, dd = _model()
    model.likelihood = {g.mods[0]: "negative_binomial"}
    X = {m: dd[m]["spatial_coords"] for m in g.mods}
    with pytest.raises(ValueError, match="negative binomial"):
        model.predict(X, Y={m: dd[m]["outputs"] for m in g.mods})
    with pytest.raises(ValueError, match="negative binomial"):
        model.predict(X, scale="response")


def test_refusals_before_any_launch():
    """argument checks of the new entries run on the host (no device needed)"""
    L = _lib()
    lib = L.load()
    one = (C.c_void_p * 1)(8)
    null1 = (C.c_void_p * 1)(None)
    v = C.c_void_p(8)
    S, N, P = (C.c_int * 1)(2), (C.c_longlong * 1)(50), (C.c_int * 1)(4)
    kind = lambda k: (C.c_int * 1)(k)
    # the constants
    need = lib.gpsa_nb_const_workspace(50, 4, 1)
    assert need > 0 and lib.gpsa_nb_const_workspace(0, 4, 1) == 0 and lib.gpsa_nb_const_workspace(50, 4, 65) == 0
    nc = lib.gpsa_nb_const
    ok = lambda **kw: (kw.get("n", 1), kw.get("Y", one), N, P, kw.get("rho", one), kw.get("nv"), kw.get("vo"), kw.get("w"), 0,
                       kw.get("csum", one), kw.get("dconst", one), kw.get("ws", v), kw.get("bytes", need), None)
    assert nc(*ok(bytes=need - 1)) == L.GPSA_EWORKSPACE
    for kw in (dict(n=0), dict(n=5), dict(Y=None), dict(Y=null1), dict(rho=None), dict(rho=null1), dict(csum=None),
               dict(csum=null1), dict(dconst=null1), dict(ws=None), dict(nv=(C.c_int * 1)(1)), dict(w=one)):
        assert nc(*ok(**kw)) == L.GPSA_EINVAL, kw
    bad_off = (C.c_void_p * 1)(C.addressof((C.c_longlong * 2)(0, 49)))  # the views do not end at N
    assert nc(*ok(nv=(C.c_int * 1)(1), vo=bad_off)) == L.GPSA_EINVAL
    # the closing pair
    wsb = lib.gpsa_elbo_loss_nb_workspace(1, S, N, P, None, kind(2))
    assert wsb > 8 * 4100 and lib.gpsa_elbo_loss_nb_workspace(0, S, N, P, None, None) == 0
    assert lib.gpsa_elbo_loss_nb_workspace(1, S, N, P, None, None) == wsb  # (no kind table: every term counted as NB)
    assert lib.gpsa_elbo_loss_nb_workspace(1, S, N, P, None, kind(1)) == 8 * 4100  # (a Poisson term has no column partials)
    head = (1, one, one, one, S, N, P)
    fwd = lib.gpsa_elbo_loss_nb_fwd
    tail = (0, None, 0, 1.0)  # skip, kl, n_kl, kl_scale
    out = lambda b=wsb: (v, v, v, b, None)
    # (zpart, nparts, n_views, view_off, w, nobs, kind, lgam, log_offset, log_disp, csum)
    tabs = lambda **kw: (kw.get("zpart"), kw.get("nparts", 0), None, None, kw.get("w"), kw.get("nobs"), kw.get("kind", kind(2)),
                         kw.get("lgam", one), None, kw.get("rho", one), kw.get("nbc", one))
    assert fwd(*head, *tabs(), *tail, *out(wsb - 1)) == L.GPSA_EWORKSPACE  # (the tables pass: only the workspace is short)
    assert fwd(*head, *tabs(), *tail, *out(8 * 4100)) == L.GPSA_EWORKSPACE  # (the Poisson closing's size is not enough)
    for kw in (dict(kind=None), dict(lgam=None), dict(lgam=null1), dict(rho=None), dict(rho=null1), dict(nbc=None),
               dict(nbc=null1), dict(kind=kind(3)), dict(kind=kind(-1)), dict(w=one), dict(zpart=one, nparts=0),
               dict(kind=kind(0)), dict(kind=kind(0), nobs=one)):
        assert fwd(*head, *tabs(**kw), *tail, *out()) == L.GPSA_EINVAL, kw
    assert fwd(*head, *tabs(), *tail, None, v, v, wsb, None) == L.GPSA_EINVAL  # no loss
    assert fwd(*head, *tabs(), *tail, v, v, None, wsb, None) == L.GPSA_EINVAL  # no workspace
    assert fwd(1, null1, one, one, S, N, P, *tabs(), *tail, *out()) == L.GPSA_EINVAL  # no draws and no partial sums
    bwd = lib.gpsa_elbo_loss_nb_bwd
    # (..., log_disp, dconst, usum) then skip, gloss, n_kl, kl_scale, dF, dnoise, dnoise_all, n_noise, dkl, ddisp
    btabs = lambda **kw: tabs(**kw) + (kw.get("usum"),)
    grads = lambda **kw: (0, kw.get("gloss", v), 0, 1.0, kw.get("dF", one), one, None, 0, None, kw.get("ddisp", one))
    assert bwd(*head, *btabs(), *grads(), v, wsb - 1, None) == L.GPSA_EWORKSPACE
    for kw in (dict(gloss=None), dict(dF=null1), dict(ddisp=None), dict(ddisp=null1)):
        assert bwd(*head, *btabs(), *grads(**kw), v, wsb, None) == L.GPSA_EINVAL, kw
    assert bwd(*head, *btabs(kind=kind(3)), *grads(), v, wsb, None) == L.GPSA_EINVAL
    # an NB term that arrives as partial sums brings its per-output sums of u
    assert bwd(*head, *btabs(zpart=one, nparts=4), *grads(), v, wsb, None) == L.GPSA_EINVAL
    assert bwd(*head, *btabs(zpart=one, nparts=4, usum=null1), *grads(), v, wsb, None) == L.GPSA_EINVAL
    # the fused LMC pass: F, W, Y, log_offset, log_disp, skip, S, N, L, P, zpart, nparts, dF, dW, usum, workspace
    lm = lib.gpsa_lmc_loglik_fused_nb_f32
    old = lib.gpsa_lmc_loglik_workspace(2 * 77, 3, 5, 512)
    need = lib.gpsa_lmc_loglik_nb_workspace(2 * 77, 3, 5, 512)
    G = (old - 256) // (3 * 5 * 4)
    assert need == ((old + 7) & ~7) + 8 * G * 5 and lib.gpsa_lmc_loglik_nb_workspace(0, 3, 5, 512) == 0
    assert lm(v, v, v, None, v, 0, 2, 77, 3, 5, v, 512, v, v, v, v, need - 1, None) == L.GPSA_EWORKSPACE
    assert lm(v, v, v, None, v, 0, 2, 77, 3, 5, v, 512, v, v, v, v, old, None) == L.GPSA_EWORKSPACE
    assert lm(v, v, v, None, v, 0, 2, 77, 3, 5, v, 512, v, v, v, None, need, None) == L.GPSA_EWORKSPACE
    for bad in (0, 1, 2, 4, 10, 12, 13, 14):  # F, W, Y, log_disp, zpart, dF, dW, usum
        args = [v, v, v, None, v, 0, 2, 77, 3, 5, v, 512, v, v, v, v, need, None]
        args[bad] = None
        assert lm(*args) == L.GPSA_EINVAL, bad
    assert lm(v, v, v, None, v, 0, 2, 77, 65, 5, v, 512, v, v, v, v, 1 << 30, None) == L.GPSA_EUNSUPPORTED
    # the fused ELBO pass: null tables, a workspace below the queried size
    M, Cn, Ln = 64, 231, 3
    qws = lib.gpsa_quadform_elbo_f32_workspace(M, Cn, Ln)
    assert qws > 0
    qf = lib.gpsa_quadform_elbo_nb_f32
    args = lambda ws, **kw: (1, kw.get("alpha", v), v, M, Cn, Ln, kw.get("mean", v), v, v, v, kw.get("Y", v), 77, 3, None, v,
                             v, v, kw.get("part", v), None, None, kw.get("rho", v), kw.get("u", v), kw.get("usum", v), 1, v,
                             ws, None)
    assert qf(*args(qws - 1)) == L.GPSA_EWORKSPACE  # (noise_u and log_offset may be NULL)
    for kw in (dict(alpha=None), dict(mean=None), dict(Y=None), dict(part=None), dict(rho=None), dict(u=None),
               dict(usum=None)):
        assert qf(*args(qws, **kw)) == L.GPSA_EINVAL, kw
    assert lib.gpsa_quadform_elbo_delta_nb_f32(*args(qws, mean=None)) == L.GPSA_EINVAL
    assert lib.gpsa_quadform_elbo_delta_nb_f32(*args(qws - 1)) in (L.GPSA_EWORKSPACE, L.GPSA_EUNSUPPORTED)
    # the plan's setters without a plan
    assert lib.gpsa_step_dispersion(None, 0, v, v, v, None) == L.GPSA_EINVAL
    assert lib.gpsa_step_likelihood(None, 0, 2, None) == L.GPSA_EINVAL


def test_negbin_kernel_resources():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_meta import demangle, library_kernels

    L = _lib()
    ks = library_kernels(L.LIB_PATH)
    by = dict(zip(demangle([k["name"] for k in ks]), ks))
    seen, lmc, n_fused, heads = set(), 0, 0, 0
    for nm, k in by.items():
        if "panel_elbo_nb_kernel<" in nm:
            n_fused += 1
            assert k["max_wg"] == 256, (nm, k)  # the launch bounds reached the instantiation
            assert "panel_elbo_pois_kernel<" not in nm
        if "panel_elbo_nb_kernel<13, 2, 2, true, true>" in nm or "panel_elbo_nb_kernel<13, 2, 4, true, true>" in nm:
            heads += 1  # the bounds the skip and Poisson heads are held to
            assert k["scratch"] == 0 and k["vgpr_spill"] <= 16 and k["sgpr_spill"] <= 400, (nm, k)
        if "lmc_mfma_nb_kernel<" in nm:
            lmc += 1
            assert k["max_wg"] == 256, (nm, k)
            assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["vgpr"] <= 256, (nm, k)  # two workgroups per CU
        for fam in ("loglik_nb_kernel<", "nb_const_kernel(", "nb_const_finish_kernel(", "nb_ddisp_kernel(",
                    "elbo_nb_finish_kernel("):
            if fam in nm:
                seen.add(fam + ("true" if "<true>" in nm else "false" if "<false>" in nm else ""))
                assert k["max_wg"] == 256, (nm, k)
                # (SGPR spills, if any, land in VGPR lanes: no scratch memory either way)
                assert k["scratch"] == 0 and k["vgpr_spill"] == 0, (nm, k)
        # the existing tests count the Poisson families by substring: no NB kernel may carry their names
        if "nb" in nm.split("(")[0]:
            assert "panel_elbo_pois_kernel<" not in nm and "lmc_mfma_pois_kernel<" not in nm
    assert len(seen) == 6 and lmc == 3 and n_fused == 12 and heads == 2, (seen, lmc, n_fused, heads)

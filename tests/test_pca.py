"""Expression PCA, the parts that need no GPU: the numpy yardstick of tests/pca_util.py against sklearn's recorded results
(tests/golden/reference_pca.npz, written by tests/golden/make_pca_golden.py), the eigengap condition the device suite's
component bar rests on, the yardstick's subspace iteration against its eigh, the C entries' declarations and pure
queries, the refusals of ``expression_pca`` that need no launch, and ``init_lmc_from_pca`` on a CPU model."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import pca_util as pu
import spatial_alignment_amd as gp
from spatial_alignment_amd import _lib, pca

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "reference_pca.npz"))
ENTRIES = [("gpsa_pca_gram_groups", "int", 2), ("gpsa_pca_gram_workspace", "long long", 3), ("gpsa_pca_gram_f32", "int", 11),
           ("gpsa_pca_project_f32", "int", 12)]
f64, f32 = torch.float64, torch.float32


def _source():
    return open(os.path.join(ROOT, "spatial_alignment_amd", "csrc", "pca.hip")).read()


@pytest.mark.parametrize("name", list(pu.VARIANTS))
def test_yardstick_against_sklearn(name):
    Y, ns, center, scale, k = pu.variant(name)
    y = pu.yardstick(Y, ns, center, scale, k)
    lam1 = y["explained_variance"][0]
    ref = {key: GOLDEN[f"{name}/{key}"] for key in ("components", "explained_variance", "explained_variance_ratio",
                                                    "singular_values")}
    assert ref["components"].shape == (k, Y.shape[1])
    assert (np.abs(y["components"] - ref["components"]) <= 1e-12 * np.maximum(1.0, np.abs(ref["components"]))).all()
    assert (np.abs(y["ratio"] - ref["explained_variance_ratio"]) <= 1e-12).all()
    assert (np.abs(y["explained_variance"] - ref["explained_variance"]) <= 1e-12 * lam1).all()
    assert (np.abs(y["singular_values"] - ref["singular_values"]) <= 1e-12 * ref["singular_values"][0]).all()
    # the scores are what the components say they are: uncorrelated, with the variances on the diagonal
    S = y["scores"]
    cov = S.T @ S / (Y.shape[0] - 1)
    assert np.abs(cov - np.diag(y["explained_variance"])).max() <= 1e-12 * lam1


def test_the_golden_file_holds_every_variant_and_a_constant_column():
    assert sorted({f.split("/")[0] for f in GOLDEN.files} - {"sklearn_version"}) == sorted(pu.VARIANTS)
    Y, ns, center, scale, k = pu.variant("scale_const")
    assert scale and np.ptp(Y[:, 7]) == 0
    _, _, inv = pu.view_stats(Y, ns, center, scale)
    assert inv[0, 7] == 0 and (np.delete(inv[0], 7) > 0).all()
    y = pu.yardstick(Y, ns, center, scale, k)
    assert (y["C"][7] == 0).all() and np.abs(y["components"][:, 7]).max() <= 1e-15  # the column contributes 0


@pytest.mark.parametrize("name", list(pu.VARIANTS))
def test_every_device_case_has_the_eigengap_the_component_bar_needs(name):
    Y, ns, center, scale, k = pu.variant(name)
    y = pu.yardstick(Y, ns, center, scale, k)
    gaps = pu.relative_gaps(y["eigenvalues"], k)
    assert gaps.shape == (k,) and gaps.min() >= pu.GAP_BAR, (name, float(gaps.min()))


@pytest.mark.parametrize("name", list(pu.VARIANTS))
def test_yardstick_subspace_iteration_against_eigh(name):
    Y, ns, center, scale, k = pu.variant(name)
    y = pu.yardstick(Y, ns, center, scale, k)
    m = pca.block_width(k, pu.OVERSAMPLE, Y.shape[1], Y.shape[0], len(y["ns"]))
    comps, lam, res, n_iter, conv = pu.subspace(y["C"], k, m)
    assert conv and n_iter == 10 and res.max() <= 1e-13
    assert np.abs(lam - y["explained_variance"]).max() <= 1e-12 * lam[0]
    assert np.abs(comps - y["components"]).max() <= 1e-10  # residual 1e-13 over a gap of 1e-3
    assert np.abs(res - pu.residuals(y["C"], comps, lam)).max() <= 1e-13


def test_yardstick_subspace_iteration_on_noise_needs_its_iterations():
    y = pu.yardstick(pu.noise_matrix(), [400], "pooled", False, pu.NOISE["k"])
    m = pu.NOISE["k"] + pu.OVERSAMPLE
    _, _, res, n_iter, conv = pu.subspace(y["C"], pu.NOISE["k"], m, max_iter=10)
    assert not conv and n_iter == 10 and res.max() > 1e-3
    comps, lam, res, n_iter, conv = pu.subspace(y["C"], pu.NOISE["k"], m, max_iter=300)
    assert conv and n_iter % 10 == 0 and n_iter < 300 and res.max() <= 1e-9
    assert np.abs(lam - y["explained_variance"]).max() <= 1e-12 * lam[0]


@pytest.mark.parametrize("name,res,n_args", ENTRIES)
def test_the_entries_are_declared_bound_and_defined(name, res, n_args):
    raw = open(os.path.join(ROOT, "include", "gpsa_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"\b" + res + r"\s+" + name + r"\s*\((.*?)\)\s*;", header, flags=re.S)
    assert m, f"{name} is not declared in include/gpsa_hip.h"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == n_args, args
    restype, argtypes = _lib.SIGNATURES[name]
    assert restype is (_lib._ll if res == "long long" else _lib._i) and len(argtypes) == n_args
    for a, t in zip(args, argtypes):
        if a.startswith("const long long* view_off"):  # the one host array
            want = C.POINTER(_lib._ll)
        elif "*" in a:
            want = _lib._vp
        else:
            want = _lib._ll if a.startswith("long long") else _lib._i
        assert t is want or t == want, (name, a, t)
    assert raw.index("csrc/register.hip") < raw.index("csrc/pca.hip") < raw.index(name + "(")
    assert re.search(r"\b" + res + r"\s+" + name + r"\s*\(", _source())


def test_the_constants_python_exports_are_the_kernels():
    from spatial_alignment_amd.ops import HipOps

    src = _source()
    for py, c in (("PCA_TILE", "PCA_T"), ("PCA_ROW_CHUNK", "PCA_KC"), ("PCA_MAX_GROUPS", "PCA_MAX_GROUPS"),
                  ("PCA_FILL", "PCA_FILL"), ("PCA_MAX_K", "PCA_MAX_K")):
        m = re.search(r"constexpr int " + c + r" = (\d+);", src)
        assert m and int(m.group(1)) == getattr(HipOps, py), c
    assert pca.MAX_K == HipOps.PCA_MAX_K
    # a kernel of this unit has one writer per element and the launches add in order: nothing in it is an atomic call
    assert not re.search(r"atomic[A-Z_(]", src)


def test_the_workspace_query_is_pure_and_the_entries_refuse_before_any_launch():
    """the pointers handed in are host memory, which a launch would not survive"""
    lib = _lib.load()
    T, K = 64, 32
    for N, P, V in ((2, 1, 1), (33, 65, 2), (1025, 129, 3), (4000, 2000, 1), (100000, 20000, 2), (100000, 1407, 1),
                    (100000, 1409, 1)):
        nt = -(-P // T)
        pairs = nt * (nt + 1) // 2
        G = 1 if pairs >= 256 else max(1, min(32, -(-256 // pairs), -(-N // K)))
        assert lib.gpsa_pca_gram_groups(N, P) == G, (N, P)
        assert lib.gpsa_pca_gram_workspace(N, P, V) == (8 * G * P * P if G > 1 else 0), (N, P, V)
    for N, P, V in ((0, 5, 1), (5, 0, 1), (5, 5, 0), (-1, 5, 1)):
        assert lib.gpsa_pca_gram_workspace(N, P, V) == 0
    buf = (C.c_double * 4096)()
    p = C.addressof(buf)
    off = (C.c_longlong * 3)(0, 2, 40)
    EINVAL, EWS = _lib.GPSA_EINVAL, _lib.GPSA_EWORKSPACE
    need = lib.gpsa_pca_gram_workspace(40, 5, 2)
    assert 0 < need <= 8 * 4096
    gram = lambda Y=p, N=40, P=5, mean=p, inv=p, vo=off, V=2, G=p, ws=p, nb=need: \
        lib.gpsa_pca_gram_f32(Y, N, P, mean, inv, vo, V, G, ws, nb, None)
    for kw in (dict(Y=None), dict(mean=None), dict(G=None), dict(N=1), dict(P=0), dict(P=2 ** 21), dict(vo=None), dict(V=0),
               dict(vo=(C.c_longlong * 3)(0, 0, 40)), dict(vo=(C.c_longlong * 3)(0, 2, 41))):
        assert gram(**kw) == EINVAL, kw
    assert gram(nb=need - 8) == EWS and gram(ws=None) == EWS
    proj = lambda Y=p, N=40, P=5, mean=p, inv=p, vo=off, V=2, comp=p, k=3, S=p, o64=0: \
        lib.gpsa_pca_project_f32(Y, N, P, mean, inv, vo, V, comp, k, S, o64, None)
    for kw in (dict(Y=None), dict(mean=None), dict(comp=None), dict(S=None), dict(N=0), dict(P=0), dict(k=0), dict(k=129),
               dict(o64=2), dict(vo=None), dict(V=0), dict(vo=(C.c_longlong * 3)(0, 40, 40))):
        assert proj(**kw) == EINVAL, kw


def test_expression_pca_refuses_by_rule_before_any_launch():
    Y = torch.zeros(12, 5)
    bad = [
        (dict(Y=Y.double()), "fp32"), (dict(Y=torch.zeros(5, 12).t()), "not contiguous"), (dict(Y=Y), "on device"),
        (dict(Y=torch.zeros(12)), "dense"), (dict(Y=np.zeros((12, 5), np.float32)), "dense"),
        (dict(n_components=0), "n_components"), (dict(n_components=6), "n_components"),
        (dict(n_components=True), "n_components"), (dict(n_components=2.0), "n_components"),
        (dict(Y=torch.zeros(5, 12), n_components=5), r"min\(P, N - V\) = 4"),
        (dict(n_samples_list=[6, 6], center="view", n_components=5), None),  # min(5, 12 - 2): allowed up to the device rule
        (dict(Y=torch.zeros(5, 12), n_samples_list=[2, 3], center="view", n_components=4), r"min\(P, N - V\) = 3"),
        (dict(n_samples_list=[11, 1]), "at least 2"), (dict(n_samples_list=[6, 5]), "sum to N"),
        (dict(n_samples_list=[]), "sum to N"), (dict(center="slice"), "center"), (dict(solver="lanczos"), "solver"),
        (dict(scale=1), "scale"), (dict(oversample=-1), "oversample"), (dict(tol=0.0), "tol"), (dict(tol=1), "tol"),
        (dict(max_iter=0), "max_iter"), (dict(check_every=0), "check_every"),
    ]
    for kw, rule in bad:
        args = dict(Y=Y, n_components=2)
        args.update(kw)
        with pytest.raises(ValueError, match=rule if rule else "on device"):
            gp.expression_pca(**args)
    with pytest.raises(ValueError, match="solver='host'"):
        gp.expression_pca(torch.zeros(600, 300), n_components=257)
    # the block's width: the oversampling gives way to the rank bound, silently
    assert pca.block_width(50, 10, 2000, 4000, 1) == 60 and pca.block_width(60, 10, 200, 64, 1) == 63
    assert pca.block_width(4, 10, 5, 100, 2) == 5 and pca.block_width(250, 10, 2000, 4000, 1) == 256


def test_close_moments_and_the_sign_rule_on_the_host():
    Y, ns, center, scale, k = pu.variant("scale_const")
    Yd = torch.from_numpy(np.asarray(Y, dtype=np.float64))
    mean, inv = pca.close_moments(Yd.sum(0, keepdim=True), (Yd * Yd).sum(0, keepdim=True), ns, True)
    _, wm, wi = pu.view_stats(Y, ns, center, scale)
    assert np.abs(mean.numpy() - wm).max() <= 1e-13 and inv[0, 7] == 0
    assert np.abs(inv.numpy() / np.where(wi > 0, wi, 1.0) - (wi > 0)).max() <= 1e-9
    assert pca.close_moments(Yd.sum(0, keepdim=True), (Yd * Yd).sum(0, keepdim=True), ns, False)[1] is None
    c = torch.tensor([[1.0, -3.0, 3.0], [0.5, 2.0, -2.0], [-1.0, 0.0, 1.0]], dtype=f64)
    want = torch.tensor([[-1.0, 3.0, -3.0], [0.5, 2.0, -2.0], [1.0, 0.0, -1.0]], dtype=f64)
    assert torch.equal(pca.sign_flip(c), want) and np.array_equal(pu.sign_rule(c.numpy()), want.numpy())
    assert np.array_equal(pca.start_block(7, 3, 5), np.random.default_rng(5).standard_normal((7, 3)))


def test_init_lmc_from_pca_on_a_cpu_model():
    from golden_io import Golden
    from model_util import build_model

    g = Golden("c3_lmc_matern12_warp")
    model, dd = build_model(g)
    m = g.mods[0]
    L_, P = (int(s) for s in model.W_dict[m].shape)
    Y = np.asarray(dd[m]["outputs"], dtype=np.float64)
    y = pu.yardstick(Y, dd[m]["n_samples_list"], "view", False, L_)
    res = gp.ExpressionPCA(components=torch.from_numpy(y["components"]),
                           explained_variance=torch.from_numpy(y["explained_variance"]))
    torch.manual_seed(0)
    fresh = torch.randn(L_, P)
    before = model.W_dict[m].detach().clone()
    assert gp.init_lmc_from_pca(model, res, modality=m) is model
    want = (y["components"] * np.sqrt(y["explained_variance"])[:, None]).astype(np.float32)
    assert model.W_dict[m].dtype == f32 and np.array_equal(model.W_dict[m].detach().numpy(), want)
    assert not torch.equal(before, model.W_dict[m].detach()) and fresh.shape == before.shape
    small = gp.ExpressionPCA(components=res.components[:2], explained_variance=res.explained_variance[:2])
    with pytest.raises(ValueError, match=r"\[n_latent_gps, P\]"):
        gp.init_lmc_from_pca(model, small, modality=m)
    with pytest.raises(ValueError, match="no LMC loadings"):
        gp.init_lmc_from_pca(model, res, modality="histology")
    g2 = Golden("c2_three_free_views")
    plain, _ = build_model(g2)
    with pytest.raises(ValueError, match="no LMC loadings"):
        gp.init_lmc_from_pca(plain, res, modality=g2.mods[0])
    # opt-in: a model built after the call is what it was before it
    again, _ = build_model(g)
    assert torch.equal(again.W_dict[m].detach(), before)


def test_the_public_names():
    import gpsa

    for name in ("expression_pca", "ExpressionPCA", "init_lmc_from_pca"):
        assert name in gp.__all__ and getattr(gpsa, name) is getattr(gp, name)
    assert hasattr(torch.ops.gpsa, "pca_gram") and hasattr(torch.ops.gpsa, "pca_project")

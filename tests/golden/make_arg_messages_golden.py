"""Recorder of tests/golden/arg_messages.json: the exception type and the exact ``str(exc)`` of every refusal that the public
toolbox entry points (neighbors, counts, gpr, ot, autocorr, image, register, pca) make before any device work - the
CPU-tensor refusal, wrong ranks and shapes of each tensor argument, the ``n_samples_list`` rules, the chunk, count and
``k`` rules, the float-valued integers (``3.0`` is taken by ``int(v) != v`` checks and refused by ``isinstance(v, int)``
ones).  tests/test_args_messages.py runs the same cases and compares: shared argument checks must not move a message or
an acceptance rule.

    python tests/golden/make_arg_messages_golden.py --commit <sha>      (no device needed; rewrites the JSON)

Every case runs on CPU tensors.  A case whose arguments pass every rule ends at the CPU-tensor refusal, which is the
last check of each entry: that pins "accepted".  The mixed-device refusal needs two devices and is not recorded.
``alignment_score`` and ``warp_image`` take a model: the golden case c1_example_fixed0, built on the host.
"""
import json
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "arg_messages.json")


def _host_model():
    """the model of the golden case c1_example_fixed0 on the host (view 0 fixed), with its coordinates and outputs"""
    import sys

    tests = os.path.dirname(HERE)
    if tests not in sys.path:
        sys.path.insert(0, tests)
    from golden_io import Golden
    from model_util import build_model

    g = Golden("c1_example_fixed0")
    model, dd = build_model(g, device="cpu")
    return model, {m: dd[m]["spatial_coords"] for m in g.mods}, {m: dd[m]["outputs"] for m in g.mods}


def cases():
    """yields (name, thunk); every thunk raises"""
    from spatial_alignment_amd import autocorr, counts, gpr, image, neighbors as nb, ot, pca, register as rg

    z = torch.zeros
    X, Y = z(6, 2), z(6, 3)
    nanX, nanY = X.clone(), Y.clone()
    nanX[1, 0], nanY[2, 1] = float("nan"), float("inf")
    f64 = torch.float64

    # ---- neighbors
    for name, call in (("knn", lambda **kw: nb.knn(X, **kw)), ("knn_regress", lambda **kw: nb.knn_regress(X, Y, **kw)),
                       ("spatial_r2", lambda **kw: nb.spatial_r2(X, Y, **kw)),
                       ("kth_neighbor_distance", lambda **kw: nb.kth_neighbor_distance(X, **kw)),
                       ("moran_i", lambda **kw: nb.moran_i(X, Y, **kw)),
                       ("spatial_graph", lambda **kw: autocorr.spatial_graph(X, **kw)),
                       ("spatial_autocorr", lambda **kw: autocorr.spatial_autocorr(X, Y, **kw))):
        yield f"{name}/cpu", call
        for k in (0, 33, 3.0, True, 6, "3"):
            yield f"{name}/k={k!r}", lambda call=call, k=k: call(k=k)
        for c in (0, 3.0, 2.5, True, -1):
            yield f"{name}/rows_per_chunk={c!r}", lambda call=call, c=c: call(rows_per_chunk=c, k=2)
    for bad in (z(6), z(6, 5), z(0, 2), z(6, 2, dtype=torch.int64), "x", None):
        tag = bad if not torch.is_tensor(bad) else f"{bad.dtype}{tuple(bad.shape)}"
        yield f"knn/query={tag}", lambda bad=bad: nb.knn(bad)
        yield f"knn/ref={tag}", lambda bad=bad: nb.knn(X, bad)
        yield f"knn_regress/X_train={tag}", lambda bad=bad: nb.knn_regress(bad, Y)
        yield f"knn_regress/X_test={tag}", lambda bad=bad: nb.knn_regress(X, Y, bad)
        yield f"moran_i/X={tag}", lambda bad=bad: nb.moran_i(bad, Y)
        yield f"spatial_graph/X={tag}", lambda bad=bad: autocorr.spatial_graph(bad)
        yield f"spatial_autocorr/X={tag}", lambda bad=bad: autocorr.spatial_autocorr(bad, Y)
        yield f"gp_regress/X={tag}", lambda bad=bad: gpr.gp_regress(bad, Y)
        yield f"prediction_baselines/X_train={tag}", lambda bad=bad: gpr.prediction_baselines(bad, Y, X, Y, [6], [6])
        yield f"prediction_baselines/X_test={tag}", lambda bad=bad: gpr.prediction_baselines(X, Y, bad, Y, [6], [6])
    for bad in (z(5, 3), z(6), z(6, 0), z(6, 3, dtype=torch.int32), "y", None):
        tag = bad if not torch.is_tensor(bad) else f"{bad.dtype}{tuple(bad.shape)}"
        yield f"knn_regress/Y_train={tag}", lambda bad=bad: nb.knn_regress(X, bad)
        yield f"moran_i/Y={tag}", lambda bad=bad: nb.moran_i(X, bad)
        yield f"spatial_autocorr/Y={tag}", lambda bad=bad: autocorr.spatial_autocorr(X, bad)
        yield f"gp_regress/Y={tag}", lambda bad=bad: gpr.gp_regress(X, bad)
        yield f"prediction_baselines/Y_train={tag}", lambda bad=bad: gpr.prediction_baselines(X, bad, X, Y, [6], [6])
        yield f"prediction_baselines/Y_test={tag}", lambda bad=bad: gpr.prediction_baselines(X, Y, X, bad, [6], [6])
        yield f"r2_score/pred={tag}", lambda bad=bad: nb.r2_score(Y, bad)
        yield f"pearson/pred={tag}", lambda bad=bad: nb.pearson(Y, bad)
    yield "knn/ref D", lambda: nb.knn(X, z(4, 3))
    yield "knn/ref k", lambda: nb.knn(X, z(4, 2), k=5)
    yield "knn/exclude_self ref", lambda: nb.knn(X, z(4, 2), k=2, exclude_self=True)
    yield "knn_regress/X_test D", lambda: nb.knn_regress(X, Y, z(4, 3))
    yield "knn_regress/weights", lambda: nb.knn_regress(X, Y, weights="gauss")
    yield "knn_regress/exclude_self", lambda: nb.knn_regress(X, Y, z(4, 2), exclude_self=True)
    yield "moran_i/nan", lambda: nb.moran_i(X, nanY, k=2)
    yield "spatial_graph/symmetric", lambda: autocorr.spatial_graph(X, k=2, symmetric="both")

    # ---- autocorr
    sa = lambda **kw: autocorr.spatial_autocorr(X, Y, k=2, **kw)
    yield "spatial_autocorr/mode", lambda: sa(mode="x")
    yield "spatial_autocorr/symmetric", lambda: sa(symmetric="both")
    yield "spatial_autocorr/n<3", lambda: autocorr.spatial_autocorr(z(2, 2), z(2, 3), k=1)
    for v in (-1, 5.0, True):
        yield f"spatial_autocorr/n_perms={v!r}", lambda v=v: sa(n_perms=v)
    for v in (0, 4.0, True):
        yield f"spatial_autocorr/perms_per_chunk={v!r}", lambda v=v: sa(perms_per_chunk=v)
    for p in (z(2, 5, dtype=torch.int64), z(2, 6), z(6, dtype=torch.int64), "p"):
        tag = p if not torch.is_tensor(p) else f"{p.dtype}{tuple(p.shape)}"
        yield f"spatial_autocorr/perms={tag}", lambda p=p: sa(perms=p)
    yield "spatial_autocorr/perms ok", lambda: sa(perms=z(2, 6, dtype=torch.int64))
    yield "spatial_autocorr/nan", lambda: autocorr.spatial_autocorr(X, torch.full((6, 3), float("nan")), k=2)
    crow, col, w = z(7, dtype=torch.int64), z(4, dtype=torch.int32), z(4, dtype=f64)
    fc = autocorr.SpatialGraph.from_csr
    yield "from_csr/cpu", lambda: fc(crow, col, w, 6)
    for n in (0, 6.0, True):
        yield f"from_csr/n={n!r}", lambda n=n: fc(crow, col, w, n)
    yield "from_csr/crow shape", lambda: fc(z(6, dtype=torch.int64), col, w, 6)
    yield "from_csr/crow float", lambda: fc(z(7), col, w, 6)
    yield "from_csr/col rank", lambda: fc(crow, z(2, 2, dtype=torch.int32), w, 6)
    yield "from_csr/w int", lambda: fc(crow, col, z(4, dtype=torch.int64), 6)
    yield "from_csr/w list", lambda: fc(crow, col, [0.0] * 4, 6)
    yield "from_csr/nnz", lambda: fc(crow, col, z(5, dtype=f64), 6)
    for p in (z(2, 2), z(3, dtype=torch.int64), "p"):
        tag = p if not torch.is_tensor(p) else f"{p.dtype}{tuple(p.shape)}"
        yield f"fdr_bh/p={tag}", lambda p=p: autocorr.fdr_bh(p)

    # ---- counts
    C = torch.ones(6, 3)
    dense_calls = (("count_stats", lambda Y, **kw: counts.count_stats(Y, **kw)),
                   ("size_factors", lambda Y, **kw: counts.size_factors(Y, **kw)),
                   ("poisson_deviance", lambda Y, **kw: counts.poisson_deviance(Y, **kw)),
                   ("deviance_feature_selection", lambda Y, **kw: counts.deviance_feature_selection(Y, **kw)),
                   ("pearson_residuals", lambda Y, **kw: counts.pearson_residuals(Y, **kw)),
                   ("deviance_residuals", lambda Y, **kw: counts.deviance_residuals(Y, 100.0, **kw)),
                   ("normalize_log1p", lambda Y, **kw: counts.normalize_log1p(Y, **kw)),
                   ("standardize_views", lambda Y, **kw: counts.standardize_views(Y, [3, 3], **kw)),
                   ("column_moments", lambda Y, **kw: counts.column_moments(Y, [3, 3], **kw)),
                   ("highly_variable_genes", lambda Y, **kw: counts.highly_variable_genes(Y, [3, 3], **kw)),
                   ("prepare_counts", lambda Y, **kw: counts.prepare_counts(Y, [3, 3], **kw)))
    for name, call in dense_calls:
        yield f"{name}/cpu", lambda call=call: call(C)
        for bad in (z(6), z(0, 3), z(6, 3, dtype=torch.bool), z(6, 3, dtype=torch.complex64), [[1.0]]):
            tag = f"{bad.dtype}{tuple(bad.shape)}" if torch.is_tensor(bad) else type(bad).__name__
            yield f"{name}/Y={tag}", lambda call=call, bad=bad: call(bad)
    for name in ("pearson_residuals", "normalize_log1p", "standardize_views"):
        call = dict(dense_calls)[name]
        yield f"{name}/inplace f64", lambda call=call: call(C.double(), inplace=True)
        yield f"{name}/inplace strided", lambda call=call: call(torch.ones(3, 6).t(), inplace=True)
    lists = ([3, 2], [6, 0], [3.0, 3.0], [2.5, 3.5], [2.5, 4.2], [6], [5, 1], [], "ab", 6, None, [np.int64(3), np.int64(3)])
    for ns in lists:
        yield f"standardize_views/n_samples_list={ns!r}", lambda ns=ns: counts.standardize_views(C, ns)
        yield f"column_moments/n_samples_list={ns!r}", lambda ns=ns: counts.column_moments(C, ns)
        yield f"highly_variable_genes/n_samples_list={ns!r}", lambda ns=ns: counts.highly_variable_genes(C, ns)
        yield f"prepare_counts/n_samples_list={ns!r}", lambda ns=ns: counts.prepare_counts(C, ns)
        yield f"expression_pca/n_samples_list={ns!r}", lambda ns=ns: pca.expression_pca(C, ns, n_components=1)
        yield f"prealign_slices/n_samples_list={ns!r}", lambda ns=ns: rg.prealign_slices(X, Y, ns)
        yield f"prediction_baselines/n_samples_list_train={ns!r}", lambda ns=ns: gpr.prediction_baselines(X, Y, X, Y, ns, [3, 3])
        yield f"prediction_baselines/n_samples_list_test={ns!r}", lambda ns=ns: gpr.prediction_baselines(X, Y, X, Y, [3, 3], ns)
    for v in (10.0, 0, True, 2):
        yield f"prepare_counts/n_top_genes={v!r}", lambda v=v: counts.prepare_counts(C, [3, 3], n_top_genes=v)
        yield f"highly_variable_genes/n_top_genes={v!r}", lambda v=v: counts.highly_variable_genes(C, [3, 3], n_top_genes=v)
        yield f"highly_variable_genes/n_bins={v!r}", lambda v=v: counts.highly_variable_genes(C, [3, 3], n_bins=v)
    pc = lambda **kw: counts.prepare_counts(C, [3, 3], **kw)
    yield "prepare_counts/transform", lambda: pc(transform="sqrt")
    yield "prepare_counts/selection", lambda: pc(selection="x")
    for v in (0, -1.0, True, float("nan"), "a", float("inf")):
        yield f"prepare_counts/theta={v!r}", lambda v=v: pc(theta=v)
    for v in (-1, True, "a", float("nan")):
        yield f"prepare_counts/min_counts={v!r}", lambda v=v: pc(min_counts=v)
        yield f"prepare_counts/max_counts={v!r}", lambda v=v: pc(max_counts=v)
        yield f"prepare_counts/min_cells={v!r}", lambda v=v: pc(min_cells=v)
    hv = lambda **kw: counts.highly_variable_genes(C, [3, 3], **kw)
    yield "highly_variable_genes/transform", lambda: hv(transform="sqrt")
    yield "highly_variable_genes/target_sum identity", lambda: hv(transform="identity", target_sum=10.0)
    yield "highly_variable_genes/target_sum", lambda: hv(transform="normalize", target_sum=-1.0)
    yield "highly_variable_genes/combine", lambda: hv(combine="x")
    yield "highly_variable_genes/min_mean", lambda: hv(min_mean="a")
    yield "highly_variable_genes/max_disp", lambda: hv(max_disp=float("nan"))
    yield "highly_variable_genes/gene_mask", lambda: hv(gene_mask=[True, False])
    yield "column_moments/transform", lambda: counts.column_moments(C, transform="sqrt")
    yield "column_moments/none", lambda: counts.column_moments(C)
    yield "column_moments/one row", lambda: counts.column_moments(torch.ones(1, 3))
    yield "normalize_log1p/target_sum", lambda: counts.normalize_log1p(C, target_sum=-1.0)
    yield "poisson_deviance/log_sz", lambda: counts.poisson_deviance(C, log_sz=z(5))
    cz = (torch.tensor([0, 1, 2]), torch.tensor([0, 1], dtype=torch.int32), torch.ones(2))
    yield "csr_counts/cpu tuple", lambda: counts.csr_counts((*cz, (2, 3)))
    yield "csr_counts/device", lambda: counts.csr_counts((*cz, (2, 3)), device="cpu")
    yield "csr_counts/type", lambda: counts.csr_counts(C)
    yield "csr_counts/shape", lambda: counts.csr_counts((*cz, (2, 0)))
    yield "csr_counts/crow rank", lambda: counts.csr_counts((z(2, 2), cz[1], cz[2], (2, 3)))
    yield "csr_counts/col list", lambda: counts.csr_counts((cz[0], [0, 1], cz[2], (2, 3)))
    yield "csr_counts/crow dtype", lambda: counts.csr_counts((z(3), cz[1], cz[2], (2, 3)))
    yield "csr_counts/crow len", lambda: counts.csr_counts((cz[0], cz[1], cz[2], (3, 3)))
    yield "csr_counts/nnz", lambda: counts.csr_counts((cz[0], cz[1], torch.ones(3), (2, 3)))
    yield "csr_counts/coo", lambda: counts.csr_counts(C.to_sparse())
    yield "prepare_counts/sparse cpu", lambda: counts.prepare_counts(C.to_sparse_csr(), [3, 3])
    yield "pearson_residuals/sparse", lambda: counts.pearson_residuals(C.to_sparse_csr())

    # ---- gpr
    gp = lambda **kw: gpr.gp_regress(X, Y, **kw)
    yield "gp_regress/cpu", gp
    yield "gp_regress/kernel", lambda: gp(kernel="x")
    for v in ((1.0,), (0.0, 1.0), (2.0, 1.0), "ab", None, (1e-3, float("inf"))):
        yield f"gp_regress/bounds={v!r}", lambda v=v: gp(bounds=v)
    for v in ([0.0, 0.0], [0.0, float("nan"), 0.0], "abc", torch.zeros(3)):
        yield f"gp_regress/theta0={v!r}", lambda v=v: gp(theta0=v)
    for v in (5.0, -1, 2.5, True, 0):
        yield f"gp_regress/max_iter={v!r}", lambda v=v: gp(max_iter=v)
    yield "gp_regress/gtol", lambda: gp(gtol=0.0)
    for v in (-1.0, float("inf"), float("nan")):
        yield f"gp_regress/jitter={v!r}", lambda v=v: gp(jitter=v)
    yield "gp_regress/nan X", lambda: gpr.gp_regress(nanX, Y)
    yield "gp_regress/nan Y", lambda: gpr.gp_regress(X, nanY)
    yield "gp_regress/nan X and Y", lambda: gpr.gp_regress(nanX, nanY)
    fit = gpr.GPRegression("rbf", False, 1e-10, X.double(), Y.double(), np.zeros(3), 0.0, np.zeros(3), Y.double(),
                           z(6, 6, dtype=f64), 0, 1, True)
    yield "GPRegression.predict/cpu", lambda: fit.predict(X)
    for bad in (z(6), z(4, 3), z(4, 5), z(0, 2), "x"):
        tag = bad if not torch.is_tensor(bad) else f"{bad.dtype}{tuple(bad.shape)}"
        yield f"GPRegression.predict/Xs={tag}", lambda bad=bad: fit.predict(bad)
    for c in (0, 3.0, 2.5, True):
        yield f"GPRegression.predict/rows_per_chunk={c!r}", lambda c=c: fit.predict(X, rows_per_chunk=c)
    yield "GPRegression.predict/nan", lambda: fit.predict(nanX)
    yield "GPRegression.log_marginal_likelihood/theta", lambda: fit.log_marginal_likelihood([0.0, 0.0])
    pb = gpr.prediction_baselines
    yield "prediction_baselines/cpu", lambda: pb(X, Y, X, Y, [3, 3], [3, 3])
    yield "prediction_baselines/P", lambda: pb(X, Y, X, z(6, 4), [3, 3], [3, 3])
    yield "prediction_baselines/X_test D", lambda: pb(X, Y, z(6, 3), Y, [3, 3], [3, 3])
    yield "prediction_baselines/kernel", lambda: pb(X, Y, X, Y, [3, 3], [3, 3], kernel="x")
    yield "prediction_baselines/views", lambda: pb(X, Y, X, Y, [3, 3], [2, 2, 2])
    yield "prediction_baselines/no training rows", lambda: pb(X, Y, X, Y, [6, 0], [3, 3])
    yield "prediction_baselines/nan second", lambda: pb(X, nanY, nanX, Y, [3, 3], [3, 3])
    yield "prediction_baselines/nan last", lambda: pb(X, Y, X, nanY, [3, 3], [3, 3])

    # ---- ot
    XB, YB = z(5, 2), z(5, 3)
    oa = lambda **kw: ot.ot_align(X, Y, XB, YB, **kw)
    yield "ot_align/cpu", oa
    for pos in range(4):
        for bad in (z(6), z(0, 2), z(6, 2, dtype=torch.int64), "x"):
            tag = bad if not torch.is_tensor(bad) else f"{bad.dtype}{tuple(bad.shape)}"
            args = [X, Y, XB, YB]
            args[pos] = bad
            yield f"ot_align/arg{pos}={tag}", lambda args=args: ot.ot_align(*args)
    yield "ot_align/D", lambda: ot.ot_align(X, Y, z(5, 3), YB)
    yield "ot_align/D=5", lambda: ot.ot_align(z(6, 5), Y, z(5, 5), YB)
    yield "ot_align/rows", lambda: ot.ot_align(X, z(5, 3), XB, YB)
    yield "ot_align/genes", lambda: ot.ot_align(X, Y, XB, z(5, 4))
    yield "ot_align/dissimilarity", lambda: oa(dissimilarity="x")
    yield "ot_align/alpha", lambda: oa(alpha=2.0)
    yield "ot_align/epsilon", lambda: oa(epsilon=0.0)
    for name in ("max_iter", "sinkhorn_iters", "sync_every"):
        for v in (5.0, 0, 2.5, True):
            yield f"ot_align/{name}={v!r}", lambda name=name, v=v: oa(**{name: v})
    yield "ot_align/tol", lambda: oa(tol=-1.0)
    yield "ot_align/T_init", lambda: oa(T_init=z(5, 6))
    yield "ot_align/T_init list", lambda: oa(T_init=[[0.0]])

    # ---- image
    img = np.zeros((8, 9, 3), dtype=np.float32)
    ip = lambda im=img, **kw: image.image_pixels(im, device="cpu", **kw)
    yield "image_pixels/cpu", ip
    yield "image_pixels/type", lambda: ip([[0.0]])
    yield "image_pixels/rank", lambda: ip(np.zeros(8, dtype=np.float32))
    yield "image_pixels/channels", lambda: ip(np.zeros((8, 9, 5), dtype=np.float32))
    yield "image_pixels/dtype", lambda: ip(np.zeros((8, 9), dtype=np.int32))
    for v in (0, 65, 2.0, True, 9):
        yield f"image_pixels/bin={v!r}", lambda v=v: ip(bin=v)
    yield "image_pixels/background", lambda: ip(background=float("inf"))
    yield "image_pixels/spots and bbox", lambda: ip(spots=z(3, 2), bbox=(0, 1, 0, 1))
    yield "image_pixels/spots", lambda: ip(spots=z(3, 3))
    yield "image_pixels/bbox", lambda: ip(bbox=(0, 1, 0))
    yield "image_pixels/bbox nan", lambda: ip(bbox=(0, 1, 0, float("nan")))

    hm = lambda *a, **kw: image.histology_modality(*a, device="cpu", **kw)
    yield "histology_modality/cpu", lambda: hm([img], [z(3, 2)])
    yield "histology_modality/no image", lambda: hm([])
    yield "histology_modality/spots_list", lambda: hm([img, img], [z(3, 2)])
    for v in (0, 4.0, True):
        yield f"histology_modality/n_samples={v!r}", lambda v=v: hm([img], [z(3, 2)], n_samples=v)

    # ---- the entries that take a model: a small one on the host
    model, Xs, Ys = _host_model()
    mod = next(iter(Xs))
    N, D = int(Xs[mod].shape[0]), int(model.n_spatial_dims)
    asc = lambda X=Xs, Yv=Ys, *a, **kw: nb.alignment_score(model, X, Yv, *a, **kw)
    yield "alignment_score/cpu", asc
    yield "alignment_score/cpu G", lambda: asc(G={mod: Xs[mod].double()})
    for name, bad in (("rows", Xs[mod][:-1]), ("rank", Xs[mod][:, 0]), ("D", z(N, D + 1)), ("list", [[0.0]])):
        yield f"alignment_score/X_spatial {name}", lambda bad=bad: asc({mod: bad})
        yield f"alignment_score/G {name}", lambda bad=bad: asc(G={mod: bad})
    for name, bad in (("rows", Ys[mod][:-1]), ("rank", Ys[mod][:, 0]), ("list", [[0.0]])):
        yield f"alignment_score/Y {name}", lambda bad=bad: asc(Yv={mod: bad})
    for k in (0, 33, 3.0, True, N):
        yield f"alignment_score/k={k!r}", lambda k=k: asc(k=k)
    yield "alignment_score/weights", lambda: asc(weights="gaussian")
    for c in (0, 3.0, 2.5, True):
        yield f"alignment_score/rows_per_chunk={c!r}", lambda c=c: asc(rows_per_chunk=c)
    views = lambda *parts: {mod: list(parts) + [np.arange(0)] * (int(model.n_views) - len(parts))}
    yield "alignment_score/small view", lambda: asc(Xs, Ys, views(np.arange(5), np.arange(5, N)), k=6)
    yield "alignment_score/one view", lambda: asc(Xs, Ys, views(np.arange(N)))
    fr = image.Frame()
    wi = lambda **kw: image.warp_image(model, img, **{"view": 1, "img_frame": fr, **kw})
    yield "warp_image/cpu", wi
    yield "warp_image/cpu fixed view", lambda: wi(view=0)
    for v in (2, -1, True, 1.0):
        yield f"warp_image/view={v!r}", lambda v=v: wi(view=v)
    yield "warp_image/img_frame", lambda: wi(img_frame=(0, 1))
    yield "warp_image/out_frame", lambda: wi(out_frame="x")
    for v in (5.0, -1, 1.5, True):
        yield f"warp_image/max_iter={v!r}", lambda v=v: wi(max_iter=v)
    for v in (2, True, 1.0):
        yield f"warp_image/order={v!r}", lambda v=v: wi(order=v)
    for v in ((0, 4), 5, (2.0, 3), (3, 4)):
        yield f"warp_image/out_shape={v!r}", lambda v=v: wi(out_shape=v)
    for v in (0, 3.0, 2.5, True):
        yield f"warp_image/rows_per_chunk={v!r}", lambda v=v: wi(rows_per_chunk=v)
    yield "warp_image/img", lambda: image.warp_image(model, np.zeros(8, np.float32), 1, img_frame=fr)

    # ---- register
    T = z(2, 6)
    rs = lambda **kw: rg.rigid_scores(X, Y, XB, YB, T, 1.0, **kw)
    rr = lambda **kw: rg.rigid_register(X, Y, XB, YB, **kw)
    yield "rigid_scores/cpu", rs
    yield "rigid_register/cpu", rr
    yield "prealign_slices/cpu", lambda: rg.prealign_slices(X, Y, [3, 3])
    for name, call in (("rigid_scores", lambda *a: rg.rigid_scores(*a, T, 1.0)), ("rigid_register", rg.rigid_register)):
        for pos, shapes in ((0, (z(6), z(6, 3), z(0, 2), "x")), (2, (z(5), z(5, 3), "x")),
                            (1, (z(5, 3), z(6), z(6, 0), z(6, 3, dtype=torch.int64), "y")), (3, (z(6, 3), z(5, 4), None))):
            for bad in shapes:
                tag = bad if not torch.is_tensor(bad) else f"{bad.dtype}{tuple(bad.shape)}"
                args = [X, Y, XB, YB]
                args[pos] = bad
                yield f"{name}/arg{pos}={tag}", lambda call=call, args=args: call(*args)
        for v in (8.0, 0, True, 8):
            yield f"{name}/candidates_per_chunk={v!r}", lambda name=name, v=v: (rs if name == "rigid_scores" else rr)(candidates_per_chunk=v)
    for bad in (z(2, 5), z(6), z(0, 6), z(2, 6, dtype=torch.int64), "t"):
        tag = bad if not torch.is_tensor(bad) else f"{bad.dtype}{tuple(bad.shape)}"
        yield f"rigid_scores/transforms={tag}", lambda bad=bad: rg.rigid_scores(X, Y, XB, YB, bad, 1.0)
    for v in (-1.0, float("inf"), float("nan")):
        yield f"rigid_scores/max_dist={v!r}", lambda v=v: rg.rigid_scores(X, Y, XB, YB, T, v)
    for name in ("n_angles", "n_shifts", "levels"):
        for v in (3.0, 0, -1, True):
            yield f"rigid_register/{name}={v!r}", lambda name=name, v=v: rr(**{name: v})
    yield "rigid_register/min_overlap", lambda: rr(min_overlap=0.0)
    yield "rigid_register/shift_extent", lambda: rr(shift_extent=-1.0)
    yield "rigid_register/max_dist", lambda: rr(max_dist=0.0)
    yield "rigid_register/one row", lambda: rg.rigid_register(z(1, 2), z(1, 3), XB, YB)
    pa = rg.prealign_slices
    yield "prealign_slices/X rank", lambda: pa(z(6), Y, [3, 3])
    yield "prealign_slices/Y rows", lambda: pa(X, z(5, 3), [3, 3])
    yield "prealign_slices/D", lambda: pa(z(6, 3), Y, [3, 3])
    for v in (2, -1, True, 1.0):
        yield f"prealign_slices/reference={v!r}", lambda v=v: pa(X, Y, [3, 3], reference=v)
    reg = rg.RigidRegistration(R=torch.eye(2, dtype=f64), t=z(2, dtype=f64))
    yield "RigidRegistration.apply", lambda: reg.apply(z(3, 3))

    # ---- pca
    ep = lambda Yp=C, ns=None, **kw: pca.expression_pca(Yp, ns, **{"n_components": 1, **kw})
    yield "expression_pca/cpu", ep
    for bad in (z(6), z(0, 3), z(6, 3, dtype=f64), torch.ones(3, 6).t(), "y"):
        tag = f"{bad.dtype}{tuple(bad.shape)}{bad.is_contiguous()}" if torch.is_tensor(bad) else bad
        yield f"expression_pca/Y={tag}", lambda bad=bad: ep(bad)
    yield "expression_pca/center", lambda: ep(center="x")
    yield "expression_pca/solver", lambda: ep(solver="x")
    yield "expression_pca/scale", lambda: ep(scale=1)
    for v in (0, 3.0, True, 6):
        yield f"expression_pca/n_components={v!r}", lambda v=v: ep(n_components=v)
        yield f"expression_pca/max_iter={v!r}", lambda v=v: ep(max_iter=v)
        yield f"expression_pca/check_every={v!r}", lambda v=v: ep(check_every=v)
    for v in (-1, 2.0, True):
        yield f"expression_pca/oversample={v!r}", lambda v=v: ep(oversample=v)
    for v in (0.0, 1, float("inf")):
        yield f"expression_pca/tol={v!r}", lambda v=v: ep(tol=v)
    for center in ("pooled", "view"):
        fitted = pca.ExpressionPCA(components=z(2, 3, dtype=f64), mean=z(2 if center == "view" else 1, 3, dtype=f64),
                                   inv_scale=None, center=center, n_views=2 if center == "view" else 1)
        yield f"transform/{center}/cpu", lambda f=fitted: f.transform(C, [3, 3])
        yield f"transform/{center}/P", lambda f=fitted: f.transform(torch.ones(6, 4), [3, 3])
        yield f"transform/{center}/dtype", lambda f=fitted: f.transform(C.double(), [3, 3])
        yield f"transform/{center}/rank", lambda f=fitted: f.transform(z(6), [3, 3])
        for bad in (z(6, 3), z(6), z(0, 2), z(6, 2, dtype=torch.int64), "s"):
            tag = bad if not torch.is_tensor(bad) else f"{bad.dtype}{tuple(bad.shape)}"
            yield f"inverse_transform/{center}/scores={tag}", lambda f=fitted, bad=bad: f.inverse_transform(bad, [3, 3])
        for ns in ([3, 2], [6], [2, 2, 2], [6, 0], [2.5, 4.2], None):
            yield f"transform/{center}/n_samples_list={ns!r}", lambda f=fitted, ns=ns: f.transform(C, ns)
            # (inverse_transform has no device check of its own: only the lists it refuses are cases)
            if center == "view" and ns not in ([2.5, 4.2],):
                yield f"inverse_transform/{center}/n_samples_list={ns!r}", lambda f=fitted, ns=ns: f.inverse_transform(z(6, 2), ns)


def record():
    """{case: [exception type, str(exc)]}; a case that raises nothing is recorded as ["none", ""]"""
    out = {}
    for name, thunk in cases():
        assert name not in out, name
        try:
            thunk()
            out[name] = ["none", ""]
        except Exception as e:  # noqa: BLE001 - the type is part of what is recorded
            out[name] = [type(e).__name__, str(e)]
    return out


def main():
    import argparse
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit whose messages are recorded")
    ap.add_argument("--out", default=PATH)
    args = ap.parse_args()
    doc = dict(commit=args.commit, messages=record())
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(doc['messages'])} messages -> {args.out}")


if __name__ == "__main__":
    main()

"""Recorder of tests/golden/toolbox_fold_bits.json: one sha256 per (case, output tensor) of the raw bytes that the toolbox
kernels sharing csrc/toolbox.hpp write (csrc/ot.hip, gpr.hip, register.hip, neighbors.hip), through ``HipOps``.
tests/test_toolbox_bits_gpu.py loads this file, rebuilds the same inputs from their seeds, runs the same entries and
compares every digest: the closing folds, the row staging, the key order and the slice heuristic were moved into one
header, and code that only moved must not move a bit.

    python tests/golden/make_toolbox_fold_golden.py --commit <sha>      (on the device; rewrites the JSON)

The JSON was recorded from the commit BEFORE the header existed (its ``commit`` field).  Inputs are the same bytes on
every host: integer draws of ``numpy.random.default_rng(seed)`` divided by whole numbers (one IEEE division each).
``parts`` is passed wherever an entry takes it, so nothing depends on the device's CU count.

ot_dist         n = 1, 64, 65 (one row past a 64-tile: the mirror write-back), D = 1 and 4 (zero padding of the staged
                rows to MAXD and beyond n).
ot_cost/ot_plan (n, m) = (1, 1); (65, 130): one row and two columns past a tile; (257, 3265): 257 workgroups of the cost
                pass (its cap, OT_COST_BLOCKS = 1024, is above 256), 5 row groups x 52 column tiles = 260 change sums and
                more than 256 rows and columns, so all three strided loads of the closings wrap.
gpr_lml_grad    N = 1, 65 (3 tiles: fewer partials than threads) with every kernel and P = 1, 5; N = 1409 (23 tile rows,
                276 partials: the strided load wraps) with every kernel and P = 1, 5.
gpr_cov         same=True at N = 65, same=False at (64, 65), every kernel, D = 3.
rigid_scores    n = 33 (two row groups at the 32-row minimum), m = 1025 (two LDS tiles), K = 1 and 9 (one candidate
                past a group of 8), parts = 1 and 3 (the merge by the key), P = 1 and 70 (both closing widths), with the
                tables; the points of A lie on a coarse grid, so equal distances occur and the index decides.
knn             nr = 513 (two LDS tiles), D = 2, k = 1 and 32, parts = 1 and 3, exclude_self on and off; the points lie
                on a 16 x 16 grid, so every query has duplicates among the references and the index decides.
"""
import hashlib
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "toolbox_fold_bits.json")
KERNELS = ("rbf", "matern12", "matern32")
THETA = (0.25, -0.5, -2.0)   # log a, log l, log tau2
OT_SHAPES = ((1, 1), (65, 130), (257, 3265))


def grid(rng, shape, lo, hi, div):
    """whole numbers in [lo, hi) over div"""
    return rng.integers(lo, hi, size=shape) / float(div)


def entries(o, dev):
    """yields (case, thunk): thunk() runs one entry on fresh copies of its inputs and returns {output name: tensor}"""
    import torch

    t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    t32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)

    for n in (1, 64, 65):
        for D in (1, 4):
            X = t64(grid(np.random.default_rng(100 + n + D), (n, D), -64, 65, 16))
            yield f"ot_dist/n{n}_D{D}", lambda X=X: dict(out=o.ot_dist(X))

    for n, m in OT_SHAPES:
        rng = np.random.default_rng(200 + n)
        G, M = t64(grid(rng, (n, m), 0, 256, 64)), t64(grid(rng, (n, m), 0, 256, 64))
        T = t64(grid(rng, (n, m), 0, 64, 64 * n * m))
        cA, cAt = t64(grid(rng, n, 0, 128, 32)), t64(grid(rng, n, 0, 128, 32))
        cB, cBt = t64(grid(rng, m, 0, 128, 32)), t64(grid(rng, m, 0, 128, 32))

        def cost(G=G, M=M, T=T, cA=cA, cB=cB, cAt=cAt, cBt=cBt):
            return dict(zip(("cost", "sums"), o.ot_cost(G.clone(), M, T, cA, cB, cAt, cBt, 0.375)))

        yield f"ot_cost/n{n}_m{m}", cost
        f, g = t64(grid(rng, n, -32, 32, 64)), t64(grid(rng, m, -32, 32, 64))
        a, b = t64(np.full(n, 1.0 / n)), t64(np.full(m, 1.0 / m))
        eps = t64(np.array([0.5]))

        def plan(C=M, f=f, g=g, a=a, b=b, eps=eps, T=T):
            return dict(zip(("T", "rowsum", "colsum", "sums"), o.ot_plan(C, f, g, a, b, eps, T.clone())))

        yield f"ot_plan/n{n}_m{m}", plan

    theta = t64(np.array(THETA))
    for N in (1, 65, 1409):
        rng = np.random.default_rng(300 + N)
        X = t64(grid(rng, (N, 2), -64, 65, 32))
        Kinv = t64(grid(rng, (N, N), -128, 129, 1024))
        for P in (1, 5):
            alpha = t64(grid(rng, (N, P), -64, 65, 64))
            for kind in KERNELS:
                yield f"gpr_lml_grad/{kind}/N{N}_P{P}", lambda kind=kind, X=X, al=alpha, Ki=Kinv: dict(
                    out=o.gpr_lml_grad(kind, X, theta, al, Ki, amplitude=True))

    rng = np.random.default_rng(400)
    XA, XB = t64(grid(rng, (65, 3), -64, 65, 32)), t64(grid(rng, (64, 3), -64, 65, 32))
    for kind in KERNELS:
        yield f"gpr_cov/{kind}/same_N65", lambda kind=kind: dict(
            out=o.gpr_cov(kind, XA, XA, theta, amplitude=True, same=True, jitter=2.0 ** -20))
        yield f"gpr_cov/{kind}/cross_64x65", lambda kind=kind: dict(out=o.gpr_cov(kind, XB, XA, theta, amplitude=True))

    n, m = 33, 1025
    rng = np.random.default_rng(500)
    RA, RB = t64(grid(rng, (m, 2), 0, 24, 4)), t64(grid(rng, (n, 2), 0, 96, 16))
    cand = np.tile(np.array([1.0, 0.0, 0.0, 1.0, 0.0, 0.0]), (9, 1))
    cand[1:, :4] = np.array([[0.0, -1.0, 1.0, 0.0], [-1.0, 0.0, 0.0, -1.0], [0.0, 1.0, -1.0, 0.0], [-1.0, 0.0, 0.0, 1.0]] * 2)
    cand[1:, 4:] = grid(rng, (8, 2), 0, 96, 16)
    for P in (1, 70):
        YA, YB = t32(grid(rng, (m, P), 0, 64, 8)), t32(grid(rng, (n, P), 0, 64, 8))
        for K in (1, 9):
            Tk = t64(cand[:K])
            for parts in (1, 3):
                yield f"rigid_scores/K{K}_P{P}_parts{parts}", lambda YA=YA, YB=YB, Tk=Tk, parts=parts: dict(zip(
                    ("sse", "n_matched", "d2_sum", "nn", "d2"),
                    o.rigid_scores(RA, YA, RB, YB, Tk, 0.03125, parts=parts, return_nn=True)))

    R = t64(grid(np.random.default_rng(600), (513, 2), 0, 16, 4))
    for k in (1, 32):
        for parts in (1, 3):
            for excl in (False, True):
                yield f"knn/k{k}_parts{parts}_{'excl' if excl else 'all'}", lambda k=k, parts=parts, excl=excl: dict(
                    zip(("idx", "d2"), o.knn(R, R, k, exclude_self=excl, parts=parts)))


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def record(o, dev):
    """{"case/output": sha256}; every entry runs twice and must repeat its bytes"""
    out = {}
    for case, thunk in entries(o, dev):
        first, second = thunk(), thunk()
        for k, t in first.items():
            d = digest(t)
            assert d == digest(second[k]), f"{case}/{k}: two runs differ"
            out[f"{case}/{k}"] = d
    return out


def main():
    import argparse
    import sys

    import torch

    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from spatial_alignment_amd import ops

    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit the library was built from")
    ap.add_argument("--out", default=PATH)
    args = ap.parse_args()
    dev = "cuda:0"
    digests = record(ops.get_ops(), dev)
    props = torch.cuda.get_device_properties(0)
    doc = dict(commit=args.commit, device=f"{props.name} ({props.gcnArchName})", digests=digests)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(digests)} digests -> {args.out}")


if __name__ == "__main__":
    main()

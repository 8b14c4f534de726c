"""Recorder of tests/golden/count_walk_bits.json: one sha256 per (case, entry, output tensor) of the raw bytes the count
kernels (csrc/counts.hip, counts_sparse.hip, moments.hip) write, through ``HipOps``.  tests/test_count_walk_bits_gpu.py
loads this file, rebuilds the same inputs from their seeds, runs the same entries and compares every digest: a change
that moves code between these units must not move a bit.

    python tests/golden/make_count_walk_golden.py --commit <sha>      (on the device; rewrites the JSON)

Inputs are the same bytes on every host: integer draws of ``numpy.random.default_rng(seed)`` and plain arithmetic (no
log / exp on the host).  Counts are whole numbers with zeros and some values >= 256 (past the y log y table); mode
"identity" also runs on a signed matrix of sixteenths, mode "expm1" on the counts over 64 (expm1 stays finite);
``log_sz`` = random - 0.5 and ``scale`` = random + 0.5.

Dense cases: [37, 1028] (three column tiles, the last 4 columns wide; float4 path; a last row group of 5 rows),
[37, 1027] (scalar path), [37, 1028] at a storage offset of one element (base not 16-byte aligned: scalar path with
P % 4 == 0), [3, 5] (fewer rows than waves), [16400, 3] (17 rows per group).  CSR cases: the [37, 1028] counts thinned to
about 30 % stored (more than 64 entries per row and tile: the ballot search and several sweep strides), with one row
fully stored and one empty; [3, 5]; [1000, 7] (32 rows per group for the counts walk, 63 for the moments walk) - each
with ``keep=None`` and with a mask that drops about a quarter of the rows, a whole 16-row group and rows on both sides
of group boundaries among them.
"""
import hashlib
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "count_walk_bits.json")
MODES = ("identity", "expm1", "normalize")


def counts_matrix(seed, N, P):
    """whole numbers in fp32: about a quarter zeros, about one in fifty >= 256"""
    rng = np.random.default_rng(seed)
    y = rng.integers(1, 9, size=(N, P))
    y = y * (rng.integers(0, 4, size=(N, P)) > 0)
    big = rng.integers(0, 50, size=(N, P)) == 0
    y = y + big * rng.integers(256, 3000, size=(N, P))
    return y.astype(np.float32)


def signed_matrix(seed, N, P):
    """signed sixteenths in fp32"""
    rng = np.random.default_rng(seed)
    return (rng.integers(-2000, 2001, size=(N, P)) / 16.0).astype(np.float32)


def row_vectors(seed, N):
    """(log_sz, scale) [N] fp64"""
    rng = np.random.default_rng(seed)
    return rng.random(N) - 0.5, rng.random(N) + 0.5


def view_sets(N):
    return [[0, N]] + ([[0, 5, 22, 37]] if N == 37 else [])


# (name, seed, N, P, storage offset in elements)
DENSE = (("d37x1028", 11, 37, 1028, 0), ("d37x1027", 12, 37, 1027, 0), ("d37x1028_off1", 11, 37, 1028, 1),
         ("d3x5", 13, 3, 5, 0), ("d16400x3", 14, 16400, 3, 0))
# (name, seed, N, P)
SPARSE = (("s37x1028", 11, 37, 1028), ("s3x5", 13, 3, 5), ("s1000x7", 15, 1000, 7))


def csr_arrays(name, seed, N, P):
    """(crow int64, col int32, val fp32): about 30 % of the counts + 1 stored (so every stored value is > 0)"""
    rng = np.random.default_rng(seed + 100)
    y = counts_matrix(seed, N, P) + 1.0
    stored = rng.integers(0, 10, size=(N, P)) < 3
    if N == 37:
        stored[7, :] = True   # a row fully stored
        stored[20, :] = False  # an empty row
    crow = np.concatenate([[0], np.cumsum(stored.sum(1))]).astype(np.int64)
    return crow, np.nonzero(stored)[1].astype(np.int32), y[stored].astype(np.float32)


def keep_mask(seed, N):
    rng = np.random.default_rng(seed + 200)
    keep = rng.integers(0, 4, size=N) > 0
    if N >= 37:
        keep[16:32] = False          # a whole 16-row group
        keep[[15, 32]] = False       # ... and the rows on both sides of its boundaries
        keep[[14, 33]] = True
    else:
        keep[:] = True
        keep[1] = False
    return keep


def _dense_tensor(torch, dev, y, offset):
    N, P = y.shape
    buf = torch.empty(N * P + offset, dtype=torch.float32, device=dev)
    Y = buf[offset:].view(N, P)
    Y.copy_(torch.from_numpy(y))
    assert Y.is_contiguous() and (offset == 0 or Y.data_ptr() % 16 != 0)
    return Y


def entries(o, dev):
    """yields (case, entry, thunk): thunk() runs the entry once and returns {output name: tensor}"""
    import torch

    t64 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64)).to(dev)
    for name, seed, N, P, offset in DENSE:
        Y = _dense_tensor(torch, dev, counts_matrix(seed, N, P), offset)
        S = _dense_tensor(torch, dev, signed_matrix(seed + 50, N, P), offset)
        E = _dense_tensor(torch, dev, counts_matrix(seed, N, P) / np.float32(64.0), offset)
        log_sz, scale = (t64(v) for v in row_vectors(seed + 300, N))
        yield name, "count_margins", lambda Y=Y: dict(zip(("row_sum", "col_sum", "row_nnz", "col_nnz", "n_invalid"),
                                                          o.count_margins(Y)))
        yield name, "count_deviance", lambda Y=Y, l=log_sz: dict(zip(("ll_sat", "abs_sat"), o.count_deviance(Y, l)))
        for off in view_sets(N):
            tag = "v" + "_".join(str(v) for v in off)
            yield name, f"standardize_views/{tag}", lambda Y=Y, off=off: dict(zip(("out", "n_constant"),
                                                                                   o.standardize_views(Y, off)))
            for mode, M in (("identity", Y), ("identity_signed", S), ("expm1", E), ("normalize", Y)):
                yield name, f"column_moments/{mode}/{tag}", lambda M=M, mode=mode, off=off, sc=scale: dict(zip(
                    ("s1", "s2", "abs1", "n_nonfinite"), o.column_moments(M, mode.split("_")[0], off, sc)))
    for name, seed, N, P in SPARSE:
        crow, col, val = (torch.from_numpy(a).to(dev) for a in csr_arrays(name, seed, N, P))
        val64 = val / 64.0
        log_sz, scale = (t64(v) for v in row_vectors(seed + 300, N))
        yield name, "csr_check", lambda a=(crow, col, val, N, P): dict(violations=o.csr_check(*a))
        for ktag, keep in (("all", None), ("masked", torch.from_numpy(keep_mask(seed, N)).to(dev))):
            yield name, f"count_margins_csr/{ktag}", lambda a=(crow, col, val, N, P), k=keep: dict(zip(
                ("row_sum", "col_sum", "row_nnz", "col_nnz", "n_invalid"), o.count_margins_csr(*a, k)))
            yield name, f"count_deviance_csr/{ktag}", lambda a=(crow, col, val, N, P), l=log_sz, k=keep: dict(zip(
                ("ll_sat", "abs_sat"), o.count_deviance_csr(*a, l, k)))
            for off in view_sets(N):
                tag = "v" + "_".join(str(v) for v in off)
                for mode in MODES:
                    v = val64 if mode == "expm1" else val
                    yield name, f"column_moments_csr/{mode}/{tag}/{ktag}", \
                        lambda a=(crow, col, v, N, P), mode=mode, off=off, sc=scale, k=keep: dict(zip(
                            ("s1", "s2", "abs1", "n_nonfinite"), o.column_moments_csr(*a, mode, off, sc, k)))


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def record(o, dev):
    """{"case/entry/output": sha256}; every entry runs twice and must repeat its bytes"""
    out = {}
    for case, entry, thunk in entries(o, dev):
        first, second = thunk(), thunk()
        for k, t in first.items():
            d = digest(t)
            assert d == digest(second[k]), f"{case}/{entry}/{k}: two runs differ"
            out[f"{case}/{entry}/{k}"] = d
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

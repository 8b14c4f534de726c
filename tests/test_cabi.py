"""The C-ABI library loads and exports every entry point include/gpsa_hip.h declares (no compute)."""
import os
import re

from spatial_alignment_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "gpsa_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(gpsa_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    lib = _lib.load()
    names = _declared()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/gpsa_hip.h but not exported"
    assert set(names) == set(_lib.SIGNATURES), set(names) ^ set(_lib.SIGNATURES)


def test_version_and_arch():
    lib = _lib.load()
    assert lib.gpsa_version() >= 100
    assert lib.gpsa_build_arch() == b"gfx950"


def test_workspace_queries_are_pure():
    lib = _lib.load()
    assert lib.gpsa_gemm_workspace(0, 200, 200, 1, 1) == 0
    assert lib.gpsa_gemm_workspace(1, 200, 200, 2, 4) == 2 * 4 * 200 * 200 * 8
    # 4 column blocks x 7 row chunks would leave the chip nearly empty: 8-row chunks (25 of them)
    # (D = 2: the register-accumulating backward, 16 inducing rows per workgroup -> 13 dX partials)
    assert lib.gpsa_kmat_bwd_workspace(0, 200, 1000, 2) == (4 * 400 + 13 * 2000 + 4 * 13 * 2) * 4
    assert lib.gpsa_kmat_bwd_workspace(0, 200, 1000, 3) == (4 * 600 + 25 * 3000 + 4 * 25 * 2) * 4
    assert lib.gpsa_kmat_bwd_workspace(0, 200, 100000, 2) == (391 * 400 + 13 * 200000 + 391 * 13 * 2) * 4
    assert lib.gpsa_kmat_bwd_workspace(0, 200, 100000, 3) == (391 * 600 + 7 * 300000 + 391 * 7 * 2) * 4
    assert lib.gpsa_quadform_workspace(0, 200, 1000, 50) >= 50 * 208 * 208 * 4


def test_loss_workspace_size_is_what_the_c_entries_ask_for():
    """torch_ops.loss_workspace_bytes restates csrc's per-term slot: the entries take that size (less its 64 spare bytes)
    and refuse 8 bytes less.  No launch: with S[0] = 0 an entry that accepts the workspace returns GPSA_EINVAL."""
    import ctypes as C

    from spatial_alignment_amd import torch_ops

    lib = _lib.load()
    for n in (1, 3):
        buf = (C.c_double * 4)()
        ptrs = (C.c_void_p * n)(*[C.addressof(buf)] * n)
        S, N, P = (C.c_int * n)(*[0] * n), (C.c_longlong * n)(*[1] * n), (C.c_int * n)(*[1] * n)
        need = torch_ops.loss_workspace_bytes(n) - 64
        for nbytes, want in ((need, _lib.GPSA_EINVAL), (need - 8, _lib.GPSA_EWORKSPACE)):
            a = (n, ptrs, ptrs, ptrs, S, N, P)
            out = (C.addressof(buf), C.addressof(buf), C.addressof(buf), nbytes, None)
            assert lib.gpsa_elbo_loss_fwd(*a, None, 0, 1.0, *out) == want
            assert lib.gpsa_elbo_loss_fused_fwd(*a, ptrs, 1, None, 0, 1.0, *out) == want
            assert lib.gpsa_elbo_loss_weighted_fwd(*a, S, ptrs, ptrs, None, 0, 1.0, *out) == want


def test_library_is_stamped_with_its_sources():
    """the library carries the sha256 of the sources it was built from; load() refuses another one"""
    lib = _lib.load()
    stamp = lib.gpsa_source_hash().decode()
    assert stamp == "GPSA_SOURCE_HASH=" + _lib.source_hash()
    assert _lib.library_hash() == _lib.source_hash()


def test_kernel_resources():
    """what the register allocator did, read from the code objects inside the built library (tools/kernel_meta.py; no
    GPU needed).  Round 4 found the hard way that an ``extern template`` declaration without __launch_bounds__ builds
    every instantiation for 1024 threads: 128 registers, the accumulators in scratch, kernels 4.7x slower - and
    numerically fine, so no parity test notices."""
    import os
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from kernel_meta import demangle, library_kernels

    from spatial_alignment_amd import _lib

    ks = library_kernels(_lib.LIB_PATH)
    names = demangle([k["name"] for k in ks])
    by = dict(zip(names, ks))
    assert len(by) > 150
    families = ("panel_mfma_kernel<", "panel_elbo_kernel<", "quad_sym_mfma_kernel<", "gram_mfma_kernel<", "big_quad_kernel<",
                "big_accum_kernel<", "gram_big_kernel_t<", "prod_big_kernel(", "whiten_mfma_kernel<", "omega_fwd_dma_kernel(",
                "omega_bwd_dma_kernel(")
    seen = {f: 0 for f in families}
    for nm, k in by.items():
        for f in families:
            if f in nm:
                seen[f] += 1
                assert k["max_wg"] == 256, (nm, k)  # the launch bounds reached the instantiation
    assert all(seen.values()), seen
    # the headline step's three contraction kernels own the whole register file (one wave per SIMD) and spill next to
    # nothing: accumulators in scratch would show as kilobytes here
    heads = 0
    for nm, k in by.items():
        if "panel_elbo_kernel<13, 2, 2" in nm or "gram_mfma_kernel<13, true, 2>" in nm or "panel_mfma_kernel<13, 3, 0, 2>" in nm:
            assert k["vgpr"] > 256 and k["scratch"] <= 512, (nm, k)  # (more than 256: one wave per SIMD, by design)
        # the headline launch (M = 200: every row tile but the last inside the matrix): NO scratch at all since round 5
        # (the alpha slab's loads are branch-free on wave-uniform row bases; round 4: 300 bytes, a memory round trip in
        # front of a third of the slab's loads), a handful of VGPR spills into the other register file, and the SGPR
        # spills (to VGPR lanes, outside the K loop) bounded
        if "panel_elbo_kernel<13, 2, 2, true, true>" in nm or "panel_elbo_kernel<13, 2, 4, true, true>" in nm:
            heads += 1
            assert k["scratch"] == 0 and k["vgpr_spill"] <= 16 and k["sgpr_spill"] <= 400, (nm, k)
        if "gram_mfma_kernel<13, true, 2>" in nm:
            assert k["scratch"] == 0 and k["sgpr_spill"] == 0 and k["vgpr_spill"] == 0, (nm, k)
    assert heads == 2  # RL 2 / 4, one barrier per two chunks


# every workspace / size query of csrc/quadform.hip: name -> (argument axes, trailing constant arguments)
_WS_QUERIES = {
    "gpsa_quadform_workspace/f32": ("gpsa_quadform_workspace", "MCL", (0,), ()),
    "gpsa_quadform_workspace/f64": ("gpsa_quadform_workspace", "MCL", (1,), ()),
    "gpsa_quadform_keep_f32_workspace": ("gpsa_quadform_keep_f32_workspace", "ML", (), ()),
    "gpsa_quadform_keep_f32_bytes": ("gpsa_quadform_keep_f32_bytes", "MCL", (), ()),
    "gpsa_quadform_elbo_f32_workspace": ("gpsa_quadform_elbo_f32_workspace", "MCL", (), ()),
    "gpsa_quadform_elbo_x3_f32_workspace": ("gpsa_quadform_elbo_x3_f32_workspace", "MCL", (), ()),
    "gpsa_quadform_bwd_omega_x3_workspace": ("gpsa_quadform_bwd_omega_x3_workspace", "MCL", (), ()),
    "gpsa_gram_batched_workspace/batch1": ("gpsa_gram_batched_workspace", "MCL", (), (1,)),
    "gpsa_gram_batched_workspace/batch3": ("gpsa_gram_batched_workspace", "MCL", (), (3,)),
    "gpsa_quadform_elbo_takes_delta": ("gpsa_quadform_elbo_takes_delta", "M", (), ()),
    "gpsa_quadform_bwd_omega_takes_delta": ("gpsa_quadform_bwd_omega_takes_delta", "MC", (), ()),
}
_WS_AXES = {"M": [1, 5, 16, 17, 100, 193, 200, 201, 208, 256, 257, 300, 500, 512, 513, 1000],
            "C": [1, 67, 260, 12500, 100000], "L": [1, 2, 50]}


def _workspace_table(lib):
    """{query: its values over the product of its axes (M outermost)}; the queries are pure host functions"""
    import itertools

    table = {}
    for key, (fn, axes, head, tail) in _WS_QUERIES.items():
        f = getattr(lib, fn)
        table[key] = [int(f(*head, *args, *tail)) for args in itertools.product(*[_WS_AXES[a] for a in axes])]
    return table


def test_quadform_workspace_queries_match_the_recorded_table():
    """tests/golden/quadform_workspaces.json holds what every workspace / size query of csrc/quadform.hip returned at
    the commit named in it, on a device with ``cus`` compute units (the slab terms scale with that count): the
    layouts behind the queries may be restated, the numbers may not move.  Off a device the library assumes 256 CUs."""
    import json

    import pytest

    lib = _lib.load()
    with open(os.path.join(ROOT, "tests", "golden", "quadform_workspaces.json")) as f:
        rec = json.load(f)
    assert rec["axes"] == _WS_AXES and sorted(rec["values"]) == sorted(_WS_QUERIES)
    cus = lib.gpsa_quadform_elbo_parts() // 2
    if cus != rec["cus"]:
        pytest.skip(f"recorded on {rec['cus']} compute units, this device has {cus}")
    got = _workspace_table(lib)
    for key, want in rec["values"].items():
        bad = [i for i, (a, b) in enumerate(zip(got[key], want)) if a != b]
        assert len(got[key]) == len(want) and not bad, (key, bad[:5], [got[key][i] for i in bad[:5]], [want[i] for i in bad[:5]])


# ---- the per-view loss entries' argument checks (host only: every refusal returns before a stream is touched) --------
_VIEW_N = 12  # rows of every term below
# what is wrong with a term -> (n_views, its row offsets); None: the views are good and the fault is elsewhere
_BAD_VIEWS = {"off[0] != 0": (3, [1, 4, 8, 12]), "off[V] != N": (3, [0, 4, 8, 11]), "decreasing": (3, [0, 8, 4, 12]),
              "V = 0": (0, [0]), "V = 65": (65, list(range(65)) + [12]), "null weight row": None,
              "null counts row": None, "fused term with two views": (2, [0, 5, 12])}
# the return code of every case at a77545a (read off that commit's checks: views_ok / skip_views_ok, the `!w[i]` and
# `!nobs[i]` tests and the fused term's `n_views[i] != 1`, all GPSA_EINVAL): the shared check must give the same
_VIEW_CODES = {kind: -1 for kind in _BAD_VIEWS}


def _per_view_call(lib, family, direction, kind, second):
    """one call of gpsa_elbo_loss_{weighted,skip}_{fwd,bwd} whose last term is wrong in the way ``kind`` names (with
    ``second`` a good term stands in front of it); device pointers are the dummy address 8, never dereferenced"""
    import ctypes as C

    n = 2 if second else 1
    bad = n - 1
    good_off = (C.c_longlong * 4)(0, 4, 8, _VIEW_N)
    nv, offs = [3] * n, [good_off] * n
    if _BAD_VIEWS[kind] is not None:
        nv[bad] = _BAD_VIEWS[kind][0]
        offs[bad] = (C.c_longlong * len(_BAD_VIEWS[kind][1]))(*_BAD_VIEWS[kind][1])
    ptr = lambda null_at=None: (C.c_void_p * n)(*[None if i == null_at else 8 for i in range(n)])
    terms = (n, ptr(), ptr(), ptr(), (C.c_int * n)(*[2] * n), (C.c_longlong * n)(*[_VIEW_N] * n), (C.c_int * n)(*[3] * n))
    views = ((C.c_int * n)(*nv), (C.c_void_p * n)(*[C.addressof(o) for o in offs]),
             ptr(bad if kind == "null weight row" else None))
    if family == "skip":
        zpart = (C.c_void_p * n)(*[8 if (kind == "fused term with two views" and i == bad) else None for i in range(n)])
        views = (zpart, 4) + views + (ptr(bad if kind == "null counts row" else None),)
    ws = (C.c_void_p(8), 8 * 4100 * n, None)
    if direction == "fwd":
        tail = (C.c_void_p(8), 3, 1.0, C.c_void_p(8), C.c_void_p(8)) + ws
    else:
        tail = (C.c_void_p(8), 3, 1.0, ptr(), ptr(), C.c_void_p(8), 4, C.c_void_p(8)) + ws
    return getattr(lib, f"gpsa_elbo_loss_{family}_{direction}")(*terms, *views, *tail)


def _per_view_cases(family):
    return [k for k in _BAD_VIEWS if family == "skip" or k not in ("null counts row", "fused term with two views")]


def test_per_view_entries_share_one_check():
    """the weighted and the skip entries refuse every malformed view table, a missing weight row, a missing counts row
    and a fused term with views of its own with the code they returned before they shared the check"""
    lib = _lib.load()
    for family in ("weighted", "skip"):
        for kind in _per_view_cases(family):
            for direction in ("fwd", "bwd"):
                assert _per_view_call(lib, family, direction, kind, second=False) == _VIEW_CODES[kind], (family, kind,
                                                                                                          direction)


def test_bad_second_term_is_refused_before_any_launch():
    """the same with a good term in front of the bad one: the refusal is the check's own code, so it came back before the
    first term's launch (off a device a launch would have answered with the runtime's error, on one it would have
    written through the dummy pointers)"""
    lib = _lib.load()
    for family in ("weighted", "skip"):
        for kind in _per_view_cases(family):
            for direction in ("fwd", "bwd"):
                assert _per_view_call(lib, family, direction, kind, second=True) == _lib.GPSA_EINVAL, (family, kind,
                                                                                                        direction)

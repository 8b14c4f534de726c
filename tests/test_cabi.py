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

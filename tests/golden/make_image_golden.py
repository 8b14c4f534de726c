"""Generate tests/golden/reference_image.npz by RUNNING THE REFERENCE's process_image (build container only).

The function is read out of the unmodified experiments/expression/visium/visium_multimodal_alignment.py at generation
time (``ast``, by name: the script itself reads data files at import and cannot be imported) and executed against a
stand-in for the AnnData object, a ``types.SimpleNamespace`` with ``uns`` / ``obsm`` dicts, with ``GRAY_PIXEL_VAL = 0.7``
as the script sets it.  Three seeded fp32 images (tests/image_util.tissue_image) of at most 24 x 31 x 3: gray borders of
exactly 0.7, the ties 0.65 / 0.75, a spot on a pixel centre so that the strict bounding box bites, and one image where
nothing survives.  Stored: the inputs and ``img_spatial`` / ``img_pixels`` - arrays only, no reference source travels.

    python tests/golden/make_image_golden.py <path of the reference checkout>
"""
import ast
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from image_util import tissue_image  # noqa: E402

SCRIPT = "experiments/expression/visium/visium_multimodal_alignment.py"


def reference_process_image(root):
    src = open(os.path.join(root, SCRIPT)).read()
    node = next(n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == "process_image")
    ns = {"np": np, "GRAY_PIXEL_VAL": 0.7}
    exec(compile(ast.Module(body=[node], type_ignores=[]), SCRIPT, "exec"), ns)
    return ns["process_image"]


def cases():
    rng = np.random.default_rng(20240607)
    a = tissue_image(24, 31, 3, seed=1)
    spots_a = np.array([[4.0, 3.0], [26.0, 20.0], [11.3, 9.9], [20.5, 14.2]])  # corners ON pixel centres: strict
    b = tissue_image(17, 23, 3, seed=2, border=3)
    spots_b = np.array([[2.5, 1.5], [19.75, 15.25], [7.0, 7.0]]) + rng.random((3, 2)) * 0.1
    c = tissue_image(9, 12, 3, seed=3)  # the spots' box is one pixel wide between two centres: nothing survives
    spots_c = np.array([[5.0, 2.0], [6.0, 7.0]])
    return [(a, spots_a), (b, spots_b), (c, spots_c)]


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    root = sys.argv[1]
    process_image = reference_process_image(root)
    out = {}
    for k, (img, spots) in enumerate(cases()):
        adata = types.SimpleNamespace(
            uns={"spatial": {"lib": {"images": {"hires": img.copy()}, "scalefactors": {"tissue_hires_scalef": 1.0}}}},
            obsm={"spatial": spots.copy()})
        adata = process_image(adata)
        out[f"img_{k}"], out[f"spots_{k}"] = img, spots
        out[f"img_spatial_{k}"] = np.asarray(adata.uns["img_spatial"], np.float64).reshape(-1, 2)
        out[f"img_pixels_{k}"] = np.asarray(adata.uns["img_pixels"], np.float32).reshape(-1, img.shape[2])
        print(f"case {k}: image {img.shape}, kept {out[f'img_spatial_{k}'].shape[0]} of {img.shape[0] * img.shape[1]}")
    out["n_cases"] = np.array(len(cases()))
    path = os.path.join(HERE, "reference_image.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

"""Generate tests/golden/pose_refine.npz by running the REFERENCE's compute_loss_and_warp_image.

    python tests/golden/make_pose_refine_golden.py     # needs the reference checkout (COPENERF_REFERENCE)

utils_poses/pose_refinement.py cannot be imported where the fixtures are made (it imports the `model`
package and tqdm), so compute_loss_and_warp_image is parsed out of its source text and compiled
unmodified, as make_golden.py loads Trainer.warp_pixel from train.py; both files are pinned by their
sha256.  The function runs in float64 on 3 frames of 9 x 13 with non-identity poses, in both directions
of perform_pose_refinement (pose_refinement.py:121-123).  The fixture holds numbers only: the inputs, the
two losses, the two warped batches and the gradient of the batch loss with respect to the relative poses.
"""
from __future__ import annotations

import ast
import hashlib
import os
import sys

import numpy as np
import torch

REF = os.environ.get("COPENERF_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(OUT), os.path.dirname(os.path.dirname(OUT))]  # tests/ and the repository root

PINNED = {
    "utils_poses/pose_refinement.py": "cacf014eee42abe51e0d7cf3d137a5762d9bc796174d76a0d0f304be2b150ac6",
    "train.py": "145aa03d8103d27fd00ba9e6255fa03b1d78313da3a88b671373e162acc16ab6",
}


def _ref_text(rel):
    with open(os.path.join(REF, rel), "rb") as f:
        raw = f.read()
    got = hashlib.sha256(raw).hexdigest()
    if got != PINNED[rel]:
        raise SystemExit(f"{rel}: sha256 {got} differs from the pinned snapshot; nothing was run")
    return raw.decode()


def load_reference_functions():
    tree = ast.parse(_ref_text("utils_poses/pose_refinement.py"))
    fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "compute_loss_and_warp_image")
    cls = next(n for n in ast.parse(_ref_text("train.py")).body if isinstance(n, ast.ClassDef) and n.name == "Trainer")
    warp = next(f for f in cls.body if isinstance(f, ast.FunctionDef) and f.name == "warp_pixel")
    ns = {"torch": torch, "np": np}
    exec(compile(ast.fix_missing_locations(ast.Module(body=[fn, warp], type_ignores=[])), REF, "exec"), ns)
    warp_fn = lambda src_frame, uv, normalize_pix=True: ns["warp_pixel"](None, src_frame, uv, normalize_pix)  # noqa: E731
    return ns["compute_loss_and_warp_image"], warp_fn


def main():
    import pose_refine_ref as R
    loss_fn, warp_fn = load_reference_functions()
    H, W, N = 9, 13, 3
    c = R.recipe(H, W, N, seed=3)
    images, depth, K = c["images"], c["depth"], c["K"]
    rel = R.stacked_poses(c["r"], c["t"], range(N - 1)).clone().requires_grad_(True)
    B = N - 1
    uv_batch = R.uv_grid(H, W)[None].repeat(B, 1, 1, 1)
    Kb = K[None].repeat(B, 1, 1)
    pos, warped_pos = loss_fn(images[:-1], images[1:], depth[:-1, None], Kb, uv_batch, rel, warp_fn)
    neg, warped_neg = loss_fn(images[1:], images[:-1], depth[1:, None], Kb, uv_batch, torch.inverse(rel), warp_fn)
    loss = (pos + neg) / 2
    (g,) = torch.autograd.grad(loss, rel)
    out = dict(images=images, depth=depth, K=K, rel=rel.detach(), loss_pos=pos.detach(), loss_neg=neg.detach(),
               warped_pos=warped_pos.detach(), warped_neg=warped_neg.detach(), grad_rel=g)
    np.savez_compressed(os.path.join(OUT, "pose_refine.npz"), **{k: v.numpy() for k, v in out.items()})
    print("wrote pose_refine", {k: tuple(v.shape) for k, v in out.items()}, "loss", float(loss.detach()))


if __name__ == "__main__":
    main()

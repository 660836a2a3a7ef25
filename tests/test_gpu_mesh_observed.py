"""The observed-only mesher on the device (cn_mesh_count_observed / cn_mesh_emit_observed) against the numpy
reference tests/tsdf_ref.py::isosurface_observed_ref, compared the way tests/test_gpu_mesh.py compares the plain
mesher: triangles and counts exact, vertices within 2e-6 x the largest |bound| of the reference's float64 positions."""
import numpy as np
import pytest
import torch

import mesh_ref as MR
import tsdf_ref as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
VTX_REL = 2e-6  # test_gpu_mesh.py's bar


@pytest.mark.parametrize("how", ["half", "slab", "random"])
@pytest.mark.parametrize("make", [MR.sphere_soft, MR.two_spheres, MR.torus])
def test_observed_mesher_matches_the_reference(make, how):
    from copenerf import ops
    u = T.punch(make(), how)
    v, t = ops.isosurface(torch.from_numpy(u).to(DEV), 0.0, *BOX, observed=True)
    rv, rt = T.isosurface_observed_ref(u, 0.0, *BOX)
    assert v.dtype == torch.float32 and t.dtype == torch.int32
    assert v.shape == (len(rv), 3) and t.shape == (len(rt), 3), (v.shape, t.shape, rv.shape, rt.shape)
    assert len(rt) > 0
    assert np.array_equal(t.cpu().numpy(), rt)
    got = v.cpu().numpy()
    assert not np.isnan(got).any()
    err = float(np.abs(got.astype(np.float64) - rv).max())
    print(make.__name__, how, "V", len(rv), "T", len(rt), "unreferenced", len(rv) - len(np.unique(rt)), "vertex max error", err)
    assert err <= VTX_REL * 1.0, err


def test_observed_mesher_odd_dims_and_threshold():
    """(5, 7, 11) with asymmetric bounds and a non-zero threshold, a seeded 10 % punched out."""
    from copenerf import ops
    rng = np.random.default_rng(3)
    x, y, z = MR.grid((5, 7, 11), (0, 0, 0), (1, 1, 1))
    u = (np.sin(5.0 * x + 0.3) * np.sin(7.0 * y + 1.1) * np.sin(9.0 * z + 2.0)).astype(np.float32)
    u[rng.random(u.shape) < 0.1] = np.nan
    lo, hi = (-0.7, -1.0, 0.1), (0.9, 0.4, 1.3)
    v, t = ops.isosurface(torch.from_numpy(u).to(DEV), 0.125, lo, hi, observed=True)
    rv, rt = T.isosurface_observed_ref(u, 0.125, lo, hi)
    assert len(rt) > 20 and np.array_equal(t.cpu().numpy(), rt) and v.shape == (len(rv), 3)
    assert float(np.abs(v.cpu().numpy().astype(np.float64) - rv).max()) <= VTX_REL * 1.3


def test_all_nan_gives_an_empty_mesh():
    from copenerf import ops
    v, t = ops.isosurface(torch.full((6, 5, 4), float("nan"), device=DEV), 0.0, *BOX, observed=True)
    assert v.shape == (0, 3) and t.shape == (0, 3) and v.dtype == torch.float32 and t.dtype == torch.int32


@pytest.mark.parametrize("make", [MR.sphere_soft, MR.two_spheres, MR.torus, MR.sphere_tie])
def test_without_nan_the_observed_calls_are_bitwise_the_plain_ones(make):
    from copenerf import ops
    u = torch.from_numpy(make()).to(DEV)
    v, t = ops.isosurface(u, 0.0, *BOX)
    vo, to = ops.isosurface(u, 0.0, *BOX, observed=True)
    assert len(t) > 0 and torch.equal(v, vo) and torch.equal(t, to)
    counts, countso = ops.mesh_count(u, 0.0, *BOX)[2], ops.mesh_count(u, 0.0, *BOX, observed=True)[2]
    assert torch.equal(counts, countso)


def test_emit_observed_writes_nothing_into_buffers_smaller_than_the_counts():
    from copenerf import ops
    u = torch.from_numpy(T.punch(MR.torus(), "random")).to(DEV)
    d, ws, counts = ops.mesh_count(u, 0.0, *BOX, observed=True)
    V, Tn = counts.tolist()
    assert V > 0 and Tn > 0
    with pytest.raises(RuntimeError, match="buffers"):
        ops.mesh_emit(d, ws, torch.empty(V, 3, device=DEV), torch.empty(Tn - 1, 3, dtype=torch.int32, device=DEV), (V, Tn), True)
    for dv, dt in ((1, 0), (0, 1)):
        v = torch.full((V - dv, 3), float("nan"), device=DEV)
        t = torch.full((Tn - dt, 3), -7, dtype=torch.int32, device=DEV)
        ops.mesh_emit(d, ws, v, t, observed=True)  # the kernel's own check against the device counts
        assert bool(torch.isnan(v).all()) and bool((t == -7).all())
    v, t = torch.empty(V, 3, device=DEV), torch.empty(Tn, 3, dtype=torch.int32, device=DEV)
    ops.mesh_emit(d, ws, v, t, (V, Tn), True)
    v2, t2 = ops.isosurface(u, 0.0, *BOX, observed=True)
    assert torch.equal(v, v2) and torch.equal(t, t2)

"""cn_mesh_area / cn_mesh_sample against the float64 restatement (tests/mesh_eval_ref.py): the area to 1e-12
relative; every sample's triangle equal to the float64 searchsorted of u0 area (the seeds keep every sample at
least 1e-9 area away from a cdf entry, asserted on the reference, no sample excluded); every point within 4 fp32
ulp of its triangle's largest corner coordinate of the barycentric expression (a square root, three weights of at
most 1.5 x 2^-24 relative error, three products and two sums: below 3.5 ulp); zero-area triangles never drawn;
bitwise repeatable."""
import numpy as np
import pytest
import torch

from mesh_eval_ref import icosphere, sample_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
ZERO_AT = (0, 4, 256, 700, 1024, 1283)  # a thread's, a wave's and a tile's first triangle among them


def _meshes():
    v, f = icosphere(3)  # 1280 triangles: two scan tiles
    out = {"icosphere": (v, f, [])}
    # zero-area triangles (a repeated corner: exactly 0 in any arithmetic), the last one at the very end
    fz = [list(t) for t in f]
    for k, at in enumerate(ZERO_AT):
        a, b = int(f[k, 0]), int(f[k, 1])
        fz.insert(at, [a, b, b] if k % 2 else [a, a, b])
    fz.append([5, 5, 5])
    fz = np.array(fz, dtype=np.int32)
    out["zero_area"] = (v, fz, [i for i, t in enumerate(fz) if len(set(t.tolist())) < 3])
    # one triangle 10^6 times the area of the others (edges 1000 times as long)
    edge = float(np.linalg.norm(v[f[0, 0]] - v[f[0, 1]]))
    big = np.array([[0, 0, 5], [1000 * edge, 0, 5], [0, 1000 * edge, 5]], dtype=np.float32)
    vb = np.concatenate([v, big])
    fb = np.concatenate([f[:600], [[len(v), len(v) + 1, len(v) + 2]], f[600:]]).astype(np.int32)
    out["one_huge"] = (vb, fb, [])
    return out


MESHES = _meshes()
SEED = {"icosphere": 3, "zero_area": 4, "one_huge": 5}
S = 20000


def _so(seed, offset=0):
    return torch.tensor([seed, offset], dtype=torch.uint64, device=DEV)


def _draw(name, n, seed, offset=0):
    from copenerf import ops
    v, f, _ = MESHES[name]
    handle, area = ops.mesh_area(torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV))
    points, tri = ops.mesh_sample(handle, n, _so(seed, offset), want_tri=True)
    return area.item(), points.cpu().numpy(), tri.cpu().numpy()


@pytest.mark.parametrize("name", list(MESHES))
def test_samples_match_the_float64_sampler(name):
    v, f, zero = MESHES[name]
    ref = sample_ref(v, f, S, SEED[name])
    assert ref["margin"].min() > 1e-9, ref["margin"].min()  # no sample near a cdf entry: the triangle is decided
    area, points, tri = _draw(name, S, SEED[name])
    print(f"{name}: area rel err {abs(area - ref['area']) / ref['area']:.2e}, cdf margin {ref['margin'].min():.2e}")
    assert abs(area - ref["area"]) <= 1e-12 * ref["area"]
    assert np.array_equal(tri, ref["tri"])
    corner = np.abs(v[f[ref["tri"]]]).max(axis=(1, 2))
    err = np.abs(points.astype(np.float64) - ref["points"]).max(1)
    print(f"{name}: max point error {np.max(err / np.spacing(corner)):.2f} ulp of the largest corner coordinate")
    assert np.all(err <= 4 * np.spacing(corner))
    assert not np.isin(tri, zero).any()
    if name == "one_huge":
        assert (tri == 600).mean() > 0.99  # a thousand to one against all the others together
    if name == "icosphere":
        # uniform by area: the octants of the sphere get their share of the samples (8 x 2500 expected, sigma 47)
        counts = np.bincount((points > 0) @ np.array([1, 2, 4]), minlength=8)
        assert np.all(np.abs(counts - S / 8) < 6 * (S * 7 / 64) ** 0.5), counts


def test_same_seed_is_bitwise_repeatable_and_seeds_and_offsets_differ():
    a0, p0, t0 = _draw("zero_area", 5000, 21)
    a1, p1, t1 = _draw("zero_area", 5000, 21)
    assert a0 == a1 and np.array_equal(p0, p1) and np.array_equal(t0, t1)
    _, p2, t2 = _draw("zero_area", 5000, 22)
    assert not np.array_equal(p0, p2) and not np.array_equal(t0, t2)
    _, p3, _ = _draw("zero_area", 5000, 21, offset=1)
    assert not np.array_equal(p0, p3)


@pytest.mark.parametrize("n", [1, 255, 1000])
def test_sample_counts_off_the_block_size(n):
    v, f, _ = MESHES["icosphere"]
    ref = sample_ref(v, f, n, 7)
    assert ref["margin"].min() > 1e-9
    _, points, tri = _draw("icosphere", n, 7)
    assert points.shape == (n, 3) and np.array_equal(tri, ref["tri"])
    corner = np.abs(v[f[ref["tri"]]]).max(axis=(1, 2))
    assert np.all(np.abs(points.astype(np.float64) - ref["points"]).max(1) <= 4 * np.spacing(corner))
    # a longer draw starts with the same samples: sample i depends on (seed, offset, i) alone
    assert np.array_equal(_draw("icosphere", n + 300, 7)[1][:n], points)


def test_area_of_an_empty_and_a_degenerate_mesh():
    from copenerf import ops
    v = torch.from_numpy(MESHES["icosphere"][0]).to(DEV)
    _, area = ops.mesh_area(v, torch.zeros(0, 3, dtype=torch.int32, device=DEV))
    assert area.item() == 0.0
    flat = torch.tensor([[0, 0, 1], [2, 2, 2], [3, 4, 4]], dtype=torch.int32, device=DEV)
    handle, area = ops.mesh_area(v, flat)
    assert area.item() == 0.0
    points, tri = ops.mesh_sample(handle, 10, _so(1), want_tri=True)  # nothing to draw from: zeros and -1
    assert (points == 0).all() and (tri == -1).all()
    bad = torch.tensor([[0, 1, 2], [0, 1, 10 ** 6], [-1, 1, 2]], dtype=torch.int32, device=DEV)  # indices outside [0, V)
    handle, area = ops.mesh_area(v, bad)
    _, tri = ops.mesh_sample(handle, 100, _so(1), want_tri=True)
    assert area.item() > 0 and (tri == 0).all()

"""LPIPS on the host: the weight loader (copenerf.metrics.load_lpips_weights) on files in the two real key
layouts, its refusals, the weight reorder against F.conv2d, and the float64 restatement's own properties
(tests/lpips_ref.py).  No device."""
import pickle

import pytest
import torch
import torch.nn.functional as F

import lpips_ref as R


@pytest.fixture(scope="module")
def weights():
    return R.make_weights(678)


def _save(tmp_path, vgg, lin):
    pv, pl = str(tmp_path / "vgg16.pth"), str(tmp_path / "vgg.pth")
    torch.save(vgg, pv)
    torch.save(lin, pl)
    return pv, pl


def test_loader_round_trips_the_two_key_layouts(tmp_path, weights):
    from copenerf import metrics
    convs, lins = weights
    vgg, lin = R.state_dicts(convs, lins)
    vgg["classifier.0.weight"] = torch.zeros(4, 4)   # entries the metric does not use are ignored
    lin["lin0.model.0.anything"] = torch.zeros(1)
    w = metrics.load_lpips_weights(*_save(tmp_path, vgg, lin))
    assert [len(w[k]) for k in ("conv", "bias", "lin")] == [13, 13, 5]
    cin = 3
    for l, (cw, cb) in enumerate(convs):
        kpad = 32 if l == 0 else 9 * cin
        assert w["conv"][l].shape == (cw.shape[0], kpad) and w["conv"][l].dtype == torch.float32
        # column (dy 3 + dx) Cin + c holds w[:, c, dy, dx]; the padding is zero
        back = w["conv"][l][:, :9 * cin].reshape(-1, 3, 3, cin).permute(0, 3, 1, 2)
        assert torch.equal(back, cw) and not w["conv"][l][:, 9 * cin:].any()
        assert torch.equal(w["bias"][l], cb)
        cin = cw.shape[0]
    for t in range(5):
        assert w["lin"][t].shape == (R.TAP_CHANNELS[t],) and torch.equal(w["lin"][t], lins[t])


def test_loader_refusals(tmp_path, weights):
    from copenerf import metrics
    convs, lins = weights
    vgg, lin = R.state_dicts(convs, lins)
    missing = dict(vgg)
    del missing["features.17.bias"]
    with pytest.raises(KeyError, match=r"features\.17\.bias"):
        metrics.load_lpips_weights(*_save(tmp_path, missing, lin))
    wrong = dict(vgg)
    wrong["features.5.weight"] = torch.zeros(128, 64, 3, 2)
    with pytest.raises(ValueError, match=r"features\.5\.weight.*\(128, 64, 3, 2\)"):
        metrics.load_lpips_weights(*_save(tmp_path, wrong, lin))
    flat = dict(lin)
    flat["lin3.model.1.weight"] = torch.zeros(512)        # not [1, C, 1, 1]
    with pytest.raises(ValueError, match=r"lin3\.model\.1\.weight"):
        metrics.load_lpips_weights(*_save(tmp_path, vgg, flat))
    nolin = dict(lin)
    del nolin["lin4.model.1.weight"]
    with pytest.raises(KeyError, match=r"lin4\.model\.1\.weight"):
        metrics.load_lpips_weights(*_save(tmp_path, vgg, nolin))
    nontensor = dict(vgg)
    nontensor["features.0.weight"] = "not a tensor"
    with pytest.raises(KeyError, match=r"features\.0\.weight"):
        metrics.load_lpips_weights(*_save(tmp_path, nontensor, lin))
    # a pickle that is no weights-only state dict: weights_only=True refuses to build the object
    pv, pl = _save(tmp_path, vgg, lin)
    with open(pv, "wb") as f:
        pickle.dump({"features.0.weight": test_loader_refusals}, f)
    with pytest.raises(ValueError, match="not a weights-only state dict"):
        metrics.load_lpips_weights(pv, pl)
    torch.save([1, 2, 3], pv)
    with pytest.raises(ValueError, match="not a state dict"):
        metrics.load_lpips_weights(pv, pl)


def test_reordered_weights_times_patches_is_conv2d():
    """On a 5 x 7 map: the gathered operand rows times the reordered matrix is F.conv2d (float64: the two
    differ by the summation order only)."""
    from copenerf import metrics
    g = torch.Generator().manual_seed(3)
    cin, cout, H, W = 4, 6, 5, 7
    x = torch.randn(2, cin, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64)
    want = F.conv2d(x, w, padding=1)
    Wm = metrics.lpips_conv_matrix(w, kpad=64)
    assert Wm.shape == (cout, 64) and not Wm[:, 9 * cin:].any()
    rows = R.patches(x.permute(0, 2, 3, 1).contiguous(), 0, H, 64)
    got = (rows @ Wm.t()).reshape(2, H, W, cout).permute(0, 3, 1, 2)
    assert (got - want).abs().max() < 1e-13
    # a band equals the same rows of the whole
    band = R.patches(x.permute(0, 2, 3, 1).contiguous(), 1, 3, 64).reshape(2, 3, W, 64)
    assert torch.equal(band, rows.reshape(2, H, W, 64)[:, 1:4])


def test_restatement_identical_images_give_zero(weights):
    convs, lins = weights
    a, _ = R.pair_inputs((3, 16, 19))
    assert torch.equal(R.lpips_layers(a, a.clone(), convs, lins), torch.zeros(1, 5, dtype=torch.float64))
    b = R.pair_inputs((3, 16, 19))[1]
    v = R.lpips_layers(a, b, convs, lins)
    assert v.shape == (1, 5) and (v > 0).all() and torch.equal(R.lpips(a, b, convs, lins), v.sum(1))


@pytest.mark.parametrize("H,W", [(37, 53), (16, 16), (17, 31)])
def test_restatement_pools_with_floor(H, W, weights):
    """Every tap has the floor-halved size, equals the stack rebuilt with explicit F.max_pool2d calls, and a
    ceil-mode pool gives other sizes wherever a side is odd."""
    convs, _ = weights
    small = [(w[:8, :(3 if l == 0 else 8)], b[:8]) for l, (w, b) in enumerate(convs)]   # 8 channels: the sizes matter
    x = R.pair_inputs((2, 3, H, W))[0]
    taps = R.features(x, small)
    h, w = H, W
    for t, f in enumerate(taps):
        assert f.shape == (2, 8, h, w), (t, f.shape)
        h, w = h // 2, w // 2
    f64 = lambda v: torch.tensor(v, dtype=torch.float64).view(1, 3, 1, 1)  # noqa: E731
    y = (x.double() - f64(R.MEAN)) / f64(R.STD)
    blocks, l = (2, 2, 3, 3, 3), 0
    for t, n in enumerate(blocks):
        if t:
            y = F.max_pool2d(y, kernel_size=2, stride=2)
            assert y.shape[-2:] == (taps[t - 1].shape[-2] // 2, taps[t - 1].shape[-1] // 2)
        for _ in range(n):
            y = F.relu(F.conv2d(y, small[l][0].double(), small[l][1].double(), padding=1))
            l += 1
        assert torch.equal(y, taps[t])
    if H % 2 or W % 2:
        assert R.features(x, small, ceil_mode=True)[1].shape != taps[1].shape

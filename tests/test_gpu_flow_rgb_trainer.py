"""SyntheticTrainer(flow_rgb="fused"): the training step with the fused flow-RGB pass (motion.flow_rgb_fused)
against the CPU oracle at the bars of tests/test_gpu_stage1.py, its graph replay against eager steps as
tests/test_gpu_configs.py checks the default's, and the default ("torch") unchanged."""
import pytest
import torch

import test_gpu_stage1 as S

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture
def fused_trainer(monkeypatch):
    """test_gpu_stage1's trainers with the fused term; counts the calls of motion.flow_rgb_fused."""
    from copenerf import train_step
    make, fused, calls = S._trainer, train_step.flow_rgb_fused, []

    def _trainer(*a, **kw):
        tr = make(*a, **kw)
        tr.flow_rgb = "fused"
        return tr

    def flow_rgb_fused(*a, **kw):
        calls.append(1)
        return fused(*a, **kw)

    monkeypatch.setattr(S, "_trainer", _trainer)
    monkeypatch.setattr(train_step, "flow_rgb_fused", flow_rgb_fused)
    return calls


@pytest.mark.parametrize("scenario,image,mode,rays", [("stage1", 2, "bf16x6", 128), ("stage1", 6, "bf16x6", 128),
                                                      ("stage1", 7, "bf16x6", 128), ("hybrid", 4, "fp32", 128)])
def test_training_step_with_the_fused_term_matches_oracle(fused_trainer, scenario, image, mode, rays):
    errs = S._step_errors(scenario, image, mode, rays)
    assert len(fused_trainer) == 1  # the step went through cn_flow_rgb_fwd
    l_bar, f_bar, pm_bar = S.BARS[mode]
    print({k: float(f"{v:.3g}") for k, v in errs.items()})
    assert errs["loss"] <= l_bar + errs["_loss_abs_slack"], errs["loss"]
    for k, e in errs.items():
        if k not in ("loss", "_loss_abs_slack"):
            assert e <= (pm_bar if k.startswith(("pose", "motion")) else f_bar), (k, e)


@pytest.mark.filterwarnings("error:The AccumulateGrad node's stream")
def test_c5_graph_stage1_joint_pose_replays_with_the_fused_term():
    """test_c5_graph_stage1_joint_pose_replays of tests/test_gpu_configs.py with flow_rgb="fused": the captured
    launch reads the frame indices on the device, so six replays follow six eager steps bit for bit, the last
    frame (no valid reference frame) included."""
    from copenerf.train_step import GraphedTrainer, SyntheticTrainer
    kw = dict(rays=256, H=48, W=64, capturable=True, schedule="reference", start_it=30000, mfma_dtype="bf16x6",
              n_images=6, joint_pose=True, stage1=True, flow_rgb="fused")
    a = SyntheticTrainer(DEV, **kw)
    b = SyntheticTrainer(DEV, **kw)
    g = GraphedTrainer(b, warmup=1)
    for _ in range(2):
        a.step()
    frames = set()
    for _ in range(6):  # every frame, incl. the world camera and the last one
        frames.add(a.image_index(a.it + 1))
        la = a.step().detach().clone()
        lb = g.step().detach().clone()
        torch.cuda.synchronize()
        assert torch.equal(la, lb), (la.item(), lb.item())
    assert frames == set(range(6))
    for pa, pb in zip(a.all_params, b.all_params):
        assert torch.equal(pa, pb)


def test_default_is_the_torch_term_and_unchanged():
    """flow_rgb="torch" is the default and gives the bits of a trainer built without the argument; the fused
    term gives another (close) loss, with and without the fused stage-1 pass, and the mode may change between
    steps."""
    from copenerf.train_step import SyntheticTrainer
    kw = dict(rays=128, H=48, W=64, schedule="reference", start_it=30000, mfma_dtype="bf16x6", n_images=6, stage1=True)
    plain = SyntheticTrainer(DEV, **kw)
    torch_ = SyntheticTrainer(DEV, flow_rgb="torch", **kw)
    fused = SyntheticTrainer(DEV, flow_rgb="fused", **kw)
    unfused_s1 = SyntheticTrainer(DEV, flow_rgb="fused", stage1_fused=False, **kw)
    assert plain.flow_rgb == "torch" and fused.flow_rgb == "fused"
    for _ in range(2):
        lp, lt, lf, lu = (tr.step().detach() for tr in (plain, torch_, fused, unfused_s1))
        assert torch.equal(lp, lt)
    for x in (lf, lu):
        assert abs(float(x) - float(lp)) <= 1e-3 * abs(float(lp))
    for pa, pb in zip(plain.all_params, torch_.all_params):
        assert torch.equal(pa, pb)
    torch_.flow_rgb = "fused"
    assert torch.isfinite(torch_.step()).item()
    torch_.flow_rgb = "eager"
    with pytest.raises(ValueError, match="flow_rgb"):
        torch_.step()

"""The parts the fused trainers share (rl_ctr_prediction_amd/step_trainer.py) that need no GPU:
the flat dense buffer and its inverse on host tensors, the re-exports trainer.py keeps, and
which class owns which method."""
import pytest
import torch


def _afm():
    from rl_ctr_prediction_amd import AFM
    from rl_ctr_prediction_amd.afm_trainer import AFM_DENSE
    torch.manual_seed(0)
    return AFM(10, 3, 4), AFM_DENSE


def _deepfm():
    from rl_ctr_prediction_amd import DeepFM
    from rl_ctr_prediction_amd.trainer import DEEPFM_DENSE
    torch.manual_seed(1)
    return DeepFM(11, 3, 4), DEEPFM_DENSE


@pytest.mark.parametrize("build", [_afm, _deepfm], ids=["AFM", "DeepFM"])
@pytest.mark.parametrize("tail", [0, 4])
def test_pack_dense_repoints_without_changing_the_model(build, tail):
    from rl_ctr_prediction_amd.step_trainer import pack_dense, split_dense
    model, names = build()
    params = dict(model.named_parameters())
    before = {k: v.clone() for k, v in model.state_dict().items()}
    ids = {n: id(p) for n, p in params.items()}
    flat, flat_grad, offsets, views, grad_views = pack_dense(params, names, torch.device("cpu"),
                                                             grad_tail=tail)
    assert list(offsets) == list(names) and all(o % 4 == 0 for o in offsets.values())
    assert flat.numel() % 4 == 0 and flat.numel() >= sum(params[n].numel() for n in names)
    # the same Parameter objects with the same values, and the same state_dict
    after = dict(model.named_parameters())
    assert {n: id(p) for n, p in after.items()} == ids
    sd = model.state_dict()
    assert list(sd) == list(before)
    for k in before:
        assert torch.equal(sd[k], before[k]), k
    # consecutive, non-overlapping, and views of the flat buffers
    end = 0
    for n in names:
        p, off, k = after[n], offsets[n], after[n].numel()
        assert off >= end and off - end < 4
        end = off + k
        assert views[n].shape == p.shape == grad_views[n].shape
        assert p.data.data_ptr() == views[n].data_ptr() == flat[off:].data_ptr()
        assert grad_views[n].data_ptr() == flat_grad[off:].data_ptr()
        views[n].fill_(off + 1.0)  # writing a view shows in flat, and in the parameter
        assert bool((flat[off:off + k] == off + 1.0).all()) and bool((p.data == off + 1.0).all())
        grad_views[n].fill_(-off - 1.0)
        assert bool((flat_grad[off:off + k] == -off - 1.0).all())
    # the gradient has the parameters' length, with `tail` floats of storage behind it
    assert flat_grad.numel() == flat.numel() and flat_grad.storage_offset() == 0
    assert flat_grad.untyped_storage().nbytes() == 4 * (flat.numel() + tail)
    assert flat.untyped_storage().nbytes() == 4 * flat.numel()
    # the inverse, on the buffer itself and on another of its layout
    back = split_dense(flat, names, offsets, views)
    assert list(back) == list(names)
    other = torch.arange(flat.numel(), dtype=torch.float32)
    split = split_dense(other, names, offsets, views)
    for n in names:
        assert back[n].data_ptr() == views[n].data_ptr() and torch.equal(back[n], views[n])
        k = views[n].numel()
        assert split[n].shape == views[n].shape
        assert torch.equal(split[n].reshape(-1), other[offsets[n]:offsets[n] + k])


def test_trainer_module_keeps_the_moved_helpers():
    from rl_ctr_prediction_amd import step_trainer, trainer
    for name in ("graph_capture", "live_pool", "flush_hooks"):
        assert getattr(trainer, name) is getattr(step_trainer, name), name


def test_every_fused_trainer_is_a_step_trainer():
    from rl_ctr_prediction_amd.afm_trainer import FusedAFMTrainer
    from rl_ctr_prediction_amd.ffm_trainer import FusedFFMTrainer
    from rl_ctr_prediction_amd.sharded import ShardedCTRTrainer
    from rl_ctr_prediction_amd.step_trainer import StepTrainer
    from rl_ctr_prediction_amd.trainer import FusedCTRTrainer
    for cls in (FusedCTRTrainer, ShardedCTRTrainer, FusedFFMTrainer, FusedAFMTrainer):
        assert issubclass(cls, StepTrainer), cls.__name__
    shared = ("step", "_step", "_graph_step", "_after_step", "reset_optimizer",
              "optimizer_state_dict", "flush", "_flush_table", "_flush_due", "__del__",
              "check_errors", "reset_loss_sum", "read_loss_sum", "_sync_step_table",
              "_replay_or_capture", "_drain_tail")
    for cls in (FusedFFMTrainer, FusedAFMTrainer):
        own = [n for n in shared if n in cls.__dict__]
        assert not own, f"{cls.__name__} defines {own} itself"
        for n in ("__init__", "_tables", "_moments", "_buffers", "_launch"):
            assert n in cls.__dict__, f"{cls.__name__} lacks {n}"
    # the big trainer keeps its own step (slots, lookahead), not the bookkeeping
    for n in ("step", "_step", "_graph_step", "_after_step", "_drain_tail"):
        assert n in FusedCTRTrainer.__dict__, n
    for n in ("reset_optimizer", "flush", "_flush_table", "__del__", "check_errors",
              "_sync_step_table", "_replay_or_capture", "optimizer_state_dict"):
        assert n not in FusedCTRTrainer.__dict__, n
    for n in ("_sync_step_table", "_replay_or_capture", "flush", "reset_optimizer", "__del__"):
        assert n not in ShardedCTRTrainer.__dict__, n


def test_refusals_come_before_the_model_is_touched():
    """A host model is refused with each class's own message, its parameters not re-pointed."""
    from rl_ctr_prediction_amd import AFM, FFM, FM, FusedAFMTrainer, FusedCTRTrainer, FusedFFMTrainer
    for cls, model in ((FusedCTRTrainer, FM(10, 4)), (FusedFFMTrainer, FFM(10, 3, 4)),
                       (FusedAFMTrainer, AFM(10, 3, 4))):
        ptrs = [p.data_ptr() for p in model.parameters()]
        with pytest.raises(RuntimeError, match=f"^{cls.__name__} needs the model on a ROCm device$"):
            cls(model)
        assert [p.data_ptr() for p in model.parameters()] == ptrs
        assert not model._forward_pre_hooks and not model._load_state_dict_pre_hooks
    with pytest.raises(TypeError, match="FusedFFMTrainer drives FFM"):
        FusedFFMTrainer(FM(10, 4))

"""Host side of the capturable fused sparse optimizers (no GPU): constructor and set_lr validation, the state_dict
layout (unchanged for capturable=False) and the checkpoint round trip of a capturable Adam on CPU tensors."""
import pytest
import torch

from torecsys_amd.optim import FusedSparseAdagrad, FusedSparseAdam, FusedSparseSGD

ALL = [FusedSparseSGD, FusedSparseAdagrad, FusedSparseAdam]


@pytest.mark.parametrize("cls", ALL)
def test_constructor_and_set_lr_validation(cls):
    assert cls(0.1).capturable is False
    assert cls(0.1, capturable=True).capturable is True
    with pytest.raises(TypeError):
        cls(0.1, capturable=1)
    with pytest.raises(ValueError):
        cls(-0.1, capturable=True)
    for capturable in (False, True):
        opt = cls(0.1, capturable=capturable)
        opt.set_lr(0.25)
        assert opt.lr == 0.25
        opt.set_lr(0)
        assert opt.lr == 0.0
        with pytest.raises(ValueError):
            opt.set_lr(-1e-3)
        with pytest.raises(ValueError):
            opt.set_lr(float("nan"))
        with pytest.raises(TypeError):
            opt.set_lr("0.1")
        with pytest.raises(TypeError):
            opt.set_lr(None)
        assert opt.lr == 0.0          # a refused value changes nothing
    with pytest.raises(RuntimeError):
        cls(0.1).lr_tensor("cpu")
    with pytest.raises(ValueError):
        FusedSparseAdam(0.1, betas=(1.0, 0.9), capturable=True)


def test_set_lr_writes_the_device_scalar():
    opt = FusedSparseSGD(0.5, capturable=True)
    t = opt.lr_tensor("cpu")
    assert t.dtype == torch.float32 and t.shape == (1,) and float(t) == 0.5
    opt.set_lr(0.125)
    assert opt.lr_tensor("cpu") is t and float(t) == 0.125


def test_by_value_state_dict_layout_is_unchanged():
    """capturable=False: exactly the keys (and values) the optimizers reported before the keyword existed"""
    p = torch.nn.Parameter(torch.zeros(5, 4))
    sgd = FusedSparseSGD(0.1)
    assert sgd.state_dict() == {"hyper": {"lr": 0.1, "eps": 0.0}, "tables": {}}
    ada = FusedSparseAdagrad(0.1, eps=1e-9, initial_accumulator_value=0.5)
    ada.state_for(p.data, p)
    sd = ada.state_dict([("w", p)])
    assert sd["hyper"] == {"lr": 0.1, "eps": 1e-9, "initial": 0.5}
    assert list(sd["tables"]) == ["w"] and sorted(sd["tables"]["w"]) == ["step", "sum"]
    assert sd["tables"]["w"]["step"] == 0 and torch.equal(sd["tables"]["w"]["sum"], torch.full((5, 4), 0.5))
    adam = FusedSparseAdam(0.01, betas=(0.8, 0.9), eps=1e-7)
    adam.state_for(p.data, p)
    assert adam.next_step_size(p.data, p) == pytest.approx(0.01 * (1 - 0.9) ** 0.5 / (1 - 0.8))
    sd = adam.state_dict([("w", p)])
    assert sd["hyper"] == {"lr": 0.01, "eps": 1e-7, "beta1": 0.8, "beta2": 0.9}
    assert sorted(sd["tables"]["w"]) == ["exp_avg", "exp_avg_sq", "step"]
    assert sd["tables"]["w"]["step"] == 1 and type(sd["tables"]["w"]["step"]) is int
    # and a capturable optimizer reports the same keys: checkpoints move between the two modes
    sd_c = FusedSparseAdam(0.01, betas=(0.8, 0.9), eps=1e-7, capturable=True).state_dict()
    assert sd_c["hyper"] == sd["hyper"]


def test_capturable_adam_checkpoint_round_trip():
    p = torch.nn.Parameter(torch.zeros(6, 3))
    a = FusedSparseAdam(0.02, betas=(0.85, 0.95), capturable=True)
    m1, m2 = a.state_for(p.data, p)
    m1.copy_(torch.arange(18.0).view(6, 3))
    m2.fill_(0.25)
    step, step_size = a.step_tensors(p.data, p)
    assert step.dtype == torch.int64 and step.shape == (1,) and int(step) == 0
    assert step_size.dtype == torch.float32 and step_size.shape == (1,)
    step.fill_(7)                              # what seven backward passes leave in the device counter
    with pytest.raises(RuntimeError):
        a.next_step_size(p.data, p)            # a capturable Adam has no host-side step
    a.set_lr(0.004)
    sd = a.state_dict([("emb.weight", p)])
    entry = sd["tables"]["emb.weight"]
    assert entry["step"] == 7 and type(entry["step"]) is int
    assert sorted(entry) == ["exp_avg", "exp_avg_sq", "step"]
    assert sd["hyper"]["lr"] == 0.004

    q = torch.nn.Parameter(torch.zeros(6, 3))
    b = FusedSparseAdam(0.5, capturable=True)
    lr_before = b.lr_tensor("cpu")
    b.load_state_dict(sd, [("emb.weight", q)])
    assert (b.lr, b.beta1, b.beta2) == (0.004, 0.85, 0.95)
    assert float(lr_before) == pytest.approx(0.004)          # the device scalar follows the loaded learning rate
    assert b.state_dict([("emb.weight", q)])["tables"]["emb.weight"]["step"] == 7      # before the first step ...
    n1, n2 = b.state_for(q.data, q)
    assert torch.equal(n1, m1) and torch.equal(n2, m2)
    assert int(b.step_tensors(q.data, q)[0]) == 7                                      # ... and in the device counter
    assert b.state_dict([("emb.weight", q)])["tables"]["emb.weight"]["step"] == 7

    # the same checkpoint restores a by-value Adam, whose host counter continues from it
    c = FusedSparseAdam(0.5)
    c.load_state_dict(sd, [("emb.weight", q)])
    c.next_step_size(q.data, q)
    assert c.state_dict([("emb.weight", q)])["tables"]["emb.weight"]["step"] == 8
    with pytest.raises(KeyError):
        b.load_state_dict(sd, [("other", q)])

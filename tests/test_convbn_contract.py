"""Host-side contract of the conv+BN level ops (vae2.ops): the marker protocol
(LazyBN / PartBN: publish, put_partials, take_partials, claim), the res_bns validation
of conv_bn_multi and the by-name mapping of the per-layer autograd inputs.  No device
work: every check is reached before any library call (the autograd functions are stubbed
where a first, legitimate hand-over has to get past them)."""
import pytest
import torch
from torch import nn

from vae2 import ops


def _x(c=8):
    return torch.zeros(1, 4, 4, c)


def _unit(cin=8, cout=8, k=1):
    return nn.Conv2d(cin, cout, k, 1, k // 2, bias=False), nn.BatchNorm2d(cout)


@pytest.fixture
def no_device(monkeypatch):
    """conv_bn_multi / fuse_sum_relu with their autograd functions stubbed out."""
    class Multi:
        @staticmethod
        def apply(specs, *flat):
            return tuple(flat[::len(flat) // len(specs)])

    class Fuse:
        @staticmethod
        def apply(out_hw, links, lazies, *terms):
            return terms[0]

    monkeypatch.setattr(ops, "_ConvBNMulti", Multi)
    monkeypatch.setattr(ops, "_FuseSum", Fuse)


def test_partbn_two_conv_bn_multi_consumers_raise(no_device):
    conv, bn = _unit()
    pb = ops.PartBN()
    ops.conv_bn_multi([_x()], [conv], [bn], True, bn_ins=[pb])
    with pytest.raises(RuntimeError, match="one consumer per marked BatchNorm output"):
        ops.conv_bn_multi([_x()], [conv], [bn], True, bn_ins=[pb])


def test_partbn_conv_bn_then_conv_bn_multi_raises(no_device):
    conv, bn = _unit()
    pb = ops.PartBN()
    ops.conv_bn(_x(), conv, bn, True, bn_part=pb)
    with pytest.raises(RuntimeError, match="one consumer per marked BatchNorm output"):
        ops.conv_bn_multi([_x(), _x()], [conv, conv], [bn, bn], True, bn_ins=[None, pb])


def test_lazybn_bn_ins_then_fuse_sum_raises(no_device):
    conv, bn = _unit()
    lz = ops.LazyBN()
    ops.conv_bn_multi([_x()], [conv], [bn], True, bn_ins=[lz])
    with pytest.raises(RuntimeError, match="one consumer per marked BatchNorm output"):
        ops.fuse_sum_relu([_x(), _x()], (4, 4), lazies=[None, lz])


def test_second_claim_raises_before_any_device_work():
    """No stub: on CPU tensors a device call could only fail otherwise (ValueError)."""
    conv, bn = _unit()
    pb, lz = ops.PartBN(), ops.LazyBN()
    pb.claim()
    lz.claim()
    with pytest.raises(RuntimeError, match="one consumer"):
        ops.conv_bn_multi([_x()], [conv], [bn], True, bn_ins=[pb])
    with pytest.raises(RuntimeError, match="one consumer"):
        ops.conv_bn(_x(), conv, bn, True, bn_part=pb)
    with pytest.raises(RuntimeError, match="one consumer"):
        ops.fuse_sum_relu([_x(), _x()], (4, 4), lazies=[None, lz])


@pytest.mark.parametrize("base", ["LazyBN", "PartBN"])
def test_marker_subclass_and_partials_round_trip(base):
    made = []

    class Counting(getattr(ops, base)):
        __slots__ = ()

        def __init__(self):
            super().__init__()
            made.append(self)

    m = Counting()
    assert made == [m]
    assert (m.save, m.relu, m.part, m.rows) == (None, False, None, 0)
    assert not hasattr(m, "__dict__")
    save, r, part = torch.zeros(32), _x(), torch.zeros(16)
    m.put_partials(part, 3)  # stale: a publish starts a new hand-off
    m.publish(save, True, r=r) if base == "PartBN" else m.publish(save, True)
    assert m.save is save and m.relu is True and m.part is None and m.rows == 0
    if base == "PartBN":
        assert m.r is r
    m.put_partials(part, 5)
    assert m.part is part and m.rows == 5
    got, rows = m.take_partials()
    assert got is part and rows == 5
    assert m.part is None and m.take_partials()[0] is None  # taken once
    assert m.rows == 5  # the hand-off's row count stays readable (tests count armed markers)


def test_res_bns_value_errors(no_device):
    conv, bn = _unit()
    xs = [_x(), _x()]
    msg = "res_bns: the shortcut layer must be a plain conv \\+ BN"
    with pytest.raises(ValueError, match=msg):  # the shortcut layer has a ReLU
        ops.conv_bn_multi(xs, [conv, conv], [bn, bn], [True, True], res_bns=[1, None])
    with pytest.raises(ValueError, match=msg):  # the layer has a residual of its own
        ops.conv_bn_multi(xs, [conv, conv], [bn, bn], [True, False], residuals=[_x(), None],
                          res_bns=[1, None])
    with pytest.raises(ValueError, match=msg):  # the shortcut's output is marked
        ops.conv_bn_multi(xs, [conv, conv], [bn, bn], [True, False],
                          bn_outs=[None, ops.LazyBN()], res_bns=[1, None])
    wide, bn_w = _unit(8, 12)
    with pytest.raises(ValueError) as e:
        ops.conv_bn_multi(xs, [conv, wide], [bn, bn_w], [True, False], res_bns=[1, None])
    assert str(e.value) == "res_bns: shortcut output (1, 4, 4, 12) != layer output (1, 4, 4, 8)"


def test_res_bns_accepts_a_plain_shortcut(no_device):
    conv, bn = _unit()
    x0, x1 = _x(), _x()
    outs = ops.conv_bn_multi([x0, x1], [conv, conv], [bn, bn], [True, False], res_bns=[1, None])
    assert outs[0] is x0 and outs[1] is x1


NAMES = ("x", "weight", "bias", "gamma", "beta", "residual")


@pytest.mark.parametrize("n", [1, 3])
def test_layer_inputs_map_by_name(n):
    assert ops._In._fields == NAMES
    # needs_input_grad of _ConvBNMulti.apply(specs, *flat): specs first, then 6 per layer
    need = ("specs",) + tuple(f"{k}{i}" for i in range(n) for k in NAMES)
    for i in range(n):
        got = ops._layer_needs(need, i)
        for k in NAMES:
            assert getattr(got, k) == f"{k}{i}"
    # gradients given by name come back at their input's position (None for specs)
    per_layer = [ops._In(**{k: f"d{k}{i}" for k in reversed(NAMES)}) for i in range(n)]
    grads = ops._level_grads(per_layer)
    assert grads == (None,) + tuple(f"d{k}{i}" for i in range(n) for k in NAMES)
    assert len(grads) == len(need)


@pytest.mark.parametrize("n", [1, 3])
def test_layer_records_from_flat_inputs(n, monkeypatch):
    """The flat argument list conv_bn_multi builds lands on the records' fields by name."""
    captured = {}

    class Multi:
        @staticmethod
        def apply(specs, *flat):
            captured["flat"] = flat
            return tuple(flat[::len(NAMES)])

    monkeypatch.setattr(ops, "_ConvBNMulti", Multi)
    monkeypatch.setattr(ops, "_bn_quad_ok", lambda t: True)  # (reads a device pointer)
    units = [_unit() for _ in range(n)]
    xs, res = [_x() for _ in range(n)], [_x() for _ in range(n)]
    ops.conv_bn_multi(xs, [u[0] for u in units], [u[1] for u in units], True, residuals=res)
    flat = captured["flat"]
    assert len(flat) == len(NAMES) * n
    ins = list(map(ops._In._make, zip(*[iter(flat)] * len(NAMES))))
    for i, (conv, bn) in enumerate(units):
        L = ops._Layer(ops.ConvSpec(conv, bn, True), ins[i])
        assert L.x is xs[i] and L.weight is conv.weight and L.bias is conv.bias
        assert L.gamma is bn.weight and L.beta is bn.bias and L.residual is res[i]
        assert L.has_res

"""vae2_ema_coeffs / vae2_ema_update_dev / vae2_ema_update and ema_decay / swap_ema() of
vae2.optim.FusedAdam and FusedSGD.

One update, with w = float32(1 - float64(decay)) and ref = e + w*(p - e) evaluated in fp64 from
the fp32 inputs: the kernel rounds p - e once and the fused multiply-add once, which gives
2^-24 * (|p - e| + |ref|).  The bound used is

    |got - ref| <= 2^-23 * (|p - e| + |ref|)

(a factor of 2 left; an unfused multiply-add also stays inside it).  The first update is a
bit copy of p.

K updates against torch.optim.swa_utils.AveragedModel + get_ema_multi_avg_fn(decay) in fp64 on
the CPU: with M the per-element maximum |p_k| over the sequence every |ema| <= M and
|p - ema| <= 2M, so one update adds at most 3 * 2^-23 * M; the recurrence contracts
(factor decay <= 1), so the errors at most add up:

    |got - ref| <= K * 2^-21 * M."""
import ctypes
import functools

import pytest
import torch

from helpers import build, make_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda"

# scalar-only, exact quads, quad + tail; the last is the smallest size at which the
# grid-stride loop of the 16-byte body takes a second trip and a tail is left
SIZES = [1, 2, 3, 4, 5, 7, 1023, 1025, 4 * 256 * 4096 + 5]
DECAYS = [0.0, 0.5, 0.999]
GUARD = 8  # sentinel floats around every device buffer: nothing outside [0, n) is written


def _weight(decay):
    """The kernels' weight: 1 - decay in double, rounded to fp32 once."""
    return float(torch.tensor(1.0 - float(torch.tensor(decay, dtype=torch.float32)),
                              dtype=torch.float64).float())


@functools.lru_cache(maxsize=None)
def _inputs(n):
    """(p, e): normal fp32 numbers of mixed magnitude."""
    g = torch.Generator().manual_seed(2000 + n % 997)
    scales = torch.tensor([1e-3, 1.0, 1e3])

    def one():
        return torch.randn(n, generator=g) * scales[torch.randint(0, 3, (n,), generator=g)]
    return one(), one()


def _dev_buf(src, offset):
    n = src.numel()
    raw = torch.full((offset + n + GUARD,), 777.0, device=DEV)
    view = raw[offset:offset + n]
    view.copy_(src)
    return raw, view


def _guards_ok(raw, offset, n):
    return bool((raw[:offset] == 777.0).all()) and bool((raw[offset + n:] == 777.0).all())


def _run(e0, ps, decay, count0=0, offset=0, host_scalar=False):
    """One update of ema (starting as e0) per vector of ps, through the C ABI, with the device
    counter starting at count0; returns ema on the CPU."""
    from vae2 import ops
    from vae2._lib import call
    n = e0.numel()
    eraw, e = _dev_buf(e0, offset)
    praw, p = _dev_buf(ps[0], offset)
    state = torch.tensor([float(count0), 0.0], dtype=torch.float64, device=DEV)
    coeffs = torch.zeros(4, device=DEV)
    s = ops.stream_ptr()
    for k, pk in enumerate(ps):
        p.copy_(pk)
        if host_scalar:
            call("vae2_ema_update", ops.ptr(e), ops.ptr(p), n, decay, int(count0 + k == 0), s)
        else:
            call("vae2_ema_coeffs", ops.ptr(state), decay, ops.ptr(coeffs), s)
            call("vae2_ema_update_dev", ops.ptr(e), ops.ptr(p), n, ops.ptr(coeffs), s)
    torch.cuda.synchronize()
    assert _guards_ok(eraw, offset, n) and _guards_ok(praw, offset, n)
    assert torch.equal(p.cpu().view(torch.int32), ps[-1].view(torch.int32))  # p is read only
    if not host_scalar:
        assert float(state[0]) == count0 + len(ps)
        assert float(coeffs[0]) == _weight(decay)
        assert float(coeffs[1]) == (1.0 if count0 + len(ps) == 1 else 0.0)
    return e.cpu()


@pytest.mark.parametrize("decay", DECAYS)
@pytest.mark.parametrize("n", SIZES)
def test_ema_update_matches_fp64(n, decay):
    p, e = _inputs(n)
    got = _run(e, [p], decay, count0=1)  # not the first update
    w = _weight(decay)
    p64, e64 = p.double(), e.double()
    ref = e64 + w * (p64 - e64)
    err = (got.double() - ref).abs()
    bound = 2.0 ** -23 * ((p64 - e64).abs() + ref.abs())
    print(f"n={n} decay={decay}: max err/bound = {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())


@pytest.mark.parametrize("decay", DECAYS)
@pytest.mark.parametrize("n", SIZES)
def test_first_update_is_a_bit_copy_and_does_not_read_ema(n, decay):
    p, _ = _inputs(n)
    got = _run(torch.full((n,), float("nan")), [p], decay, count0=0)
    assert torch.equal(got.view(torch.int32), p.view(torch.int32))


@pytest.mark.parametrize("offset", [0, 1])
def test_first_update_copies_any_bit_pattern(offset):
    """Signalling and quiet NaNs with payloads, infinities, subnormals and -0 arrive bit for
    bit, through the 16-byte body (n = 11: two quads and a tail) and the scalar path."""
    bits = torch.tensor([0x7FA00001, 0x7FC12345, -0x00400001, 0x7F800000, -0x00800000,
                         0x00000001, -0x7FFFFFFF, -0x80000000, 0x007FFFFF, 0x3F800000,
                         0x7F7FFFFF], dtype=torch.int32)
    got = _run(torch.zeros(bits.numel()), [bits.view(torch.float32)], 0.5, offset=offset)
    assert torch.equal(got.view(torch.int32), bits)


def _sequence(n, k, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g) for _ in range(k)]


def test_misaligned_pointers_take_the_scalar_path_with_the_same_bits():
    """ema and p one float into their allocations; guards on both sides are checked by _run."""
    n = 1025
    ps = _sequence(n, 3)
    e0 = torch.full((n,), float("nan"))
    aligned = _run(e0, ps, 0.9)
    assert bool(torch.isfinite(aligned).all())
    assert torch.equal(_run(e0, ps, 0.9, offset=1), aligned)


def test_host_scalar_form_same_bits():
    n = 1025
    ps = _sequence(n, 3)
    e0 = torch.full((n,), float("nan"))
    dev = _run(e0, ps, 0.9)
    assert torch.equal(_run(e0, ps, 0.9, host_scalar=True), dev)
    assert torch.equal(_run(e0, ps, 0.9, host_scalar=True, offset=1), dev)


def _averaged_model(ps, decay):
    """torch's EMA of the sequence, in fp64 on the CPU."""
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn

    class M(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros_like(ps[0], dtype=torch.float64))
    m = M()
    avg = AveragedModel(m, multi_avg_fn=get_ema_multi_avg_fn(decay))
    for pk in ps:
        with torch.no_grad():
            m.p.copy_(pk.double())
        avg.update_parameters(m)
    return avg.module.p.detach()


def _check_trajectory(what, got, ps, decay):
    ref = _averaged_model(ps, decay)
    big = torch.stack([pk.double().abs() for pk in ps]).max(dim=0).values
    err = (got.double().cpu() - ref).abs()
    bound = len(ps) * 2.0 ** -21 * big
    print(f"{what}: max err = {float(err.max()):.3e}, max err/bound = "
          f"{float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all()), what


@pytest.mark.parametrize("decay", [0.5, 0.999])
def test_trajectory_matches_averaged_model(decay):
    K, n = 20, 1025
    ps = _sequence(n, K, seed=6)
    # torch takes 1 - decay in double; the kernels round it to fp32: |w - (1 - d)| <= 2^-25, a
    # term of at most 2^-25 * 2M per update, far inside the factor left by the bound
    got = _run(torch.full((n,), float("nan")), ps, decay)
    _check_trajectory(f"decay={decay}", got, ps, decay)


# ------------------------------------------------------- FusedAdam / FusedSGD ----

KINDS = ["adam", "sgd"]


def _make_opt(kind, nets, sgd_lr=1e-2, **kw):
    from vae2.optim import FusedAdam, FusedSGD
    if kind == "adam":
        return FusedAdam(nets, lr=1e-3, **kw)
    return FusedSGD(nets, lr=sgd_lr, momentum=0.9, weight_decay=1e-4, **kw)


def _fill_grads(opt, seed):
    g = torch.Generator().manual_seed(seed)
    for f in opt.flats:
        f.grad.copy_(torch.randn(f.numel, generator=g))


def _tiny_opt(kind, **kw):
    ed, ez = build(make_cfg("tiny"), seed=0)
    ed.to(DEV), ez.to(DEV)
    return _make_opt(kind, [ez, ed], **kw)


def _logged_step(opt):
    """opt.step() and the names of the kernels it launched."""
    from vae2 import _lib
    lib = _lib.load()
    lib.vae2_kernel_log(1)
    try:
        opt.step()
        buf = ctypes.create_string_buffer(1 << 14)
        lib.vae2_kernel_log_read(buf, len(buf))
    finally:
        lib.vae2_kernel_log(0)
    return buf.value.decode().split(";")


@pytest.mark.parametrize("kind", KINDS)
def test_optimizer_ema_off_and_on(kind):
    off, on = _tiny_opt(kind, ema_decay=None), _tiny_opt(kind, ema_decay=0.9)
    assert off.ema is None and len(on.ema) == len(on.flats) == 2
    snaps = []
    for k in range(3):
        _fill_grads(off, 30 + k)
        _fill_grads(on, 30 + k)
        names_off, names_on = _logged_step(off), _logged_step(on)
        assert not [nm for nm in names_off if "ema_" in nm], names_off
        ema_names = [nm for nm in names_on if "ema_" in nm]
        assert sorted(ema_names) == ["ema_coeffs_kernel"] + ["ema_update_kernel"] * len(on.flats)
        # exactly the launches without it, with the average between the last parameter update
        # and the re-pack
        last = max(i for i, nm in enumerate(names_off) if "adam" in nm or "sgd" in nm)
        assert last < len(names_off) - 1  # the re-pack follows
        assert names_on == names_off[:last + 1] + ["ema_coeffs_kernel"] + \
            ["ema_update_kernel"] * len(on.flats) + names_off[last + 1:]
        snaps.append([f.data.cpu().clone() for f in on.flats])
    torch.cuda.synchronize()
    for fo, fn in zip(off.flats, on.flats):
        assert torch.equal(fo.data, fn.data)  # the average never feeds back
    assert on.ema_updates == 3 and off.ema_updates == 0
    for j, e in enumerate(on.ema):
        assert e.data_ptr() != on.flats[j].data.data_ptr()
        _check_trajectory(f"{kind} ema[{j}]", e, [s[j] for s in snaps], 0.9)
    # configuration, not state
    assert "ema_decay" not in on.param_groups[0]
    assert set(on.state_dict()) == set(off.state_dict()) == {"state", "param_groups"}
    assert set(on.state_dict()["param_groups"][0]) == set(off.state_dict()["param_groups"][0])


@pytest.mark.parametrize("kind", KINDS)
def test_ema_updates_setter_and_first_update_on_device(kind):
    opt = _tiny_opt(kind, ema_decay=0.5)
    opt.ema_updates = 7  # as after a resume: the next update averages
    for e, f in zip(opt.ema, opt.flats):
        e.copy_(f.data)
    before = [f.data.cpu().clone() for f in opt.flats]
    _fill_grads(opt, 40)
    opt.step()
    assert opt.ema_updates == 8
    for e, f, b in zip(opt.ema, opt.flats, before):
        assert not torch.equal(e, f.data)
        _check_trajectory("resumed", e, [b, f.data.cpu()], 0.5)
    opt.ema_updates = 0  # the next update copies
    _fill_grads(opt, 41)
    opt.step()
    assert opt.ema_updates == 1
    for e, f in zip(opt.ema, opt.flats):
        assert torch.equal(e, f.data)


@pytest.mark.parametrize("kind", KINDS)
def test_first_update_semantics_under_replay(kind):
    """A graph captured before the first update: replay 1 copies, replays 2 and 3 average (the
    device counter decides, not the capture)."""
    from vae2.graph import StepGraph
    a, b = _tiny_opt(kind, ema_decay=0.9), _tiny_opt(kind, ema_decay=0.9)
    for e in a.ema + b.ema:
        e.fill_(float("nan"))  # the first update must not read it
    graph = StepGraph(b.step, warmup=0)
    assert b.ema_updates == 0 and b.step_count == 0  # the capture itself ran nothing
    for k in range(3):
        _fill_grads(a, 50 + k)
        _fill_grads(b, 50 + k)
        a.step()
        graph.replay()
    torch.cuda.synchronize()
    assert a.ema_updates == b.ema_updates == 3
    for fa, fb, ea, eb in zip(a.flats, b.flats, a.ema, b.ema):
        assert torch.equal(fa.data, fb.data)
        assert bool(torch.isfinite(ea).all()) and not torch.equal(ea, fa.data)
        assert torch.equal(ea, eb)


def _setup(kind, ema_decay=0.9, arch="tiny", B=2, hw=(32, 64), seed=0, sgd_lr=1e-2):
    from vae2.model import FullModel_encdec
    ed, ez = build(make_cfg(arch, hw=hw), seed=seed)
    fm = FullModel_encdec(ez, ed, None, None, None, None, None, 1.0, 0.1, 1.0, 0.0).to(DEV)
    fm.train()
    fm.defer_checks = True
    opt = _make_opt(kind, [fm.encz_model, fm.encdec_model], sgd_lr=sgd_lr, ema_decay=ema_decay)
    g = torch.Generator().manual_seed(7)
    xs = [torch.randn(B, 9, *hw, generator=g).to(DEV) for _ in range(3)]
    eps = torch.randn(B, ez.z_dim, 1, 1, generator=g).to(DEV)
    code = torch.randn(B, ez.z_dim, 1, 1, generator=g).to(DEV)

    def step():
        opt.zero_grad()
        fm.set_noise(eps, code)
        loss = fm(*xs, 1.0)[0][0]
        loss.backward()
        opt.step()
        return loss

    def evaluate():
        """(loss, x2t_hat) of an eval-mode forward on the fixed inputs."""
        was = fm.training
        fm.eval()
        try:
            with torch.no_grad():
                fm.set_noise(eps, code)
                out = fm(*xs, 1.0)
            torch.cuda.synchronize()
            return out[0][0].clone(), out[2].clone()
        finally:
            fm.train(was)
    return fm, opt, step, evaluate


@pytest.mark.parametrize("kind", KINDS)
def test_whole_step_graph_replay_matches_eager_with_ema(kind):
    from vae2.graph import StepGraph
    fa, oa, step_a, _ = _setup(kind)
    fb, ob, step_b, _ = _setup(kind)
    losses_a = [float(step_a()) for _ in range(5)]
    g = StepGraph(step_b, warmup=2)  # executes 2 eager steps, captures the 3rd
    losses_b = [float(g.replay()) for _ in range(3)]
    torch.cuda.synchronize()
    assert losses_a[2:] == losses_b, (losses_a, losses_b)
    assert len(set(losses_a)) == 5, losses_a
    for fa_, fb_, ea, eb in zip(oa.flats, ob.flats, oa.ema, ob.ema):
        assert torch.equal(fa_.data, fb_.data)
        assert torch.equal(ea, eb) and not torch.equal(ea, fa_.data)
    assert oa.ema_updates == ob.ema_updates == 5
    assert oa.step_count == ob.step_count == 5


@pytest.mark.parametrize("kind", KINDS)
def test_swap_ema_runs_the_model_with_the_average_and_restores(kind):
    # (plain SGD at 1e-2 leaves this model's eval-mode outputs non-finite after three steps,
    # and NaN compares unequal to itself: a small rate keeps the comparison meaningful)
    fm, opt, step, evaluate = _setup(kind, ema_decay=0.5, sgd_lr=1e-6)
    with pytest.raises(RuntimeError, match="ema_updates"):
        with opt.swap_ema():
            pass
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    params0 = [f.data.clone() for f in opt.flats]
    ema0 = [e.clone() for e in opt.ema]
    ptrs0 = [p.data_ptr() for p in fm.parameters()]
    bufs0 = {k: v.clone() for k, v in fm.named_buffers()}
    loss0, x0 = evaluate()
    assert bool(torch.isfinite(x0).all()) and bool(torch.isfinite(loss0).all())

    # a twin whose parameters are the average (and whose buffers are the live ones)
    ft, ot, _, evaluate_t = _setup(kind, ema_decay=None)
    ft.load_state_dict(fm.state_dict())
    with torch.no_grad():
        for f, e in zip(ot.flats, ema0):
            f.data.copy_(e)
    for plan in ot.packs:
        plan.bump_versions()
    loss_t, x_t = evaluate_t()
    assert bool(torch.isfinite(x_t).all()) and bool(torch.isfinite(loss_t).all())
    assert not torch.equal(x_t, x0)  # the average is another model

    with opt.swap_ema() as inside:
        assert inside is opt
        for f, e, p0, e0 in zip(opt.flats, opt.ema, params0, ema0):
            assert torch.equal(f.data, e0) and torch.equal(e, p0)
        assert [p.data_ptr() for p in fm.parameters()] == ptrs0  # contents moved, not views
        loss_s, x_s = evaluate()  # stale packed weights would give x0 here
        assert torch.equal(x_s, x_t) and torch.equal(loss_s, loss_t)
        sd = {k: v.clone() for k, v in fm.state_dict().items()}
    assert any(k.endswith("running_mean") for k in bufs0)
    for k, v in fm.named_buffers():  # BatchNorm statistics are not averaged
        assert torch.equal(v, bufs0[k]), k
        assert k not in sd or torch.equal(sd[k], bufs0[k]), k

    def restored():
        for f, e, p0, e0 in zip(opt.flats, opt.ema, params0, ema0):
            assert torch.equal(f.data, p0) and torch.equal(e, e0)
        loss1, x1 = evaluate()
        assert torch.equal(x1, x0) and torch.equal(loss1, loss0)
    restored()

    class Boom(Exception):
        pass
    with pytest.raises(Boom):
        with opt.swap_ema():
            raise Boom()
    restored()
    assert opt.ema_updates == 3


def test_swap_ema_refuses_a_capture():
    opt = _tiny_opt("sgd", ema_decay=0.5)
    _fill_grads(opt, 60)
    opt.step()
    torch.cuda.synchronize()
    before = [f.data.clone() for f in opt.flats]
    # refused before anything is read or launched, so the (empty) capture itself stays legal
    x = torch.zeros(4, device=DEV)
    with torch.cuda.graph(torch.cuda.CUDAGraph()):
        x.add_(1.0)
        with pytest.raises(RuntimeError, match="capture"):
            with opt.swap_ema():
                pass
    torch.cuda.synchronize()
    for f, x in zip(opt.flats, before):
        assert torch.equal(f.data, x)

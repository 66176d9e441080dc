"""GPU checks of gradient-norm tracking on the flat gradient buffer: tbx_grad_norms through FlatGrads.norms against torch on the CPU in
float64, at the smallest layouts that can go wrong - a dozen segments of lengths 1, 3, 4, 5, 63, 64, 65, CHUNK-1, CHUNK, CHUNK+1, 2*CHUNK+7
(under 100 k elements), packed (align=1: chunk starts off the 16-byte grid, single-element head and tail) and aligned (align=64: gaps, filled
with a sentinel that must be neither read nor written) -, and one eager training step with track_grad_norm=2.

Tolerances. Yardstick: `seg.double().norm(p)` rounded to float32. All summands are non-negative, so a float64 sum of n squares carries a
relative error of at most n * 2^-53 (~1e-11 here) whatever its order; the only rounding that counts is the final conversion to float32,
once on each side: at most 1 float32 ulp (relative 2^-23) per norm and for the total. coef: the kernel rounds the total (2^-24) and the
quotient (2^-24), so it is within 2 ulp (2^-22) of the float64 evaluation of min(1, max_norm / (total + 1e-6))."""
import math
from importlib import import_module

import pytest
import torch

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -23
SENTINEL = 3.0e38  # in the gaps of the aligned layout: finite, so a gap that is read wrecks a norm and a gap that is scaled changes


@pytest.fixture(scope="module")
def DP(tb):
    return import_module("trafficbots_amd.pl_modules.data_parallel")


@pytest.fixture(scope="module")
def hip(tb):
    h = import_module("trafficbots_amd.hip")
    h.load()
    return h


def _lengths(CH):
    return [1, 3, 4, 5, 63, 64, 65, CH - 1, CH, CH + 1, 2 * CH + 7, 1000]


@pytest.fixture(scope="module")
def values(hip):
    """Per segment, float32 on the CPU, made once and never changed: magnitudes from 1e-20 to 1e18, segment 4 tiny throughout (its squares,
    ~1e-40, are below float32's normal range), segment 8 huge throughout (a float32 sum of its squares overflows)."""
    g = torch.Generator().manual_seed(20)
    out = []
    for i, k in enumerate(_lengths(hip.GRAD_CHUNK)):
        lo, hi = ((-20.0, -19.5) if i == 4 else (17.0, 18.0) if i == 8 else (-20.0, 18.0))
        mag = 10.0 ** (lo + (hi - lo) * torch.rand(k, generator=g, dtype=torch.float64))
        sign = torch.where(torch.rand(k, generator=g) < 0.5, -1.0, 1.0).double()
        out.append((mag * sign).float())
    assert sum(v.numel() for v in out) < 100_000
    assert float((out[4].double() ** 2).max()) < 1.1754944e-38  # every square of segment 4 is subnormal (or zero) in float32
    assert math.isinf(float((out[8] ** 2).sum())) and math.isfinite(float(out[8].double().norm().float()))  # float32 overflows, float64 not
    return out


def _layout(DP, values, align, dev):
    """A FlatGrads over parameters of the segments' sizes; the buffer = sentinel in the gaps, the values in the segments. -> (flat, mask of
    the segments' elements)."""
    ps = [torch.nn.Parameter(torch.zeros(v.numel(), device=dev)) for v in values]
    flat = DP.FlatGrads(ps, align=align)
    mask = torch.zeros(flat.flat.numel(), dtype=torch.bool, device=dev)
    for o, v in zip(flat.offsets, values):
        mask[o:o + v.numel()] = True
    _fill(flat, values)
    if align == 1:
        assert bool(mask.all()) and any((flat.flat.data_ptr() + 4 * o) % 16 for o in flat.offsets)  # misaligned segment starts
    else:
        assert int((~mask).sum()) > 0
    return flat, mask


def _fill(flat, values):
    flat.flat.fill_(SENTINEL)
    for view, v in zip(flat.views, values):
        view.copy_(v)


def _want(values, p):
    """float64 on the CPU: (norms, total) as float64 tensors."""
    norms = torch.stack([v.double().norm(p) for v in values])
    return norms, norms.norm(p)


def _close(got, want64, ulps=1):
    """|got - float32(want64)| <= ulps * 2^-23 * |float32(want64)|, NaN == NaN, inf == inf."""
    got, want = got.detach().cpu().double().reshape(-1), want64.float().double().reshape(-1)
    fin = torch.isfinite(want)
    same_special = torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(got[~fin & ~torch.isnan(want)], want[~fin & ~torch.isnan(want)])
    err = (got[fin] - want[fin]).abs()
    ok = bool((err <= ulps * ULP * want[fin].abs()).all())
    if not (ok and same_special):
        print("worst relative error / 2^-23:", float((err / want[fin].abs().clamp_min(1e-300)).max() / ULP) if fin.any() else None)
    return ok and same_special


def _coef64(total64, max_norm):
    return torch.clamp(max_norm / (total64 + 1e-6), max=1.0)


@pytest.mark.parametrize("align", [1, 64])
@pytest.mark.parametrize("p", [2.0, math.inf])
def test_norms_total_coef_and_scale_against_float64(DP, values, align, p):
    dev = torch.device("cuda:0")
    flat, mask = _layout(DP, values, align, dev)
    before = flat.flat.clone()
    norms64, total64 = _want(values, p)
    # clipping off (None, 0, negative): everything reported, the buffer untouched
    for off in (None, 0.0, -1.0):
        r = flat.norms(p, off)
        assert _close(r.per_param, norms64) and _close(r.total, total64)
        assert int(r.nonfinite) == 0 and float(r.coef) == 1.0 and torch.equal(flat.flat, before)
    assert r.per_param.dtype == r.total.dtype == r.coef.dtype == torch.float32 and r.nonfinite.dtype == torch.int32
    assert r.per_param.shape == (len(values),) and r.total.dim() == r.coef.dim() == r.nonfinite.dim() == 0
    # a max_norm above the total does not bite: coef is exactly 1 and no bit of the buffer moves
    r = flat.norms(p, float(total64) * 4.0)
    assert float(r.coef) == 1.0 and torch.equal(flat.flat, before) and _close(r.per_param, norms64) and _close(r.total, total64)
    # a max_norm below it bites: the norms are those BEFORE the clip, the segments are scaled by the kernel's own coef, the gaps stay
    for max_norm in (5.0, float(total64) * 0.75):
        _fill(flat, values)
        r = flat.norms(p, max_norm)
        assert _close(r.per_param, norms64) and _close(r.total, total64) and int(r.nonfinite) == 0
        assert 0.0 < float(r.coef) < 1.0 and _close(r.coef, _coef64(total64, max_norm), ulps=2)
        assert torch.equal(flat.flat, torch.where(mask, before * r.coef, before))
        assert torch.equal(flat.flat[~mask], before[~mask])


@pytest.mark.parametrize("align", [1, 64])
@pytest.mark.parametrize("p", [2.0, math.inf])
def test_non_finite_elements_are_counted_and_propagate(DP, values, align, p):
    dev = torch.device("cuda:0")
    vals = [v.clone() for v in values]
    vals[2][1] = float("nan")  # a NaN in a 4-element segment (the single-element path), an Inf in the middle of the three-chunk one
    vals[10][vals[10].numel() // 2] = float("-inf")
    flat, mask = _layout(DP, vals, align, dev)
    before = flat.flat.clone()
    norms64, total64 = _want(vals, p)
    assert math.isnan(float(norms64[2])) and math.isinf(float(norms64[10])) and math.isnan(float(total64))
    r = flat.norms(p, None)
    assert int(r.nonfinite) == 2 and _close(r.per_param, norms64) and _close(r.total, total64)
    assert int(torch.isfinite(r.per_param).sum()) == len(vals) - 2
    assert torch.equal(flat.flat.view(torch.int32), before.view(torch.int32))  # (bits: the buffer holds a NaN)
    # with a clip, as clip_grad_norm_(error_if_nonfinite=False): a NaN total is a NaN coefficient, and the gradients become NaN
    r = flat.norms(p, 5.0)
    assert math.isnan(float(r.coef)) and bool(torch.isnan(flat.flat[mask]).all()) and torch.equal(flat.flat[~mask], before[~mask])
    # an Inf alone: total = inf, coef = 0, x * 0 (inf * 0 = NaN), which is what torch's own expression gives
    vals[2][1] = 1.0
    _fill(flat, vals)
    before = flat.flat.clone()
    r = flat.norms(p, 5.0)
    assert int(r.nonfinite) == 1 and math.isinf(float(r.total)) and float(r.coef) == 0.0
    want = torch.where(mask, before * r.coef, before)
    assert torch.allclose(flat.flat, want, rtol=0.0, atol=0.0, equal_nan=True) and int(torch.isnan(flat.flat).sum()) == 1


@pytest.mark.parametrize("p", [2.0, math.inf])
def test_two_calls_are_bit_equal(DP, values, p):
    dev = torch.device("cuda:0")
    flat, _ = _layout(DP, values, 1, dev)
    outs = []
    for _ in range(2):
        _fill(flat, values)
        flat.norm_plan().partial.fill_(float("nan"))  # the workspace's content does not matter
        r = flat.norms(p, 5.0)
        outs.append((r.per_param.clone(), r.total.clone(), r.coef.clone(), r.nonfinite.clone(), flat.flat.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_captured_call_replays_on_refilled_gradients(DP, values):
    """The three launches in one torch.cuda.graph; the buffer is refilled with other gradients and the graph replayed: the eager call's
    results on those gradients, bit for bit (nothing in the call is read by, or comes from, the host at replay)."""
    dev = torch.device("cuda:0")
    flat, _ = _layout(DP, values, 64, dev)
    other = [(-0.5 * v).flip(0).contiguous() for v in values]
    flat.norm_plan()  # (the tables are copied to the device once, outside the capture)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        flat.norms(2.0, 5.0)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    _fill(flat, values)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        r = flat.norms(2.0, 5.0)
    _fill(flat, other)
    graph.replay()
    got = [t.clone() for t in (r.per_param, r.total, r.coef, r.nonfinite, flat.flat)]
    _fill(flat, other)
    e = flat.norms(2.0, 5.0)
    for a, b in zip(got, (e.per_param, e.total, e.coef, e.nonfinite, flat.flat)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    norms64, total64 = _want(other, 2.0)
    assert _close(got[0], norms64) and _close(got[1], total64)


def test_training_step_tracks_every_live_parameter(tb, DP, monkeypatch):
    """One seeded eager step at the data-parallel worker's shape with live = FlatGrads and track_grad_norm=2: one logged key per live
    parameter plus the total, under Lightning's names; per_param = the float64 norms of the gradients as they were between the exchange
    and the clip; total * coef = the 2-norm of the clipped buffer. The first step (no FlatGrads yet: torch's multi-tensor norms) logs the
    same keys.
    Then track_grad_norm=-1: from the same gradients, the step leaves the parameters the parent's statements (vector_norm, mul_ by the
    clamped quotient, optimizer.step) leave, bit for bit - run on a second module and optimizer that hold the first ones' state from before
    the step, and fed the step's own gradients: a second backward is not required to repeat the first bit for bit (the attention
    backward has a scatter form that adds with float atomics), and the statements under test start at the gradients."""
    import copy

    dev = torch.device("cuda:0")
    W = import_module("trafficbots_amd.pl_modules.waymo_motion")
    scfg = tb.config.default_sim_cfg()
    scfg["time_step_end"] = 20
    torch.manual_seed(7)
    wm = W.WaymoMotion(model=tb.config.default_model_cfg(n_tgt_knn=4), data_size=tb.synthetic.DATA_SIZE, **scfg).to(dev).train()
    (opt,), _ = wm.configure_optimizers()
    batch = {k: v.to(dev) for k, v in tb.synthetic.make_scene(2, 8, 64, 8, seed=0).items()}
    step = lambda **kw: DP.train_step(wm, opt, {k: v.clone() for k, v in batch.items()}, **kw)
    logged = {}
    monkeypatch.setattr(wm, "log_dict", lambda d, **kw: logged.update(d))

    step(track_grad_norm="2")  # the first step finds the live parameters
    live = DP.live_parameters(wm.model)
    name_of = {id(q): k for k, q in wm.named_parameters()}
    keys = {f"grad_2.0_norm/{name_of[id(q)]}" for q in live} | {"grad_2.0_norm_total"}
    assert set(logged) == keys and len(keys) == len(live) + 1 and all(k.startswith("grad_2.0_norm/model.") for k in keys - {"grad_2.0_norm_total"})
    first = wm.last_grad_norms
    assert first.per_param.is_cuda and bool(torch.isfinite(first.per_param).all()) and int(first.nonfinite) == 0

    flat = DP.FlatGrads(live, align=64)
    seen = {}
    real = DP.allreduce_gradients

    def keep(params, *a, **k):
        out = real(params, *a, **k)
        seen["grads"] = params.flat.clone()  # after the exchange, before the clip
        return out

    monkeypatch.setattr(DP, "allreduce_gradients", keep)
    logged.clear()
    step(live=flat, track_grad_norm=2)
    r = wm.last_grad_norms
    assert r is not first and set(logged) == keys and len(r.names) == len(live)
    assert logged["grad_2.0_norm_total"].data_ptr() == r.total.data_ptr() and all(v.is_cuda and v.dim() == 0 for v in logged.values())
    g = seen["grads"].cpu()
    norms64 = torch.stack([g[o:o + q.numel()].double().norm() for o, q in zip(flat.offsets, live)])
    assert _close(r.per_param, norms64) and _close(r.total, norms64.norm()) and int(r.nonfinite) == 0
    assert _close(r.coef, _coef64(norms64.norm(), 5.0), ulps=2)
    after64 = float(flat.flat.cpu().double().norm())
    assert abs(float(r.total.double() * r.coef.double()) - after64) <= 2.0 ** -22 * after64
    for i in (0, len(live) // 2, len(live) - 1):
        assert logged[f"grad_2.0_norm/{r.names[i]}"].data_ptr() == r.per_param[i].data_ptr()

    # tracking off: the parent's statements
    wm2 = W.WaymoMotion(model=tb.config.default_model_cfg(n_tgt_knn=4), data_size=tb.synthetic.DATA_SIZE, **scfg).to(dev).train()
    wm2.load_state_dict(wm.state_dict())
    (opt2,), _ = wm2.configure_optimizers()
    opt2.load_state_dict(copy.deepcopy(opt.state_dict()))
    logged.clear()
    wm.last_grad_norms = None
    step(live=flat, track_grad_norm=-1)
    assert not logged and wm.last_grad_norms is None
    twin = dict(wm2.named_parameters())
    buf = seen["grads"].clone()
    for o, q in zip(flat.offsets, live):
        twin[name_of[id(q)]].grad = buf[o:o + q.numel()].view_as(q)
    total = torch.linalg.vector_norm(buf)
    buf.mul_((5.0 / (total + 1e-6)).clamp(max=1.0))
    opt2.step()
    for k, q in wm.named_parameters():
        assert torch.equal(q, twin[k]), k


def test_graphed_step_tracks_between_replay_and_optimizer(tb, DP, monkeypatch):
    """GraphedTrainStep(track_grad_norm="inf"): after the replay and the exchange, one tracking + clipping call on the static flat buffer;
    the logged inf norms are those of the buffer as it was before the clip (float32 maxima: exact), under Lightning's keys."""
    dev = torch.device("cuda:0")
    W = import_module("trafficbots_amd.pl_modules.waymo_motion")
    scfg = tb.config.default_sim_cfg()
    scfg["time_step_end"] = 14
    torch.manual_seed(3)
    wm = W.WaymoMotion(model=tb.config.default_model_cfg(n_tgt_knn=4), data_size=tb.synthetic.DATA_SIZE, **scfg).to(dev).train()
    (opt,), _ = wm.configure_optimizers()
    batch = {k: v.to(dev) for k, v in tb.synthetic.make_scene(2, 8, 64, 8, seed=0).items()}
    gs = DP.GraphedTrainStep(wm, opt, batch, warmup=1, track_grad_norm="inf")
    seen, logged = {}, {}
    monkeypatch.setattr(wm, "log_dict", lambda d, **kw: logged.update(d))
    real = DP.allreduce_gradients
    monkeypatch.setattr(DP, "allreduce_gradients", lambda params, *a, **k: (real(params, *a, **k), seen.__setitem__("grads", params.flat.clone()))[0])
    gs(batch)
    r = wm.last_grad_norms
    name_of = {id(q): k for k, q in wm.named_parameters()}
    keys = {f"grad_inf_norm/{name_of[id(q)]}" for q in gs.live} | {"grad_inf_norm_total"}
    assert set(logged) == keys
    g = seen["grads"]
    want = torch.stack([g[o:o + q.numel()].abs().max() for o, q in zip(gs.flat.offsets, gs.live)])
    assert torch.equal(r.per_param, want) and torch.equal(r.total, want.max()) and int(r.nonfinite) == 0
    assert torch.equal(gs.flat.flat, g * r.coef)  # (the gaps are zero)

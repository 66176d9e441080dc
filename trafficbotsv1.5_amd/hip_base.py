"""ctypes glue shared by the hip_* wrapper modules: return-code check, device-pointer helpers, the current stream, the attention
segment descriptor and the cache of images derived from weights (tbx_pack_weight* images, padded and stacked copies: per weights
version, or per training step inside a PackScope).
There is no CPU path: every helper raises on tensors that are not on a HIP device."""
import ctypes as C
import os
from typing import List, Optional, Sequence

import numpy as np
import torch

from .abi import *  # noqa: F401,F403  (constants, structures, load, declared_symbols: the C-ABI mirror)
from .abi import load  # noqa: F401


def _check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"{what}: tbx error {rc}: {load().tbx_error_string(rc).decode()}")


_HOST_PTRS = False  # hip.knarpe_attn_form only: its descriptor is checked, never dereferenced, so host tensors may stand in


def _ptr(t: Optional[torch.Tensor], dtype=None) -> Optional[int]:
    if t is None:
        return None
    if not t.is_cuda and not _HOST_PTRS:
        raise RuntimeError("tbx kernels need device tensors (HIP); there is no CPU path")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"expected {dtype}, got {t.dtype}")
    return t.data_ptr()


def _cptr(t: Optional[torch.Tensor], dtype=None) -> Optional[int]:
    if t is not None and not t.is_contiguous():
        raise RuntimeError("tbx kernels need contiguous tensors")
    return _ptr(t, dtype)


# ---- keyed dropout: the Python restatement of csrc/drop_key.h (the only one) --------------------------------------------------
def drop_rate(p: float):
    """drop_key.h drop_rate: (thresh, scale) of the float32 p that crosses the C ABI. The drop_thresh / drop_scale fields of the tile
    structs and the row chain's dropout stage are filled from here, so that they draw the library-filled launches' mask."""
    pf = np.float32(p)
    if not pf > 0:
        return 0, 1.0
    th = float(pf) * 4294967296.0
    return (1 if th < 1.0 else int(th)), float(np.float32(1.0) / (np.float32(1.0) - pf))


def drop_stream_key(seed: int, site: int, step: int):
    """drop_key.h stream_key -> (lo, hi)."""
    sd, m32 = seed % (1 << 64), 0xFFFFFFFF
    return ((sd & m32) ^ ((site * 0x85EBCA6B) & m32) ^ ((step * 0x27D4EB2F) & m32),
            ((sd >> 32) + site * 0xC2B2AE35 + step * 0x165667B1) & m32)


def drop_mix(counter, lo: int, hi: int):
    """drop_key.h drop_mix over a numpy array of counters -> uint32 array."""
    x = np.asarray(counter).astype(np.uint32)
    with np.errstate(over="ignore"):
        x = (x ^ np.uint32(lo)) * np.uint32(0x9E3779B1)
        x = x ^ np.uint32(hi)
        x = (x ^ (x >> np.uint32(16))) * np.uint32(0x7FEB352D)
        x = (x ^ (x >> np.uint32(15))) * np.uint32(0x846CA68B)
        return x ^ (x >> np.uint32(16))


ACTION_NOISE_SITE = 0x4143544E  # drop_key.h ACTION_NOISE_SITE ("ACTN"): none of the dropout sites' ids


def action_noise_bits(seed: int, step: int, scene_row):
    """drop_key.h action_noise_bits over a numpy array of scene rows -> (h1, h2) uint32 arrays: the integer part of the action noise
    of (seed, 1-based closed-loop step, row = scene * n_ag + agent of the engine's batch), exact."""
    lo, hi = drop_stream_key(seed, ACTION_NOISE_SITE, step)
    with np.errstate(over="ignore"):
        r = np.asarray(scene_row).astype(np.uint32) * np.uint32(2)
        return drop_mix(r, lo, hi), drop_mix(r + np.uint32(1), lo, hi)


def action_noise(seed: int, step: int, scene_row):
    """drop_key.h action_noise in float64 -> [len(scene_row), 2]: Box-Muller on u1 = (h1 + 1) * 2^-32 in (0, 1], theta = 2 pi h2 * 2^-32.
    What tbx_sim_step logs into out_act_noise agrees with this to 1e-5."""
    h1, h2 = action_noise_bits(seed, step, scene_row)
    r = np.sqrt(-2.0 * np.log((h1.astype(np.float64) + 1.0) * 2.0 ** -32))
    th = 2.0 * np.pi * (h2.astype(np.float64) * 2.0 ** -32)
    return np.stack([r * np.cos(th), r * np.sin(th)], -1)


def _fill_drop(a, drop: dict) -> None:
    """The drop_* fields of a tile struct from drop = dict(p, seed int64[1] device tensor, step, sites = site ids, None: not dropped)."""
    a.drop_thresh, a.drop_scale = drop_rate(drop["p"])
    a.drop_seed, a.drop_step = _ptr(drop["seed"], torch.int64), int(drop["step"])
    for i, st in enumerate(drop["sites"]):
        a.drop_site[i] = -1 if st is None else int(st)


def drop_struct(drop) -> Optional[Drop]:
    """tbx_drop_t of drop = (p, seed int64[1] device tensor or None, site, rows_per_scene, time_batch, time0) - the only place that knows
    the order; None (no dropout) stays None: the library's NULL."""
    if drop is None:
        return None
    p, seed, site, rps, tb, t0 = drop
    return Drop(_ptr(seed, torch.int64), float(p), int(site), int(rps), int(tb), int(t0))


DEFERRED = None  # hip.defer(): the list that collects launch descriptors instead of launching them


def stream_ptr() -> int:
    if DEFERRED is not None:  # a launch that has no deferred form inside a one-queue step would run out of order
        raise RuntimeError("a kernel launch inside hip.defer() that is neither tbx_front nor tbx_knarpe_dec_layer")
    return torch.cuda.current_stream().cuda_stream


class Seg:
    """One target segment of a KNARPE attention call: a K/V table + the KNN set that indexes it."""

    def __init__(self, kv, k_off, v_off, n_tgt, idx, invalid, emb=None, batch_div=1, rel=None):
        """emb [n,S,k,128] (materialised embedding) or rel [n,S,k,3] (relative pose; embedding rebuilt in-kernel)."""
        assert kv.dim() == 2 and kv.stride(1) == 1 and kv.dtype in (torch.float32, torch.bfloat16)
        assert (emb is None) != (rel is None), "exactly one of emb / rel"
        self.kv, self.k_off, self.v_off, self.n_tgt, self.batch_div = kv, k_off, v_off, n_tgt, batch_div
        self.idx, self.invalid, self.emb, self.rel = idx, invalid, emb, rel
        self.k = idx.shape[-1]

    def c(self) -> AttnSeg:
        return AttnSeg(_ptr(self.kv), _cptr(self.idx, torch.int32), _cptr(self.invalid, torch.uint8),
                       _cptr(self.emb, torch.float32), _cptr(self.rel, torch.float32), self.kv.stride(0), self.k_off, self.v_off,
                       self.n_tgt, self.batch_div, self.k, int(self.kv.dtype == torch.bfloat16))


def _attn_args(qbuf, q_off: int, qt_off: int, rpe_k_bias, n_batch: int, n_src: int, segs: Sequence[Seg], freqs, drop) -> Attn:
    """The part of tbx_attn_t every attention entry point reads: query side, segments, freqs = (freqs_xy, freqs_yaw) and
    drop = None, or (p, seed int64[1] device tensor, call id[, time_batch, time0]). The caller adds its outputs / gradients."""
    a = Attn(qbuf=_ptr(qbuf, torch.float32), rpe_k_bias=_ptr(rpe_k_bias, torch.float32), freqs_xy=_cptr(freqs[0]), freqs_yaw=_cptr(freqs[1]),
             ldq=qbuf.stride(0), q_off=q_off, qt_off=qt_off, n_batch=n_batch, n_src=n_src, n_seg=len(segs), time_batch=1)
    for i, s in enumerate(segs[:2]):  # (a third segment is the library's to refuse: n_seg says so)
        a.seg[i] = s.c()
    if drop is not None:
        a.p_drop, a.drop_seed, a.drop_call = float(drop[0]), _ptr(drop[1], torch.int64), int(drop[2])
        if len(drop) > 3:
            a.time_batch, a.time0 = int(drop[3]), int(drop[4])
    return a


def weights_stamp(tensors) -> tuple:
    """(version, data_ptr) of each tensor that is not None: THE freshness rule of images derived from weights (_derived, WaymoMotion's
    rollout engines). An in-place update (optimizer step, load_state_dict) bumps the version; `p.data = ` or `.to()` moves the storage."""
    return tuple([(t._version, t.data_ptr()) for t in tensors if t is not None])


class PackScope:
    """The derived weight images of one training step (open_pack_scope .. close_pack_scope; reopen_pack_scope for its backward): each weight
    is packed ONCE PER STEP into the scope, not into the per-Parameter cache. A captured step (GraphedTrainStep) replays after the optimizer
    has moved the weights: an image cached before the capture would never be re-packed (its launch is not in the graph)."""

    def __init__(self, plans: Optional[dict] = None, plan_key=None):
        self.images = {}  # _derived's entries: key -> (stamp, image)
        self.pinned = {}  # id -> tensor: the sources of images and groups, alive while the scope is (the ids in keys stay unique)
        self.groups = {}  # id(tensor) -> pack_group's requests
        self.plans, self.plan_key = plans, plan_key  # the owner's recorded lists (None: no owner) and this scope's key in them
        self.record = {}  # pack key -> (_place(weight), _place(bias), wt, groups) of this scope's Parameter-sourced mfma32 requests


_PACK_SCOPE: Optional[PackScope] = None  # the open scope: written by open_ / reopen_ / close_pack_scope only


def _place(t: Optional[torch.Tensor]):
    """(base tensor, offset relative to the base's, shape, stride) of a view; (t,) of a tensor that is no view; None for None. A view of
    an nn.Parameter is described by the Parameter, not by its storage: the description survives `p.data = ...` (FlatAdamW re-points the
    weights into one buffer)."""
    if t is None:
        return None
    base = t._base
    if base is None:
        return (t,)
    return base, t.storage_offset() - base.storage_offset(), t.shape, t.stride()


def _at(place):
    """The tensor a _place describes, on its base tensor's CURRENT storage (None for None)."""
    if place is None or len(place) == 1:
        return place if place is None else place[0]
    base, off, shape, stride = place
    with torch.no_grad():
        return base.as_strided(shape, stride, base.storage_offset() + off)


def _name(t: Optional[torch.Tensor]):
    """t's part of a cache key: its _place with the base tensor's id (restated: this runs on every cache hit)."""
    if t is None:
        return None
    base = t._base
    if base is None:
        return id(t)
    return id(base), t.storage_offset() - base.storage_offset(), t.shape, t.stride()


def _derived(key: tuple, sources, make=None, *args):
    """The image `key` (which names `sources`: tensors or None) while weights_stamp(sources) holds, else make(*args)'s, stored - in the
    open scope (the sources pinned) or on the first source's base tensor (dropped with the Parameter). make=None: look up only (None on a
    miss). A hit builds nothing: `make` is a module-level function, not a closure."""
    stamp, scope = weights_stamp(sources), _PACK_SCOPE
    if scope is not None:
        cache = scope.images
    else:
        owner = sources[0]._base
        owner = sources[0] if owner is None else owner
        cache = getattr(owner, "_tbx_derived", None)
        if cache is None:
            cache = owner._tbx_derived = {}
    hit = cache.get(key)
    if hit is not None and hit[0] == stamp:
        return hit[1]
    if make is None:
        return None
    out = make(*args)
    cache[key] = (stamp, out)
    if scope is not None:
        scope.pinned.update((id(t), t) for t in sources if t is not None)
    return out


def padded_weight(w: torch.Tensor, k_pad: int) -> torch.Tensor:
    """w [n, k] zero-padded to k_pad columns; a derived image (_derived: per weights version, or per training step in a PackScope)."""
    if w.shape[1] == k_pad:
        return w
    return _derived(("padded", _name(w), k_pad), (w,), _make_padded, w, k_pad)


@torch.no_grad()
def _make_padded(w, k_pad):
    out = torch.zeros(w.shape[0], k_pad, dtype=torch.float32, device=w.device)
    out[:, :w.shape[1]].copy_(w)
    return out


def _pack_key(w, bias, wt, groups, split, gemv, mfma32) -> tuple:
    return ("pack", _name(w), _name(bias), wt, groups, split, gemv, mfma32)


def packed_weights_mfma32_multi(reqs) -> None:
    """reqs = [(w, bias | None, wt, groups)]: the tbx_pack_weight_mfma32 images of all of them in ONE launch
    (tbx_pack_weight_mfma32_multi), left where packed_weight(.., mfma32=True) looks them up. Requests whose image is current are skipped."""
    from .abi import PackJob

    lib, jobs, made = load(), [], []
    for w, bias, wt, groups in reqs:
        assert w.is_cuda and w.dim() == 2 and w.stride(1) == 1 and w.dtype == torch.float32
        key = _pack_key(w, bias, wt, groups, False, False, True)
        if _derived(key, (w, bias)) is not None:
            continue
        n, k = (w.shape[1], w.shape[0] // groups) if wt else (w.shape[0] // groups, w.shape[1])
        size = lib.tbx_pack_weight_mfma32_size(n, k, groups)
        if size <= 0:
            _check(int(size), "tbx_pack_weight_mfma32_size")
        if bias is not None:
            assert bias.is_cuda and bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == groups * n
        out = torch.empty(size, dtype=torch.float32, device=w.device)
        j = PackJob()
        j.w, j.bias, j.out, j.n, j.k, j.ld, j.groups, j.wt = _ptr(w), _ptr(bias), _ptr(out), n, k, w.stride(0), groups, int(wt)
        jobs.append(j)
        made.append((key, (w, bias), out))
    if not jobs:
        return
    arr = (PackJob * len(jobs))(*jobs)
    _check(lib.tbx_pack_weight_mfma32_multi(arr, len(jobs), stream_ptr()), "tbx_pack_weight_mfma32_multi")
    for key, sources, out in made:
        _derived(key, sources, lambda: out)  # (a miss: this closure is not on the hit path)


def pack_group(tensors, reqs) -> None:
    """Inside a PackScope: the first packed_weight(.., mfma32=True) request for any of `tensors` packs ALL of `reqs` in one launch (the
    folded weights of an attention module: its three LINEARs' images and the W^T images of their input gradients)."""
    if _PACK_SCOPE is None:
        return
    reqs = list(reqs)
    for t in tensors:
        _PACK_SCOPE.groups[id(t)] = reqs
        _PACK_SCOPE.pinned[id(t)] = t


# The image requests of a training step whose sources are nn.Parameters (ready when the step starts) are kept, per owner (the model:
# the list dies with it) and key, as recorded during the previous step: open_pack_scope packs all of them in ONE launch (a 16-scene step
# asked for ~80 of them one by one, forward and backward). An entry names its Parameters and the views' places in them (_place), so
# the views are rebuilt on the Parameters' current storage.
def open_pack_scope(owner=None, plan_key=None) -> PackScope:
    """Open a new PackScope; with a list recorded for (owner, plan_key), its images first (one launch). -> the scope."""
    global _PACK_SCOPE
    plans = None if owner is None else getattr(owner, "_tbx_pack_plans", None)
    if owner is not None and plans is None:
        plans = owner._tbx_pack_plans = {}
    _PACK_SCOPE = scope = PackScope(plans, plan_key)
    plan = plans.get(plan_key) if plans is not None else None
    if plan:
        plan = [e for e in plan if e[0][0].is_cuda and (e[1] is None or e[1][0].is_cuda)]  # (a model moved off the device: not packed)
        reqs = [(_at(w), _at(b), wt, groups) for w, b, wt, groups in plan]
        packed_weights_mfma32_multi(reqs)
        for e, r in zip(plan, reqs):
            scope.record[_pack_key(r[0], r[1], r[2], r[3], False, False, True)] = e
    return scope


def reopen_pack_scope(scope: Optional[PackScope]) -> PackScope:
    """Make `scope` (a closed one: its step's backward goes on with its images) the open scope again; None: a new scope of no owner."""
    global _PACK_SCOPE
    _PACK_SCOPE = scope if scope is not None else PackScope()
    return _PACK_SCOPE


def close_pack_scope(scope: Optional[PackScope] = None) -> None:
    """No scope open any more; the scope's Parameter-sourced requests become the list the next scope of its owner and key starts from."""
    global _PACK_SCOPE
    scope = _PACK_SCOPE if scope is None else scope
    if scope is not None and scope.plans is not None:
        scope.plans[scope.plan_key] = list(scope.record.values())
    _PACK_SCOPE = None


def packed_weight(w: torch.Tensor, bias: Optional[torch.Tensor] = None, wt: bool = False, groups: int = 1,
                  split: bool = False, gemv: bool = False, mfma32: bool = False) -> torch.Tensor:
    """tbx_pack_weight image of a LINEAR weight (+ bias), derived (_derived) from the views' places in their nn.Parameters: re-packed
    after an in-place update or a move, reused otherwise (chains are rebuilt every eager step), per training step inside a PackScope.
    split=True: the tbx_pack_weight_split image (bf16 hi + lo halves) for stages flagged F_WSPLIT.
    gemv=True: the tbx_pack_weight_gemv image (column streams) for the F_WGEMV stages of live-row chains.
    mfma32=True: the tbx_pack_weight_mfma32 image (per-wave units of bf16 hi + lo fragments) for tbx_layer_tile."""
    key = _pack_key(w, bias, wt, groups, split, gemv, mfma32)
    scope = _PACK_SCOPE if mfma32 else None
    if scope is not None and key not in scope.record:
        wp, bp = _place(w), _place(bias)
        if isinstance(wp[0], torch.nn.Parameter) and (bp is None or isinstance(bp[0], torch.nn.Parameter)):
            scope.record[key] = (wp, bp, wt, groups)  # (open_pack_scope: next step's plan)
    return _derived(key, (w, bias), _make_pack, key, scope, w, bias, wt, groups, split, gemv, mfma32)


def _make_pack(key, scope, w, bias, wt, groups, split, gemv, mfma32):
    # (the arguments are checked here: a hit is the same view of the same storage as when its image was made)
    assert w.is_cuda and w.dim() == 2 and w.stride(1) == 1 and w.dtype == torch.float32
    grp = None if scope is None else scope.groups.get(id(w))
    if grp is not None and any(r[0] is w and r[1] is bias and bool(r[2]) == bool(wt) and r[3] == groups for r in grp):
        packed_weights_mfma32_multi(grp)  # pack_group: this request's image and its siblings' in one launch
        return _derived(key, (w, bias))
    n, k = (w.shape[1], w.shape[0] // groups) if wt else (w.shape[0] // groups, w.shape[1])
    if bias is not None:
        assert bias.is_cuda and bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == groups * n
    lib = load()
    size = (lib.tbx_pack_weight_mfma32_size if mfma32 else (lib.tbx_pack_weight_gemv_size if gemv else lib.tbx_pack_weight_size))(n, k, groups)
    if size <= 0:
        _check(int(size), "tbx_pack_weight_size")
    out = torch.empty(size, dtype=torch.float32, device=w.device)
    fn = lib.tbx_pack_weight_mfma32 if mfma32 else (lib.tbx_pack_weight_gemv if gemv else (lib.tbx_pack_weight_split if split else lib.tbx_pack_weight))
    _check(fn(_ptr(w), _ptr(bias), n, k, w.stride(0), groups, int(wt), _ptr(out), stream_ptr()), "tbx_pack_weight")
    return out


def stacked_linear(linears, pad_out_to: int = 0):
    """(W [G * n, k], b [G * n]) = the weights / biases of G equally shaped nn.Linear layers stacked along the output dimension
    (each block zero-padded to pad_out_to output rows if given): branches that read the same input become ONE LINEAR stage
    (G * n outputs), parallel branches one block-diagonal stage (groups = G). A derived image (_derived)."""
    src = [l.weight for l in linears] + [l.bias for l in linears]
    return _derived(("stacked", tuple(map(id, src)), pad_out_to), src, _make_stacked, src, pad_out_to)


@torch.no_grad()
def _make_stacked(src, pad_out_to):
    ws, bs = src[:len(src) // 2], src[len(src) // 2:]
    n, k = ws[0].shape
    npad = max(n, pad_out_to)
    W = torch.zeros(len(ws) * npad, k, dtype=torch.float32, device=ws[0].device)
    B = torch.zeros(len(ws) * npad, dtype=torch.float32, device=ws[0].device)
    for g, (w, b) in enumerate(zip(ws, bs)):
        W[g * npad:g * npad + n].copy_(w)
        B[g * npad:g * npad + n].copy_(b)
    return W, B

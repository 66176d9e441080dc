"""ctypes wrappers of the TRAINING entry points of libtbx_hip.so (include/tbx_hip.h): keyed dropout and the one-pass glue ops, the tall
LINEAR / weight-gradient kernels of the time-batched pass, LayerNorm / PointNet-tail / masked-max-pool forward + backward, the attention
backward (atomics and inverse-list forms), the per-step state machine (tbx_train_chain_*) and the collision term of the reward
(include/tbx_hip_reward.h), and the imitation terms with the configuration's criteria / angular types (include/tbx_hip_il.h, libtbx_il.so).
Re-exported by hip.py."""
import ctypes as C
import os
from typing import List, Optional, Sequence

import torch

from .abi import *  # noqa: F401,F403  (constants, structures, load, declared_symbols: the C-ABI mirror)
from .abi import load, load_il  # noqa: F401
from .hip_base import Seg, _attn_args, _check, _cptr, _derived, _name, _ptr, drop_mix, drop_rate, drop_stream_key, drop_struct, packed_weight, stream_ptr


def keyed_dropout(x: torch.Tensor, p: float, seed: torch.Tensor, site: int, rows_per_scene: int, time_batch: int = 1,
                  time0: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """tbx_keyed_dropout on x viewed as [rows, cols = x.shape[-1]] (contiguous); rows_per_scene = rows per batch entry."""
    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
    cols = x.shape[-1]
    rows = x.numel() // cols if cols else 0
    y = torch.empty_like(x) if out is None else out
    rc = load().tbx_keyed_dropout(_ptr(x), _ptr(y), rows, cols, drop_struct((p, seed, site, rows_per_scene, time_batch, time0)), stream_ptr())
    _check(rc, "tbx_keyed_dropout")
    return y


def tall_linear_ok(x: torch.Tensor, k: int, n: int) -> bool:
    """Shapes tbx_tall_linear takes: row-major fp32 rows of k values (a 2-D view after flattening the leading dimensions), k and n
    multiples of 64 up to 1024, 16-byte aligned, leading dimension a multiple of 4."""
    return (x.is_cuda and x.dtype == torch.float32 and x.shape[-1] == k and k % 64 == 0 and n % 64 == 0 and k <= 1024 and n <= 1024
            and x.stride(-1) == 1 and x.data_ptr() % 16 == 0)


def _pad128(w: torch.Tensor, b: Optional[torch.Tensor]):
    """(w, b) zero-padded to multiples of 128 in both dimensions (tbx_tall_linear's image for a 64-wide layer); a derived image
    (hip_base._derived: per weights version, or per training step inside a PackScope)."""
    n, k = w.shape
    npad, kpad = -(-n // 128) * 128, -(-k // 128) * 128
    if (npad, kpad) == (n, k):
        return w, b
    return _derived(("pad128", _name(w), _name(b)), (w, b), _make_pad128, w, b, npad, kpad)


@torch.no_grad()
def _make_pad128(w, b, npad, kpad):
    n, k = w.shape
    wp = torch.zeros(npad, kpad, dtype=torch.float32, device=w.device)
    wp[:n, :k].copy_(w)
    bp = None
    if b is not None:
        bp = torch.zeros(npad, dtype=torch.float32, device=w.device)
        bp[:n].copy_(b)
    return wp, bp


def tall_linear(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor] = None, wt: bool = False, relu: bool = False,
                bf16: bool = False, out: Optional[torch.Tensor] = None, out16: Optional[torch.Tensor] = None, drop=None) -> torch.Tensor:
    """y = x W^T (+ b) over many rows on the split-bf16 matrix path (tbx_tall_linear; bf16: ONE bf16 product per term,
    tbx_tall_linear_bf16; one tbx_linear_t either way). wt: w is stored [k x n] (the input gradient dx = dy W of a Linear with weight W [n_out, n_in]: x = dy,
    w = W, wt = True). drop (with relu): tbx_keyed_dropout's arguments - dropout(relu(.)) in the same launch; together with out16 the
    library refuses it (TBX_ERR_UNSUPPORTED: no kernel path for dropout beside the bfloat16 copy is tested)."""
    n, k = (w.shape[1], w.shape[0]) if wt else (w.shape[0], w.shape[1])
    x2 = x.reshape(-1, k)
    if x2.stride(1) != 1 or x2.stride(0) % 4 or x2.data_ptr() % 16:
        x2 = x2.contiguous()
    wp, bp = _pad128(w, b)  # (a 64-wide layer: the image of the zero-padded weight; k / n below stay the valid widths)
    img = packed_weight(wp, bp, wt=wt, mfma32=True)
    y = torch.empty(x2.shape[0], n, dtype=torch.float32, device=x.device) if out is None else out
    # (out: rows may be a column block of a wider table - leading dimension a multiple of 4 floats, 16-byte aligned)
    assert y.shape == (x2.shape[0], n) and y.stride(1) == 1 and y.stride(0) % 4 == 0 and y.data_ptr() % 16 == 0 and y.dtype == torch.float32
    a = Linear(x=_ptr(x2, torch.float32), image=_ptr(img, torch.float32), y=_ptr(y), m=x2.shape[0], k=k, ldx=x2.stride(0), n=n,
               has_bias=int(b is not None), relu=int(relu), ldy=y.stride(0))
    if out16 is not None:  # the same rows as bfloat16 as well
        assert out16.shape == y.shape and out16.dtype == torch.bfloat16 and out16.is_contiguous()
        a.y16, a.ldy16 = _ptr(out16, torch.bfloat16), n
    if drop is not None:  # dropout(relu(.)) in the launch: drop = (p, seed, site, rows_per_scene, time_batch, time0)
        assert relu
        a.drop = drop_struct(drop)
    fn = load().tbx_tall_linear_bf16 if bf16 else load().tbx_tall_linear
    _check(fn(C.byref(a), stream_ptr()), "tbx_tall_linear")
    return y if out is not None else y.view(*x.shape[:-1], n)


def linear_wgrad_ok(dy: torch.Tensor, x: torch.Tensor) -> bool:
    """Shapes tbx_linear_wgrad takes: 2-D row-major fp32 views, n, k and both leading dimensions multiples of 4, 16-B aligned."""
    return (dy.dim() == 2 and x.dim() == 2 and dy.is_cuda and dy.dtype == torch.float32 and x.dtype == torch.float32
            and dy.stride(1) == 1 and x.stride(1) == 1 and dy.shape[1] % 4 == 0 and x.shape[1] % 4 == 0
            and dy.stride(0) % 4 == 0 and x.stride(0) % 4 == 0 and dy.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0)


def linear_wgrad(dy: torch.Tensor, x: torch.Tensor, want_db: bool = True, bf16: bool = False):
    """(dw [n,k], db [n] | None) = (dy^T x, sum_rows dy) for dy [rows,n], x [rows,k] (tbx_linear_wgrad; bf16: one bf16 product per
    term with fp32 accumulation, tbx_linear_wgrad_bf16)."""
    rows, n = dy.shape
    k = x.shape[1]
    lib = load()
    splits = lib.tbx_linear_wgrad_splits(rows, n, k)
    if splits <= 0:
        _check(int(splits), "tbx_linear_wgrad_splits")
    scratch = torch.empty(splits, n * k + n, dtype=torch.float32, device=dy.device)
    dw = torch.empty(n, k, dtype=torch.float32, device=dy.device)
    db = torch.empty(n, dtype=torch.float32, device=dy.device) if want_db else None
    fn = lib.tbx_linear_wgrad_bf16 if bf16 else lib.tbx_linear_wgrad
    _check(fn(_ptr(dy), dy.stride(0), _ptr(x), x.stride(0), rows, n, k, _ptr(dw), _ptr(db), _ptr(scratch), splits, stream_ptr()), "tbx_linear_wgrad")
    return dw, db


def attn_fold_fwd(w, b, wr, br, wo, bo):
    """tbx_attn_fold_fwd: (w_in [640,128], b_in [640], w_kv [256,128], b_kv [256], bias_k [128], w_out [128,640], b_out [128]) of one
    AttentionRPE module from in_proj (w [384,128], b [384]), linear_rpe (wr [256,128], br [256]) and out_proj (wo [128,128], bo [128])."""
    for t, shp in ((w, (384, 128)), (b, (384,)), (wr, (256, 128)), (br, (256,)), (wo, (128, 128)), (bo, (128,))):
        assert t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == shp and t.is_contiguous(), shp
    e = lambda *s: torch.empty(*s, dtype=torch.float32, device=w.device)
    out = (e(640, 128), e(640), e(256, 128), e(256), e(128), e(128, 640), e(128))
    _check(load().tbx_attn_fold_fwd(_ptr(w), _ptr(b), _ptr(wr), _ptr(br), _ptr(wo), _ptr(bo), *[_ptr(t) for t in out], stream_ptr()), "tbx_attn_fold_fwd")
    return out


def attn_fold_bwd(w, b, wr, br, wo, grads):
    """tbx_attn_fold_bwd: grads = the seven output gradients (None = zero) -> (d_w, d_b, d_wr, d_br, d_wo, d_bo)."""
    e = lambda *s: torch.empty(*s, dtype=torch.float32, device=w.device)
    out = (e(384, 128), e(384), e(256, 128), e(256), e(128, 128), e(128))
    g = [None if t is None else t.contiguous() for t in grads]
    _check(load().tbx_attn_fold_bwd(_ptr(w), _ptr(b), _ptr(wr), _ptr(br), _ptr(wo), *[_cptr(t, torch.float32) for t in g], *[_ptr(t) for t in out],
                                    stream_ptr()), "tbx_attn_fold_bwd")
    return out


def glue_ok(x: torch.Tensor) -> bool:
    """Tensors the one-pass glue kernels (tbx_residual_drop_*, tbx_relu_drop_*) take: fp32 on the device, last dimension % 4 == 0."""
    return x.is_cuda and x.dtype == torch.float32 and x.dim() >= 2 and x.shape[-1] % 4 == 0 and x.numel() > 0


def residual_drop_fwd(x, y, zero_y, zero_out, drop=None):
    """zero_out[row] ? 0 : x + dropout(zero_y[row] ? 0 : y); zero_* u8 per row or None. drop = None or (p, seed int64[1] device tensor,
    site, rows_per_scene, time_batch, time0), here and below."""
    assert glue_ok(x) and x.is_contiguous() and y.is_contiguous() and y.shape == x.shape and y.dtype == torch.float32
    cols = x.shape[-1]
    rows = x.numel() // cols
    for z in (zero_y, zero_out):
        assert z is None or (z.dtype == torch.uint8 and z.is_contiguous() and z.numel() == rows)
    out = torch.empty_like(x)
    _check(load().tbx_residual_drop_fwd(_ptr(x), _ptr(y), _ptr(zero_y), _ptr(zero_out), rows, cols, drop_struct(drop), _ptr(out), stream_ptr()),
           "tbx_residual_drop_fwd")
    return out


def residual_drop_bwd(dout, zero_y, zero_out, drop=None):
    """-> (dy, dx); dx is dout itself when there is no zero_out mask."""
    assert glue_ok(dout) and dout.is_contiguous()
    cols = dout.shape[-1]
    rows = dout.numel() // cols
    dy = torch.empty_like(dout)
    dx = torch.empty_like(dout) if zero_out is not None else None
    _check(load().tbx_residual_drop_bwd(_ptr(dout), _ptr(zero_y), _ptr(zero_out), rows, cols, drop_struct(drop), _ptr(dy), _ptr(dx), stream_ptr()),
           "tbx_residual_drop_bwd")
    return dy, (dx if dx is not None else dout)


def relu_drop_fwd(z, drop=None):
    assert glue_ok(z) and z.is_contiguous()
    cols = z.shape[-1]
    h = torch.empty_like(z)
    _check(load().tbx_relu_drop_fwd(_ptr(z), z.numel() // cols, cols, drop_struct(drop), _ptr(h), stream_ptr()), "tbx_relu_drop_fwd")
    return h


def relu_drop_bwd(dh, h, p: float):
    assert glue_ok(dh) and dh.is_contiguous() and h.is_contiguous() and h.shape == dh.shape
    cols = dh.shape[-1]
    dz = torch.empty_like(dh)
    _check(load().tbx_relu_drop_bwd(_ptr(dh), _ptr(h), dh.numel() // cols, cols, float(p), _ptr(dz), stream_ptr()), "tbx_relu_drop_bwd")
    return dz


def pair_bias_relu(h, pa, pm, relu: bool):
    """h [n, A, M, d] += pa [n, A, d] + pm [n, M, d] (broadcast), relu'd if `relu`, in place (tbx_pair_bias_relu)."""
    n, A, M, d = h.shape
    assert glue_ok(h) and h.is_contiguous() and pa.shape == (n, A, d) and pm.shape == (n, M, d)
    pa, pm = pa.contiguous(), pm.contiguous()
    _check(load().tbx_pair_bias_relu(_ptr(h, torch.float32), _ptr(pa, torch.float32), _ptr(pm, torch.float32), n, A, M, d, int(bool(relu)), stream_ptr()),
           "tbx_pair_bias_relu")
    return h


def pointnet_tail_ok(z: torch.Tensor) -> bool:
    """z [G, W, 64] fp32 on the device, W <= 32: the shapes tbx_pointnet_tail_* / tbx_masked_maxpool_* take."""
    return z.is_cuda and z.dtype == torch.float32 and z.dim() == 3 and z.shape[2] == 64 and 0 < z.shape[1] <= 32 and z.shape[0] > 0


def pointnet_tail_fwd(z: torch.Tensor, invalid_u8: torch.Tensor, drop=None) -> torch.Tensor:
    """[relu(z) (* keyed dropout) | its max over the group's valid rows], invalid rows zeroed. drop = None or (p, seed int64[1] device
    tensor, site, rows_per_scene, time_batch, time0) - tbx_keyed_dropout's arguments for the [G * W, 64] view."""
    assert pointnet_tail_ok(z) and z.is_contiguous() and invalid_u8.dtype == torch.uint8 and invalid_u8.is_contiguous()
    G, W, Cc = z.shape
    assert invalid_u8.numel() == G * W
    out = torch.empty(G, W, 2 * Cc, dtype=torch.float32, device=z.device)
    _check(load().tbx_pointnet_tail_fwd(_ptr(z), _ptr(invalid_u8), G, W, Cc, drop_struct(drop), _ptr(out), stream_ptr()), "tbx_pointnet_tail_fwd")
    return out


def pointnet_tail_bwd(dout: torch.Tensor, out: torch.Tensor, invalid_u8: torch.Tensor, p: float) -> torch.Tensor:
    G, W, C2 = out.shape
    assert dout.shape == out.shape and dout.is_contiguous() and dout.dtype == torch.float32
    dz = torch.empty(G, W, C2 // 2, dtype=torch.float32, device=out.device)
    _check(load().tbx_pointnet_tail_bwd(_ptr(dout), _ptr(out), _ptr(invalid_u8), G, W, C2 // 2, float(p), _ptr(dz), stream_ptr()),
           "tbx_pointnet_tail_bwd")
    return dz


def masked_maxpool_fwd(x: torch.Tensor, invalid_u8: torch.Tensor) -> torch.Tensor:
    G, W, C2 = x.shape
    assert x.is_contiguous() and x.dtype == torch.float32 and invalid_u8.numel() == G * W
    y = torch.empty(G, C2, dtype=torch.float32, device=x.device)
    _check(load().tbx_masked_maxpool_fwd(_ptr(x), _ptr(invalid_u8), G, W, C2, _ptr(y), stream_ptr()), "tbx_masked_maxpool_fwd")
    return y


def masked_maxpool_bwd(dy: torch.Tensor, x: torch.Tensor, invalid_u8: torch.Tensor) -> torch.Tensor:
    G, W, C2 = x.shape
    assert dy.is_contiguous() and dy.shape == (G, C2) and dy.dtype == torch.float32
    dx = torch.empty_like(x)
    _check(load().tbx_masked_maxpool_bwd(_ptr(dy), _ptr(x), _ptr(invalid_u8), G, W, C2, _ptr(dx), stream_ptr()), "tbx_masked_maxpool_bwd")
    return dx


def layernorm_bwd_ok(x: torch.Tensor) -> bool:
    return x.is_cuda and x.dtype == torch.float32 and x.shape[-1] == 128 and x.numel() > 0


def layernorm_fwd(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float):
    """(y, mean [rows], rstd [rows]) of LayerNorm_128 (tbx_layernorm_fwd)."""
    assert layernorm_bwd_ok(x) and x.is_contiguous()
    rows = x.numel() // 128
    y = torch.empty_like(x)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    _check(load().tbx_layernorm_fwd(_ptr(x), _ptr(gamma.contiguous(), torch.float32), _ptr(beta.contiguous(), torch.float32), float(eps), rows, 128,
                                    _ptr(y), _ptr(mean), _ptr(rstd), stream_ptr()), "tbx_layernorm_fwd")
    return y, mean, rstd


def layernorm_bwd(x: torch.Tensor, dy: torch.Tensor, gamma: torch.Tensor, mean: torch.Tensor, rstd: torch.Tensor, add: Optional[torch.Tensor] = None):
    """(dx, dgamma, dbeta) of y = LayerNorm_128(x) * gamma + beta given dy, with the forward's per-row mean / rstd (tbx_layernorm_bwd).
    add [rows, 128]: dx = add + that gradient in the same pass (tbx_layernorm_bwd_add: the residual branch's gradient of x)."""
    assert layernorm_bwd_ok(x) and x.is_contiguous() and dy.is_contiguous() and dy.shape == x.shape and dy.dtype == torch.float32
    assert add is None or (add.is_contiguous() and add.shape == x.shape and add.dtype == torch.float32)
    rows = x.numel() // 128
    assert mean.numel() == rows and rstd.numel() == rows and mean.is_contiguous() and rstd.is_contiguous()
    lib = load()
    n = lib.tbx_layernorm_bwd_partials(rows)
    scratch = torch.empty(n, 256, dtype=torch.float32, device=x.device)
    dx = torch.empty_like(x)
    dg = torch.empty(128, dtype=torch.float32, device=x.device)
    db = torch.empty(128, dtype=torch.float32, device=x.device)
    _check(lib.tbx_layernorm_bwd_add(_ptr(x), _ptr(dy), _ptr(gamma.contiguous(), torch.float32), _ptr(mean, torch.float32), _ptr(rstd, torch.float32),
                                     rows, 128, _ptr(add), _ptr(dx), _ptr(dg), _ptr(db), _ptr(scratch), stream_ptr()), "tbx_layernorm_bwd_add")
    return dx, dg, db


def _attn_bwd(qbuf, q_off, qt_off, rpe_k_bias, n_batch, n_src, segs, dout, dqbuf, dkv, dbias_k, freqs_xy, freqs_yaw, drop, inv=None, coef=None):
    """tbx_knarpe_attn_bwd: coef / inv = None for the atomics form, the scratch and the inverse lists for the form without."""
    a = _attn_args(qbuf, q_off, qt_off, rpe_k_bias, n_batch, n_src, segs, (freqs_xy, freqs_yaw), drop)
    a.dout, a.ldo, a.dqbuf, a.dbias_k, a.coef = _ptr(dout, torch.float32), dout.stride(0), _ptr(dqbuf, torch.float32), _ptr(dbias_k, torch.float32), _ptr(coef)
    for i in range(min(len(segs), 2)):
        a.dkv[i] = _ptr(dkv[i], torch.float32)
        if inv is not None:
            a.inv_ptr[i], a.inv_list[i] = _cptr(inv[i][0], torch.int32), _cptr(inv[i][1], torch.int32)
    _check(load().tbx_knarpe_attn_bwd(C.byref(a), stream_ptr()), "tbx_knarpe_attn_bwd")


def knarpe_attn_bwd(qbuf, q_off: int, qt_off: int, rpe_k_bias, n_batch: int, n_src: int, segs: Sequence[Seg], dout, dqbuf,
                    dkv: Sequence[torch.Tensor], dbias_k, freqs_xy=None, freqs_yaw=None, drop=None):
    """dK / dV are accumulated into dkv with atomics (zero it first)."""
    _attn_bwd(qbuf, q_off, qt_off, rpe_k_bias, n_batch, n_src, segs, dout, dqbuf, dkv, dbias_k, freqs_xy, freqs_yaw, drop)


def knn_inverse(idx, invalid, n_tgt: int, tgt_batch_div: int = 1):
    """Inverse lists of a K-nearest set idx / invalid [n_batch, n_src, k] -> (inv_ptr [n_tables, n_tgt+1], inv_list [n_tables, cap])."""
    n, S, k = idx.shape
    nt = n // tgt_batch_div
    ptr = torch.empty(nt, n_tgt + 1, dtype=torch.int32, device=idx.device)
    lst = torch.empty(nt, S * tgt_batch_div * k, dtype=torch.int32, device=idx.device)
    rc = load().tbx_knn_inverse(_cptr(idx, torch.int32), _cptr(invalid, torch.uint8), n, S, k, n_tgt, tgt_batch_div, _ptr(ptr), _ptr(lst),
                                stream_ptr())
    _check(rc, "tbx_knn_inverse")
    return ptr, lst


def knarpe_attn_bwd_gather(qbuf, q_off: int, qt_off: int, rpe_k_bias, n_batch: int, n_src: int, segs: Sequence[Seg], dout, dqbuf,
                           dkv: Sequence[torch.Tensor], dbias_rows, inv: Sequence, freqs_xy=None, freqs_yaw=None, drop=None):
    """Backward through inverse K-nearest lists (inv[i] = knn_inverse(...) of segment i): no dK / dV atomics."""
    coef = torch.empty(n_batch * n_src, sum(s.k for s in segs), 8, dtype=torch.float32, device=qbuf.device)
    _attn_bwd(qbuf, q_off, qt_off, rpe_k_bias, n_batch, n_src, segs, dout, dqbuf, dkv, dbias_rows, freqs_xy, freqs_yaw, drop, inv, coef)


def dropout_keep_mask(seed: int, call: int, n_rows: int, k_tot: int, p: float, n_head: int = 4, step: int = 0) -> torch.Tensor:
    """Host restatement of the attention kernels' mask (csrc/attn_core.h DropKey over csrc/drop_key.h): bool [n_rows, n_head, k_tot]
    - for tests and for anyone who needs the mask a (seed, call) pair produces."""
    import numpy as np

    row = np.arange(n_rows, dtype=np.uint32)[:, None, None]
    h = np.arange(n_head, dtype=np.uint32)[None, :, None]
    t = np.arange(k_tot, dtype=np.uint32)[None, None, :]
    with np.errstate(over="ignore"):
        counter = (row * np.uint32(128) + t) * np.uint32(4) + h
    return torch.from_numpy(drop_mix(counter, *drop_stream_key(seed, call, step)) >= np.uint32(drop_rate(p)[0]))


def train_chain_fwd(args: TrainChainArgs, mean: torch.Tensor, stride_n: int, stride_t: int, t0: int, t1: int):
    _check(load().tbx_train_chain_fwd(C.byref(args), _ptr(mean, torch.float32), stride_n, stride_t, t0, t1, stream_ptr()), "tbx_train_chain_fwd")


def train_chain_fwd_windows(args: TrainChainArgs, mean: Optional[torch.Tensor], stride_n: int, stride_t: int, t0: int, t1: int, hv, hp, hm, valid, navi_valid):
    """tbx_train_chain_fwd over [t0, t1) (t0 == t1: none) + the policy inputs of step t1 + 1 into hv u8 [n,A,W], hp / hm f32 [n,A,W,3], valid /
    navi_valid [n,A] (bool or u8 storage)."""
    _check(load().tbx_train_chain_fwd_windows(C.byref(args), _cptr(mean, torch.float32), stride_n, stride_t, t0, t1, _ptr(hv, torch.uint8),
                                              _ptr(hp, torch.float32), _ptr(hm, torch.float32), _ptr(valid), _ptr(navi_valid), stream_ptr()),
           "tbx_train_chain_fwd_windows")


def train_chain_bwd(args: TrainChainArgs, mean: torch.Tensor, stride_n: int, stride_t: int, d_reward: torch.Tensor, d_mean: torch.Tensor):
    _check(load().tbx_train_chain_bwd(C.byref(args), _ptr(mean, torch.float32), stride_n, stride_t, _ptr(d_reward, torch.float32),
                                      _ptr(d_mean, torch.float32), stream_ptr()), "tbx_train_chain_bwd")


def train_chain_bwd_pose(args: TrainChainArgs, mean: torch.Tensor, stride_n: int, stride_t: int, d_reward: torch.Tensor,
                         d_pred_pose: Optional[torch.Tensor], d_mean: torch.Tensor):
    """tbx_train_chain_bwd_pose: the reverse walk with d_pred_pose [n,T,A,3] (None: tbx_train_chain_bwd) added to the predictions' adjoint."""
    _check(load().tbx_train_chain_bwd_pose(C.byref(args), _ptr(mean, torch.float32), stride_n, stride_t, _ptr(d_reward, torch.float32),
                                           _cptr(d_pred_pose, torch.float32), _ptr(d_mean, torch.float32), stream_ptr()), "tbx_train_chain_bwd_pose")


def _collision_log_args(pose: torch.Tensor, valid: torch.Tensor, ag_size: torch.Tensor, n_k: int):
    """The shared leading arguments of tbx_collision_reward_fwd / _bwd for views pose [rows, T, A, 3] f32 / valid [rows, T, A] u8 or bool of
    any strides (the xyz triple contiguous): a permuted time slice of an agent-major log is read where it lies."""
    rows, T, A, three = pose.shape
    assert three == 3 and pose.stride(3) == 1 and tuple(valid.shape) == (rows, T, A) and valid.dtype in (torch.uint8, torch.bool)
    assert ag_size.dtype == torch.float32 and ag_size.is_contiguous() and tuple(ag_size.shape) == (rows // n_k, A, 3)
    return (_ptr(pose, torch.float32), _ptr(valid), rows, int(n_k), A, T, pose.stride(0), pose.stride(2), pose.stride(1), valid.stride(0),
            valid.stride(2), valid.stride(1), _ptr(ag_size))


def collision_reward_fwd(pose: torch.Tensor, valid: torch.Tensor, ag_size: torch.Tensor, reduce_with_max: bool, n_k: int = 1,
                         out: Optional[torch.Tensor] = None, want_arg: bool = True):
    """tbx_collision_reward_fwd -> (c [rows, T, A] f32 - the unweighted term, written into the view `out` if given -, arg int32 [rows, T, A]
    | None: the max mode's partner, for collision_reward_bwd)."""
    rows, T, A, _ = pose.shape
    c = torch.empty(rows, T, A, dtype=torch.float32, device=pose.device) if out is None else out
    assert tuple(c.shape) == (rows, T, A) and c.dtype == torch.float32
    arg = torch.empty(rows, T, A, dtype=torch.int32, device=pose.device) if (want_arg and reduce_with_max) else None
    _check(load().tbx_collision_reward_fwd(*_collision_log_args(pose, valid, ag_size, n_k), int(bool(reduce_with_max)), _ptr(c), c.stride(0),
                                           c.stride(2), c.stride(1), _ptr(arg), stream_ptr()), "tbx_collision_reward_fwd")
    return c, arg


def collision_reward_bwd(pose: torch.Tensor, valid: torch.Tensor, ag_size: torch.Tensor, reduce_with_max: bool, g: torch.Tensor,
                         arg: Optional[torch.Tensor], n_k: int = 1) -> torch.Tensor:
    """tbx_collision_reward_bwd -> d_pose [rows, T, A, 3] (dense) from g = dL/dc, a [rows, T, A] view of any strides."""
    rows, T, A, _ = pose.shape
    assert tuple(g.shape) == (rows, T, A) and g.dtype == torch.float32
    assert arg is None or (arg.is_contiguous() and tuple(arg.shape) == (rows, T, A))
    d_pose = torch.empty(rows, T, A, 3, dtype=torch.float32, device=pose.device)
    _check(load().tbx_collision_reward_bwd(*_collision_log_args(pose, valid, ag_size, n_k), int(bool(reduce_with_max)), _ptr(g), g.stride(0),
                                           g.stride(2), g.stride(1), _ptr(arg, torch.int32), _ptr(d_pose), stream_ptr()), "tbx_collision_reward_bwd")
    return d_pose


def il_reward_args(pred_valid: torch.Tensor, pred_pose: torch.Tensor, pred_motion: torch.Tensor, gt_valid: torch.Tensor, gt_pose: torch.Tensor,
                   gt_motion: torch.Tensor, codes: Sequence[int], weights: Sequence[float], gt_offset: int, n_k: int = 1) -> IlReward:
    """tbx_il_reward_t for the views pred_valid [rows, T, A] u8 / bool, pred_pose / pred_motion [rows, T, A, 3] f32 of any strides (the
    triples contiguous) - a permuted agent-major log is read where it lies - and the dense ground truth [rows / n_k, A, Tg(, 3)].
    codes = (crit_pos, crit_rot, crit_spd, angular), weights = (w_pos, w_rot, w_spd); slot t is compared with ground-truth index t + gt_offset."""
    rows, T, A, three = pred_pose.shape
    assert three == 3 and pred_pose.stride(3) == 1 and pred_motion.stride(3) == 1 and tuple(pred_motion.shape) == (rows, T, A, 3)
    assert tuple(pred_valid.shape) == (rows, T, A) and pred_valid.dtype in (torch.uint8, torch.bool)
    assert pred_pose.dtype == pred_motion.dtype == gt_pose.dtype == gt_motion.dtype == torch.float32 and gt_valid.dtype in (torch.uint8, torch.bool)
    assert rows % n_k == 0 and gt_valid.dim() == 3 and tuple(gt_valid.shape[:2]) == (rows // n_k, A)
    Tg = gt_valid.shape[2]
    assert tuple(gt_pose.shape) == tuple(gt_motion.shape) == (rows // n_k, A, Tg, 3)
    assert gt_valid.is_contiguous() and gt_pose.is_contiguous() and gt_motion.is_contiguous()
    a = IlReward()
    a.pred_valid, a.pred_pose, a.pred_motion = _ptr(pred_valid), _ptr(pred_pose), _ptr(pred_motion)
    a.gt_valid, a.gt_pose, a.gt_motion = _ptr(gt_valid), _ptr(gt_pose), _ptr(gt_motion)
    a.rows, a.n_k, a.n_ag, a.n_step, a.n_step_gt, a.gt_offset = rows, int(n_k), A, T, Tg, int(gt_offset)
    for name, t in (("valid_stride", pred_valid), ("pose_stride", pred_pose), ("motion_stride", pred_motion)):
        setattr(a, name, (C.c_int64 * 3)(t.stride(0), t.stride(1), t.stride(2)))
    a.crit_pos, a.crit_rot, a.crit_spd, a.angular = (int(c) for c in codes)
    a.w_pos, a.w_rot, a.w_spd = (float(w) for w in weights)
    return a


def il_reward_fwd(pred_valid, pred_pose, pred_motion, gt_valid, gt_pose, gt_motion, codes, weights, gt_offset: int, n_k: int = 1,
                  out4: Optional[torch.Tensor] = None, out_sum: Optional[torch.Tensor] = None) -> torch.Tensor:
    """tbx_il_reward_fwd on [rows, T, A(, 3)] views (il_reward_args). out4: a [rows, T, A, 4] f32 view of any strides (the four columns
    contiguous) that receives r_pos, r_rot, r_spd and their sum; else only the sum, into the [rows, T, A] view out_sum (default: a new
    tensor). Returns the tensor written."""
    a = il_reward_args(pred_valid, pred_pose, pred_motion, gt_valid, gt_pose, gt_motion, codes, weights, gt_offset, n_k)
    rows, T, A = pred_valid.shape
    if out4 is not None:
        assert tuple(out4.shape) == (rows, T, A, 4) and out4.dtype == torch.float32 and out4.stride(3) == 1 and out4.device == pred_pose.device
        base, out = out4.data_ptr(), out4
        a.out_pos, a.out_rot, a.out_spd, a.out_sum = base, base + 4, base + 8, base + 12
    else:
        out = torch.empty(rows, T, A, dtype=torch.float32, device=pred_pose.device) if out_sum is None else out_sum
        assert tuple(out.shape) == (rows, T, A) and out.dtype == torch.float32 and out.device == pred_pose.device
        a.out_sum = _ptr(out)
    a.out_stride = (C.c_int64 * 3)(out.stride(0), out.stride(1), out.stride(2))
    _check(load_il().tbx_il_reward_fwd(C.byref(a), stream_ptr()), "tbx_il_reward_fwd")
    return out


def il_reward_bwd(pred_valid, pred_pose, pred_motion, gt_valid, gt_pose, gt_motion, codes, weights, gt_offset: int, g: torch.Tensor, n_k: int = 1):
    """tbx_il_reward_bwd -> (d_pred_pose [rows, T, A, 3], d_pred_spd [rows, T, A]), dense, from g = dL/d(sum), a [rows, T, A] view of any strides."""
    a = il_reward_args(pred_valid, pred_pose, pred_motion, gt_valid, gt_pose, gt_motion, codes, weights, gt_offset, n_k)
    rows, T, A = pred_valid.shape
    assert tuple(g.shape) == (rows, T, A) and g.dtype == torch.float32 and g.device == pred_pose.device
    d_pose = torch.empty(rows, T, A, 3, dtype=torch.float32, device=pred_pose.device)
    d_spd = torch.empty(rows, T, A, dtype=torch.float32, device=pred_pose.device)
    a.g, a.g_stride = _ptr(g), (C.c_int64 * 3)(g.stride(0), g.stride(1), g.stride(2))
    a.d_pred_pose, a.d_pred_spd = _ptr(d_pose), _ptr(d_spd)
    _check(load_il().tbx_il_reward_bwd(C.byref(a), stream_ptr()), "tbx_il_reward_bwd")
    return d_pose, d_spd


def train_chain_bwd_state(args: TrainChainArgs, mean: torch.Tensor, stride_n: int, stride_t: int, d_reward: torch.Tensor,
                          d_pred_pose: Optional[torch.Tensor], d_pred_spd: Optional[torch.Tensor], d_mean: torch.Tensor):
    """tbx_train_chain_bwd_state (libtbx_il.so): the reverse walk with d_pred_pose [n,T,A,3] / d_pred_spd [n,T,A] (dense; None: absent) added
    to the predictions' adjoint."""
    assert d_pred_pose is None or d_pred_pose.is_contiguous()
    assert d_pred_spd is None or d_pred_spd.is_contiguous()
    _check(load_il().tbx_train_chain_bwd_state(C.byref(args), _ptr(mean, torch.float32), stride_n, stride_t, _ptr(d_reward, torch.float32),
                                               _cptr(d_pred_pose, torch.float32), _cptr(d_pred_spd, torch.float32), _ptr(d_mean, torch.float32),
                                               stream_ptr()), "tbx_train_chain_bwd_state")

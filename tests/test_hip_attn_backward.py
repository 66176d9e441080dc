"""The KNARPE attention backward (tbx_knarpe_attn_bwd in its atomics and its gather form, tbx_knn_inverse) and the forward it
differentiates, against ONE float64 evaluation of the factorised formula of include/tbx_hip.h (K6) differentiated by autograd, at the
shapes where the kernels take another path: slots 64..127 (the second slot of a lane), a segment boundary that is no multiple of 8,
the relative-pose form, shared tables (batch_div > 1) in the gather form, inverse lists of every length, wide layouts, row counts
that do not fill a workgroup, K = 1, dbias_k on and off, the dropout mask of high slots / the second segment / time-batched calls.

Tolerances: the kernel pair's stated bound (forward rtol 2e-4 / atol 2e-5, gradients rtol 2e-3 / atol 2e-4), here against float64.
The GPU test prints, per case and block, the kernel's worst err / (atol + rtol |ref|) and the same figure of the fp32 CPU evaluation
of the reference (profiles/MEASUREMENT_LOG.md, "Attention backward: float64 reference sweep")."""
import functools
import math
from importlib import import_module

import numpy as np
import pytest
import torch

from oracle import hptr_ops as H

FWD_TOL = dict(rtol=2e-4, atol=2e-5)
GRAD_TOL = dict(rtol=2e-3, atol=2e-4)
D, NH, DH, DR = 128, 4, 32, 128
SENTINEL = 7.5


def _layout(layout, n_seg):
    """ldq / q_off / qt_off, kv = [(ld_kv, k_off, v_off) per segment], ldo; the defaults are the training step's packed rows."""
    lay = dict(ldq=640, q_off=0, qt_off=128, kv=[(256, 0, 128)] * n_seg, ldo=640)
    lay.update(layout or {})
    return lay


def freqs():
    """The `pose_rpe` buffers of the attention modules (float32, as the kernels read them)."""
    return H.make_freqs_xy(32, 1e3), H.make_freqs_rad(64)


# Defects that test_inputs_discriminate_the_defects injects INTO THE REFERENCE (never into anything that runs on a GPU).
DEFECTS = ("hi_slots", "seg2_slot0", "batch_div", "masked_dkv", "no_scale", "dv_no_keep")


def _evaluate(qbuf, bias_k, kvs, idx, invalid, emb_or_rel, n_tgt, batch_div, n, S, keep, p, layout, dtype, defect=None):
    assert defect is None or defect in DEFECTS
    lay = _layout(layout, len(kvs))
    rows = n * S
    qbuf, bias_k = qbuf.to(dtype), bias_k.to(dtype)
    q = qbuf[:, lay["q_off"]:lay["q_off"] + D].reshape(rows, NH, DH)
    qt = qbuf[:, lay["qt_off"]:lay["qt_off"] + NH * DR].reshape(rows, NH, DR)
    fxy, fyw = (f.to(dtype) for f in freqs())
    b = torch.arange(n)[:, None, None]
    ks, vs, es, ms = [], [], [], []
    for i, (kv, ix, iv, pe) in enumerate(zip(kvs, idx, invalid, emb_or_rel)):
        _, k_off, v_off = lay["kv"][i]
        table = b // batch_div[i]  # consecutive batch entries share a table
        if defect == "batch_div" and i == 1:  # (iii) the entry's own index, folded into the tables that exist
            table = b % (n // batch_div[i])
        flat = (table * n_tgt[i] + ix.long()).reshape(rows, -1)
        kv = kv.to(dtype)
        ks.append(kv[:, k_off:k_off + D][flat].reshape(rows, -1, NH, DH))
        vs.append(kv[:, v_off:v_off + D][flat].reshape(rows, -1, NH, DH))
        pe = pe.to(dtype)
        e = H.pe_xy_yaw(pe[..., :2], pe[..., 2], fxy, fyw) if pe.shape[-1] == 3 else pe  # relative pose -> embedding, or materialised
        es.append(e.reshape(rows, -1, DR))
        ms.append(iv.bool().reshape(rows, -1))
    k, v, e, m = torch.cat(ks, 1), torch.cat(vs, 1), torch.cat(es, 1), torch.cat(ms, 1)
    dead = m.all(-1)
    kf = None
    if keep is not None:
        kf = keep.to(dtype) / (1 - p)  # [rows, 4, sum k]
        if defect == "seg2_slot0":  # (ii) the second segment's slots counted from 0 again
            k0 = ks[0].shape[1]
            kf = torch.cat([kf[..., :k0], kf[..., :kf.shape[-1] - k0]], -1)

    def attend(q, qt, bias_k, k, v, masked):
        raw = (torch.einsum("rhc,rthc->rht", q, k) + torch.einsum("rhc,rtc->rht", qt, e)
               + torch.einsum("rhc,hc->rh", q, bias_k.view(NH, DH)).unsqueeze(-1))
        sc = raw / DH ** 0.5
        if defect == "no_scale":  # (v) the same probabilities, dS without 1 / sqrt(d_head)
            sc = sc.detach() + (raw - raw.detach())
        if defect == "hi_slots":  # (i) nothing flows back through the scores of slots >= 64
            sc = torch.cat([sc[..., :64], sc[..., 64:].detach()], -1)
        if masked:  # rows without any valid target are un-masked (and their output zeroed below)
            sc = sc.masked_fill((m & ~dead[:, None]).unsqueeze(1), float("-inf"))
        a = torch.softmax(sc, -1)
        w = a if kf is None else a * kf
        ov = torch.einsum("rht,rthc->rhc", w, v)
        if defect == "dv_no_keep" and kf is not None:  # (vi) same value, dV weighted by the undropped probability
            leak = torch.einsum("rht,rthc->rhc", a.detach(), v)
            ov = torch.einsum("rht,rthc->rhc", w, v.detach()) + leak - leak.detach()
        return torch.cat([ov.reshape(rows, D), torch.einsum("rht,rtc->rhc", w, e).reshape(rows, NH * DR)], 1)

    if defect == "masked_dkv":  # (iv) same value and query gradients; K / V receive what the un-masked softmax would send them
        leak = attend(q.detach(), qt.detach(), bias_k.detach(), k, v, False)
        out = attend(q, qt, bias_k, k.detach(), v.detach(), True) + leak - leak.detach()
    else:
        out = attend(q, qt, bias_k, k, v, True)
    return out.masked_fill(dead[:, None], 0.0), dead


def reference(qbuf, bias_k, kvs, idx, invalid, emb_or_rel, n_tgt, batch_div, n, S, keep=None, p=0.0, layout=None):
    """include/tbx_hip.h K6 in plain torch, float64 on the CPU, differentiable by autograd -> (out [n * S, 640], dead [n * S]).
      score[h,t] = (q_h . k_h[idx_t] + qt_h . e_t + q_h . bias_k,h) / sqrt(32), masked pairs -> -inf, rows without a valid target un-masked
      out        = [ sum_t a[h,t] m[h,t] / (1 - p) v_h[idx_t] | sum_t a[h,t] m[h,t] / (1 - p) e_t ], zero where `dead`
    Per segment i (lists of 1-2 entries): kvs[i] [n / batch_div[i] * n_tgt[i], ld_kv] - batch entry b reads table b // batch_div[i];
    idx[i] / invalid[i] [n, S, k_i]; emb_or_rel[i] [n, S, k_i, 128] (materialised embedding) or [n, S, k_i, 3] (relative pose: the
    embedding is oracle.hptr_ops.pe_xy_yaw with `freqs()` in float64). keep [n * S, 4, sum k]: the kept (row, head, slot) of the call
    (hip.dropout_keep_mask; `keep_mask` below for time-batched calls), the second segment's slots continuing the first's.
    layout: dict(ldq, q_off, qt_off, kv = [(ld_kv, k_off, v_off)], ldo) - the columns the kernels are told to read; default: q | qt
    packed in 640 columns, K | V in 256. Inputs of any float type are promoted; `out` and the gradients arrive in qbuf's / the leaves'
    type (float64 leaves: nothing is rounded)."""
    out, dead = _evaluate(qbuf, bias_k, kvs, idx, invalid, emb_or_rel, n_tgt, batch_div, n, S, keep, p, layout, torch.float64)
    return out.to(qbuf.dtype), dead


def keep_mask(hip, seed, call, n, S, k_tot, p, time_batch=1, time0=0):
    """[n * S, 4, k_tot] bool from hip.dropout_keep_mask: batch entry b is step time0 + b % time_batch of scene b // time_batch, its
    row s the scene's row (b // time_batch) * S + s (include/tbx_hip.h, tbx_attn_t)."""
    if time_batch == 1 and time0 == 0:
        return hip.dropout_keep_mask(seed, call, n * S, k_tot, p)
    per_step = [hip.dropout_keep_mask(seed, call, n // time_batch * S, k_tot, p, step=time0 + t).view(n // time_batch, S, NH, k_tot)
                for t in range(time_batch)]
    return torch.stack(per_step, 1).reshape(n * S, NH, k_tot)  # [scene, step, S, ...] = batch entry order


# ---------------------------------------------------------------------------------------------------------------- the cases
# segs: (n_tgt, k, batch_div). The smallest shapes at which each path of csrc/attn.hip's backward / csrc/knn.hip's inverse can go wrong.
WIDE = dict(ldq=704, q_off=64, qt_off=192, kv=[(256, 0, 128), (512, 128, 384)], ldo=768)
CASES = {
    "k65": dict(n=3, S=7, segs=[(130, 65, 1)], form="emb"),  # slot 64, K % 8 != 0, 21 rows (% 4 != 0)
    "k128": dict(n=2, S=5, segs=[(2048, 128, 1)], form="rel"),  # ktot and n_tgt at their limits, most tokens never selected
    "straddle": dict(n=6, S=7, segs=[(40, 60, 1), (16, 9, 3)], form="rel"),  # boundary at slot 60, 64 inside segment 2, shared table
    "k1": dict(n=2, S=9, segs=[(1, 1, 1)], form="emb"),  # dS == 0, one token selected by all
    "wide": dict(n=4, S=6, segs=[(23, 7, 1), (11, 5, 2)], form="emb", layout=WIDE),
    "drop_hi": dict(n=3, S=7, segs=[(130, 65, 1), (16, 9, 3)], form="rel", p=0.25),  # mask of slots >= 64 and of segment 2
    "tb": dict(n=6, S=9, segs=[(13, 5, 3)], form="emb", p=0.3, time_batch=3, time0=1),  # 2 scenes x 3 steps
}
DROP_SEED, DROP_CALL = 0x1234_5678_9ABC_DEF1, 3


def list_counts(ix, iv, n_tgt, div):
    """[n / div, n_tgt] inverse-list lengths: un-masked pairs per (table, target token)."""
    n = ix.shape[0]
    tok = ((torch.arange(n) // div)[:, None, None] * n_tgt + ix)[~iv]
    return torch.bincount(tok, minlength=n // div * n_tgt).view(n // div, n_tgt)


@functools.lru_cache(maxsize=None)
def make_case(name):
    """Host inputs of a case (float32, seeded) - shared by the tests, never modified."""
    c = CASES[name]
    g = torch.Generator().manual_seed(sorted(CASES).index(name) + 40)
    n, S, segs = c["n"], c["S"], c["segs"]
    lay = _layout(c.get("layout"), len(segs))
    rows = n * S
    d = dict(c, name=name, rows=rows, lay=lay, n_tgt=[s[0] for s in segs], k=[s[1] for s in segs], div=[s[2] for s in segs], p=c.get("p", 0.0),
             qbuf=torch.randn(rows, lay["ldq"], generator=g), bias_k=torch.randn(D, generator=g), kvs=[], idx=[], inv=[], pe=[])
    for i, (T, K, div) in enumerate(segs):
        d["kvs"].append(torch.randn(n // div * T, lay["kv"][i][0], generator=g))
        ix = (torch.rand(n, S, K, generator=g) ** 2 * T).long().clamp_(max=T - 1)  # skewed: list lengths from 0 to many
        ix[..., 0] = 0  # token 0 is selected by every row
        iv = torch.rand(n, S, K, generator=g) < 0.3
        iv[0, 2] = True  # a row without any valid target
        if name == "straddle" and i == 1:
            iv[3:6] = True  # a table nobody selects
        d["idx"].append(ix)  # (masked pairs keep an in-range index)
        d["inv"].append(iv)
        if c["form"] == "emb":
            d["pe"].append(torch.randn(n, S, K, DR, generator=g))
        else:
            d["pe"].append(torch.cat([torch.randn(n, S, K, 2, generator=g) * 20.0, (torch.rand(n, S, K, 1, generator=g) * 2 - 1) * math.pi], -1))
    d["dout"] = torch.randn(rows, lay["ldo"], generator=g)
    d["counts"] = [list_counts(d["idx"][i], d["inv"][i], T, div) for i, (T, K, div) in enumerate(segs)]
    return d


def _grads(d, hip, dtype, defect=None):
    """out, dead and the gradient blocks of sum(out * dout[:, :640]) for the case's inputs evaluated in `dtype`."""
    keep = None
    if d["p"] > 0:
        keep = keep_mask(hip, DROP_SEED, DROP_CALL, d["n"], d["S"], sum(d["k"]), d["p"], d.get("time_batch", 1), d.get("time0", 0))
    leaves = [t.to(dtype).clone().requires_grad_(True) for t in (d["qbuf"], d["bias_k"], *d["kvs"])]
    out, dead = _evaluate(leaves[0], leaves[1], leaves[2:], d["idx"], d["inv"], d["pe"], d["n_tgt"], d["div"], d["n"], d["S"], keep, d["p"],
                          d["lay"], dtype, defect)
    (out * d["dout"][:, :D + NH * DR].to(dtype)).sum().backward()
    lay, gq = d["lay"], leaves[0].grad
    blocks = {"fwd": out.detach(), "dq": gq[:, lay["q_off"]:lay["q_off"] + D], "dqt": gq[:, lay["qt_off"]:lay["qt_off"] + NH * DR],
              "dbias": leaves[1].grad}
    for i, (_, k_off, v_off) in enumerate(lay["kv"]):
        blocks[f"dK{i}"], blocks[f"dV{i}"] = leaves[2 + i].grad[:, k_off:k_off + D], leaves[2 + i].grad[:, v_off:v_off + D]
    other = torch.ones_like(gq, dtype=torch.bool)
    other[:, lay["q_off"]:lay["q_off"] + D] = other[:, lay["qt_off"]:lay["qt_off"] + NH * DR] = False
    assert not gq[other].any()  # the reference reads the same columns as the kernel: nothing else carries a gradient
    return blocks, dead


@functools.lru_cache(maxsize=None)
def case_reference(name, hip):
    """(float64 blocks, dead, fp32-evaluation blocks) of a case: computed once, shared, read only."""
    d = make_case(name)
    ref, dead = _grads(d, hip, torch.float64)
    f32, dead32 = _grads(d, hip, torch.float32)
    assert torch.equal(dead, dead32)
    return ref, dead, f32


def worst(got, ref, rtol, atol):
    """max err / (atol + rtol |ref|): <= 1 is torch.testing.assert_close's criterion."""
    got, ref = got.detach().cpu().double(), ref.double()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all())
    return float(((got - ref).abs() / (atol + rtol * ref.abs())).max())


def tol_of(block):
    return FWD_TOL if block == "fwd" else GRAD_TOL


# ---------------------------------------------------------------------------------------------------------------- CPU
DEFECT_CASES = {"hi_slots": ("k65", "k128", "straddle", "drop_hi"),  # sum k > 64
                "seg2_slot0": ("drop_hi",),  # two segments and dropout
                "batch_div": ("straddle", "wide"),  # two shared second tables (drop_hi has ONE: every in-range choice is the right one)
                "masked_dkv": ("k65", "k128", "straddle", "wide", "drop_hi", "tb"),  # (K = 1: a masked pair is a dead row)
                "no_scale": ("k65", "k128", "straddle", "wide", "drop_hi", "tb"),  # (K = 1: dS == 0)
                "dv_no_keep": ("drop_hi", "tb")}  # dropout


@pytest.mark.parametrize("defect", DEFECTS)
def test_inputs_discriminate_the_defects(tb, defect):
    """The cases' shapes and data can see each class of fault the GPU test exists for: the float64 reference with one defect injected
    into it differs from the unmodified reference by >= 10 x the gradient tolerance in at least one gradient block, in every case the
    defect applies to. Nothing is launched."""
    hip = import_module("trafficbots_amd.hip")
    assert set(DEFECT_CASES) == set(DEFECTS)
    for name in DEFECT_CASES[defect]:
        ref, dead, _ = case_reference(name, hip)
        bad, dead_b = _grads(make_case(name), hip, torch.float64, defect)
        assert torch.equal(dead, dead_b)
        fig = {b: worst(bad[b], ref[b], **GRAD_TOL) for b in ref if b not in ("fwd", "dbias")}
        print(f"attn_bwd_defect {defect:11s} {name:9s} " + " ".join(f"{b}={v:.3g}" for b, v in fig.items()))
        assert max(fig.values()) >= 10.0, (defect, name, fig)


def test_case_inputs_cover_the_inverse_list_shapes():
    """Host data only: list lengths 0, 1, 2, 3 and an odd one >= 5 in `k65` and `straddle` (the dkv loop takes two pairs per trip plus a
    tail), a token selected by every row with a valid first pair, never-selected tokens, a row without a valid target everywhere, a table
    nobody selects, ~30 % masked pairs."""
    for name in CASES:
        d = make_case(name)
        for i, (T, K, div) in enumerate(d["segs"]):
            ix, iv, cnt = d["idx"][i], d["inv"][i], d["counts"][i]
            assert int(ix.min()) >= 0 and int(ix.max()) < T and bool((ix[..., 0] == 0).all()) and bool(iv[0, 2].all())
            assert int(cnt.sum()) == int((~iv).sum()) and cnt.shape == (d["n"] // div, T)
            if iv.numel() >= 100 and not (name == "straddle" and i == 1):
                assert 0.2 < float(iv.float().mean()) < 0.4
        if name in ("k65", "straddle"):
            seen = set(torch.cat([c.flatten() for c in d["counts"]]).tolist())
            assert {0, 1, 2, 3} <= seen and any(v >= 5 and v % 2 for v in seen), sorted(seen)
            assert any(v >= 6 and v % 2 == 0 for v in seen)
    assert bool((make_case("straddle")["counts"][1][1] == 0).all()) and int(make_case("straddle")["counts"][1][0].sum()) > 0
    assert int((make_case("k128")["counts"][0] == 0).sum()) > 2048  # most tokens never selected
    k1 = make_case("k1")
    assert int(k1["counts"][0].max()) >= 5 and 0 < int(k1["inv"][0].sum()) < k1["rows"]


# ---------------------------------------------------------------------------------------------------------------- GPU
def check_inverse_lists(ptr, lst, ix, iv, n_tgt, div):
    """The lists are exactly the un-masked pairs (global row * k + slot) grouped by target token, per table - every token."""
    n, S, K = ix.shape
    ptr, lst = ptr.cpu().numpy().astype(np.int64), lst.cpu().numpy().astype(np.int64)
    assert ptr.shape == (n // div, n_tgt + 1) and lst.shape == (n // div, S * div * K)
    pair = np.arange(n * S * K).reshape(n // div, S * div * K)  # a table's rows are consecutive: so are its pair ids
    tok, ok = ix.numpy().reshape(n // div, -1), ~iv.numpy().reshape(n // div, -1)
    for t in range(n // div):
        assert ptr[t, 0] == 0 and (np.diff(ptr[t]) >= 0).all() and ptr[t, n_tgt] == ok[t].sum()
        want_tok, want_pair = tok[t][ok[t]], pair[t][ok[t]]
        assert (np.diff(ptr[t]) == np.bincount(want_tok, minlength=n_tgt)).all()
        got_tok, got_pair = np.repeat(np.arange(n_tgt), np.diff(ptr[t])), lst[t, :ptr[t, n_tgt]]
        o_w, o_g = np.lexsort((want_pair, want_tok)), np.lexsort((got_pair, got_tok))
        assert (got_pair[o_g] == want_pair[o_w]).all()  # (same tokens' counts above: equal multisets per token)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_attention_forward_backward_vs_float64_reference(tb, name):
    """hip.knarpe_attn, hip.knarpe_attn_bwd (atomics) and hip.knn_inverse + hip.knarpe_attn_bwd_gather called directly on a case of
    CASES, each against the float64 reference: flags and forward; dq, dqt, dK / dV per segment and the column sum of the dbias_k rows in
    both forms, with dbias_k and without; exact zeros of rows without a valid target (and of dq / dqt at K = 1); gather == atomics at
    rtol 1e-4 / atol 1e-5; the gather form bit-identical run to run; sentinels outside the q / qt and K / V columns intact, every token
    row's K / V columns overwritten, never-selected tokens exactly zero; the inverse lists complete. Measured on MI355X: the kernels' worst
    err / (atol + rtol |ref|) is 0.136 (forward, `drop_hi`) and 0.026 over all gradient blocks - the fp32 CPU evaluation's own figures."""
    dev = torch.device("cuda:0")
    hip = import_module("trafficbots_amd.hip")
    d = make_case(name)
    ref, dead, f32 = case_reference(name, hip)
    n, S, rows, lay, n_seg = d["n"], d["S"], d["rows"], d["lay"], len(d["segs"])
    q_off, qt_off = lay["q_off"], lay["qt_off"]
    fxy, fyw = (f.to(dev) for f in freqs())
    qbuf, bias_k, dout = d["qbuf"].to(dev), d["bias_k"].to(dev), d["dout"].to(dev)
    kvs = [kv.to(dev) for kv in d["kvs"]]
    idx = [ix.to(torch.int32).to(dev).contiguous() for ix in d["idx"]]
    inv = [iv.to(torch.uint8).to(dev).contiguous() for iv in d["inv"]]
    pe = [e.to(dev).contiguous() for e in d["pe"]]
    emb = d["form"] == "emb"
    segs = [hip.Seg(kvs[i], lay["kv"][i][1], lay["kv"][i][2], d["n_tgt"][i], idx[i], inv[i], pe[i] if emb else None, d["div"][i],
                    rel=None if emb else pe[i]) for i in range(n_seg)]
    drop = None
    if d["p"] > 0:
        drop = (d["p"], torch.tensor([DROP_SEED], dtype=torch.int64).to(dev), DROP_CALL, d.get("time_batch", 1), d.get("time0", 0))
    failed = []

    def compare(form, got):  # print every figure of the form, then assert
        for b, g in got.items():
            a_, f_ = worst(g, ref[b], **tol_of(b)), worst(f32[b], ref[b], **tol_of(b))
            print(f"attn_bwd_sweep {name:9s} {form:12s} {b:6s} kernel={a_:.4f} fp32ref={f_:.4f}")
            if not a_ <= 1.0:
                failed.append((form, b, a_))

    # ---- forward and flags
    out = torch.full((rows, lay["ldo"]), SENTINEL, device=dev)
    flag = torch.full((rows,), 9, dtype=torch.uint8, device=dev)
    hip.knarpe_attn(qbuf, q_off, qt_off, bias_k, n, S, segs, out, flag, fxy, fyw, drop=drop)
    assert torch.equal(flag.cpu(), dead.to(torch.uint8))
    compare("forward", {"fwd": out[:, :D + NH * DR]})
    assert bool((out[:, D + NH * DR:] == SENTINEL).all())

    # ---- the backward, both forms, with and without dbias_k
    other_q = torch.ones(lay["ldq"], dtype=torch.bool)
    other_q[q_off:q_off + D] = other_q[qt_off:qt_off + NH * DR] = False
    lists = [hip.knn_inverse(idx[i], inv[i], d["n_tgt"][i], d["div"][i]) for i in range(n_seg)]
    for i in range(n_seg):
        check_inverse_lists(lists[i][0], lists[i][1], d["idx"][i], d["inv"][i], d["n_tgt"][i], d["div"][i])

    def backward(gather, want_db, repeat=False):
        dq = torch.full((rows, lay["ldq"]), SENTINEL, device=dev)
        db = torch.full((rows, D), SENTINEL, device=dev) if want_db else None
        if gather:  # no pre-zeroing: every token's K and V columns are overwritten
            dkv = [torch.full_like(kv, SENTINEL) for kv in kvs]
            hip.knarpe_attn_bwd_gather(qbuf, q_off, qt_off, bias_k, n, S, segs, dout, dq, dkv, db, lists, fxy, fyw, drop=drop)
        else:
            dkv = [torch.zeros_like(kv) for kv in kvs]
            hip.knarpe_attn_bwd(qbuf, q_off, qt_off, bias_k, n, S, segs, dout, dq, dkv, db, fxy, fyw, drop=drop)
        dq, dkv, db = dq.cpu(), [t.cpu() for t in dkv], (db.cpu() if want_db else None)
        got = {"dq": dq[:, q_off:q_off + D], "dqt": dq[:, qt_off:qt_off + NH * DR]}
        for i, (_, k_off, v_off) in enumerate(lay["kv"]):
            got[f"dK{i}"], got[f"dV{i}"] = dkv[i][:, k_off:k_off + D], dkv[i][:, v_off:v_off + D]
        if want_db:
            got["dbias"] = db.double().sum(0)
        if not repeat:  # (a repeated run is held to bit equality with the first below)
            compare(("gather" if gather else "atomics") + ("" if want_db else "/no_db"), got)
        # rows flagged dead: exactly zero; K = 1: dS == 0, so dq and dqt are exactly zero while dV is not
        assert not got["dq"][dead].any() and not got["dqt"][dead].any()
        if name == "k1":
            assert not got["dq"].any() and not got["dqt"].any() and bool(got["dV0"].any())
        # untouched memory: dqbuf outside q / qt, dkv outside K / V (atomics: still the caller's zeros)
        assert bool((dq[:, other_q] == SENTINEL).all())
        for i, (ld, k_off, v_off) in enumerate(lay["kv"]):
            other = torch.ones(ld, dtype=torch.bool)
            other[k_off:k_off + D] = other[v_off:v_off + D] = False
            assert bool((dkv[i][:, other] == (SENTINEL if gather else 0.0)).all())
            never = (d["counts"][i] == 0).flatten()
            assert bool((got[f"dK{i}"] != SENTINEL).all()) and bool((got[f"dV{i}"] != SENTINEL).all())  # every token row written
            assert not got[f"dK{i}"][never].any() and not got[f"dV{i}"][never].any()  # never selected: exactly 0.0
        return got, dq, dkv

    got_a, _, _ = backward(False, True)
    backward(False, False)
    got_g, dq_g, dkv_g = backward(True, True)
    _, dq_g2, dkv_g2 = backward(True, True, repeat=True)
    _, dq_n, dkv_n = backward(True, False)
    _, dq_n2, dkv_n2 = backward(True, False, repeat=True)
    # gather against atomics at the existing bound; the gather form has no atomics: run-to-run identical, with and without dbias_k
    for b in got_a:
        torch.testing.assert_close(got_g[b], got_a[b], rtol=1e-4, atol=1e-5)
    assert torch.equal(dq_g, dq_g2) and all(torch.equal(a, b) for a, b in zip(dkv_g, dkv_g2))
    assert torch.equal(dq_n, dq_n2) and all(torch.equal(a, b) for a, b in zip(dkv_n, dkv_n2))
    assert not failed, failed

"""Cases, inputs and the float64 reference of the forward sweep of tbx_knarpe_attn_fwd (tests/test_hip_attn_forward.py): one case per
launch form of csrc/attn.hip at the smallest shape that reaches it, each recording the form code (tbx_knarpe_attn_fwd_form) it exists
for. Nothing here runs on a GPU.

The reference is the one of tests/test_hip_attn_backward.py (`_evaluate`: include/tbx_hip.h K6 in plain torch), extended - the
reference, not the kernels' wrappers - by two things:
  * bf16 tables: the reference reads the same bf16-rounded table promoted to float64 (the kernel's inputs ARE those bf16 values; only
    its arithmetic is under test);
  * the value fold: out128[h * 32 + j] = (sum a v)[h * 32 + j] + W_v[h * 32 + j, :] . (sum a e)_h + b_v[h * 32 + j], zero for rows
    without a valid target, with `scale` = the sum of the magnitudes of the added terms (the convention of tests/sim_step_ref.py).

Inputs as the backward sweep draws them (seeded; qbuf and tables randn; relative poses xy ~ N(0, 20 m), yaw uniform in +-pi - larger
coordinates test fp32 sin, not launch forms; ~30 % of the pairs masked; token 0 selected by every row), and every case has a row without
a valid target at row 2 and at the LAST row of the launch (inside the ragged quad where the row count is no multiple of 4).

Tolerances: the 640-wide forms are held to the kernel pair's stated bound (FWD_TOL: rtol 2e-4 / atol 2e-5) against float64; the folded
forms to C_FOLD * 2^-23 * scale, C_FOLD = 4 x the float32 CPU evaluation's worst figure (test_float32_yardstick_of_the_folded_cases).

Not here: the forms behind environment variables - TBX_ATTN_RING (the bf16 ring and R = 2) and TBX_ATTN_XCD=0. The library reads them
once per process and the tests set no environment variable. The folded launcher switches to a wave per row at 1024 rows (not at 193 as
the 640-wide launcher does without dropout): the folded cases of 21 .. 240 rows are its 4-waves-per-row form, the `_1k` ones and
`fold_loop` its wave-per-row form."""
import functools
import math

import torch

import test_hip_attn_backward as B
from test_hip_attn_backward import D, DH, DR, FWD_TOL, NH, WIDE, freqs, keep_mask, worst  # noqa: F401

OUTW = D + NH * DR  # 640
ULP = 2.0 ** -23
SENTINEL = 7.5
DROP_SEED, DROP_CALL = 0x0FED_CBA9_8765_4321, 7

# form codes (include/tbx_hip.h TBX_ATTN_FORM_*; trafficbots_amd.abi mirrors them - compared in test_cases_take_their_forms)
SPLIT4, WAVE, RING, FORM_MASK = 1, 2, 3, 0xF
DROP, KV16, FOLD, FOLD_LOOP, BATCH_MAJOR, XCD = 0x10, 0x20, 0x40, 0x80, 0x100, 0x200

# segs: (n_tgt, k, batch_div)
K65, TWO, SHARED = [(130, 65, 1)], [(130, 65, 1), (16, 9, 3)], [(23, 7, 1), (11, 5, 2)]
CASES = {
    # ---- the LDS ring: fp32 tables, relative poses, 193 .. 1536 rows without dropout
    "ring_min": dict(n=1, S=193, segs=K65, form="rel", code=RING | XCD),  # grid 49 (% 8 != 0), ragged quad, slot 64
    "ring_k128": dict(n=2, S=100, segs=[(2048, 128, 1)], form="rel", code=RING | XCD),  # ktot and n_tgt at their limits
    "ring_straddle": dict(n=6, S=40, segs=[(40, 60, 1), (16, 9, 3)], form="rel", code=RING | XCD),  # boundary at slot 60, 64 in segment 2
    "ring_k1": dict(n=1, S=197, segs=[(1, 1, 1)], form="rel", code=RING | XCD),
    "ring_shared4": dict(n=8, S=30, segs=SHARED, form="rel", code=RING | XCD),  # shared tables, n % 4 == 0: the ring has no batch-major order
    "ring_max": dict(n=4, S=384, segs=[(50, 12, 1)], form="rel", code=RING | XCD),  # 1536 rows: the last ring size
    # ---- the ring with dropout (1024 .. 1536 rows)
    "ring_drop": dict(n=4, S=257, segs=[(130, 65, 1), (16, 9, 2)], form="rel", p=0.25, code=RING | DROP),  # mask of slots >= 64, segment 2
    "ring_tb": dict(n=6, S=171, segs=[(13, 5, 3)], form="rel", p=0.3, time_batch=3, time0=1, code=RING | DROP),
    # ---- a wave per row
    "wave_emb": dict(n=1, S=193, segs=K65, form="emb", code=WAVE | XCD),
    "wave_wide": dict(n=3, S=67, segs=[(23, 7, 1), (11, 5, 3)], form="emb", layout=WIDE, code=WAVE | XCD),
    "wave_rel": dict(n=1, S=1537, segs=[(40, 33, 1)], form="rel", code=WAVE | XCD),  # the first size past the ring
    "wave_bm": dict(n=8, S=200, segs=[(23, 7, 1), (11, 5, 4)], form="rel", code=WAVE | BATCH_MAJOR | XCD),
    "wave_shared": dict(n=6, S=270, segs=[(23, 7, 1), (11, 5, 3)], form="rel", code=WAVE | XCD),  # shared, n % 4 != 0: not batch-major
    "wave_bm_emb": dict(n=4, S=50, segs=SHARED, form="emb", code=WAVE | BATCH_MAJOR | XCD),
    "wave_drop": dict(n=1, S=1541, segs=[(40, 33, 1)], form="rel", p=0.3, code=WAVE | DROP),
    "wave_drop_emb": dict(n=2, S=513, segs=[(23, 7, 1)], form="emb", p=0.2, code=WAVE | DROP),
    # ---- bf16 tables (never the ring by default)
    "kv16_split": dict(n=3, S=7, segs=TWO, form="rel", kv16=True, code=SPLIT4 | KV16 | XCD),
    "kv16_wave": dict(n=1, S=193, segs=[(130, 65, 1), (16, 9, 1)], form="rel", kv16=True, code=WAVE | KV16 | XCD),
    "kv16_wave_emb": dict(n=1, S=193, segs=K65, form="emb", kv16=True, code=WAVE | KV16 | XCD),
    # ---- the value fold in the epilogue
    "fold_split": dict(n=3, S=7, segs=TWO, form="rel", fold=True, code=SPLIT4 | FOLD | XCD),
    "fold_split_kv16": dict(n=3, S=7, segs=TWO, form="emb", fold=True, kv16=True, code=SPLIT4 | FOLD | KV16 | XCD),
    "fold_wave": dict(n=1, S=193, segs=K65, form="emb", fold=True, code=SPLIT4 | FOLD | XCD),  # (below the folded launcher's 1024 rows)
    "fold_wave_kv16": dict(n=1, S=193, segs=K65, form="rel", fold=True, kv16=True, code=SPLIT4 | FOLD | KV16 | XCD),
    "fold_bm": dict(n=4, S=60, segs=SHARED, form="rel", fold=True, code=SPLIT4 | FOLD | XCD),
    "fold_wave_1k": dict(n=1, S=1026, segs=K65, form="rel", fold=True, code=WAVE | FOLD),  # ragged quad: a live row, a dead row, 2 spare waves
    "fold_wave_1k_kv16": dict(n=1, S=1026, segs=K65, form="emb", fold=True, kv16=True, code=WAVE | FOLD | KV16),
    "fold_bm_1k": dict(n=4, S=257, segs=SHARED, form="rel", fold=True, code=WAVE | FOLD | BATCH_MAJOR),
    # 514 quads against the grid cap of 2 x 256 CUs: two workgroups walk two quads, the last quad is ragged
    "fold_loop": dict(n=1, S=2053, segs=[(40, 12, 1)], form="rel", fold=True, code=WAVE | FOLD | FOLD_LOOP),
}
FOLDED = tuple(k for k, c in CASES.items() if c.get("fold"))

# The folded forms' bound is C_FOLD * 2^-23 * scale. C_FOLD = 4 x the worst figure of the float32 CPU evaluation of the reference
# against its float64 evaluation on the folded cases' inputs (the margin of sim_step_cases.C), rounded up to a whole number of at most
# two significant digits; test_float32_yardstick_of_the_folded_cases measures the figure again and holds it to C_FOLD / 4. Not taken
# from any kernel's output. Measured (profiles/MEASUREMENT_LOG.md): 9.14 (`fold_wave_1k`; the relative-pose cases lead, 1.9 .. 2.9 with
# a materialised embedding) -> 4 x 9.14 = 36.6 -> 37: 4.4e-6 of the scale.
FOLD_YARDSTICK = 9.14
C_FOLD = 37.0


def fold_image_floats():
    """Floats of the tbx_pack_weight_gemv image of the value fold (4 groups x 32 outputs, k = 128): a bias row + 32 weight rows."""
    return (1 + (DR // 16) * 4) * D * 4


@functools.lru_cache(maxsize=None)
def make_case(name):
    """Host inputs of a case (float32, seeded) - shared by the tests, never modified. `kvs`: the tables as drawn; `kvs_in`: what the
    kernel and the reference read (the bf16-rounded values in the bf16 cases, the same tensors otherwise)."""
    c = CASES[name]
    g = torch.Generator().manual_seed(sorted(CASES).index(name) + 900)
    n, S, segs = c["n"], c["S"], c["segs"]
    lay = B._layout(c.get("layout"), len(segs))
    rows = n * S
    d = dict(c, name=name, rows=rows, lay=lay, n_tgt=[s[0] for s in segs], k=[s[1] for s in segs], div=[s[2] for s in segs], p=c.get("p", 0.0),
             kv16=bool(c.get("kv16")), fold=bool(c.get("fold")), qbuf=torch.randn(rows, lay["ldq"], generator=g),
             bias_k=torch.randn(D, generator=g), kvs=[], kvs_in=[], idx=[], inv=[], pe=[])
    for i, (T, K, div) in enumerate(segs):
        assert n % div == 0
        kv = torch.randn(n // div * T, lay["kv"][i][0], generator=g)
        d["kvs"].append(kv)
        d["kvs_in"].append(kv.to(torch.bfloat16).to(torch.float32) if d["kv16"] else kv)
        ix = (torch.rand(n, S, K, generator=g) ** 2 * T).long().clamp_(max=T - 1)
        ix[..., 0] = 0  # token 0 is selected by every row
        iv = torch.rand(n, S, K, generator=g) < 0.3
        iv[0, 2] = True  # rows without any valid target: row 2 ...
        iv[n - 1, S - 1] = True  # ... and the last row of the launch
        d["idx"].append(ix)  # (masked pairs keep an in-range index)
        d["inv"].append(iv)
        if c["form"] == "emb":
            d["pe"].append(torch.randn(n, S, K, DR, generator=g))
        else:
            d["pe"].append(torch.cat([torch.randn(n, S, K, 2, generator=g) * 20.0, (torch.rand(n, S, K, 1, generator=g) * 2 - 1) * math.pi], -1))
    if d["fold"]:
        d["w_v"], d["b_v"] = torch.randn(D, DR, generator=g) * DR ** -0.5, torch.randn(D, generator=g)
    return d


# Defects that test_inputs_discriminate_the_defects injects INTO THE REFERENCE (never into anything that runs on a GPU).
DEFECTS = ("ragged_quad", "hi_slots", "seg2_slot0", "batch_div", "bm_rows", "fold_head0", "fold_no_bias", "kv_unrounded")


def _keep(d, hip):
    if not d["p"] > 0:
        return None
    return keep_mask(hip, DROP_SEED, DROP_CALL, d["n"], d["S"], sum(d["k"]), d["p"], d.get("time_batch", 1), d.get("time0", 0))


def fold(out640, dead, w_v, b_v, dtype, defect=None):
    """The value half of linear_rpe applied to the 640-wide row -> (out128 [rows, 128], scale [rows, 128])."""
    ov, e = out640[:, :D].to(dtype), out640[:, D:].to(dtype).reshape(-1, NH, DR)
    w, b = w_v.to(dtype).view(NH, DH, DR), b_v.to(dtype)
    if defect == "fold_head0":  # every head's block of W_v meets head 0's sums
        e = e[:, :1].expand(-1, NH, -1)
    if defect == "fold_no_bias":
        b = torch.zeros_like(b)
    out = ov + torch.einsum("hjk,rhk->rhj", w, e).reshape(-1, D) + b
    scale = ov.abs() + torch.einsum("hjk,rhk->rhj", w.abs(), e.abs()).reshape(-1, D) + b_v.to(dtype).abs()
    return out.masked_fill(dead[:, None], 0.0), scale


def evaluate(d, hip, dtype=torch.float64, defect=None):
    """-> (out [rows, 640] or, folded, [rows, 128]; dead [rows]; scale or None) of a case evaluated in `dtype` on the CPU."""
    assert defect is None or defect in DEFECTS
    n, S, rows = d["n"], d["S"], d["rows"]
    kvs, inv = d["kvs_in"], d["inv"]
    if defect == "kv_unrounded":
        kvs = d["kvs"]
    if defect == "hi_slots":  # slots >= 64 of the row (the second index register, the second slot of a lane) contribute nothing
        hi = torch.arange(sum(d["k"])) >= 64
        inv = [iv | h for iv, h in zip(inv, hi.split(d["k"]))]
    inner = defect if defect in ("seg2_slot0", "batch_div") else None
    out, dead = B._evaluate(d["qbuf"], d["bias_k"], kvs, d["idx"], inv, d["pe"], d["n_tgt"], d["div"], n, S, _keep(d, hip), d["p"], d["lay"],
                            dtype, inner)
    scale = None
    if d["fold"]:
        out, scale = fold(out, dead, d["w_v"], d["b_v"], dtype, defect)
    if defect == "bm_rows":  # quad q, wave r of a group of 4 batch entries writes row 4 q + r, not row r * S + q
        out = out.view(n // 4, 4, S, -1).transpose(1, 2).reshape(rows, -1)
    if defect == "ragged_quad" and rows % 4:  # the rows of the last, ragged quad left unwritten
        out = out.clone()
        out[rows // 4 * 4:] = SENTINEL
    return out, dead, scale


@functools.lru_cache(maxsize=None)
def case_reference(name, hip):
    """(float64 out, dead, scale | None, float32-evaluation out) of a case: computed once, shared, read only."""
    d = make_case(name)
    ref, dead, scale = evaluate(d, hip, torch.float64)
    f32, dead32, _ = evaluate(d, hip, torch.float32)
    assert torch.equal(dead, dead32)
    return ref, dead, scale, f32


def fold_units(got, ref, scale):
    """max err / (2^-23 * scale) over the elements with a scale (rows without a valid target are exact zeros, compared apart)."""
    got, ref = got.detach().cpu().double(), ref.double()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all())
    live = scale > 0
    return float(((got - ref).abs()[live] / (ULP * scale.double()[live])).max())


def figure(d, got, ref, scale):
    """The worst error of `got` in units of the case's bound: <= 1 passes."""
    if d["fold"]:
        return fold_units(got, ref, scale) / C_FOLD
    return worst(got, ref, **FWD_TOL)


def applies(defect, d):
    code, two = d["code"], len(d["segs"]) == 2
    return {"ragged_quad": d["rows"] % 4 != 0 and code & FORM_MASK != SPLIT4,
            "hi_slots": sum(d["k"]) > 64,
            "seg2_slot0": two and d["p"] > 0,
            "batch_div": two and d["div"][1] > 1 and d["n"] // d["div"][1] >= 2,  # (ONE shared table: every in-range choice is the right one)
            "bm_rows": bool(code & BATCH_MAJOR),
            "fold_head0": d["fold"], "fold_no_bias": d["fold"], "kv_unrounded": d["kv16"]}[defect]


def launch_args(d, place, fold_image=None, out=None, flag=None, hip=None):
    """(args, kwargs) of hip.knarpe_attn / hip.knarpe_attn_form for a case: `place` moves a host tensor to where the call wants it (the
    identity: host tensors, which only the form query accepts)."""
    lay, emb = d["lay"], d["form"] == "emb"
    kvs = [place(kv.to(torch.bfloat16) if d["kv16"] else kv) for kv in d["kvs_in"]]
    idx = [place(ix.to(torch.int32).contiguous()) for ix in d["idx"]]
    inv = [place(iv.to(torch.uint8).contiguous()) for iv in d["inv"]]
    pe = [place(e.contiguous()) for e in d["pe"]]
    segs = [hip.Seg(kvs[i], lay["kv"][i][1], lay["kv"][i][2], d["n_tgt"][i], idx[i], inv[i], pe[i] if emb else None, d["div"][i],
                    rel=None if emb else pe[i]) for i in range(len(d["segs"]))]
    fxy, fyw = (place(f) for f in freqs())
    drop = None
    if d["p"] > 0:
        drop = (d["p"], place(torch.tensor([DROP_SEED], dtype=torch.int64)), DROP_CALL, d.get("time_batch", 1), d.get("time0", 0))
    qbuf, bias_k = place(d["qbuf"]), place(d["bias_k"])
    inputs = dict(qbuf=qbuf, bias_k=bias_k, kvs=kvs, idx=idx, inv=inv, pe=pe, fxy=fxy, fyw=fyw)
    args = (qbuf, lay["q_off"], lay["qt_off"], bias_k, d["n"], d["S"], segs, out, flag, fxy, fyw)
    return args, dict(drop=drop, fold=fold_image), inputs


def shape_case(n, S, segs, form="rel", p=0.0, kv16=False, fold=False, **kw):
    """A case dict of host tensors nobody reads (torch.empty): what the form query needs."""
    lay = B._layout(kw.get("layout"), len(segs))
    d = dict(kw, n=n, S=S, segs=segs, form=form, p=p, kv16=kv16, fold=fold, lay=lay, rows=n * S, n_tgt=[s[0] for s in segs],
             k=[s[1] for s in segs], div=[s[2] for s in segs], qbuf=torch.empty(n * S, lay["ldq"]), bias_k=torch.empty(D), kvs_in=[], idx=[],
             inv=[], pe=[])
    for i, (T, K, div) in enumerate(segs):
        d["kvs_in"].append(torch.empty(n // div * T, lay["kv"][i][0]))
        d["idx"].append(torch.empty(n, S, K, dtype=torch.int32))
        d["inv"].append(torch.empty(n, S, K, dtype=torch.uint8))
        d["pe"].append(torch.empty(n, S, K, DR if form == "emb" else 3))
    return d


def form_of(hip, d):
    """hip.knarpe_attn_form of a case on host tensors of its shapes."""
    out = torch.empty(d["rows"], D if d["fold"] else d["lay"]["ldo"])
    flag = torch.empty(d["rows"], dtype=torch.uint8)
    img = torch.empty(fold_image_floats()) if d["fold"] else None
    args, kw, _ = launch_args(d, lambda t: t, img, out, flag, hip)
    return hip.knarpe_attn_form(*args, **kw)

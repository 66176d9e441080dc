"""tbx_knarpe_attn_fwd in every launch form csrc/attn.hip dispatches to by default - 4 waves per row, a wave per row (plain, batch-major,
the persistent folded quad loop), the LDS ring; fp32 and bf16 tables, with and without dropout, with and without the value fold -
against ONE float64 evaluation of the factorised formula of include/tbx_hip.h (K6), at the edges where this family goes wrong: slots
64..127, a segment boundary that is no multiple of 8, K = 1 and ktot = 128, a ragged last quad with a row without a valid target in
it, shared tables with and without the batch-major order, grids that are no multiple of 8 under the XCD map, the folded form's spare
waves, the dropout mask of high slots. Cases, reference and tolerances: tests/attn_fwd_cases.py.

Every case records the form code it exists for, and tbx_knarpe_attn_fwd_form - the launchers' own decision - is asked for it on the CPU
(test_cases_take_their_forms) and again on the GPU before the launch: a case that no longer reaches its form fails, it does not pass
in silence. The GPU test prints, per case, the kernel's worst error in units of its bound next to the fp32 CPU evaluation's
(profiles/MEASUREMENT_LOG.md, "Attention forward: float64 reference sweep")."""
from importlib import import_module

import pytest
import torch

import attn_fwd_cases as K
from attn_fwd_cases import BATCH_MAJOR, DROP, FOLD, FOLD_LOOP, FORM_MASK, KV16, RING, SPLIT4, WAVE, XCD


def _hip():
    return import_module("trafficbots_amd.hip")


def _name(code):
    flags = [n for n in ("DROP", "KV16", "FOLD", "FOLD_LOOP", "BATCH_MAJOR", "XCD") if code & getattr(K, n)]
    return "|".join([{SPLIT4: "SPLIT4", WAVE: "WAVE", RING: "RING"}.get(code & FORM_MASK, str(code))] + flags) if code > 0 else str(code)


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_cases_take_their_forms(tb):
    """tbx_knarpe_attn_fwd_form on host tensors of each case's shapes returns exactly the code the case records; the neighbours of the
    thresholds flip it; bf16 tables never take the ring by default; the combinations no kernel is built for return the call's error."""
    hip = _hip()
    names = ("SPLIT4", "WAVE", "RING", "MASK", "DROP", "KV16", "FOLD", "FOLD_LOOP", "BATCH_MAJOR", "XCD")
    assert [getattr(hip, "ATTN_FORM_" + n) for n in names] == [SPLIT4, WAVE, RING, FORM_MASK, DROP, KV16, FOLD, FOLD_LOOP, BATCH_MAJOR, XCD]
    import re

    header = dict(re.findall(r"TBX_ATTN_FORM_(\w+) = (\w+)", hip.HEADER_PATH.read_text()))
    assert {n: int(v, 0) for n, v in header.items()} == {n: getattr(hip, "ATTN_FORM_" + n) for n in names}  # the header's values
    for name in K.CASES:
        d = K.make_case(name)
        got = K.form_of(hip, d)
        print(f"attn_fwd_form {name:18s} {d['rows']:5d} rows  {_name(got)}")
        assert got == d["code"], (name, _name(got), _name(d["code"]))
    assert {c["code"] & FORM_MASK for c in K.CASES.values()} == {SPLIT4, WAVE, RING}
    for flag in (DROP, KV16, FOLD, FOLD_LOOP, BATCH_MAJOR, XCD):
        assert any(c["code"] & flag for c in K.CASES.values())

    one = [(40, 12, 1)]
    f = lambda rows, **kw: K.form_of(hip, K.shape_case(1, rows, kw.pop("segs", one), **kw))
    # 4 waves per row below 193 rows without dropout, then the ring up to 1536 rows (relative poses, fp32 tables), then a wave per row
    assert f(192) == SPLIT4 | XCD and f(193) == RING | XCD
    assert f(1536) == RING | XCD and f(1537) == WAVE | XCD
    assert f(192, form="emb") == SPLIT4 | XCD and f(193, form="emb") == WAVE | XCD  # a materialised embedding: never the ring
    two = [(40, 12, 1), (16, 9, 1)]
    for seg_forms in (("emb", "rel"), ("rel", "emb")):  # one segment of the two with an embedding: no ring either
        d = K.shape_case(1, 193, two)
        i = seg_forms.index("emb")
        d["pe"][i] = torch.empty(1, 193, two[i][1], K.DR)
        img, out, flag = None, torch.empty(193, 640), torch.empty(193, dtype=torch.uint8)
        args, kw, _ = K.launch_args(d, lambda t: t, img, out, flag, hip)
        segs = args[6]
        segs[i].emb, segs[i].rel = d["pe"][i], None
        assert hip.knarpe_attn_form(*args, **kw) == WAVE | XCD
    # with dropout: 4 waves per row below 1024 rows, the ring up to 1536, no XCD order
    assert f(1023, p=0.1) == SPLIT4 | DROP and f(1024, p=0.1) == RING | DROP
    assert f(1536, p=0.1) == RING | DROP and f(1537, p=0.1) == WAVE | DROP
    assert f(1023, p=0.1, form="emb") == SPLIT4 | DROP and f(1024, p=0.1, form="emb") == WAVE | DROP
    # bf16 tables: never the ring by default, at any size
    for rows in (192, 193, 1024, 1536, 1537, 4096):
        code = f(rows, kv16=True)
        assert code & FORM_MASK == (SPLIT4 if rows < 193 else WAVE) and code & KV16 and not code & DROP, (rows, _name(code))
    assert f(1024, kv16=True, p=0.1) == -2 and f(64, kv16=True, p=0.1) == -2  # bf16 tables: inference only
    # the folded launcher: a wave per row from 1024 rows, the quad loop past 2 x 256 CUs' workgroups (no GPU here: 256 CUs assumed)
    assert f(1023, fold=True) == SPLIT4 | FOLD | XCD and f(1024, fold=True) == WAVE | FOLD
    assert f(2048, fold=True) == WAVE | FOLD and f(2049, fold=True) == WAVE | FOLD | FOLD_LOOP
    assert f(1024, fold=True, kv16=True) == WAVE | FOLD | KV16
    assert f(64, fold=True, p=0.1) == -2  # the fold: inference only
    # the batch-major order: shared tables and n % 4 == 0, the plain wave-per-row kernel only
    shared = lambda n, S, **kw: K.form_of(hip, K.shape_case(n, S, [(23, 7, 1), (11, 5, 2)], **kw))
    assert shared(4, 50, form="emb") == WAVE | BATCH_MAJOR | XCD and shared(6, 50, form="emb") == WAVE | XCD
    assert shared(4, 50) == RING | XCD and shared(4, 40) == SPLIT4 | XCD and shared(4, 400) == WAVE | BATCH_MAJOR | XCD
    assert shared(4, 400, p=0.2) == WAVE | BATCH_MAJOR | DROP
    # the call's own argument checks, in its order
    d = K.shape_case(1, 8, one)
    args, kw, _ = K.launch_args(d, lambda t: t, None, torch.empty(8, 640), torch.empty(8, dtype=torch.uint8), hip)
    assert hip.knarpe_attn_form(*args[:7], torch.empty(8, 636), args[8], *args[9:], **kw) == -2  # ldo < 640
    assert hip.knarpe_attn_form(*args[:7], torch.empty(8, 644)[:, 1:641], args[8], *args[9:], **kw) == -3  # out not 16-byte aligned
    assert f(8, segs=[(40, 129, 1)]) == -2 and f(8, p=1.0) == -1
    assert hip.load().tbx_knarpe_attn_fwd_form(None) == -1


@pytest.mark.parametrize("defect", K.DEFECTS)
def test_inputs_discriminate_the_defects(tb, defect):
    """The cases' shapes and data can see each class of fault the GPU test exists for: the float64 reference with one defect injected
    into it moves at least one compared element by >= 10 x the case's tolerance, in every case the defect applies to. Nothing is
    launched."""
    hip = _hip()
    hit = [name for name in K.CASES if K.applies(defect, K.make_case(name))]
    assert hit, defect
    for name in hit:
        d = K.make_case(name)
        ref, dead, scale, _ = K.case_reference(name, hip)
        bad, _, _ = K.evaluate(d, hip, torch.float64, defect)
        fig = K.figure(d, bad, ref, scale)
        print(f"attn_fwd_defect {defect:12s} {name:18s} {fig:.3g}")
        assert fig >= 10.0, (defect, name, fig)


def test_defects_cover_the_forms():
    """Host data only: every wave-per-row and ring case with a ragged last quad, every case past 64 slots, both two-segment dropout ...
    - the table of which defect is looked for where, so that a case dropped from CASES is missed here."""
    where = {df: [n for n in K.CASES if K.applies(df, K.make_case(n))] for df in K.DEFECTS}
    assert {"ring_min", "ring_k1", "ring_tb", "wave_emb", "wave_rel", "wave_drop", "fold_wave_1k", "fold_loop"} <= set(where["ragged_quad"])
    assert {"ring_min", "ring_k128", "ring_straddle", "ring_drop", "wave_emb", "kv16_split", "kv16_wave", "fold_split", "fold_wave_1k"} <= set(where["hi_slots"])
    assert where["seg2_slot0"] == ["ring_drop"]
    assert {"ring_straddle", "ring_shared4", "ring_drop", "wave_bm", "wave_shared", "wave_bm_emb", "fold_bm", "fold_bm_1k"} <= set(where["batch_div"])
    assert where["bm_rows"] == ["wave_bm", "wave_bm_emb", "fold_bm_1k"]
    assert where["fold_head0"] == where["fold_no_bias"] == list(K.FOLDED) and len(K.FOLDED) == 9
    assert len(where["kv_unrounded"]) == 6
    for name in K.CASES:  # the inputs' own promises
        d = K.make_case(name)
        for ix, iv, T in zip(d["idx"], d["inv"], d["n_tgt"]):
            assert int(ix.min()) >= 0 and int(ix.max()) < T and bool((ix[..., 0] == 0).all())
            assert bool(iv[0, 2].all()) and bool(iv[-1, -1].all())
            if iv.numel() >= 5000:  # (the two forced rows weigh less)
                assert 0.25 < float(iv.float().mean()) < 0.35


def test_float32_yardstick_of_the_folded_cases(tb):
    """The folded forms' tolerance is not taken from a kernel: C_FOLD is at least 4 x the worst error, in units of 2^-23 * scale, of the
    reference evaluated in float32 on the CPU against its float64 evaluation on the folded cases' inputs - and not more than 8 x, so that
    a bound that has grown loose is seen."""
    hip = _hip()
    fig = {}
    for name in K.FOLDED:
        ref, dead, scale, f32 = K.case_reference(name, hip)
        fig[name] = K.fold_units(f32, ref, scale)
        print(f"attn_fwd_yardstick {name:18s} {fig[name]:.3g}")
        assert not f32[dead].any() and not ref[dead].any() and bool((scale[~dead] > 0).all())
    v = max(fig.values())
    print(f"attn_fwd_yardstick worst {v:.4g} (C_FOLD = {K.C_FOLD})")
    assert v > 0 and 4 * v <= K.C_FOLD <= 8 * v, (v, K.C_FOLD)
    assert abs(v - K.FOLD_YARDSTICK) <= 0.05 * K.FOLD_YARDSTICK, (v, K.FOLD_YARDSTICK)


# ---------------------------------------------------------------------------------------------------------------- GPU
GUARD_ROWS, GUARD_COLS, GUARD_FLAGS, FLAG_SENTINEL = 8, 16, 64, 9


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(K.CASES))
def test_attention_forward_vs_float64_reference(tb, name):
    """hip.knarpe_attn called directly on a case of attn_fwd_cases.CASES: the form code asked of the library on the device is the
    recorded one; the flags equal the reference's rows without a valid target and those rows are exactly 0.0; the output lies within the
    case's bound of the float64 reference (640-wide: rtol 2e-4 / atol 2e-5; folded: C_FOLD * 2^-23 * scale); `out` and the flags are
    views into sentinel-filled allocations - 16 columns past the row, 8 rows before and behind, 64 flag bytes either side - and every
    guard is intact (a spare wave that repeats the last row, or a ragged quad, would show here); a second launch is bit-identical (no
    atomics: an LDS-ring hazard would show); the inputs are unchanged bit for bit. Measured on MI355X: the kernels' worst figure is 0.247
    of the 640-wide bound (`ring_tb`) and 0.256 of the folded one (`fold_loop`) - the fp32 CPU evaluation's own figures (0.246, 0.229).
    The sweep found the folded forms storing the bias instead of zeros in rows without a valid target (fixed in csrc/attn.hip)."""
    dev = torch.device("cuda:0")
    hip = _hip()
    d = K.make_case(name)
    ref, dead, scale, f32 = K.case_reference(name, hip)
    rows, width = d["rows"], (K.D if d["fold"] else K.OUTW)
    ld = (K.D if d["fold"] else d["lay"]["ldo"]) + GUARD_COLS
    img = None
    if d["fold"]:  # as engine.attn_fold_image builds it
        img = hip.packed_weight(d["w_v"].to(dev), d["b_v"].to(dev), groups=K.NH, gemv=True)
        assert img.numel() == K.fold_image_floats()
    img0 = None if img is None else img.clone()

    def buffers():
        big = torch.full((rows + 2 * GUARD_ROWS, ld), K.SENTINEL, device=dev)
        flags = torch.full((rows + 2 * GUARD_FLAGS,), FLAG_SENTINEL, dtype=torch.uint8, device=dev)
        return big, flags, big[GUARD_ROWS:GUARD_ROWS + rows], flags[GUARD_FLAGS:GUARD_FLAGS + rows]

    big, flags, out, flag = buffers()
    args, kw, inputs = K.launch_args(d, lambda t: t.to(dev), img, out, flag, hip)
    code = hip.knarpe_attn_form(*args, **kw)
    assert code == d["code"], (name, _name(code), _name(d["code"]))
    before = {k: [t.clone() for t in (v if isinstance(v, list) else [v])] for k, v in inputs.items()}
    hip.knarpe_attn(*args, **kw)
    big2, flags2, out2, flag2 = buffers()
    hip.knarpe_attn(*args[:7], out2, flag2, *args[9:], **kw)
    torch.cuda.synchronize()
    big, flags, big2, flags2 = big.cpu(), flags.cpu(), big2.cpu(), flags2.cpu()
    got = big[GUARD_ROWS:GUARD_ROWS + rows, :width]
    fig, fig32 = K.figure(d, got, ref, scale), K.figure(d, f32, ref, scale)
    print(f"attn_fwd_sweep {name:18s} {_name(code):28s} {rows:5d} rows  kernel={fig:.4f} fp32ref={fig32:.4f}")
    # flags and exact zeros
    assert torch.equal(flags[GUARD_FLAGS:GUARD_FLAGS + rows], dead.to(torch.uint8))
    assert not got[dead].any() and int(dead.sum()) >= 2 and bool(dead[2]) and bool(dead[-1])
    # guards: the rows before and behind, the columns past the row, the flag bytes either side
    guard = torch.ones_like(big, dtype=torch.bool)
    guard[GUARD_ROWS:GUARD_ROWS + rows, :width] = False
    assert bool((big[guard] == K.SENTINEL).all()), "a guard of `out` was written"
    assert bool((flags[:GUARD_FLAGS] == FLAG_SENTINEL).all()) and bool((flags[GUARD_FLAGS + rows:] == FLAG_SENTINEL).all())
    assert bool((got != K.SENTINEL).all()), "an element of `out` was left unwritten"
    # run to run
    assert torch.equal(big, big2) and torch.equal(flags, flags2)
    # inputs
    for k, v in inputs.items():
        for a, b in zip(v if isinstance(v, list) else [v], before[k]):
            assert torch.equal(a, b), k  # (no NaN among them: equal values are equal bits but for the sign of zero, and randn draws none)
    for k, v in inputs.items():  # ... and they are the case's
        host = {"qbuf": [d["qbuf"]], "bias_k": [d["bias_k"]], "kvs": d["kvs_in"], "pe": d["pe"]}.get(k)
        for a, h in zip(v if isinstance(v, list) else [v], host or []):
            assert torch.equal(a.cpu().float(), h), k
    assert img is None or torch.equal(img, img0)
    assert fig <= 1.0, (name, fig, fig32)

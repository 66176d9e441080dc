"""CPU-only checks of the drop-in boundary: the C-ABI library loads and exports exactly the symbols include/tbx_hip.h and the
topical headers it includes declare, argument validation returns error codes (no compute without a GPU), state-dict layout equals the reference's,
host-side schedules (teacher forcing masks, scene-centric re-keying) equal the oracle's."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest
import torch

from oracle import trafficbots_oracle as O


@pytest.fixture(scope="module")
def hip(tb):
    h = import_module("trafficbots_amd.hip")
    h.load()
    return h


def test_library_exports_every_declared_symbol(hip):
    """One library, one symbol list: the tbx_* functions libtbx_hip.so exports are exactly the entry points include/tbx_hip.h and the four
    topical headers it includes declare - 73 in its own text (ABI 7 as it was laid down + tbx_knarpe_attn_fwd_form) + 1 / 3 / 1 / 1 added
    since -, each bound with argtypes, and the package names no other library."""
    import re
    import subprocess

    lib = hip.load()
    syms = hip.declared_symbols()
    assert set(syms) >= {"tbx_version", "tbx_error_string", "tbx_knn_embed", "tbx_pose_embed", "tbx_knarpe_attn_fwd",
                         "tbx_rowchain", "tbx_rowchain_ex", "tbx_knarpe_attn_bwd", "tbx_agent_prep", "tbx_tl_prep", "tbx_map_prep", "tbx_sim_step",
                         "tbx_rollout_metrics", "tbx_collision_reward_fwd", "tbx_collision_reward_bwd", "tbx_train_chain_bwd_pose",
                         "tbx_loss_shape", "tbx_tf_threshold"}
    nm = subprocess.run(["nm", "-D", "--defined-only", str(hip.LIB_PATH)], check=True, capture_output=True, text=True).stdout
    exported = [l.split()[2] for l in nm.splitlines() if len(l.split()) == 3 and l.split()[1] == "T" and l.split()[2].startswith("tbx_")]
    assert sorted(exported) == sorted(syms) and len(syms) == 79
    # ... counted header by header, each from its own text
    main = hip.HEADER_PATH.read_text()
    decl = r"^(?:int|int64_t|const char\*)\s+(tbx_\w+)\s*\("
    count = lambda txt: len(set(re.findall(decl, txt, flags=re.M)))
    assert count(main) == 73
    for name, n in (("tbx_hip_metrics.h", 1), ("tbx_hip_reward.h", 3), ("tbx_hip_loss.h", 1), ("tbx_hip_tf.h", 1)):
        assert f'#include "{name}"' in main and count((hip.HEADER_PATH.parent / name).read_text()) == n, name
    for s in syms:
        assert hasattr(lib, s), s
        assert getattr(lib, s).argtypes is not None or s in ("tbx_error_string", "tbx_version"), s  # (those two: called with what ctypes infers)
    assert lib.tbx_version() == 7  # (an added entry point changes no existing one: no bump)
    assert lib.tbx_error_string(-2).decode().startswith("shape")
    # no second library: the package's Python names libtbx_hip.so and, for profiling, libtbx_hip_clk.so
    for py in sorted(hip.LIB_PATH.parent.parent.glob("*.py")):
        assert set(re.findall(r"libtbx_hip_\w+\.so", py.read_text())) <= {"libtbx_hip_clk.so"}, py.name


def test_argument_validation_returns_codes_without_a_gpu(hip):
    lib = hip.load()
    # null pointers / bad sizes are rejected before any launch
    assert lib.tbx_knn_embed(None, None, None, None, 1, 1, 1, 1, 1, 1.0, None, None, None, None, None, None, 128, None) == -1
    assert lib.tbx_rowchain(None, 0, 0, 0, 16, 132, None) == -1
    st = (hip.Stage * 1)(hip.Stage(op=hip.OP_LINEAR, src=0, dst=1, k=128, n=128, ld=128))
    assert lib.tbx_rowchain(st, 1, 16, 0, 24, 132, None) == -2      # tile_rows must be 16, 32 or 48
    assert lib.tbx_rowchain(st, 1, 16, 0, 16, 130, None) == -3      # ldw % 4
    assert lib.tbx_rowchain(st, 1, 16, 0, 16, 132, None) == -1      # LINEAR without a weight pointer
    assert lib.tbx_sim_step(None, 7, None, None) == -1
    with pytest.raises(RuntimeError):
        hip.pose_embed(torch.zeros(4, 3), torch.zeros(32), torch.zeros(64), 128)  # CPU tensor: no fallback path


def test_rowchain_refuses_before_launch(hip):
    """check_stage / rowchain_launch of csrc/rowchain.hip return these codes before anything is launched (no GPU here; the pointers are
    never read). ARG = -1, UNSUPPORTED = -2, ALIGN = -3."""
    lib, S = hip.load(), hip.Stage
    P, Q, M = 0x10000, 0x20000, 0x30000  # 16-byte aligned stand-ins for device pointers

    def ex(st, n_rows=16, group_rows=0, tile=16, ldw0=132, ldw1=132, aux=260):
        return lib.tbx_rowchain_ex((S * len(st))(*st), len(st), n_rows, group_rows, tile, ldw0, ldw1, aux, None)

    def live(st, rows=4):
        return lib.tbx_rowchain_live((S * len(st))(*st), len(st), 16, rows, 132, 132, 260, None)

    load2 = dict(op=hip.OP_LOAD, dst=hip.BUF1, n=128, ld=128, src=hip.AUX, src_col=4, reserved=64, ld2=64, p0=P, p2=Q)
    assert ex([S(flags=hip.F_LOAD2, **{**load2, "p0": P + 4})]) == -3                          # LOAD2, misaligned pointer
    assert ex([S(flags=hip.F_LOAD2, **{**load2, "p2": Q + 8})]) == -3
    assert ex([S(flags=hip.F_LOAD2 | hip.F_ACCUM, **load2)]) == -1                             # LOAD2 with ACCUM
    lin = dict(op=hip.OP_LINEAR, src=hip.BUF0, dst=hip.BUF1, k=64, n=64, ld=64, p0=P)
    assert ex([S(flags=hip.F_WPACK | hip.F_ROWZERO, **lin)]) == -1                             # ROWZERO without ROWSKIP
    assert ex([S(flags=hip.F_WPACK | hip.F_ROWSKIP, **lin)]) == -2                             # ROWSKIP without its mask
    assert ex([S(op=hip.OP_STORE, src=hip.BUF0, n=4, ld=8, p0=P, p1=M, reserved=2, div=4, k=16,
                 flags=hip.F_MASKED_SUM | hip.F_OUT_BF16)]) == -2                              # MASKED_SUM into bfloat16
    assert ex([S(op=hip.OP_POOLMAX, src=hip.BUF0, dst=hip.BUF0, n=16, k=32, ld=16, p0=P, flags=hip.F_POOL_KEEP)]) == -1  # POOL_KEEP, dst == src
    assert ex([S(op=hip.OP_LAYERNORM, src=hip.BUF0, dst=hip.BUF0, n=516, p0=P, p1=Q)], ldw0=520, ldw1=520) == -2  # LAYERNORM wider than 512
    assert ex([S(flags=hip.F_WPACK, **{**lin, "dst": hip.BUF0, "dst_col": 48})]) == -2         # in place, columns overlap (k = 64)
    assert ex([S(flags=hip.F_WPACK, **{**lin, "dst": hip.BUF0, "k": 20, "dst_col": 16})]) == -2  # ... with the source's pad columns [20, 32)
    assert ex([S(flags=hip.F_WPACK, reserved=2, div=(16 << 16) | 24, **{**lin, "n": 20, "k": 16})]) == -2  # grouped, n % 16 != 0
    gemv = dict(lin, flags=hip.F_WGEMV)
    assert live([S(**gemv), S(op=hip.OP_GROUPMAX, src=hip.BUF1, dst=hip.BUF1, dst_col=64, n=64)]) == -2
    assert live([S(**gemv), S(op=hip.OP_POOLMAX, src=hip.BUF1, n=64, ld=64, p0=Q)]) == -2
    assert live([S(**gemv), S(op=hip.OP_DROPOUT, dst=hip.BUF1, n=64, p0=M, f0=1.0)]) == -2
    assert live([S(flags=hip.F_WPACK, **lin)]) == -2                                           # a LINEAR of a live program must be WGEMV
    assert live([S(**lin)]) == -2
    assert ex([S(**gemv)]) == -2                                                               # ... and only of a live program
    assert live([S(**gemv)], rows=3) == -2
    copy = [S(op=hip.OP_COPY, src=hip.BUF0, dst=hip.BUF1, n=4)]
    assert ex(copy, n_rows=40, group_rows=20, tile=16) == -2                                   # group_rows > tile_rows
    assert ex(copy, n_rows=40, group_rows=11, tile=16) == -1                                   # n_rows % group_rows != 0
    assert ex(copy, tile=48, ldw0=400, ldw1=400) == -2                                         # (400 + 400 + 260) * 48 * 4 B > 160 KiB
    assert ex(copy, tile=16, ldw0=1028, ldw1=1028, aux=512) == -2                              # (1028 + 1028 + 512) * 16 * 4 B > 160 KiB


def test_state_dict_layout_equals_reference(tb, golden_dir):
    M = import_module("trafficbots_amd.models.traffic_bots")
    model = M.TrafficBots(**tb.config.default_model_cfg())
    want = dict(l.split(" ", 1) for l in (golden_dir / "state_dict_keys.txt").read_text().strip().split("\n"))
    got = {k: str(tuple(v.shape)) for k, v in model.state_dict().items()}
    assert got == want
    assert sum(p.numel() for p in model.parameters()) == 10657094
    # a reference-shaped (Lightning-prefixed) checkpoint loads strictly
    W = import_module("trafficbots_amd.pl_modules.waymo_motion")
    wm = W.WaymoMotion(model=tb.config.default_model_cfg(), data_size=tb.synthetic.DATA_SIZE, **tb.config.default_sim_cfg())
    ckpt = {"model." + k: v for k, v in model.state_dict().items()}
    missing, unexpected = wm.load_state_dict(ckpt, strict=True)
    assert not missing and not unexpected
    opt, sch = wm.configure_optimizers()
    assert len(opt[0].param_groups) == 2 and opt[0].param_groups[0]["lr"] == 2e-4


def test_host_schedules_equal_oracle(tb):
    batch = tb.synthetic.make_scene(2, 8, 64, 8, seed=3)
    full = {**batch, **tb.synthetic.to_history_batch(batch)}
    SC = import_module("trafficbots_amd.data_modules.scene_centric").SceneCentricPreProcessing
    for training in (True, False):
        pp = SC(time_step_current=10, tl_mode="lane", navi_mode="dest", dropout_p_history=-1, data_size=tb.synthetic.DATA_SIZE)
        pp.train(training)
        b = pp({k: v.clone() for k, v in full.items()})
        bo = O.scene_centric(full, training=training)
        for k in bo:
            if k.startswith(("sc/", "gt/", "ref/")):
                assert torch.equal(b[k], bo[k]), k
    TF = import_module("trafficbots_amd.utils.teacher_forcing").TeacherForcing
    for cfg in (dict(step_spawn_agent=10, step_warm_start=10), dict(step_spawn_agent=90, step_warm_start=10),
                dict(step_spawn_agent=0, step_warm_start=-1)):
        tf = TF(**cfg)
        tf.init(bo["gt/ag_valid"], bo["gt/ag_pose"], bo["gt/ag_motion"], bo["gt/tl_state"], 0)
        assert torch.equal(tf.ag_teacher_forcing, O.Sim.teacher_forcing_mask(bo["gt/ag_valid"], **cfg))
        ag, tl = tf.get(5, None, None, None)
        assert torch.equal(ag["valid"], tf.ag_teacher_forcing[:, :, 5]) and bool(tl["valid"].all())
        ag, tl = tf.get(200, None, None, None)
        assert not bool(ag["valid"].any()) and not bool(tl["valid"].any())


def test_chain_program_encoding(hip):
    """The Chain builder encodes strides / groups / flags the way include/tbx_hip.h documents (host logic only)."""
    ch = hip.Chain(16, 132)
    w = torch.zeros(256, 128)
    ch._add(op=hip.OP_COPY, src=0, dst=1, n=4)
    st = ch.stages[0]
    assert (st.op, st.src, st.dst, st.n) == (hip.OP_COPY, 0, 1, 4)
    assert C.sizeof(hip.Stage) == 88 and C.sizeof(hip.AttnSeg) == 72


def test_ctypes_mirrors_have_the_layout_gcc_gives_the_header(hip, tmp_path):
    """sizeof of every struct that crosses the C ABI, as gcc lays out include/tbx_hip.h, equals the ctypes mirror's."""
    import subprocess
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    pairs = [("tbx_stage_t", hip.Stage), ("tbx_attn_seg_t", hip.AttnSeg), ("tbx_attn_t", hip.Attn), ("tbx_dec_mid_t", hip.DecMid), ("tbx_dec_layer_t", hip.DecLayer), ("tbx_heads_tail_t", hip.HeadsTail), ("tbx_knn_job_t", hip.KnnJob), ("tbx_pose_embed_job_t", hip.PoseEmbedJob), ("tbx_sim_state_t", hip.SimState),
             ("tbx_train_chain_t", hip.TrainChainArgs), ("tbx_rule_ctx_t", hip.RuleCtx), ("tbx_layer_tile_t", hip.LayerTile),
             ("tbx_heads_tile_t", hip.HeadsTile), ("tbx_window_tile_t", hip.WindowTile), ("tbx_agent_prep_args_t", hip.AgentPrepArgs), ("tbx_tl_rows_t", hip.TlRows), ("tbx_front_t", hip.Front), ("tbx_tl_tail_t", hip.TlTail), ("tbx_pack_job_t", hip.PackJob),
             ("tbx_drop_t", hip.Drop), ("tbx_linear_t", hip.Linear), ("tbx_loss_shape_t", hip.LossShape), ("tbx_tf_threshold_t", hip.TfThreshold)]
    src = tmp_path / "sz.c"
    # ... and offsetof of every field (same names on both sides): runs of same-sized pointers keep sizeof when two fields swap
    fields = [(c, t, f[0]) for c, t in pairs for f in t._fields_]
    src.write_text('#include "tbx_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){' +
                   "".join(f'printf("%zu\\n", sizeof({c}));' for c, _ in pairs) +
                   "".join(f'printf("%zu\\n", offsetof({c}, {f}));' for c, _, f in fields) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", str(root / "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[:len(pairs)] == [C.sizeof(t) for _, t in pairs]
    for (c, t, f), off in zip(fields, out[len(pairs):]):
        assert getattr(t, f).offset == off, (c, f, getattr(t, f).offset, off)


def test_python_dropout_rule_equals_drop_key_header(hip, tmp_path):
    """csrc/drop_key.h - the one definition of the keyed-dropout mask - compiled by a plain g++ (no HIP), against its Python restatement
    in hip_base: (thresh, scale) of p, the stream key of (seed, site, step), the hash, the row key, and hip_train.dropout_keep_mask."""
    import subprocess
    from pathlib import Path
    B, T = import_module("trafficbots_amd.hip_base"), import_module("trafficbots_amd.hip_train")
    root = Path(__file__).resolve().parent.parent
    ps = [0.05, 0.1, 0.15, 0.2, 0.3, 0.5, 0.999, 1e-11]
    keys = [(0, 0, 0), (1, 2, 3), (0x0123456789ABCDEF, 7, 90), (2**64 - 1, 0xFFFFFFFF, 0xFFFFFFFF), (-5 % 2**64, 41, 10), (977, 1000003, 79)]
    counters = [0, 1, 2, 3, 127, 128, 511, 512, 65535, 65536, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF, 123456789, 3141592653]
    rows = [(0, 1, 1, 0), (5, 1, 1, 3), (17, 4, 1, 0), (17, 4, 3, 2), (1000, 7, 5, 11), (2_000_000_123, 640, 80, 10)]  # row, rows_per_scene, time_batch, time0
    seed, call, step, p_mask, shape = 0x5DEECE66D, 3, 12, 0.1, (5, 4, 24)  # dropout_keep_mask's (n_rows, n_head, k_tot)
    arr = lambda name, ty, vals: f"const {ty} {name}[] = {{" + ", ".join(vals) + "};\n"
    src = tmp_path / "dk.cpp"
    src.write_text('#include "drop_key.h"\n#include <stdio.h>\nusing namespace tbx_drop;\n' +
                   arr("ps", "float", [repr(p) + "f" for p in ps]) + arr("cs", "uint32_t", [f"{c}u" for c in counters]) +
                   arr("ks", "uint64_t", [f"{v}ull" for k in keys for v in k]) + arr("rs", "int64_t", [f"{v}ll" for r in rows for v in r]) +
                   "int main() {\n"
                   "  for (float p : ps) { const Rate r = drop_rate(p); printf(\"%u %.9g\\n\", r.thresh, r.scale); }\n"
                   f"  for (int i = 0; i < {len(keys)}; ++i) {{\n"
                   "    const StreamKey k = stream_key(ks[3 * i], (uint32_t)ks[3 * i + 1], (uint32_t)ks[3 * i + 2]);\n"
                   "    printf(\"%u %u\\n\", k.lo, k.hi);\n"
                   "    for (uint32_t c : cs) printf(\"%u\\n\", drop_mix(c, k.lo, k.hi));\n  }\n"
                   f"  for (int i = 0; i < {len(rows)}; ++i) {{\n"
                   "    const int64_t* r = rs + 4 * i;\n"
                   "    const RowKey a = row_key<int64_t>(r[0], (int)r[1], (int)r[2], (int)r[3]), b = row_key<uint32_t>((uint32_t)r[0], (int)r[1], (int)r[2], (int)r[3]);\n"
                   "    const RowKey c = row_key<int>((int)r[0], (int)(r[0] / r[1]), (int)r[1], (int)r[2], (int)r[3]);\n"
                   "    printf(\"%u %u %u %u %u %u\\n\", a.step, a.scene_row, b.step, b.scene_row, c.step, c.scene_row);\n  }\n"
                   f"  const StreamKey k = stream_key({seed}ull, {call}u, {step}u);\n"
                   f"  for (uint32_t row = 0; row < {shape[0]}; ++row) for (uint32_t h = 0; h < {shape[1]}; ++h) for (uint32_t t = 0; t < {shape[2]}; ++t)\n"
                   f"    printf(\"%d\\n\", (int)(drop_mix((row * 128u + t) * 4u + h, k.lo, k.hi) >= drop_rate({p_mask!r}f).thresh));\n"
                   "  return 0;\n}\n")
    exe = tmp_path / "dk"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", str(root / "trafficbotsv1.5_amd" / "csrc"), str(src), "-o", str(exe)], check=True)
    out = iter(subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n"))
    for p in ps:
        th, sc = next(out).split()
        got = B.drop_rate(p)
        assert (int(th), np.float32(float(sc))) == (got[0], np.float32(got[1])), (p, th, sc, got)
    assert B.drop_rate(0.1)[0] == 429496736 and B.drop_rate(1e-11)[0] == 1 and B.drop_rate(0.0) == (0, 1.0)
    for k in keys:
        lo, hi = (int(v) for v in next(out).split())
        assert B.drop_stream_key(*k) == (lo, hi), k
        want = [int(next(out)) for _ in counters]
        assert B.drop_mix(np.array(counters, dtype=np.uint32), lo, hi).tolist() == want, k
    for row, rps, tb_, t0 in rows:  # batch entry b = row // rps is step t0 + b % time_batch of scene b // time_batch
        b = row // rps
        assert [int(v) for v in next(out).split()] == [t0 + b % tb_, (b // tb_) * rps + row % rps] * 3, (row, rps, tb_, t0)
    want = torch.tensor([int(next(out)) for _ in range(shape[0] * shape[1] * shape[2])], dtype=torch.bool).view(shape)
    got = T.dropout_keep_mask(seed, call, shape[0], shape[2], p_mask, n_head=shape[1], step=step)
    assert got.dtype == torch.bool and torch.equal(got, want) and 0 < int((~want).sum()) < want.numel() // 2


def test_new_entry_points_validate_arguments_without_a_gpu(hip):
    lib = hip.load()
    assert lib.tbx_keyed_dropout(None, None, 4, 4, C.byref(hip.Drop(seed=None, p=0.1, site=0, rows_per_scene=2, time_batch=1, time0=0)), None) == -1
    assert lib.tbx_linear_wgrad_splits(0, 128, 128) == -1
    assert 1 <= lib.tbx_linear_wgrad_splits(2_000_000, 128, 128) <= 1024
    assert lib.tbx_linear_wgrad_splits(100, 128, 128) == 2  # at least 64 rows per split
    assert lib.tbx_linear_wgrad(None, 128, None, 128, 1000, 128, 128, None, None, None, 4, None) == -1
    assert lib.tbx_train_chain_fwd(None, None, 0, 0, 0, 1, None) == -1
    args = hip.TrainChainArgs()
    args.n_batch, args.n_ag, args.n_step, args.n_step_gt, args.n_node, args.window = 1, 4, 10, 11, 20, 11
    assert lib.tbx_train_chain_fwd(C.byref(args), None, 8, 0, 0, 1, None) == -1  # null state pointers
    assert lib.tbx_train_chain_bwd(C.byref(args), None, 8, 8, None, None, None) == -1


def test_knn_inverse_validates_its_arguments_without_a_gpu(hip):
    """tbx_knn_inverse calls that must be refused BEFORE any launch (placeholder device addresses, never dereferenced)."""
    lib = hip.load()
    ARG, UNSUPPORTED = -1, -2
    dp = lambda i: 0x10000 * (i + 1)

    def f(n_batch=6, n_src=7, k=9, n_tgt=16, div=3, idx=dp(0), invalid=dp(1), ptr=dp(2), lst=dp(3)):
        return lib.tbx_knn_inverse(idx, invalid, n_batch, n_src, k, n_tgt, div, ptr, lst, None)

    assert f(n_tgt=2049) == UNSUPPORTED                       # one workgroup scans a table's counts in LDS: n_tgt <= 2048
    assert f(n_batch=7) == ARG and f(n_batch=2) == ARG        # n_batch % tgt_batch_div != 0
    assert f(n_batch=7, n_tgt=2049) == ARG                    # (precedence: the arguments before the shape)
    assert f(n_batch=3 << 20, n_src=64, k=128) == UNSUPPORTED  # pair ids are 32-bit
    for bad in (dict(idx=None), dict(invalid=None), dict(ptr=None), dict(lst=None), dict(n_batch=0), dict(n_src=0), dict(k=0), dict(n_tgt=0),
                dict(div=0)):
        assert f(**bad) == ARG, bad


def test_attention_entry_points_validate_their_argument_struct_without_a_gpu(hip):
    """tbx_knarpe_attn_fwd / _fwd_mfma / _bwd on tbx_attn_t structs that must be refused BEFORE any launch (placeholder device
    addresses, never dereferenced), with the codes the positional entry points gave for the same arguments: the checks of the query
    side and the segments, the dropout fields, and what each entry point adds."""
    lib = hip.load()
    ARG, UNSUPPORTED, ALIGN = -1, -2, -3
    dp = lambda i: 0x10000 * (i + 1)  # 16-byte aligned, distinct
    fwd, mfma, bwd = lib.tbx_knarpe_attn_fwd, lib.tbx_knarpe_attn_fwd_mfma, lib.tbx_knarpe_attn_bwd

    def args(**kw):  # a well-formed call of every entry point (relative-pose segments, the atomics backward), then the changes
        a = hip.Attn(qbuf=dp(0), rpe_k_bias=dp(1), freqs_xy=dp(2), freqs_yaw=dp(3), out=dp(4), row_no_valid=dp(5), dout=dp(6), dqbuf=dp(7),
                     dbias_k=dp(8), ldq=896, q_off=0, qt_off=128, n_batch=2, n_src=4, n_seg=2, ldo=640, time_batch=1)
        for i, k in enumerate((24, 64)):
            a.seg[i] = hip.AttnSeg(kv=dp(10 + i), idx=dp(12 + i), invalid=dp(14 + i), rel_pose=dp(16 + i), ld_kv=256, k_off=0, v_off=128,
                                   n_tgt=100, batch_div=1, k=k)
            a.dkv[i] = dp(18 + i)
        for name, v in kw.items():
            obj, _, field = name.rpartition("__")  # seg0__k -> a.seg[0].k
            setattr(a.seg[int(obj[3:])] if obj else a, field, v)
        return C.byref(a)

    for f in (fwd, mfma, bwd):
        assert f(None, None) == ARG
        assert f(args(qbuf=None), None) == ARG
        assert f(args(n_batch=0), None) == ARG
        assert f(args(n_seg=3), None) == UNSUPPORTED
        assert f(args(n_seg=0), None) == UNSUPPORTED
        assert f(args(ldo=636), None) == UNSUPPORTED
        assert f(args(seg0__k=65), None) == UNSUPPORTED          # 65 + 64 targets
        assert f(args(ldq=898), None) == ALIGN
        assert f(args(seg1__kv=None), None) == ARG
        assert f(args(seg1__kv=dp(11) + 8), None) == ALIGN
        assert f(args(seg1__kv_bf16=1), None) == UNSUPPORTED     # one element type per call
        assert f(args(p_drop=1.0), None) == ARG
        assert f(args(p_drop=-0.5), None) == ARG
        assert f(args(time_batch=0), None) == ARG
        assert f(args(time0=-1), None) == ARG
        assert f(args(p_drop=0.1), None) == ARG                  # dropout without a seed
        assert f(args(n_seg=3, qbuf=dp(0) + 4), None) == UNSUPPORTED  # (precedence: the shape before the alignment)
    for f in (fwd, bwd):
        assert f(args(rpe_k_bias=None), None) == ARG
        assert f(args(freqs_xy=None), None) == ARG                # a relative-pose segment needs the frequencies
        assert f(args(seg0__rel_pose=None), None) == ARG          # neither embedding nor relative pose
        assert f(args(seg0__emb=dp(20) + 4), None) == ALIGN
    # the forward entry points: outputs
    for f in (fwd, mfma):
        assert f(args(out=None), None) == ARG
        assert f(args(row_no_valid=None), None) == ARG
        assert f(args(out=dp(4) + 4), None) == ALIGN
    assert fwd(args(out=dp(4) + 4, n_seg=3), None) == ALIGN       # the VALU forward looks at `out` first ...
    assert mfma(args(out=dp(4) + 4, n_seg=3), None) == UNSUPPORTED  # ... the matrix-core forward at the shape
    assert fwd(args(p_drop=0.1, drop_seed=dp(21), seg0__kv_bf16=1, seg1__kv_bf16=1), None) == UNSUPPORTED  # bf16 tables: no dropout
    # the value fold: its own row width, and no dropout
    assert fwd(args(fold_image=dp(22), ldo=128, p_drop=0.1, drop_seed=dp(21)), None) == UNSUPPORTED
    assert fwd(args(fold_image=dp(22) + 4, ldo=128), None) == ALIGN
    assert fwd(args(fold_image=dp(22), ldo=64), None) == ALIGN
    assert fwd(args(fold_image=dp(22), ldo=128, n_seg=3), None) == UNSUPPORTED
    # the matrix-core forward: relative-pose segments only, frequencies always, K/V columns in 8-element steps, 32-bit table offsets
    assert mfma(args(seg0__emb=dp(20)), None) == UNSUPPORTED
    assert mfma(args(seg0__emb=dp(20), seg0__rel_pose=None), None) == ARG
    assert mfma(args(freqs_yaw=None, n_seg=3), None) == ARG
    assert mfma(args(seg1__v_off=132), None) == ALIGN
    assert mfma(args(seg0__n_tgt=1 << 22), None) == UNSUPPORTED
    assert mfma(args(seg0__emb=dp(20), seg0__k_off=4), None) == UNSUPPORTED  # (precedence: the form before the alignment)
    # the backward: gradients, fp32 tables only, the inverse lists of the form without atomics
    assert bwd(args(dout=None), None) == ARG
    assert bwd(args(dqbuf=dp(7) + 8), None) == ALIGN
    assert bwd(args(seg0__kv_bf16=1, seg1__kv_bf16=1), None) == UNSUPPORTED
    assert bwd(args(dkv=(C.c_void_p * 2)(dp(18), None)), None) == ARG
    assert bwd(args(coef=dp(23)), None) == ARG                    # no inverse lists
    assert bwd(args(coef=dp(23), inv_ptr=(C.c_void_p * 2)(dp(24), dp(25)), inv_list=(C.c_void_p * 2)(dp(26), None)), None) == ARG
    assert bwd(args(coef=dp(23), inv_ptr=(C.c_void_p * 2)(dp(24), dp(25)), inv_list=(C.c_void_p * 2)(dp(26), dp(27)), n_batch=3, seg1__batch_div=2),
               None) == ARG


def test_dropout_and_tall_linear_structs_are_validated_without_a_gpu(hip):
    """tbx_drop_t / tbx_linear_t calls that must be refused BEFORE any launch (placeholder device addresses, never dereferenced): the
    rules the structs add, the shared key set-up (csrc/drop_key.h make_key) behind every entry point that takes a tbx_drop_t, and each of
    the six positional tall-LINEAR call shapes (plain, dual, relu_drop; each also as _bf16) written as a struct, with the code the
    positional entry point gave for the same bad input."""
    lib = hip.load()
    ARG, UNSUPPORTED, ALIGN = -1, -2, -3
    dp = lambda i: 0x10000 * (i + 1)  # 16-byte aligned, distinct
    drop = lambda **kw: hip.Drop(**{**dict(seed=dp(9), p=0.1, site=3, rows_per_scene=64, time_batch=1, time0=0), **kw})

    def lin(drop_=None, **kw):  # a well-formed plain call (128 rows of 128 -> 128), then the changes
        a = hip.Linear(**{**dict(x=dp(0), image=dp(1), y=dp(2), m=128, k=128, ldx=128, n=128, has_bias=1, relu=0, ldy=128), **kw})
        if drop_ is not None:
            a.drop = drop_
        return C.byref(a)

    for f in (lib.tbx_tall_linear, lib.tbx_tall_linear_bf16):
        assert f(None, None) == ARG                                                  # a NULL struct
        assert f(lin(drop(), relu=0), None) == ARG                                   # drop.p > 0 without relu
        assert f(lin(drop(), relu=1, y16=dp(3), ldy16=128), None) == UNSUPPORTED     # drop.p > 0 with y16
        assert f(lin(drop(p=1.0), relu=1), None) == ARG                              # p >= 1
        assert f(lin(drop(p=1.5), relu=1), None) == ARG
        assert f(lin(drop(rows_per_scene=48), relu=1), None) == ARG                  # rows % rows_per_scene != 0
        # the plain shape (tbx_tall_linear, _bf16)
        assert f(lin(x=None), None) == ARG
        assert f(lin(m=0), None) == ARG
        assert f(lin(k=100), None) == UNSUPPORTED
        assert f(lin(n=1088), None) == UNSUPPORTED
        assert f(lin(ldx=64), None) == ARG
        assert f(lin(ldy=130), None) == ARG
        assert f(lin(y=dp(2) + 4), None) == ALIGN
        assert f(lin(k=100, y=dp(2) + 4), None) == UNSUPPORTED                       # (precedence: the shape before the alignment)
        # the dual shape (tbx_tall_linear_dual, _bf16)
        assert f(lin(y16=dp(3), ldy16=64), None) == ALIGN
        assert f(lin(y16=dp(3), ldy16=130), None) == ALIGN
        assert f(lin(y16=dp(3) + 4, ldy16=128), None) == ALIGN
        assert f(lin(y16=dp(3), ldy16=128, ldx=64), None) == ARG                     # (precedence: the fp32 side first)
        # the relu_drop shape (tbx_tall_linear_relu_drop, _bf16: relu = 1)
        assert f(lin(drop(p=-0.5), relu=1), None) == ARG
        assert f(lin(drop(p=-0.5), relu=1, k=100), None) == ARG                      # (precedence: p < 0 before everything else)
        assert f(lin(drop(seed=None), relu=1), None) == ARG
        assert f(lin(drop(time_batch=0), relu=1), None) == ARG
        assert f(lin(drop(time0=-1), relu=1), None) == ARG
        assert f(lin(drop(rows_per_scene=0), relu=1), None) == ARG
        assert f(lin(drop(p=1.0), relu=1, k=100), None) == UNSUPPORTED               # (precedence: the shape before the key)
        assert f(lin(drop(), relu=1, m=1 << 31, ldx=128), None) == UNSUPPORTED       # 32-bit row arithmetic under dropout ...
        assert f(lin(drop(rows_per_scene=48), relu=1, m=1 << 31), None) == ARG       # ... after the key's own checks
    # the entry points that take a tbx_drop_t: same key rules behind each one's own checks
    x, y, o = dp(0), dp(1), dp(2)
    bad_keys = (drop(p=1.0), drop(seed=None), drop(rows_per_scene=48), drop(rows_per_scene=0), drop(time_batch=0), drop(time0=-1))
    for d in bad_keys:
        assert lib.tbx_keyed_dropout(x, y, 128, 128, C.byref(d), None) == ARG
        assert lib.tbx_residual_drop_fwd(x, y, None, None, 128, 128, C.byref(d), o, None) == ARG
        assert lib.tbx_residual_drop_bwd(x, None, None, 128, 128, C.byref(d), y, o, None) == ARG
        assert lib.tbx_relu_drop_fwd(x, 128, 128, C.byref(d), o, None) == ARG
        assert lib.tbx_pointnet_tail_fwd(x, y, 8, 16, 64, C.byref(d), o, None) == ARG
    neg = C.byref(drop(p=-0.5))
    assert lib.tbx_keyed_dropout(x, y, 128, 128, None, None) == ARG                  # this call IS the dropout: no key, p <= 0
    assert lib.tbx_keyed_dropout(x, y, 128, 128, C.byref(drop(p=0.0)), None) == ARG
    assert lib.tbx_keyed_dropout(x, y, 128, 128, neg, None) == ARG
    for seed in (dp(9), None):  # a NaN p is not > 0 either: refused, never a launch on the neutral key (whose seed is NULL)
        assert lib.tbx_keyed_dropout(x, y, 128, 128, C.byref(drop(p=float("nan"), seed=seed)), None) == ARG
    assert lib.tbx_keyed_dropout(x, y, 0, 128, C.byref(drop()), None) == 0            # an empty tensor, after a good key
    assert lib.tbx_keyed_dropout(x, y, 0, 128, C.byref(drop(p=1.0)), None) == ARG
    assert lib.tbx_residual_drop_fwd(x, y, None, None, 128, 128, neg, o, None) == ARG
    assert lib.tbx_relu_drop_fwd(x, 128, 128, neg, o, None) == ARG
    # the glue ops' own precedence: pointers, alignment, shape, an empty tensor, then the key
    assert lib.tbx_relu_drop_fwd(None, 128, 128, C.byref(drop(p=1.0)), o, None) == ARG
    assert lib.tbx_relu_drop_fwd(x + 4, 128, 126, C.byref(drop(p=1.0)), o, None) == ALIGN
    assert lib.tbx_relu_drop_fwd(x, 128, 126, C.byref(drop(p=1.0)), o, None) == UNSUPPORTED
    assert lib.tbx_relu_drop_fwd(x, 0, 128, C.byref(drop(p=1.0)), o, None) == 0
    assert lib.tbx_relu_drop_fwd(x, 0, 128, None, o, None) == 0
    assert lib.tbx_residual_drop_bwd(x, None, None, 128, 128, C.byref(drop(p=1.0)), y, o + 4, None) == ALIGN
    # PointNet tail: pointers, the shape, then the key
    assert lib.tbx_pointnet_tail_fwd(x, None, 8, 16, 64, C.byref(drop(p=1.0)), o, None) == ARG
    assert lib.tbx_pointnet_tail_fwd(x, y, 8, 33, 64, C.byref(drop(p=1.0)), o, None) == UNSUPPORTED
    assert lib.tbx_pointnet_tail_fwd(x, y, 8, 16, 64, C.byref(drop(rows_per_scene=24)), o, None) == ARG  # 128 rows % 24


def test_group_tile_rows_picks_the_least_wasteful_tile(hip):
    assert hip.group_tile_rows(11, 64) == 16          # small grid: one window per 16-row tile (shortest critical path)
    assert hip.group_tile_rows(11, 4096) == 48        # 4 windows in 48 rows (92 %) beat 2 in 32 (69 %)
    assert hip.group_tile_rows(20, 4096) == 48        # 2 polylines in 48 rows beat 1 in 32
    assert hip.group_tile_rows(20, 100) == 32
    assert hip.group_tile_rows(16, 4096) == 32        # 2 x 16 fills 32 rows exactly
    assert hip.group_tile_rows(5, 4096) == 32         # 6 in 32 (94 %) vs 9 in 48 (94 %): the smaller tile


def test_lights_per_scene_view_of_expanded_light_tokens(tb):
    """RolloutEngine steps the lights once per scene: the per-scene view of tokens that encode_scene expanded per rollout."""
    E = import_module("trafficbots_amd.utils.rollout_engine")
    n_scene, K, L, M = 3, 4, 5, 7
    g = torch.Generator().manual_seed(0)
    per_scene = {"tl_token_pose": torch.randn(n_scene, L, 3, generator=g), "tl_token_valid": torch.rand(n_scene, L, generator=g) > 0.3,
                 "knn_idx_tl2mp": torch.randint(0, M, (n_scene, L, 2), generator=g), "tl_token_attr": torch.randn(n_scene, L, 8, generator=g)}
    expanded = {k: v.repeat_interleave(K, 0) for k, v in per_scene.items()}
    expanded.update(mp_batch_div=K, n_mp=M, mp_feat_flat=torch.randn(n_scene * M, 8, generator=g), _kv_mp={"cached": 1})
    view = E.lights_per_scene(expanded, K)
    for k, v in per_scene.items():
        assert torch.equal(view[k], v), k
    assert view["mp_batch_div"] == 1 and view["tl_batch_div"] == K and view["ag_mp_batch_div"] == K and view["n_mp"] == M
    assert view["mp_feat_flat"] is expanded["mp_feat_flat"] and "_kv_mp" not in view


def test_tl_nll_all_steps_equals_the_per_step_loop(tb):
    """train_graph.tl_nll_all_steps (waymo_motion.py:270-283 for every step at once) vs the step loop with Categorical."""
    TG = import_module("trafficbots_amd.train_graph")
    from torch.distributions import Categorical

    g = torch.Generator().manual_seed(1)
    n, T, L, Tt = 2, 12, 5, 9  # ground truth ends before the rollout does
    logits = torch.randn(n, T, L, 5, generator=g)
    tl_gt = torch.nn.functional.one_hot(torch.randint(0, 5, (n, L, Tt), generator=g), 5).bool()
    inv = torch.rand(n, L, generator=g) < 0.3
    nll, nll_inv = TG.tl_nll_all_steps(logits, tl_gt, inv)
    for step in range(1, T + 1):
        if step < Tt:
            want = -Categorical(logits=logits[:, step - 1]).log_prob(tl_gt[:, :, step].max(-1)[1])
            torch.testing.assert_close(nll[:, :, step - 1], want)
            assert torch.equal(nll_inv[:, :, step - 1], inv)
        else:
            assert float(nll[:, :, step - 1].abs().max()) == 0.0 and bool(nll_inv[:, :, step - 1].all())


def test_graphed_train_step_refuses_without_the_ordered_memset_path(tb, monkeypatch):
    """hipGraph memset nodes replay out of order on ROCm's AQL-packet fast path (stale bias gradients): GraphedTrainStep must
    refuse to capture unless DEBUG_CLR_GRAPH_PACKET_CAPTURE=0 was in the environment (pl_modules/data_parallel.py)."""
    from importlib import import_module

    import pytest

    DP = import_module("trafficbots_amd.pl_modules.data_parallel")
    for bad in (None, "1", ""):
        if bad is None:
            monkeypatch.delenv("DEBUG_CLR_GRAPH_PACKET_CAPTURE", raising=False)
        else:
            monkeypatch.setenv("DEBUG_CLR_GRAPH_PACKET_CAPTURE", bad)
        with pytest.raises(RuntimeError, match="DEBUG_CLR_GRAPH_PACKET_CAPTURE=0"):
            DP.GraphedTrainStep(object(), object(), {})


def test_schedule_switches_follow_the_environment_and_replace(tb, monkeypatch):
    """engine.Schedule: every boolean switch is on by default except the opt-ins (measured slower: front_big, attn_fold_big, pool_proj;
    a different arithmetic: kv_bf16, split_bf16, attn_mfma, linear_bf16), `TBX_<NAME>=0 / 1` flips it in from_env(), replace() leaves the original alone, and a
    schedule is a value (two equal ones compare equal: engines are cached by it)."""
    import dataclasses
    from importlib import import_module

    E = import_module("trafficbots_amd.engine")
    for k in list(__import__("os").environ):
        if k.startswith("TBX_"):
            monkeypatch.delenv(k)
    d = E.Schedule.from_env()
    off = {"front_big", "attn_fold_big", "pool_proj", "kv_bf16", "split_bf16", "attn_mfma", "linear_bf16"}
    bools = [f.name for f in dataclasses.fields(E.Schedule) if isinstance(getattr(d, f.name), bool)]
    assert {"knn_aux_big", "prime_graph", "fused_tail", "front_fused", "dec_tail_mfma", "front_big"} <= set(bools)
    for name in bools:
        assert getattr(d, name) == (name not in off), name
    assert d == E.Schedule.from_env() and hash(dataclasses.astuple(d)) == hash(dataclasses.astuple(E.Schedule.from_env()))
    for name, env in (("knn_aux_big", "TBX_KNN_AUX_BIG"), ("prime_graph", "TBX_PRIME_GRAPH"), ("fused_tail", "TBX_FUSED_TAIL")):
        monkeypatch.setenv(env, "0")
        assert getattr(E.Schedule.from_env(), name) is False
        monkeypatch.delenv(env)
    monkeypatch.setenv("TBX_FRONT_BIG", "1")
    assert E.Schedule.from_env().front_big is True
    r = d.replace(knn_aux_big=False)
    assert r.knn_aux_big is False and d.knn_aux_big is True and r != d


def test_training_metrics_class_equals_the_captured_steps_loss(tb):
    """models/metrics/training.py::TrainingMetrics (the reference-shaped accumulator: update(buffer, ...) / compute()) and
    train_graph.training_loss (the fused expression the captured training step uses, itself checked against the reference's golden
    loss dict in tests/test_hip_training.py) give the same numbers on the same rollout log - both switch settings of
    loss_for_teacher_forcing, and a batch without a valid light drops its term the way the reference's `if counter > 0` does."""
    from importlib import import_module
    from types import SimpleNamespace

    TG = import_module("trafficbots_amd.train_graph")
    TM = import_module("trafficbots_amd.models.metrics.training")
    D = import_module("trafficbots_amd.models.modules.distributions")
    g = torch.Generator().manual_seed(0)
    n, A, T, L, M = 3, 9, 30, 5, 20
    r = lambda *s: torch.rand(*s, generator=g)
    for tf_loss, no_lights in ((True, False), (False, False), (True, True)):
        cfg = tb.config.default_sim_cfg()["training_metrics"]
        cfg["loss_for_teacher_forcing"] = tf_loss
        ro = dict(pred_valid=r(n, A, T) < 0.8, tf=r(n, A, T) < 0.2, reward_valid=r(n, A, T) < 0.9, reward=-r(n, A, T),
                  tl_nll_invalid=(r(n, L, T) < 0.3) | no_lights, tl_nll=r(n, L, T))
        post = D.DiagGaussian(torch.randn(n, A, 16, generator=g), torch.randn(n, A, 16, generator=g) * 0.3, valid=r(n, A) < 0.9)
        prior = D.DiagGaussian(torch.zeros(n, A, 16), torch.zeros(16), valid=r(n, A) < 0.8)
        navi = D.DestCategorical(logits=torch.randn(n, A, M, generator=g), valid=r(n, A) < 0.9)
        navi_gt = torch.randint(0, M, (n, A), generator=g)
        want = TG.training_loss(cfg, ro, navi, navi_gt, post, prior)
        buf = SimpleNamespace(pred_valid=ro["pred_valid"], mask_teacher_forcing=ro["tf"], tl_state_nll=ro["tl_nll"],
                              tl_state_nll_invalid=ro["tl_nll_invalid"],
                              diffbar_reward={"diffbar_reward_valid": ro["reward_valid"], "diffbar_reward": ro["reward"]})
        m = TM.TrainingMetrics(prefix="training", train_navi=True, train_latent=True, **cfg)
        got = m(buf, None, navi, navi_gt, post, prior)
        for k in ("loss", "vae_kl", "diffbar_reward", "navi_loss"):
            torch.testing.assert_close(got[f"training/{k}"], want[k], rtol=1e-6, atol=1e-6)
        if no_lights:
            assert "training/tl_state_loss" not in got and float(want["tl_state_loss"]) == 0.0
        else:
            torch.testing.assert_close(got["training/tl_state_loss"], want["tl_state_loss"], rtol=1e-6, atol=1e-6)


def test_multi_tensor_copy_of_the_engine_refill(tb):
    """RolloutEngine._copy_all (the ~80 copies of a scene commit as a few multi-tensor launches): same-dtype contiguous pairs of equal
    shape are grouped by dtype, everything else - dtype conversions, strided views, broadcasts - falls back to copy_, aliased pairs
    are skipped; every destination ends equal to its source."""
    R = import_module("trafficbots_amd.utils.rollout_engine").RolloutEngine
    g = torch.Generator().manual_seed(0)
    f = lambda *s: torch.randn(*s, generator=g)
    same = f(4, 3)
    base = torch.zeros(6, 8)
    pairs = [(torch.zeros(4, 3), f(4, 3)), (torch.zeros(5), f(5)),                                  # float32, contiguous: one group
             (torch.zeros(7, dtype=torch.uint8), (torch.rand(7, generator=g) < 0.5).to(torch.uint8)),  # uint8: another group
             (torch.zeros(2, 3, dtype=torch.int64), torch.randint(0, 9, (2, 3), generator=g)),          # int64
             (torch.zeros(4, dtype=torch.float32), torch.randint(0, 9, (4,), generator=g)),            # conversion: copy_
             (base[:, ::2], f(6, 4)),                                                                 # strided destination: copy_
             (torch.zeros(3, 4), f(1, 4)),                                                            # broadcast source: copy_
             (same, same)]                                                                            # aliased: skipped
    want = [s.clone() for _, s in pairs]
    R._copy_all(pairs)
    for (d, _), w in zip(pairs, want):
        assert torch.equal(d, w.to(d.dtype).expand_as(d))
    R._copy_all([])  # (nothing to do)


def test_training_flags_the_time_batched_step_cannot_honour_raise(tb):
    """training_detach_model_input / training_deterministic_action (waymo_motion.py:158-161, :370): the training step batches the
    decoder over time, exact only with detached inputs and deterministic actions (the defaults). False used to be accepted and
    ignored - plausible, wrong gradients; now the constructor refuses, like every other non-default branch."""
    W = import_module("trafficbots_amd.pl_modules.waymo_motion")
    for flag in ("training_detach_model_input", "training_deterministic_action"):
        scfg = tb.config.default_sim_cfg()
        assert scfg[flag] is True
        scfg[flag] = False
        with pytest.raises(NotImplementedError, match=flag):
            W.WaymoMotion(model=tb.config.default_model_cfg(), data_size=tb.synthetic.DATA_SIZE, **scfg)


def test_dynamics_init_holds_step_zero_until_the_first_forward(tb):
    """The reference's prologue `self.dynamics.init(tl_state=tl_state_gt, **ag_tokens)` (waymo_motion.py:228): between it and the
    first `forward` the state attributes read step 0 of the ground truth (teacher_forcing.get is handed them, :233-235)."""
    W = import_module("trafficbots_amd.pl_modules.waymo_motion")
    wm = W.WaymoMotion(model=tb.config.default_model_cfg(n_tgt_knn=4), data_size=tb.synthetic.DATA_SIZE, **tb.config.default_sim_cfg())
    g = torch.Generator().manual_seed(0)
    n, A, T, L = 2, 5, 11, 3
    tok = dict(gt_valid=torch.rand(n, A, T, generator=g) > 0.2, gt_pose=torch.randn(n, A, T, 3, generator=g), gt_motion=torch.randn(n, A, T, 3, generator=g),
               ag_type=torch.eye(3)[torch.randint(0, 3, (n, A), generator=g)].bool(), ag_attr=torch.randn(n, A, 6, generator=g),
               ag_size=torch.rand(n, A, 3, generator=g), ag_latent=torch.randn(n, A, 16, generator=g), ag_latent_valid=torch.ones(n, A, dtype=torch.bool),
               ag_navi=torch.randint(0, 7, (n, A), generator=g), ag_navi_valid=torch.rand(n, A, generator=g) > 0.5,
               ag_navi_log_prob=torch.zeros(n, A))
    tl = torch.eye(5)[torch.randint(0, 5, (n, L, T), generator=g)].bool()
    dyn = wm.dynamics
    with pytest.raises(RuntimeError):
        dyn.ag_pose
    dyn.init(tl_state=tl, **tok)
    wm.model.init()
    assert torch.equal(dyn.ag_valid, tok["gt_valid"][:, :, 0]) and torch.equal(dyn.ag_pose, tok["gt_pose"][:, :, 0])
    assert torch.equal(dyn.ag_motion, tok["gt_motion"][:, :, 0]) and torch.equal(dyn.tl_state, tl[:, :, 0])
    assert torch.equal(dyn.ag_navi_valid, tok["ag_navi_valid"]) and not dyn.mask_navi_reached.any() and not dyn.ag_disabled.any()
    assert dyn.ag_navi is tok["ag_navi"] and dyn.ag_type is tok["ag_type"]
    with pytest.raises(RuntimeError):  # no engine yet: the reference's order is init -> forward -> disable_*
        dyn.disable_navi({"dest_reached_this_step": torch.zeros(n, A, dtype=torch.bool)})
    tf = wm.teacher_forcing_reactive_replay
    tf.init(ag_valid=tok["gt_valid"], ag_pose=tok["gt_pose"], ag_motion=tok["gt_motion"], tl_state=tl, current_epoch=0)
    ag_override, tl_override = tf.get(1, dyn.ag_valid, dyn.ag_pose, dyn.ag_motion)
    assert ag_override["pose"].shape == (n, A, 3) and tl_override["state"].shape == (n, L, 5)


def test_light_tokens_per_rollout_is_a_copy_with_encode_scenes_layout(tb):
    """joint_future_pred's own expansion of pre_compute's light tokens (the reference's :458-462): every per-light tensor repeated K
    times along the batch, map targets still indexed per scene (mp_batch_div = K), caches dropped, the caller's dict untouched; the
    rollout engine's per-scene view (lights_per_scene) of the result is the original."""
    W = import_module("trafficbots_amd.pl_modules.waymo_motion")
    E = import_module("trafficbots_amd.utils.rollout_engine")
    n_scene, K, L, M = 2, 4, 5, 7
    g = torch.Generator().manual_seed(1)
    tl = {"tl_token_pose": torch.randn(n_scene, L, 3, generator=g), "tl_token_valid": torch.rand(n_scene, L, generator=g) > 0.3,
          "knn_idx_tl2mp": torch.randint(0, M, (n_scene, L, 2), generator=g), "rel_tl2tl": torch.randn(n_scene, L, 2, 3, generator=g),
          "rpe_tl2tl": None, "mp_batch_div": 1, "n_mp": M, "mp_feat_flat": torch.randn(n_scene * M, 8, generator=g), "_kv_mp": {"cached": 1}}
    before = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in tl.items()}
    ex = W.WaymoMotion._tl_tokens_per_rollout(tl, K)
    assert ex is not tl and "_kv_mp" not in ex and ex["mp_batch_div"] == K and ex["n_mp"] == M and ex["rpe_tl2tl"] is None
    assert ex["mp_feat_flat"] is tl["mp_feat_flat"]
    for k in ("tl_token_pose", "tl_token_valid", "knn_idx_tl2mp", "rel_tl2tl"):
        assert torch.equal(ex[k], tl[k].repeat_interleave(K, 0)), k
    for k, v in before.items():  # the caller's dict: same keys, same values
        assert (torch.equal(tl[k], v) if torch.is_tensor(v) else tl[k] == v), k
    view = E.lights_per_scene(ex, K)
    for k in ("tl_token_pose", "tl_token_valid", "knn_idx_tl2mp", "rel_tl2tl"):
        assert torch.equal(view[k], tl[k]), k


def test_rule_navi_check_validates_arguments_without_a_gpu(hip):
    lib = hip.load()
    assert lib.tbx_rule_navi_check(None, None, None, 1, None, None, None, None, None, None, None, 1, 1, 0, None, None, None) == -1
    one = C.c_void_p(16)  # (never dereferenced: validation happens before the launch)
    assert lib.tbx_rule_navi_check(one, one, one, 2, None, None, None, None, None, None, None, 3, 4, 0, one, one, None) == -1  # n % div
    assert lib.tbx_rule_navi_check(one, one, one, 1, one, None, None, None, None, None, None, 1, 4, 20, one, one, None) == -1  # partial dest tables
    assert lib.tbx_rule_navi_check(one, one, one, 1, None, None, None, None, None, one, None, 1, 4, 0, one, one, None) == -1   # goal without its threshold


def test_host_descriptor_paths_read_their_host_arrays_in_bounds(hip):
    """The entry points that take HOST arrays / structures (job lists, stage programs, nested descriptors) walk them on the host before
    any launch: driven here with well-formed host data and placeholder device addresses on a machine WITHOUT a GPU, each returns an
    error code (bad argument, or the launch error once validation has passed) - never a crash. Under tools/sanitize_host.sh
    (AddressSanitizer + UBSan on the host halves) these are the reads that get checked."""
    if torch.cuda.is_available():
        pytest.skip("placeholder device addresses: the no-GPU form of this test (a launch would dereference them)")
    lib = hip.load()
    dp = lambda i: 0x10000 * (i + 1)  # 16-byte aligned, distinct, never dereferenced on the host
    jobs = (hip.KnnJob * 3)()
    for j, (n_src, n_tgt, k) in enumerate(((64, 64, 25), (64, 1024, 64), (64, 128, 24))):
        jb = jobs[j]
        jb.src_pose, jb.src_invalid, jb.tgt_pose, jb.tgt_invalid = dp(8 * j), dp(8 * j + 1), dp(8 * j + 2), dp(8 * j + 3)
        jb.idx, jb.invalid, jb.rel_pose, jb.emb = dp(8 * j + 4), dp(8 * j + 5), dp(8 * j + 6), None
        jb.n_batch, jb.n_src, jb.n_tgt, jb.tgt_batch_div, jb.k, jb.dist_limit = 1, n_src, n_tgt, 1, k, 1500.0
    for n in (1, 2, 3):
        assert lib.tbx_knn_embed_multi(jobs, n, dp(40), dp(41), 128, None, None) < 0
    assert lib.tbx_knn_embed_multi(jobs, 0, dp(40), dp(41), 128, None, None) == -1
    jobs[1].k = 4096  # more neighbours than targets
    assert lib.tbx_knn_embed_multi(jobs, 3, dp(40), dp(41), 128, None, None) < 0
    pe = hip.PoseEmbedJob()
    pe.pose3, pe.freqs_xy, pe.freqs_yaw, pe.out, pe.n, pe.pe_dim, pe.ld_out, pe.col_off = dp(50), dp(51), dp(52), dp(53), 64, 128, 128, 0
    jobs[1].k = 64
    assert lib.tbx_knn_embed_multi(jobs, 3, dp(40), dp(41), 128, C.byref(pe), None) < 0
    # a full stage program (MAX_STAGES entries) and one past it
    st = (hip.Stage * (hip.MAX_STAGES + 1))()
    for s in st:
        s.op, s.src, s.dst, s.k, s.n, s.ld, s.p0 = hip.OP_LINEAR, 0, 1, 128, 128, 128, dp(60)
    assert lib.tbx_rowchain(st, hip.MAX_STAGES, 16, 0, 16, 132, None) < 0
    assert lib.tbx_rowchain(st, hip.MAX_STAGES + 1, 16, 0, 16, 132, None) < 0
    # nested descriptors: zero-initialised (every pointer NULL) and partially filled
    for cls, fn in ((hip.DecLayer, lib.tbx_knarpe_dec_layer), (hip.LayerTile, lib.tbx_layer_tile), (hip.HeadsTile, lib.tbx_heads_tile),
                    (hip.WindowTile, lib.tbx_window_tile), (hip.Front, lib.tbx_front)):
        d = cls()
        assert fn(C.byref(d), None) < 0, cls.__name__
    fr = hip.Front()
    fr.jobs, fr.n_jobs = C.cast(jobs, C.c_void_p), 3
    assert lib.tbx_front(C.byref(fr), None) < 0
    # round 6: the paired launches (two nested descriptors each), the job array of the multi-image pack, the new glue entry points
    da, db = hip.DecLayer(), hip.DecLayer()
    assert lib.tbx_knarpe_dec_layer_pair(C.byref(da), C.byref(db), None) < 0 and lib.tbx_knarpe_dec_layer_pair(None, C.byref(db), None) == -1
    fa, fb = hip.Front(), hip.Front()
    assert lib.tbx_front_pair(C.byref(fa), C.byref(fb), None) < 0 and lib.tbx_front_pair(C.byref(fa), None, None) == -1
    pj = (hip.PackJob * 50)()  # (more than one launch's worth: 48 jobs per launch)
    for i, j in enumerate(pj):
        j.w, j.bias, j.out, j.n, j.k, j.ld, j.groups, j.wt = dp(70 + 2 * i), None, dp(71 + 2 * i), 128, 128, 128, 1, i & 1
    assert lib.tbx_pack_weight_mfma32_multi(pj, 0, None) == 0  # nothing to do
    assert lib.tbx_pack_weight_mfma32_multi(None, 3, None) == -1
    pj[49].k = 100  # an unsupported width in the LAST job: found by the host-side walk of its group
    assert lib.tbx_pack_weight_mfma32_multi(pj, 50, None) < 0
    pj[49].k, pj[7].out = 128, None
    assert lib.tbx_pack_weight_mfma32_multi(pj, 50, None) == -1
    assert lib.tbx_pair_bias_relu(None, dp(1), dp(2), 1, 4, 8, 128, 1, None) == -1 and lib.tbx_pair_bias_relu(dp(0), dp(1), dp(2), 1, 4, 8, 126, 1, None) == -1
    assert lib.tbx_pair_bias_relu(dp(0), dp(1), dp(2), 0, 4, 8, 128, 1, None) == 0  # an empty batch
    assert lib.tbx_layernorm_bwd_add(dp(0), dp(1), dp(2), dp(3), dp(4), 16, 64, dp(5), dp(6), dp(7), dp(8), dp(9), None) < 0  # cols != 128
    assert lib.tbx_layernorm_bwd_add(dp(0), dp(1), dp(2), dp(3), dp(4), 16, 128, 0x10004, dp(6), dp(7), dp(8), dp(9), None) < 0  # misaligned `add`
    ss = hip.SimState()
    assert lib.tbx_sim_step(C.byref(ss), 7, None, None) == -1 and lib.tbx_sim_step(C.byref(ss), 3, None, None) == -1
    rc = hip.RuleCtx()
    assert lib.tbx_rule_check(C.byref(rc), dp(1), dp(2), dp(3), dp(4), 1, 0, 1, dp(5), None) == -1


def test_clip_on_the_flat_gradient_buffer_equals_clip_grad_norm(tb):
    """pl_modules/data_parallel.clip_gradients on a FlatGrads (one 2-norm + one scale of the flat buffer) against
    torch.nn.utils.clip_grad_norm_ on the same gradients as a parameter list: same total norm, same clipped gradients (fp32 summation
    order apart), both when the norm exceeds the bound and when it does not."""
    DP = import_module("trafficbots_amd.pl_modules.data_parallel")
    g = torch.Generator().manual_seed(3)
    shapes = [(128, 128), (128,), (640, 128), (5,), (1, 128)]
    for scale, max_norm in ((10.0, 5.0), (1e-3, 5.0)):
        pa = [torch.nn.Parameter(torch.zeros(s)) for s in shapes]
        pb = [torch.nn.Parameter(torch.zeros(s)) for s in shapes]
        grads = [torch.randn(s, generator=g) * scale for s in shapes]
        for p, q, gr in zip(pa, pb, grads):
            p.grad, q.grad = gr.clone(), gr.clone()
        flat = DP.FlatGrads(pa)
        total = DP.clip_gradients(flat, max_norm)
        ref = torch.nn.utils.clip_grad_norm_(pb, max_norm)
        torch.testing.assert_close(total, ref, rtol=1e-6, atol=0)
        for i, (p, q) in enumerate(zip(pa, pb)):
            assert p.grad.data_ptr() == flat.views[i].data_ptr()  # still the flat buffer's slice
            torch.testing.assert_close(p.grad, q.grad, rtol=2e-6, atol=0)
        assert DP.clip_gradients(flat, 0) is None


def test_derived_weight_images_follow_the_weights_stamp_and_the_scope(tb):
    """hip_base._derived, the one cache of images derived from weights: a hit on repeat; a miss after an in-place op, after
    increment_version (what FlatAdamW.step does after updating through its flat buffer) and after `q.data = other`; images made inside a
    PackScope live in the scope, not on the Parameter, and die with it. packed_weight's requests recorded in a scope (a view, a whole
    Parameter), rebuilt (_at) after the Parameters' `.data` was re-pointed, alias the new storage and keep their cache keys."""
    import gc
    import weakref

    HB = import_module("trafficbots_amd.hip_base")
    q = torch.nn.Parameter(torch.arange(6.0))
    made = []

    def get():
        return HB._derived(("test", HB._name(q)), (q,), lambda: made.append(1) or q.detach() * 2)

    a = get()
    assert get() is a and len(made) == 1
    with torch.no_grad():
        q.add_(1.0)
    assert torch.equal(get(), q.detach() * 2) and len(made) == 2
    torch.autograd.graph.increment_version([q])
    get()
    assert len(made) == 3
    flat = torch.zeros(10)
    q.data = flat[2:8]
    get()
    assert len(made) == 4 and get() is not None and len(made) == 4
    with torch.no_grad():
        flat.add_(1.0)  # through the flat buffer: q's version counter does not see it ...
    assert len(made) == 4 and get() is not None and len(made) == 4
    torch.autograd.graph.increment_version([q])  # ... until it is bumped
    assert torch.equal(get(), q.detach() * 2) and len(made) == 5
    on_q = dict(q._tbx_derived)
    scope = HB.open_pack_scope()
    try:
        b = get()
        assert len(made) == 6 and get() is b and len(made) == 6
        assert q._tbx_derived == on_q and id(q) in scope.pinned
    finally:
        HB.close_pack_scope(scope)
    gone = weakref.ref(b)
    del b, scope
    gc.collect()
    assert gone() is None
    get()
    assert len(made) == 6  # the Parameter's own image is still current
    # packed_weight's requests, recorded in a scope of an owner (the images are seeded: packing needs the GPU), become the owner's plan;
    # rebuilt on the Parameters' new storage, as open_pack_scope does, they alias it and keep the keys they were recorded under
    owner, w2 = torch.nn.Module(), torch.nn.Parameter(torch.arange(12.0).view(3, 4))
    reqs = [(w2[1:], q[2:5]), (w2, q[:3])]  # a view of each Parameter, and a whole Parameter with a view
    scope = HB.open_pack_scope(owner, "k")
    for w, bias in reqs:
        key = HB._pack_key(w, bias, False, 1, False, False, True)
        scope.images[key] = (HB.weights_stamp((w, bias)), "image")
        assert HB.packed_weight(w, bias, mfma32=True) == "image"
    HB.close_pack_scope(scope)
    keys = list(scope.record)
    assert len(keys) == 2 and [e[:2] for e in owner._tbx_pack_plans["k"]] == [scope.record[k][:2] for k in keys]
    other, flat = torch.arange(20.0), torch.arange(30.0)
    q.data, w2.data = other[7:13], flat[5:17].view(3, 4)
    now = [(w2[1:], q[2:5]), (w2, q[:3])]  # the same requests on the new storage
    for k, (wp, bp, wt, groups), (w, bias) in zip(keys, owner._tbx_pack_plans["k"], now):
        v, vb = HB._at(wp), HB._at(bp)
        assert HB._pack_key(v, vb, wt, groups, False, False, True) == k
        assert v.data_ptr() == w.data_ptr() and torch.equal(v, w) and vb.data_ptr() == bias.data_ptr() and torch.equal(vb, bias)
        assert v.data_ptr() >= flat.data_ptr() and vb.data_ptr() >= other.data_ptr()  # (the new storage)
    assert HB._at(owner._tbx_pack_plans["k"][1][0]) is w2  # a whole Parameter is rebuilt as itself


# ---- the closed-loop step family: tbx_sim_step / tbx_agent_prep / tbx_tl_prep and the step tails of tbx_knarpe_dec_layer share their
# checks (csrc/step_core.h). Descriptors of placeholder device addresses that are valid up to the launch: without a GPU the launch itself
# fails (TBX_ERR_LAUNCH), which is how a test sees that every argument check passed.
_ARG, _UNSUPPORTED, _ALIGN, _LAUNCH = -1, -2, -3, -4
_dp = lambda i: 0x10000 * (i + 1)  # 16-byte aligned, distinct, never dereferenced on the host
_STEP_W = 11                       # window of the step descriptors below


def _no_gpu_only():
    if torch.cuda.is_available():
        pytest.skip("placeholder device addresses reach the launch: the no-GPU form of this test (a launch would dereference them)")


def _sim_state(hip, n_ag=4, n_tl=3):
    st = hip.SimState()
    for i, (name, ty) in enumerate(hip.SimState._fields_):
        if ty is C.c_void_p and not name.startswith(("ov_", "player_", "act_", "out_act_", "now_")):
            setattr(st, name, _dp(100 + i))
    st.n_batch, st.n_ag, st.n_tl, st.window, st.n_step_gt, st.n_step_tl_gt, st.n_step_out, st.n_node = 1, n_ag, n_tl, _STEP_W, 91, 91, 80, 20
    return st


def _prep_args(hip, n_tok=4, n_ag=4):
    a = hip.AgentPrepArgs()
    for i, (name, ty) in enumerate(hip.AgentPrepArgs._fields_):
        if ty is C.c_void_p:
            setattr(a, name, _dp(200 + i))
    a.n_tok, a.n_ag, a.window, a.pe_dim, a.n_mp, a.mp_batch_div = n_tok, n_ag, _STEP_W, 64, 16, 1
    return a


def _tl_rows(hip):
    return hip.TlRows(_dp(300), _dp(301), _dp(302), 16, 0)


def _dec_layer(hip, n_rows):
    """A last-layer tail_mfma32 tbx_knarpe_dec_layer descriptor of n_rows rows without a tail."""
    t = hip.DecLayer()
    m = t.mid
    for i, name in enumerate(("qkv", "x", "rpe_k_bias_self", "rpe_k_bias_cross", "freqs_xy", "freqs_yaw", "fold_self_image", "out_proj_image",
                              "q_image", "qfold_image", "fold_cross_image", "ln_weight", "ln_bias")):
        setattr(m, name, _dp(400 + i))
    for j, sg in enumerate((m.self_seg, m.cross_seg[0])):
        sg.kv, sg.idx, sg.invalid, sg.rel_pose = (_dp(420 + 4 * j + q) for q in range(4))
        sg.ld_kv, sg.k_off, sg.v_off, sg.n_tgt, sg.batch_div, sg.k = 256, 0, 128, 8, 1, 4
    m.ld_qkv, m.q_off, m.qt_off, m.n_cross, m.n_batch, m.n_src = 896, 0, 384, 1, 1, n_rows
    for i, name in enumerate(("out_proj2_image", "linear1_image", "linear2_image", "norm2_weight", "norm2_bias", "src_invalid")):
        setattr(t, name, _dp(440 + i))
    t.tail_mfma32 = 1
    return t


def _agents_tail(hip, sim, prep):
    """(descriptor, keep-alive): the agents' step tail on (sim, prep) behind the heads."""
    t = _dec_layer(hip, sim.n_batch * sim.n_ag)
    h = hip.HeadsTail()
    for i in range(9):
        h.images[i] = _dp(500 + i)
    for i, name in enumerate(("navi_emb", "latent_emb", "navi_valid", "latent_invalid", "type_mask")):
        setattr(h, name, _dp(510 + i))
    h.action_out, h.mask_stride = sim.action_mean, sim.n_batch * sim.n_ag
    h.sim_parts, h.sim_state, h.next_prep = hip.SIM_AGENTS | hip.SIM_ADVANCE, C.addressof(sim), C.addressof(prep)
    t.heads = C.addressof(h)
    return t, (h, sim, prep)


def _lights_tail(hip, sim, rows):
    """(descriptor, keep-alive): the lights' step tail on sim, its riding rows = the fields of `rows`."""
    t = _dec_layer(hip, sim.n_batch * sim.n_tl)
    L = hip.TlTail()
    for i in range(4):
        L.kv_images[i], L.norm_weight[i], L.norm_bias[i] = _dp(600 + i), _dp(610 + i), _dp(620 + i)
    for i in range(3):
        L.mlp_images[i] = _dp(630 + i)
    L.kv_out, L.tl_invalid, L.logits_out, L.ld_kv, L.n_state = _dp(640), rows.tl_invalid, sim.tl_logits, 1024, 5
    L.sim_parts, L.sim_state = hip.SIM_LIGHTS | hip.SIM_ADVANCE, C.addressof(sim)
    L.prep_attr, L.prep_row_invalid, L.prep_ld_attr = rows.attr, rows.row_invalid, rows.ld_attr
    t.lights = C.addressof(L)
    return t, (L, sim, rows)


def _set(**kw):
    def f(obj):
        for k, v in kw.items():
            setattr(obj, k, v)
    return f


def test_step_descriptors_are_valid_up_to_the_launch(hip):
    """The descriptors the tests below break in one place each pass every argument check of every entry point that takes them."""
    _no_gpu_only()
    lib = hip.load()
    assert lib.tbx_agent_prep(C.byref(_prep_args(hip)), None) == _LAUNCH
    assert lib.tbx_tl_prep(_dp(0), 1, 3, _STEP_W, C.byref(_tl_rows(hip)), None) == _LAUNCH
    assert lib.tbx_knarpe_dec_layer(C.byref(_dec_layer(hip, 4)), None) == _LAUNCH
    t, keep = _agents_tail(hip, _sim_state(hip), _prep_args(hip))
    assert lib.tbx_knarpe_dec_layer(C.byref(t), None) == _LAUNCH
    t, keep = _lights_tail(hip, _sim_state(hip), _tl_rows(hip))
    assert lib.tbx_knarpe_dec_layer(C.byref(t), None) == _LAUNCH


@pytest.mark.parametrize("fault, code", [
    (_set(window=24), _UNSUPPORTED), (_set(pe_dim=96), _UNSUPPORTED), (_set(ag_type_idx=None), _ARG), (_set(navi_row=None), _ARG),
    (_set(n_ag=3), _UNSUPPORTED)], ids=["window-24", "pe_dim-96", "type_mask-without-ag_type_idx", "dest-without-navi_row", "n_tok-not-a-multiple-of-n_ag"])
def test_agents_tail_refuses_what_agent_prep_refuses(hip, fault, code):
    """tbx_agent_prep and the agents' step tail of tbx_knarpe_dec_layer on the same tbx_agent_prep_args_t: the same code."""
    _no_gpu_only()
    lib = hip.load()
    sim, prep = _sim_state(hip), _prep_args(hip)
    t, keep = _agents_tail(hip, sim, prep)
    assert lib.tbx_agent_prep(C.byref(prep), None) == _LAUNCH and lib.tbx_knarpe_dec_layer(C.byref(t), None) == _LAUNCH
    fault(prep)
    assert lib.tbx_agent_prep(C.byref(prep), None) == code
    assert lib.tbx_knarpe_dec_layer(C.byref(t), None) == code


@pytest.mark.parametrize("fault, code, float4_only", [
    (_set(attr=None), _ARG, False), (_set(ld_attr=5 + _STEP_W - 1), _ARG, False), (_set(ld_attr=18), _ALIGN, False),
    (_set(attr=_dp(301) + 4), _ALIGN, True)], ids=["attr-null", "ld_attr-below-5+window", "ld_attr-not-a-multiple-of-4", "attr-misaligned"])
def test_every_writer_of_the_lights_rows_checks_them_alike(hip, fault, code, float4_only):
    """tbx_sim_step with tl_rows, the lights' step tail of tbx_knarpe_dec_layer and (but for the alignment, which only the float4
    stores of the riding forms need) tbx_tl_prep on the same rows: the same code."""
    _no_gpu_only()
    lib = hip.load()
    sim, rows = _sim_state(hip), _tl_rows(hip)
    parts = hip.SIM_LIGHTS | hip.SIM_ADVANCE
    assert lib.tbx_sim_step(C.byref(sim), parts, C.byref(rows), None) == _LAUNCH
    fault(rows)
    t, keep = _lights_tail(hip, sim, rows)
    assert lib.tbx_sim_step(C.byref(sim), parts, C.byref(rows), None) == code
    assert lib.tbx_knarpe_dec_layer(C.byref(t), None) == code
    assert lib.tbx_tl_prep(_dp(0), 1, 3, _STEP_W, C.byref(rows), None) == (_LAUNCH if float4_only else code)


@pytest.mark.parametrize("fault", [
    _set(hist_tl=None), _set(dest_thresh=None), _set(player_valid=_dp(700)), _set(act_seed=_dp(701), out_act_noise=_dp(702))], ids=["lights-pointer-null", "agents-pointer-null", "player_valid-without-player_action", "act_seed-without-out_act_log_prob"])
def test_step_tails_refuse_the_state_sim_step_refuses(hip, fault):
    """tbx_sim_step and the step tails of tbx_knarpe_dec_layer on the same tbx_sim_state_t: the same code. The rule is the full list of
    the stand-alone call whatever the parts, so either side's pointer is missed by both tails and by every choice of parts."""
    _no_gpu_only()
    lib = hip.load()
    sim = _sim_state(hip)
    ta, keep_a = _agents_tail(hip, sim, _prep_args(hip))
    tl, keep_l = _lights_tail(hip, sim, _tl_rows(hip))
    assert lib.tbx_knarpe_dec_layer(C.byref(ta), None) == _LAUNCH and lib.tbx_knarpe_dec_layer(C.byref(tl), None) == _LAUNCH
    fault(sim)
    for parts in (hip.SIM_AGENTS | hip.SIM_LIGHTS | hip.SIM_ADVANCE, hip.SIM_AGENTS | hip.SIM_ADVANCE, hip.SIM_LIGHTS):
        assert lib.tbx_sim_step(C.byref(sim), parts, None, None) == _ARG
    assert lib.tbx_knarpe_dec_layer(C.byref(ta), None) == _ARG and lib.tbx_knarpe_dec_layer(C.byref(tl), None) == _ARG


def test_sim_step_parts_grammar_of_the_one_entry_point(hip):
    """The four call shapes the three former entry points had - the whole step, one side, TBX_SIM_APPEND alone, the lights with their
    rows riding - are accepted up to the launch; what they refused is still TBX_ERR_ARG."""
    _no_gpu_only()
    lib = hip.load()
    sim, rows = _sim_state(hip), _tl_rows(hip)
    A, L, ADV, NO_DIS, NO_APP, APP = hip.SIM_AGENTS, hip.SIM_LIGHTS, hip.SIM_ADVANCE, hip.SIM_NO_DISABLE, hip.SIM_NO_APPEND, hip.SIM_APPEND
    step = lambda parts, r=None: lib.tbx_sim_step(C.byref(sim), parts, C.byref(r) if r is not None else None, None)
    for parts in (A | L | ADV, A, L, A | ADV, L | ADV, ADV, APP, A | L | ADV | NO_DIS | NO_APP):
        assert step(parts) == _LAUNCH, parts
    for parts in (L, L | ADV, A | L | ADV):
        assert step(parts, rows) == _LAUNCH, parts
    for parts in (APP | A, NO_DIS, NO_APP, NO_DIS | ADV, 0, 64):
        assert step(parts) == _ARG, parts
    for parts in (A, A | ADV, APP, L | NO_APP):  # rows without the lights' part, or with windows that are left alone
        assert step(parts, rows) == _ARG, parts

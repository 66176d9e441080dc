"""CPU-only checks of gradient-norm tracking (Lightning's track_grad_norm on the flat gradient buffer): the C ABI of tbx_grad_norms (header,
export from libtbx_grad.so, the ctypes mirror's layout as gcc lays out the header, every refusal before a launch), FlatGrads.norm_plan's segment / chunk tables
and names for a packed and an aligned layout, the key format of Lightning 1.5.8's `grad_norm` utility, WaymoMotion.log_grad_norm, and that
clip_gradients without tracking is the expression it always was. The kernels themselves: tests/test_hip_grad_norm.py."""
import ctypes as C
import math
import subprocess
from importlib import import_module
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
ARG, ALIGN = -1, -3


@pytest.fixture(scope="module")
def hip(tb):
    h = import_module("trafficbots_amd.hip")
    h.load()
    return h


@pytest.fixture(scope="module")
def DP(tb):
    return import_module("trafficbots_amd.pl_modules.data_parallel")


def test_entry_point_is_declared_exported_and_typed(hip):
    """tbx_grad_norms is the one tbx_* function libtbx_grad.so exports, declared in include/tbx_hip_grad.h and bound with argtypes by
    hip.load_grad(); libtbx_hip.so and include/tbx_hip.h - ABI 7's closed list - do not carry it."""
    import re

    lib = hip.load_grad()
    assert lib.tbx_grad_norms.argtypes == [C.POINTER(hip.GradNorms), C.c_void_p] and lib.tbx_grad_norms.restype is C.c_int
    nm = subprocess.run(["nm", "-D", "--defined-only", str(hip.GRAD_LIB_PATH)], check=True, capture_output=True, text=True).stdout
    assert [l.split()[2] for l in nm.splitlines() if len(l.split()) == 3 and l.split()[1] == "T" and l.split()[2].startswith("tbx_")] == ["tbx_grad_norms"]
    txt = (hip.HEADER_PATH.parent / "tbx_hip_grad.h").read_text()
    assert re.findall(r"^(?:int|int64_t|const char\*)\s+(tbx_\w+)\s*\(", txt, flags=re.M) == ["tbx_grad_norms"]
    assert "tbx_grad_norms" not in hip.declared_symbols() and "tbx_hip_grad.h" not in hip.HEADER_PATH.read_text()
    assert hip.load().tbx_version() == 7
    for name, val in (("TBX_GRAD_CHUNK", hip.GRAD_CHUNK), ("TBX_GRAD_NORM_2", hip.GRAD_NORM_2), ("TBX_GRAD_NORM_INF", hip.GRAD_NORM_INF)):
        assert f"#define {name} {val} " in txt, name


def test_ctypes_mirror_has_the_layout_gcc_gives_the_header(hip, tmp_path):
    """tbx_hip_grad.h included FIRST (it includes tbx_hip.h for the codes) compiles as C with -Wall -Werror; sizeof and every offsetof of
    tbx_grad_norms_t equal hip.GradNorms'."""
    fields = [f[0] for f in hip.GradNorms._fields_]
    src, exe = tmp_path / "gn.c", tmp_path / "gn"
    src.write_text('#include "tbx_hip_grad.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%zu\\n", sizeof(tbx_grad_norms_t));'
                   + "".join(f'printf("%zu\\n", offsetof(tbx_grad_norms_t, {f}));' for f in fields) + "return 0;}\n")
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == C.sizeof(hip.GradNorms)
    for f, off in zip(fields, out[1:]):
        assert getattr(hip.GradNorms, f).offset == off, f


def _stand_in(hip, **over):
    """A tbx_grad_norms_t that passes every check, on stand-in pointers (never dereferenced: each call below is refused before a launch)."""
    a = hip.GradNorms()
    for i, name in enumerate(("g", "seg_off", "seg_len", "chunk_seg", "chunk_off", "chunk_len", "partial", "partial_nf", "norms", "total",
                              "nonfinite", "coef")):
        setattr(a, name, 0x10000 * (i + 1))
    a.n, a.n_seg, a.n_chunk, a.chunk_max, a.norm_type, a.max_norm = 100, 2, 3, hip.GRAD_CHUNK, hip.GRAD_NORM_2, 5.0
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_bad_arguments_are_refused_before_any_launch(hip):
    lib = hip.load_grad()
    call = lambda **over: lib.tbx_grad_norms(C.byref(_stand_in(hip, **over)), None)
    assert lib.tbx_grad_norms(None, None) == ARG
    for k in ("g", "seg_off", "seg_len", "chunk_seg", "chunk_off", "chunk_len", "partial", "partial_nf", "norms", "total", "nonfinite", "coef"):
        assert call(**{k: None}) == ARG, k
    for over in (dict(n=0), dict(n=-4), dict(n_seg=0), dict(n_seg=-1), dict(n_chunk=-1), dict(chunk_max=hip.GRAD_CHUNK + 1), dict(chunk_max=0),
                 dict(norm_type=1), dict(norm_type=3), dict(norm_type=-1)):
        assert call(**over) == ARG, over
    assert call(g=0x10002) == ALIGN
    with pytest.raises(RuntimeError):  # CPU tensors: no fallback path
        z = torch.zeros
        hip.grad_norms_args(z(8), z(1, dtype=torch.int64), z(1, dtype=torch.int64), z(1, dtype=torch.int32), z(1, dtype=torch.int64),
                            z(1, dtype=torch.int32), 8, z(1, dtype=torch.float64), z(1, dtype=torch.int32), z(4), hip.GRAD_NORM_2, 5.0)


def _module(CH):
    """Mixed sizes around the chunk length CH: below, exactly one, two and a bit, three and one."""
    m = torch.nn.Module()
    m.inner = torch.nn.Module()
    for i, s in enumerate([(3, 5), (1,), (CH,), (2, CH + 3), (64,), (7, 9), (3 * CH + 1,), (4,), (CH - 1,)]):
        (m if i % 2 else m.inner).register_parameter(f"w{i}", torch.nn.Parameter(torch.randn(s, generator=torch.Generator().manual_seed(i))))
    return m


@pytest.mark.parametrize("align", [1, 64])
def test_norm_plan_tiles_every_segment_once_and_names_the_parameters(hip, DP, align):
    m = _module(hip.GRAD_CHUNK)
    named = list(m.named_parameters())
    flat = DP.FlatGrads([p for _, p in named], align=align)
    plan = flat.norm_plan(m)
    assert flat.norm_plan() is plan  # cached
    CH = hip.GRAD_CHUNK
    assert plan.names == [k for k, _ in named] and "inner.w0" in plan.names
    assert plan.seg_off.tolist() == flat.offsets and plan.seg_len.tolist() == [p.numel() for _, p in named]
    assert plan.seg_off.dtype == plan.seg_len.dtype == plan.chunk_off.dtype == torch.int64
    assert plan.chunk_seg.dtype == plan.chunk_len.dtype == torch.int32
    cs, co, cl = plan.chunk_seg.tolist(), plan.chunk_off.tolist(), plan.chunk_len.tolist()
    assert plan.n_seg == len(named) and plan.n_chunk == len(cs) == len(co) == len(cl)
    assert plan.partial.numel() == plan.n_chunk and plan.partial.dtype == torch.float64 and plan.partial_nf.dtype == torch.int32
    assert cs == sorted(cs) and plan.chunk_max == max(cl) == CH and min(cl) >= 1
    covered = torch.zeros(flat.flat.numel(), dtype=torch.int32)
    for s, (off, (_, p)) in enumerate(zip(flat.offsets, named)):
        mine = [(o, l) for c, o, l in zip(cs, co, cl) if c == s]
        assert len(mine) == -(-p.numel() // CH)
        at = off
        for o, l in mine:  # consecutive, in order, inside the segment
            assert o == at and 1 <= l <= CH
            at += l
        assert at == off + p.numel()
        assert all(l == CH for _, l in mine[:-1])
    for o, l in zip(co, cl):
        covered[o:o + l] += 1
    in_seg = torch.zeros_like(covered)
    for off, (_, p) in zip(flat.offsets, named):
        in_seg[off:off + p.numel()] = 1
    assert torch.equal(covered, in_seg)  # every element of a segment in exactly one chunk, a gap in none
    assert (int((in_seg == 0).sum()) > 0) == (align == 64)
    with pytest.raises(KeyError):
        flat.norm_plan(torch.nn.Linear(2, 2))  # a module that does not own the parameters


def test_key_format_is_lightning_1_5_8s(DP):
    """pytorch_lightning/utilities/grads.py (1.5.8): f"grad_{float(norm_type)}_norm/{name}" per parameter with a gradient and
    f"grad_{norm_type}_norm_total"."""
    assert DP.grad_norm_type(-1) is None and DP.grad_norm_type(-1.0) is None
    assert DP.grad_norm_type(2) == DP.grad_norm_type(2.0) == DP.grad_norm_type("2") == 2.0
    assert DP.grad_norm_type("inf") == DP.grad_norm_type(float("inf")) == math.inf
    with pytest.raises(NotImplementedError):
        DP.grad_norm_type(1)
    names = ["model.a.weight", "model.a.bias", "model.b"]
    per = torch.tensor([3.0, 4.0, 12.0])
    for nt, pre in ((2, "grad_2.0_norm"), (2.0, "grad_2.0_norm"), ("inf", "grad_inf_norm")):
        res = DP.GradNormResult(per, torch.tensor(13.0), torch.tensor(0, dtype=torch.int32), torch.tensor(1.0), names, DP.grad_norm_type(nt))
        d = res.as_dict()
        assert list(d) == [f"{pre}/{k}" for k in names] + [f"{pre}_total"]
        assert all(v.dim() == 0 for v in d.values())
        assert d[f"{pre}/model.b"].data_ptr() == per[2].data_ptr()  # a view of the vector, not a copy
        assert float(d[f"{pre}_total"]) == 13.0
    try:
        from pytorch_lightning.utilities.grads import grad_norm  # the reference's own utility, where it is installed
    except Exception:
        return
    lin = torch.nn.Linear(3, 2)
    lin(torch.ones(1, 3)).sum().backward()
    for nt in (2, "inf"):
        res = DP.clip_gradients(list(lin.parameters()), None, track=nt, module=lin)
        assert set(res.as_dict()) == set(grad_norm(lin, nt))


def test_clip_gradients_tracks_a_plain_parameter_list_with_torch(DP):
    """train_step's first eager step has no FlatGrads yet: per-tensor norms by torch, the same result object, the same clip."""
    lin = torch.nn.Linear(5, 3)
    (lin(torch.arange(10.0).view(2, 5)) ** 2).sum().backward()
    g0 = [p.grad.clone() for p in lin.parameters()]
    res = DP.clip_gradients(list(lin.parameters()), 0.5, track=2, module=lin)
    assert res.names == ["weight", "bias"] and int(res.nonfinite) == 0
    assert torch.equal(res.per_param, torch.stack([g.norm() for g in g0]))
    assert float(res.coef) < 1.0
    for p, g in zip(lin.parameters(), g0):
        assert torch.equal(p.grad, g * res.coef)
    res = DP.clip_gradients(list(lin.parameters()), None, track="inf", module=lin)  # tracking without a clip
    assert float(res.coef) == 1.0 and torch.equal(res.total, torch.stack([p.grad.abs().max() for p in lin.parameters()]).max())


def test_waymo_motion_log_grad_norm_calls_log_dict(tb):
    W = import_module("trafficbots_amd.pl_modules.waymo_motion")
    assert W.WaymoMotion.last_grad_norms is None
    seen = []

    class Probe:
        def log_dict(self, d, **kw):
            seen.append((d, kw))

    d = {"grad_2.0_norm/model.x": torch.tensor(1.0), "grad_2.0_norm_total": torch.tensor(1.0)}
    W.WaymoMotion.log_grad_norm(Probe(), d)
    assert seen == [(d, dict(on_step=True, on_epoch=False, prog_bar=False, logger=True))]  # the reference's statement (waymo_motion.py:841)
    if W.LightningModule.__module__ == W.__name__:  # the stand-in: log_dict lands in `logged`
        lm = W.LightningModule()
        lm.log_dict(d, on_step=True)
        assert lm.logged == d


def test_train_entry_points_take_lightnings_argument(DP):
    import inspect

    for fn in (DP.train_step, DP.GraphedTrainStep.__init__):
        assert inspect.signature(fn).parameters["track_grad_norm"].default == -1


def test_clip_without_tracking_is_the_expression_it_was(DP):
    """clip_gradients(flat, 5.0) with track=None on CPU tensors: vector_norm of the buffer, mul_ by clip_grad_norm_'s coefficient - bit
    for bit -, for a norm above and below max_norm; max_norm None / 0 leaves the buffer alone."""
    for scale in (3.0, 1e-3):
        ps = [torch.nn.Parameter(torch.randn(s, generator=torch.Generator().manual_seed(i))) for i, s in enumerate([(33, 7), (5,), (129,)])]
        for i, p in enumerate(ps):
            p.grad = torch.randn(p.shape, generator=torch.Generator().manual_seed(100 + i)) * scale
        flat = DP.FlatGrads(ps, align=64)
        want = flat.flat.clone()
        total_want = torch.linalg.vector_norm(want)
        want.mul_((5.0 / (total_want + 1e-6)).clamp(max=1.0))
        total = DP.clip_gradients(flat, 5.0)
        assert torch.equal(total, total_want) and torch.equal(flat.flat, want)
        assert (float(total) > 5.0) == (scale == 3.0)
        assert DP.clip_gradients(flat, None) is None and DP.clip_gradients(flat, 0.0) is None and torch.equal(flat.flat, want)

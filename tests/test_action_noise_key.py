"""CPU-only checks of the action noise of the sampled closed-loop step (csrc/drop_key.h action_noise): the
header's definition compiled by a plain g++ against its Python restatement (hip_base.action_noise_bits / action_noise), the
statistics of the restatement under the bounds the GPU test holds the kernel's log to, and the off state of the argument group."""
import ctypes as C
import subprocess
from importlib import import_module
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
SEEDS = (0x5DEECE66D, 2**64 - 977)


@pytest.fixture(scope="module")
def base(tb):
    return import_module("trafficbots_amd.hip_base")


def noise_stats(eps: np.ndarray) -> dict:
    """eps [steps, rows, 2] (float64) -> the five statistics and their 5-sigma bounds for N = eps.size independent N(0, 1) draws:
    |mean| <= 5 / sqrt(N), |var - 1| <= 5 sqrt(2 / N), and |corr| <= 5 / sqrt(N) between the two dimensions of an agent, one agent at
    consecutive steps, and neighbouring rows at one step. The bounds are conditions (the standard errors of the estimators under the
    null hypothesis, times 5), not measurements. Shared with tests/test_hip_sampled_actions.py."""
    n = eps.size
    corr = lambda a, b: float(np.corrcoef(a.ravel(), b.ravel())[0, 1])
    got = {"mean": float(eps.mean()), "var": float(eps.var()) - 1.0, "corr_dims": corr(eps[..., 0], eps[..., 1]),
           "corr_steps": corr(eps[:-1], eps[1:]), "corr_rows": corr(eps[:, :-1], eps[:, 1:])}
    bound = {k: 5.0 / np.sqrt(n) for k in got}
    bound["var"] = 5.0 * np.sqrt(2.0 / n)
    return {k: (got[k], bound[k]) for k in got}


def test_python_action_noise_equals_drop_key_header(base, tmp_path):
    """4,096 (row, step) counters for two seeds: the integer part (two hashes per draw) is equal, eps within 1e-5 absolute of the
    float64 restatement. Why 1e-5: theta = 2 pi h2 2^-32 is formed from (float)h2, a rounding of up to 2 pi 2^-24 = 3.7e-7 rad; logf (or
    log1pf), sqrtf and sincosf add a few 2^-24 relative each; times r <= 6.66 that is <= ~4e-6, rounded up. (u1 next to 1 goes through
    log1pf of the exact distance to 1 - see the header -, else (float)(h1 + 1) alone would cost up to 2e-4 there.)"""
    rows, steps = 128, 32  # rows x steps = 4,096; plus the corners of the counter range
    extra = [(0xFFFFFFFF, 0x7FFFFFFF), (0x7FFFFFFF, 1), (1, 0xFFFFFFFF), (123456789, 90)]  # (step, row)
    src = tmp_path / "an.cpp"
    src.write_text('#include "drop_key.h"\n#include <stdio.h>\nusing namespace tbx_drop;\n'
                   "static void one(uint64_t seed, uint32_t step, uint32_t row) {\n"
                   "  const NoiseBits b = action_noise_bits(seed, step, row);\n  const Noise2 e = action_noise(seed, step, row);\n"
                   '  printf("%u %u %.9g %.9g\\n", b.h1, b.h2, e.e0, e.e1);\n}\n'
                   "int main() {\n" + f"  const uint64_t seeds[] = {{{SEEDS[0]}ull, {SEEDS[1]}ull}};\n"
                   "  for (uint64_t seed : seeds) {\n"
                   f"    for (uint32_t step = 1; step <= {steps}; ++step) for (uint32_t row = 0; row < {rows}; ++row) one(seed, step, row);\n"
                   + "".join(f"    one(seed, {s}u, {r}u);\n" for s, r in extra) +
                   "  }\n"
                   # the edges of the float part: u1 = 2^-32 (largest r), u1 = 1 (r = 0), u1 just below 1, both halves' boundary
                   "  const uint32_t h1s[] = {0u, 0xFFFFFFFFu, 0xFFFFFFFEu, 0xFFFFFF00u, 0x80000000u, 0x7FFFFFFFu, 0xFF000000u};\n"
                   "  for (uint32_t h1 : h1s) { const Noise2 e = action_noise(NoiseBits{h1, 0x20000000u}); printf(\"%.9g %.9g\\n\", e.e0, e.e1); }\n"
                   "  return 0;\n}\n")
    exe = tmp_path / "an"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", str(ROOT / "trafficbotsv1.5_amd" / "csrc"), str(src), "-o", str(exe)], check=True)
    out = iter(subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().split("\n"))
    worst = 0.0
    for seed in SEEDS:
        cases = [(step, np.arange(rows)) for step in range(1, steps + 1)] + [(s, np.array([r])) for s, r in extra]
        for step, rr in cases:
            h1, h2 = base.action_noise_bits(seed, step, rr)
            eps = base.action_noise(seed, step, rr)
            for j in range(len(rr)):
                a, b, e0, e1 = next(out).split()
                assert (int(a), int(b)) == (int(h1[j]), int(h2[j])), (seed, step, rr[j])
                d = max(abs(float(e0) - eps[j, 0]), abs(float(e1) - eps[j, 1]))
                worst = max(worst, d)
                assert d <= 1e-5, (seed, step, rr[j], e0, e1, eps[j])
    for h1 in (0, 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFF00, 0x80000000, 0x7FFFFFFF, 0xFF000000):
        e0, e1 = (float(v) for v in next(out).split())
        r = np.sqrt(-2.0 * np.log((h1 + 1.0) * 2.0 ** -32))
        th = 2.0 * np.pi * 0x20000000 * 2.0 ** -32
        assert abs(e0 - r * np.cos(th)) <= 1e-5 and abs(e1 - r * np.sin(th)) <= 1e-5, (h1, e0, e1, r)
        assert np.hypot(e0, e1) <= np.sqrt(64 * np.log(2)) * (1 + 1e-6)
    print(f"[action noise, g++ float vs float64 restatement] max |d eps| {worst:.3g}")


def test_restatement_is_standard_normal_and_uncorrelated(base):
    """The restatement alone over 32 x 128 rows x 20 steps x 2 = 163,840 draws passes the five 5-sigma bounds (noise_stats) the
    GPU test holds the kernel's log to: the reference side of that comparison is itself sound."""
    for seed in SEEDS:
        rows = np.arange(32 * 128)
        eps = np.stack([base.action_noise(seed, step, rows) for step in range(1, 21)], 0)
        assert eps.shape == (20, 4096, 2) and eps.size == 163840
        for k, (got, bound) in noise_stats(eps).items():
            print(f"[restatement seed {seed:#x}] {k} {got:+.3g} (bound {bound:.3g})")
            assert abs(got) <= bound, (seed, k, got, bound)
        assert np.abs(eps).max() <= np.sqrt(64 * np.log(2))
    # another seed, step or row is another draw
    a = base.action_noise(SEEDS[0], 1, rows)
    assert not np.any(a == base.action_noise(SEEDS[1], 1, rows)) and not np.any(a == base.action_noise(SEEDS[0], 2, rows))
    assert base.ACTION_NOISE_SITE > 0xFFFF  # no dropout site (they count up from 1 within a pass) reaches it


def test_zero_initialised_state_has_sampling_off_and_a_seed_needs_its_logs(tb):
    hip = import_module("trafficbots_amd.hip")
    lib = hip.load()
    st = hip.SimState()
    assert not st.act_seed and not st.out_act_noise and not st.out_act_log_prob
    assert [list(r) for r in st.act_log_std] == [[0.0, 0.0]] * 3
    # the group sits behind everything the deterministic step reads: an older caller's shorter, zero-padded struct means "off"
    assert hip.SimState.act_seed.offset == hip.SimState.now_reached.offset + C.sizeof(C.c_void_p)
    assert C.sizeof(hip.SimState) == hip.SimState.out_act_log_prob.offset + C.sizeof(C.c_void_p)
    # a seed without both logs is refused before any launch (no GPU needed: nothing is dereferenced on the host)
    for name, ty in hip.SimState._fields_:
        if ty is C.c_void_p and not name.startswith(("ov_", "player_", "act_", "out_act_")):
            setattr(st, name, 64)
    st.n_batch = st.n_ag = st.n_tl = st.window = st.n_step_out = st.n_node = 1
    st.act_seed = 64
    assert lib.tbx_sim_step(C.byref(st), hip.SIM_AGENTS, None, None) == -1
    st.out_act_noise = 64
    assert lib.tbx_sim_step(C.byref(st), hip.SIM_AGENTS, None, None) == -1

#!/usr/bin/env python
"""Static audit of the waits in the decoder-layer kernels (csrc/dec_mid.hip): compiles the file to gfx950 device assembly - no GPU
involved - and prints, per kernel,

  * the scalar waits (s_waitcnt with lgkmcnt) and scalar loads in front of the first vector load, and that load's line in the body;
  * the totals of scalar loads, lgkmcnt(0) waits and s_cselect in the body;
  * the resource usage (VGPRs, AGPRs, scratch bytes per lane, LDS bytes) of the instantiation (-Rpass-analysis=kernel-resource-usage);
  * for each group of nine or more global_load_dwordx4 between two s_barrier (a weight unit is eight fragments and the bias; the
    scheduler spreads its loads among the stage's MFMAs, so the group is the vector loads of the barrier interval), the LOWEST vmcnt
    waited for behind the group's first and behind its last load, before the next s_barrier - a unit is requested two stages ahead of
    its use and vmcnt retires in order, so a wait behind the last load that is lower than the group's size waits for loads the stage
    has only just requested. The intervals are taken in LISTING order: a block the compiler laid out of line (a rarely taken branch
    placed behind the loop it belongs in front of) is counted with the stage it follows in the file, not the one it runs in - a low
    wait in the last group of a kernel has to be looked up in the listing before it is blamed on that stage.

  * with --paths (the default for any --src but dec_mid.hip, e.g. csrc/front.hip, whose kernels branch once into one of several
    inlined bodies): the same counts per PATH, a path being the listing between two unconditional ends (s_branch, s_endpgm; pieces of
    fewer than 300 instructions are left out) - with its vmcnt(0) waits, barriers and MFMAs, which tell the bodies apart (window +
    projection: MFMAs and >= 10 barriers; rider: MFMAs and fewer barriers; search / pose embedding / dispatch: no MFMA), the scalar
    loads at a REGISTER offset (an argument picked at run time; a constant offset is an immediate), the scalar loads that stand between
    a barrier and the next global_load_dwordx4 of its interval (a unit request behind a scalar round trip), and its load groups.
    s_cselect counts every scalar select - the K-nearest bisection's pivot update is one per key bit - so the selects of argument
    offsets are read from the register-offset column, not from it.

    python tools/wait_audit.py [--src FILE] [--asm FILE.s [--rpass FILE]] [--kernel SUBSTRING] [--groups] [--paths]

--asm reads an assembly file made before (with --rpass: the compiler's remarks saved from that run) instead of compiling.
--groups lists every load group; without it a kernel's groups are summarised as a histogram of their lowest waits."""
import argparse
import collections
import pathlib
import re
import subprocess
import sys
import tempfile

ROOT = pathlib.Path(__file__).resolve().parent.parent
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage"]


def compile_asm(src: pathlib.Path):
    with tempfile.TemporaryDirectory() as d:
        out = pathlib.Path(d) / "k.s"
        r = subprocess.run(["hipcc", *FLAGS, str(src), "-o", str(out)], capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit(r.stderr)
        return out.read_text(), r.stderr


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, r.stdout.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def kernels(asm: str):
    """(symbol, body lines) of every kernel: the lines between its label and its .Lfunc_end."""
    syms = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M)
    lines = asm.splitlines()
    start = {}
    for i, l in enumerate(lines):
        m = re.match(r"([A-Za-z_][\w$.]*):", l)  # (a label at column 0, a comment may follow)
        if m:
            start[m.group(1)] = i
    for s in syms:
        i = start[s]
        j = next(k for k in range(i, len(lines)) if lines[k].startswith(".Lfunc_end"))
        yield s, [l.split(";")[0].strip() for l in lines[i + 1:j]]


def resources(remarks: str):
    """symbol -> {field: value} from the kernel-resource-usage remarks."""
    out, cur = {}, None
    for l in remarks.splitlines():
        m = re.search(r"remark: (.*)$", l)
        if not m:
            continue
        t = m.group(1).strip()
        f = re.match(r"Function Name: (\S+)", t)
        if f:
            cur = out.setdefault(f.group(1), {})
        elif cur is not None and ":" in t:
            k, v = t.split(":", 1)
            cur[k.strip()] = v.split("[-R")[0].strip()
    return out


VMEM = re.compile(r"(global|buffer|flat)_load")
VMCNT = re.compile(r"vmcnt\((\d+)\)")


def audit(body):
    ins = [l for l in body if l and not l.startswith((".", ";")) and not l.endswith(":")]
    first = next((i for i, l in enumerate(ins) if VMEM.match(l)), len(ins))
    head = ins[:first]
    r = dict(first_vmem_line=first + 1,
             head_waits=sum(1 for l in head if l.startswith("s_waitcnt") and "lgkmcnt" in l),
             head_s_load=sum(1 for l in head if l.startswith(("s_load", "s_buffer_load"))),
             s_load=sum(1 for l in ins if l.startswith(("s_load", "s_buffer_load"))),
             lgkm0=sum(1 for l in ins if l.startswith("s_waitcnt") and "lgkmcnt(0)" in l),
             s_cselect=sum(1 for l in ins if l.startswith("s_cselect")), n_ins=len(ins))
    # the weight-unit requests of a stage: the global_load_dwordx4 between two barriers in listing order (the scheduler spreads a unit's
    # nine loads among the stage's MFMAs, so "consecutive" means consecutive among the vector loads of the interval)
    groups, start = [], 0
    bars = [i for i, l in enumerate(ins) if l.startswith("s_barrier")] + [len(ins)]
    for end in bars:
        seg = ins[start:end]
        lds = [i for i, l in enumerate(seg) if l.startswith("global_load_dwordx4")]
        if len(lds) >= 9:
            vm = [(i, int(m.group(1))) for i, l in enumerate(seg) if l.startswith("s_waitcnt") for m in [VMCNT.search(l)] if m]
            low = min((c for i, c in vm if i > lds[0]), default=None)
            low_after = min((c for i, c in vm if i > lds[-1]), default=None)
            groups.append((start + lds[0] + 1, len(lds), low, low_after, sum(l.startswith("v_mfma") for l in seg)))
        start = end + 1
    r["groups"] = groups
    return r


def paths(body):
    """the listing's regions between two s_branch / s_endpgm, in listing order (blocks laid out of line are counted where they stand)"""
    ins = [l for l in body if l and not l.startswith((".", ";")) and not l.endswith(":")]
    out, cur = [], []
    for l in ins:
        cur.append(l)
        if l.startswith(("s_endpgm", "s_branch")):
            out.append(cur)
            cur = []
    if cur:
        out.append(cur)
    return out


def path_row(ins):
    r = audit(ins)
    bars = sum(l.startswith("s_barrier") for l in ins)
    mfma = sum(l.startswith("v_mfma") for l in ins)
    vm0 = sum(1 for l in ins if l.startswith("s_waitcnt") and "vmcnt(0)" in l)
    kind = ("window + projection" if bars >= 10 else "rider") if mfma else "search / embedding / dispatch"
    # scalar loads between a barrier and the first wide vector load behind it (before the next barrier)
    late, seen_bar, pending = 0, False, 0
    for l in ins:
        if l.startswith("s_barrier"):
            seen_bar, pending = True, 0
        elif seen_bar and l.startswith(("s_load", "s_buffer_load")):
            pending += 1
        elif seen_bar and l.startswith("global_load_dwordx4"):
            late += pending
            seen_bar, pending = False, 0
    reg_off = sum(1 for l in ins if re.match(r"s_(buffer_)?load_\w+\s+\S+\s+\S+\s+s\d+", l.replace(",", " ")))
    return r, bars, mfma, vm0, kind, late, reg_off


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--src", default=str(ROOT / "trafficbotsv1.5_amd" / "csrc" / "dec_mid.hip"))
    ap.add_argument("--asm")
    ap.add_argument("--rpass")
    ap.add_argument("--kernel", default=None, help="substring of the demangled kernel name (default: dec_layer_mf for dec_mid.hip, every kernel otherwise)")
    ap.add_argument("--groups", action="store_true")
    ap.add_argument("--paths", action="store_true")
    a = ap.parse_args()
    is_mid = pathlib.Path(a.src).name == "dec_mid.hip"
    if a.kernel is None:
        a.kernel = "dec_layer_mf" if is_mid else ""
    a.paths = a.paths or not is_mid
    if a.asm:
        asm = pathlib.Path(a.asm).read_text()
        remarks = pathlib.Path(a.rpass).read_text() if a.rpass else ""
    else:
        asm, remarks = compile_asm(pathlib.Path(a.src))
    res = resources(remarks)
    ks = list(kernels(asm))
    names = demangle([s for s, _ in ks])
    print("kernel | waits / s_load before 1st vector load (its line) | s_load, lgkmcnt(0), s_cselect, instructions | VGPR AGPR scratch LDS")
    for sym, body in sorted(ks, key=lambda t: names[t[0]]):
        name = re.sub(r"\(anonymous namespace\)::|^void ", "", names[sym]).split("(")[0]
        if a.kernel not in name:
            continue
        r = audit(body)
        u = res.get(sym, {})
        use = " ".join(u.get(k, "?") for k in ("VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]"))
        print(f"{name} | {r['head_waits']} / {r['head_s_load']} ({r['first_vmem_line']}) | {r['s_load']}, {r['lgkm0']}, {r['s_cselect']}, {r['n_ins']} | {use}")
        if a.paths:
            f = lambda v: "-" if v is None else v
            for i, ins in enumerate(paths(body)):
                if len(ins) < 300:  # (dispatch code, early returns, the out-of-line halves of cosf / sinf)
                    continue
                q, bars, mfma, vm0, kind, late, reg_off = path_row(ins)
                print(f"    path {i} ({kind}): {q['n_ins']} instructions, s_load {q['s_load']} ({reg_off} at a register offset), lgkmcnt(0) {q['lgkm0']}, vmcnt(0) {vm0}, s_cselect {q['s_cselect']}, "
                      f"barriers {bars}, mfma {mfma}; scalar waits / loads before its 1st vector load: {q['head_waits']} / {q['head_s_load']}; "
                      f"s_load between a barrier and its next global_load_dwordx4: {late}")
                for line, n, low, low_after, m in q["groups"]:
                    print(f"        instruction {line:6d}: {n:2d} x global_load_dwordx4 ({m} mfma), lowest vmcnt before the next barrier: "
                          f"{f(low)} behind the first load, {f(low_after)} behind the last")
            continue
        if a.groups:
            for line, n, low, low_after, mfma in r["groups"]:
                f = lambda v: "-" if v is None else v
                print(f"    instruction {line:6d}: {n:2d} x global_load_dwordx4 ({mfma} mfma in the interval), lowest vmcnt before the next barrier: "
                      f"{f(low)} behind the first load, {f(low_after)} behind the last")
        else:
            h = collections.Counter("-" if g[3] is None else g[3] for g in r["groups"])
            print(f"    {len(r['groups'])} load groups, by lowest vmcnt behind their last load: " + ", ".join(f"vmcnt({k}) x{h[k]}" for k in sorted(h, key=lambda v: (v == "-", v if v != "-" else 0))))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Price the 256x256 BF6 GEMM kernel by instruction count.

    python tools/insn_model.py [--G 31] [--clock-ghz 2.0] [--asm FILE | --src FILE] [--json]

Builds the device assembly of atom_amd/csrc/gemm_w4a4_f6.hip with the Makefile's flags (or reads --asm), cuts the headline
instantiation gemm_w4a4_f6q_kernel<Cfg<256,256,4,3,2,0>, 0, false, true> into the regions its control flow has, counts the
instruction classes per region (static) and along the path a launch with G int4 groups takes (dynamic), and prices the result
with the per-SIMD costs the project's probes measured (profiles/r06/pk_mfma_probe.txt, profiles/r05/rate_probe.txt,
profiles/r01_gemm_experiments.txt section 5): everything a wave issues adds up on its SIMD, two waves share a SIMD.

    cycles per SIMD = 2 waves x (16 x MFMA + 32 x scale MFMA + 4 x VALU + 4 x LDS)

Two classes of matrix instruction: `mfma` is the dot products (BF6 v_mfma_f32_16x16x128_f8f6f4, INT8 v_mfma_i32_16x16x64_i8: 16 cycles),
`mfma_scale` the scale-product tiles (v_mfma_f32_16x16x1_4b_f32, scale_tile4 in the kernel source: 8 passes = 32 pipe cycles; the
v_mfma_f32_4x4x1_16b_f32 of the -DATOM_F6_SCALE4X4 probe build counts here too, its 8 pipe cycles priced as 32 as well -- the probe
measured 18-24 issue cycles for it, profiles/f6q_scale_mfma/probe.txt).

Regions, found from the loop labels and the MFMA counts (the BF6 MFMA marks a K step: 32 per step; the INT8 MFMA the keeper):
    prologue   kernel entry .. header of the main loop: tile setup, prologue LDS-DMA, first fragments, K steps 0-2 (96 MFMA)
    loop       the main loop body: three K steps on compile-time stage slots (96 MFMA)
    tail_ct    main loop exit .. header of the generic loop: up to two K steps on compile-time slots (64 MFMA)
    tail_gen   the generic loop body: one K step on run-time slots, executed twice (32 MFMA)
    keeper     generic loop exit .. end: the carried pair, the INT8 keeper step and the output stores (64 INT8 MFMA per copy;
               a kernel with a whole-tile store path has two copies, and the dynamic count takes the one whose stores use a
               scalar base)
The static count of a region includes its not-taken side blocks (for example the G < 6 prologue), as a listing would.
Exits with status 1 if the instantiation spills, uses scratch memory, or does not have the expected shape.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "atom_amd", "csrc")
HEADLINE = "gemm_w4a4_f6q_kernelINS0_3CfgILi256ELi256ELi4ELi3ELi2ELi0EEELi0ELb0ELb1EEE"
CLASSES = ("mfma", "mfma_scale", "valu", "lds", "vmem", "salu", "waitcnt", "barrier")
COST = {"mfma": 16, "mfma_scale": 32, "valu": 4, "lds": 4}          # cycles per instruction on a SIMD shared by two waves
WAVES_PER_SIMD = 2


class ModelError(RuntimeError):
    pass


def makefile_flags():
    """HIPCC, ARCH and CXXFLAGS as atom_amd/csrc/Makefile sets them."""
    v = {}
    with open(os.path.join(CSRC, "Makefile")) as f:
        for line in f:
            m = re.match(r"^(HIPCC|ARCH|CXXFLAGS)\s*[:?]?=\s*(.*)$", line)
            if m:
                v[m.group(1)] = m.group(2).strip()
    hipcc = os.environ.get("HIPCC", v["HIPCC"])
    flags = v["CXXFLAGS"].replace("$(ARCH)", v["ARCH"]).split()
    return hipcc, flags


def build_asm(src=None, extra=()):
    hipcc, flags = makefile_flags()
    src = src or os.path.join(CSRC, "gemm_w4a4_f6.hip")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "f6.s")
        cmd = [hipcc] + flags + list(extra) + ["-I", CSRC, "-S", "--cuda-device-only", src, "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise ModelError("assembly build failed:\n" + r.stderr[-4000:])
        with open(out) as f:
            return f.read()


def kernel_text(asm, key=HEADLINE):
    """(body lines, footer/metadata facts) of the kernel whose mangled name contains `key`."""
    lines = asm.splitlines()
    start = [i for i, l in enumerate(lines) if re.match(r"^_Z\S*" + re.escape(key) + r"\S*:", l)]
    if len(start) != 1:
        raise ModelError("headline instantiation found %d times" % len(start))
    s = start[0]
    name = lines[s].split(":")[0]
    # the body ends at the last s_endpgm in front of the kernel descriptor
    k = next(i for i in range(s, len(lines)) if lines[i].strip().startswith(".amdhsa_kernel"))
    e = max(i for i in range(s, k) if lines[i].strip().startswith("s_endpgm"))
    facts = {"name": name}
    for l in lines[k:k + 140]:
        m = re.match(r"^;\s*(NumVgprs|NumAgprs|TotalNumVgprs|ScratchSize|Occupancy|codeLenInByte|TotalNumSgprs)\s*[:=]\s*(\d+)", l)
        if m:
            facts[m.group(1)] = int(m.group(2))
        m = re.match(r"^\s*\.amdhsa_private_segment_fixed_size\s+(\d+)", l)
        if m:
            facts["private_segment_fixed_size"] = int(m.group(1))
        if l.startswith("\t.section") and "Kernel info" not in l and "NumVgprs" in facts:
            break
    # spill counts from the code object metadata
    for i, l in enumerate(lines):
        if l.strip().startswith(".name:") and l.split()[-1] == name:
            for x in lines[i:i + 16]:
                m = re.match(r"^\s*\.(sgpr_spill_count|vgpr_spill_count):\s*(\d+)", x)
                if m:
                    facts[m.group(1)] = int(m.group(2))
    return lines[s + 1:e + 1], facts


def classify(line):
    t = line.strip()
    if not t or t.startswith((";", ".", "//")) or t.endswith(":") or re.match(r"^\.?[A-Za-z_][\w.$]*:", t):
        return None
    op = t.split()[0]
    if op.startswith(("v_mfma_f32_16x16x1_", "v_mfma_f32_4x4x1_")):
        return "mfma_scale"
    if op.startswith("v_mfma"):
        return "mfma"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith("s_waitcnt"):
        return "waitcnt"
    if op.startswith("s_barrier"):
        return "barrier"
    if op.startswith("s_"):
        return "salu"
    return None


def count(lines):
    c = {k: 0 for k in CLASSES}
    for l in lines:
        k = classify(l)
        if k:
            c[k] += 1
    return c


def n_ops(lines, prefix):
    return sum(1 for l in lines if l.strip().startswith(prefix))


def loops(body):
    """[(header line, back-edge line)] of the innermost loops, in program order."""
    out = []
    for i, l in enumerate(body):
        m = re.match(r"^(\.LBB\d+_\d+):.*Inner Loop Header", l)
        if m:
            lab = m.group(1)
            j = max(k for k in range(i, len(body)) if re.match(r"^\s+s_c?branch\w*\s+" + re.escape(lab) + r"\s*$", body[k]))
            # blocks of the loop that the compiler placed behind the back edge carry the header's name in their comment
            tag = "in Loop: Header=" + lab[2:] + " "
            nxt = [k for k in range(j + 1, len(body)) if re.match(r"^\.LBB\d+_\d+:", body[k])]
            for n, k in enumerate(nxt):
                if tag not in body[k]:
                    break
                j = (nxt[n + 1] if n + 1 < len(nxt) else len(body)) - 1
            out.append((i, j))
    return out


def regions(body):
    lp = loops(body)
    step_loops = [(a, b) for a, b in lp if n_ops(body[a:b + 1], "v_mfma_f32_16x16x128_f8f6f4") > 0]
    if len(step_loops) != 2:
        raise ModelError("expected the main loop and the generic tail loop, found %d K-step loops" % len(step_loops))
    (m0, m1), (g0, g1) = step_loops
    reg = {
        "prologue": body[:m0],
        "loop": body[m0:m1 + 1],
        "tail_ct": body[m1 + 1:g0],
        "tail_gen": body[g0:g1 + 1],
    }
    keeper = body[g1 + 1:]
    i8 = [i for i, l in enumerate(keeper) if l.strip().startswith("v_mfma_i32_16x16x64_i8")]
    if len(i8) == 64:
        reg["keeper"] = keeper
    elif len(i8) == 128:                      # two copies: cut at the last label in front of the second copy's first MFMA
        cut = max(i for i in range(i8[63], i8[64]) if re.match(r"^\.LBB\d+_\d+:", keeper[i]))
        a, b = keeper[:cut], keeper[cut:]
        # what precedes the branch that picks a copy (the carried pair, the wait and the barrier) is common to both
        br = [i for i in range(i8[0]) if re.match(r"^\s+s_cbranch", keeper[i])]
        first = br[-1] + 1 if br else 0
        common, a = a[:first], a[first:]

        def scalar_base(x):
            st = [l for l in x if l.strip().startswith("global_store")]
            return sum(1 for l in st if re.search(r"\bs\[\d+:\d+\]", l)) * 2 > len(st)
        whole, ragged = (a, b) if scalar_base(a) else (b, a)
        if scalar_base(ragged) or not scalar_base(whole):
            raise ModelError("keeper: cannot tell the whole-tile copy from the ragged one")
        reg["keeper"] = common + whole
        reg["keeper_ragged"] = common + ragged
    else:
        raise ModelError("keeper region has %d INT8 MFMA, expected 64 per copy" % len(i8))
    expect = {"prologue": 96, "loop": 96, "tail_ct": 64, "tail_gen": 32}
    for k, n in expect.items():
        got = n_ops(reg[k], "v_mfma_f32_16x16x128_f8f6f4")
        if got != n:
            raise ModelError("region %s has %d BF6 MFMA, expected %d" % (k, got, n))
    return reg


def schedule(G):
    """How often each region runs for G int4 groups (the kernel's own step schedule; G >= 6: a regular first step)."""
    if G < 6:
        raise ModelError("the dynamic count covers G >= 6 (a launch whose K loop starts on the compile-time-slot body)")
    s, n_loop = 3, 0
    while s + 4 < G:
        s += 3
        n_loop += 1
    n_ct = 0
    for _ in range(2):
        if s + 2 < G:
            s += 1
            n_ct += 1
    n_gen = G - s
    return {"prologue": 1, "loop": n_loop, "tail_ct": n_ct / 2.0, "tail_gen": n_gen, "keeper": 1}


def check_resources(body, facts):
    bad = []
    for k in ("ScratchSize", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count"):
        if facts.get(k, 0) != 0:
            bad.append("%s = %d" % (k, facts[k]))
    n = n_ops(body, "scratch_") + sum(1 for l in body if re.match(r"^\s+buffer_(load|store)\S*\s.*\boffen\b.*s\[0:3\]", l))
    if n:
        bad.append("%d scratch memory instructions" % n)
    if facts.get("Occupancy", 2) < 2:
        bad.append("occupancy %d" % facts["Occupancy"])
    return bad


def model(asm, G=31, clock_ghz=2.0):
    body, facts = kernel_text(asm)
    reg = regions(body)
    static = {k: count(v) for k, v in reg.items()}
    sched = schedule(G)
    dyn = {c: sum(static[r][c] * sched[r] for r in sched) for c in CLASSES}
    cyc = {r: WAVES_PER_SIMD * sum(COST[c] * static[r][c] for c in COST) for r in static}
    total = sum(cyc[r] * sched[r] for r in sched)
    loop = reg["loop"]
    return {
        "kernel": facts["name"], "facts": facts, "spill_or_scratch": check_resources(body, facts),
        "G": G, "clock_ghz": clock_ghz, "static": static, "runs": sched, "dynamic": dyn,
        "region_cycles": cyc, "cycles_per_simd": total, "predicted_us": total / (clock_ghz * 1e3),
        "per_step": {"mfma": static["loop"]["mfma"] / 3.0, "mfma_scale": static["loop"]["mfma_scale"] / 3.0, "valu": static["loop"]["valu"] / 3.0, "lds": static["loop"]["lds"] / 3.0,
                     "cycles": cyc["loop"] / 3.0},
        "loop_waits": sorted((w, sum(1 for l in loop if l.strip() == w)) for w in {l.strip() for l in loop if l.strip().startswith("s_waitcnt")}),
        "valu_per_mfma": dyn["valu"] / dyn["mfma"] if dyn["mfma"] else 0.0,
    }


def render(r):
    o = []
    f = r["facts"]
    o.append("kernel   %s" % r["kernel"])
    o.append("resources: %d VGPR, %d AGPR, scratch %d B, spills vgpr %d sgpr %d, occupancy %d, code %d B" % (
        f.get("NumVgprs", -1), f.get("NumAgprs", -1), f.get("ScratchSize", -1), f.get("vgpr_spill_count", -1),
        f.get("sgpr_spill_count", -1), f.get("Occupancy", -1), f.get("codeLenInByte", -1)))
    o.append("")
    o.append("static counts per wave")
    o.append("%-14s %6s %10s %6s %6s %6s %6s %8s %8s %6s %10s" % (("region",) + CLASSES + ("runs", "cycles/run")))
    for k in ("prologue", "loop", "tail_ct", "tail_gen", "keeper", "keeper_ragged"):
        if k in r["static"]:
            s = r["static"][k]
            runs = r["runs"].get(k, 0)
            o.append("%-14s %6d %10d %6d %6d %6d %6d %8d %8d %6g %10d" % ((k,) + tuple(s[c] for c in CLASSES) + (runs, r["region_cycles"][k])))
    o.append("(tail_ct holds two K steps; runs counts it in halves.  keeper_ragged is the copy a ragged tile takes.)")
    o.append("")
    p = r["per_step"]
    o.append("main loop per K step: %.0f MFMA, %.0f scale MFMA, %.2f VALU (%.3f per MFMA), %.0f LDS, %.0f cycles" % (
        p["mfma"], p["mfma_scale"], p["valu"], p["valu"] / p["mfma"], p["lds"], p["cycles"]))
    o.append("main loop waits: " + ", ".join("%s x%d" % (w.replace("s_waitcnt ", ""), n) for w, n in r["loop_waits"]))
    o.append("")
    d = r["dynamic"]
    o.append("dynamic counts per wave at G = %d: %d MFMA, %d scale MFMA, %d VALU (%.2f per MFMA), %d LDS, %d VMEM, %d SALU" % (
        r["G"], d["mfma"], d["mfma_scale"], d["valu"], r["valu_per_mfma"], d["lds"], d["vmem"], d["salu"]))
    o.append("model: 2 waves x (16 x MFMA + 32 x scale MFMA + 4 x VALU + 4 x LDS) = %d cycles per SIMD = %.2f us at %.3f GHz" % (
        r["cycles_per_simd"], r["predicted_us"], r["clock_ghz"]))
    if r["spill_or_scratch"]:
        o.append("FAIL: " + "; ".join(r["spill_or_scratch"]))
    return "\n".join(o)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--G", type=int, default=31, help="int4 groups of the launch (K = 128 (G + 1)); default 31 = K 4096")
    ap.add_argument("--clock-ghz", type=float, default=2.0)
    ap.add_argument("--asm", help="read this device assembly instead of building it")
    ap.add_argument("--src", help="build this source file instead of atom_amd/csrc/gemm_w4a4_f6.hip")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    try:
        asm = open(a.asm).read() if a.asm else build_asm(a.src)
        r = model(asm, a.G, a.clock_ghz)
    except ModelError as e:
        print("insn_model: %s" % e, file=sys.stderr)
        return 1
    print(json.dumps(r) if a.json else render(r))
    return 1 if r["spill_or_scratch"] else 0


if __name__ == "__main__":
    sys.exit(main())

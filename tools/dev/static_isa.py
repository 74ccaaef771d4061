#!/usr/bin/env python3
"""Static instruction table of one k_substeps instantiation: what the vector slots are spent on, per phase and per line (no GPU needed).

    python tools/dev/static_isa.py [kernel-symbol-substring] [--phase N] [--lines LO HI] [--post] [--spills] [--min K]

Sibling of static_valu.py, which it supersedes.  Builds the engine with the flags of build_engine plus -gline-tables-only into a scratch directory
(MQE_SKIP_BUILD=1: reuse the last build; MQE_EXTRA_FLAGS: more flags; MQE_ISA_SRC: another translation unit than mqe_engine.hip, e.g.
one that includes the headers and instantiates a single kernel explicitly -- a build of a minute instead of three), disassembles the kernel, symbolizes every instruction with its
inline chain and attributes it to the line of phys_substep (or post_body, or k_substeps itself) that transitively issued it.  Beside
the VALU total of each phase it prints the instructions that compute nothing: plain v_mov_b32, DPP moves, v_readlane /
v_readfirstlane, v_writelane, v_cndmask and s_nop.  The phases are the TSTAMP taps of csrc/kernels_physics.hpp.

    --phase N     restrict the line report to phase N (the tap number in the table's first column; 15 = store / integrate)
    --lines LO HI restrict the line report to these source lines of kernels_physics.hpp
    --post        line report of the epilogue (post_body, kernels_step.hpp)
    --min K       lines with fewer than K VALU instructions are left out of a line report (default 4)
    --spills      the scalar spills: every v_writelane into a spill VGPR with the instruction that produced the value, every v_readlane
                  out of one with the first instruction that consumes it, both by kind and by source line, and how many of the reloads
                  sit inside the substep loop (the loop whose body holds the four s_setprio)

The first line printed is the kernel's resource line from the code object's metadata (VGPRs, SGPRs, SGPR spills, VGPR spills, scratch,
LDS), as tools/dev/kernel_resources.sh reads it, with the SGPR spill count that script leaves out."""
import collections, os, re, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CSRC = os.path.join(ROOT, "multiagent-quadruped-environment_amd", "csrc")
LLVM = "/opt/rocm/lib/llvm/bin"
T = "/tmp/static_isa"
COLS = ("valu", "mov", "dpp_mov", "readlane", "writelane", "cndmask", "s_nop")


def classify(op):
    """the columns an instruction counts in"""
    c = []
    if op.startswith("v_"):
        c.append("valu")
        if op in ("v_mov_b32_e32", "v_mov_b32_e64"): c.append("mov")
        elif op.startswith("v_mov_b32_dpp"): c.append("dpp_mov")
        elif op.startswith(("v_readlane_b32", "v_readfirstlane_b32")): c.append("readlane")
        elif op.startswith("v_writelane_b32"): c.append("writelane")
        elif op.startswith("v_cndmask"): c.append("cndmask")
    elif op == "s_nop":
        c.append("s_nop")
    return c


def code_object(lib, out):
    subprocess.check_call([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={out}.fat", lib])
    subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={out}.fat", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={out}"])
    return out


def resources(co, name):
    """the kernel's metadata entry as a dict of its scalar fields"""
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True).stdout
    for blk in notes.split("- .agpr_count:")[1:]:
        blk = ".agpr_count:" + blk
        f = dict(re.findall(r"\.(\w+):\s*(\S+)", blk))
        if f.get("name") == name:
            return f
    return {}


def sregs(tok):
    """scalar registers an operand names: 's4' -> {4}, 's[4:5]' -> {4, 5}, 'vcc' -> {'vcc'}"""
    tok = tok.strip().rstrip(",")
    m = re.fullmatch(r"s(\d+)", tok)
    if m: return {int(m.group(1))}
    m = re.fullmatch(r"s\[(\d+):(\d+)\]", tok)
    if m: return set(range(int(m.group(1)), int(m.group(2)) + 1))
    return set()


def disassemble(co, name):
    """[(address, mnemonic, [operands])] of one kernel"""
    dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", f"--disassemble-symbols={name}", co], capture_output=True, text=True).stdout
    ins = []
    for l in dis.splitlines():
        m = re.match(r"\s+(\S+)\s*(.*?)\s*// ([0-9A-F]{12}):", l)
        if m:
            ins.append((int(m.group(3), 16), m.group(1), [t.strip() for t in m.group(2).split(",")] if m.group(2) else []))
    return ins


def substep_loop(ins):
    """(head address, back-edge address) of the innermost loop that holds every s_setprio of the kernel, or None"""
    prio = [a for a, op, _ in ins if op == "s_setprio"]
    if not prio: return None
    best = None
    for a, op, args in ins:
        if op.startswith(("s_cbranch", "s_branch")) and args:
            imm = int(args[0], 0) & 0xFFFF
            tgt = a + 4 + 4 * (imm - 0x10000 if imm & 0x8000 else imm)
            if tgt <= min(prio) and a >= max(prio) and (best is None or a - tgt < best[1] - best[0]):
                best = (tgt, a)
    return best


def main():
    argv = sys.argv[1:]
    sym_sub = argv[0] if argv and not argv[0].startswith("--") else "k_substepsILi2ELi0ELi1ELb0ELb0EE"
    opt = lambda k, n: [int(x) for x in argv[argv.index(k) + 1: argv.index(k) + 1 + n]] if k in argv else None
    lines_rng, only_phase, min_valu = opt("--lines", 2), opt("--phase", 1), (opt("--min", 1) or [4])[0]
    os.makedirs(T, exist_ok=True)
    fp = ["-fno-hip-fp32-correctly-rounded-divide-sqrt", "-fno-honor-nans", "-fno-honor-infinities", "-fno-signed-zeros", "-fno-math-errno",
          "-freciprocal-math", "-fgpu-flush-denormals-to-zero"]
    if not os.environ.get("MQE_SKIP_BUILD"):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC", "-Wno-unused-value", "-Wno-comment", "-fno-slp-vectorize",
                               *fp, *os.environ.get("MQE_EXTRA_FLAGS", "").split(), "-gline-tables-only", "-I", CSRC, os.environ.get("MQE_ISA_SRC") or os.path.join(CSRC, "mqe_engine.hip"), "-o", f"{T}/dbg.so"])
    co = code_object(f"{T}/dbg.so", f"{T}/dev.co")
    syms = subprocess.run([f"{LLVM}/llvm-readelf", "-s", "-W", co], capture_output=True, text=True).stdout
    name = [l.split()[-1] for l in syms.splitlines() if sym_sub in l and " FUNC " in l][0]
    ins = disassemble(co, name)
    out = subprocess.run([f"{LLVM}/llvm-symbolizer", f"--obj={co}", "--inlines", "--functions=short", "--output-style=LLVM"],
                         input="\n".join(hex(a) for a, _, _ in ins) + "\n", capture_output=True, text=True).stdout
    blocks = out.strip().split("\n\n")
    src = open(os.path.join(CSRC, "kernels_physics.hpp")).read().split("\n")
    src_step = open(os.path.join(CSRC, "kernels_step.hpp")).read().split("\n")
    taps = [(i + 1, int(re.search(r"TSTAMP\((\d+)\)", l).group(1))) for i, l in enumerate(src) if re.match(r"\s*TSTAMP\(\d+\);", l)]
    NAMES = {0: "prologue", 1: "load", 2: "FK", 3: "inertia+Mcols", 4: "-", 5: "schur", 6: "Minv rows", 7: "v*", 8: "spheres/prims", 9: "terrain", 10: "pairs/self",
             11: "records", 12: "-", 13: "GS", 14: "lambda->v, limits", 15: "store/integrate"}

    def phase(ln):
        for line, tap in taps:
            if ln < line: return tap
        return 15

    # where[i] = (kind, line): kind = phase number of phys_substep, "post" (post_body) or "kern" (k_substeps itself)
    where = []
    for b in blocks:
        ls = b.strip().split("\n")
        frames = [(ls[i], ls[i + 1]) for i in range(0, len(ls) - 1, 2)]
        ln = None
        for fn, loc in frames:
            if fn.startswith("phys_substep") and "kernels_physics.hpp" in loc: ln = int(loc.split(":")[-2])
        if ln is not None and ln > 0: where.append((phase(ln), ln)); continue
        if ln == 0: where.append((-1, 0)); continue              # inside phys_substep, no source line
        pl = None
        for fn, loc in frames:
            if fn.startswith("post_body") and "kernels_step.hpp" in loc: pl = int(loc.split(":")[-2])
        if pl is not None or any("post_body" in f[0] for f in frames): where.append(("post", pl or 0)); continue
        kl = 0
        for fn, loc in frames:
            if fn.startswith("k_substeps") and "kernels_physics.hpp" in loc: kl = int(loc.split(":")[-2])
        where.append(("kern", kl))
    where += [("kern", 0)] * (len(ins) - len(where))

    res = resources(co, name)
    vg = int(res.get("vgpr_count", 0) or 0)
    print(name)
    print("  resources: VGPR %s  SGPR %s  SGPR spills %s  VGPR spills %s  scratch %s B  LDS(static) %s B  waves/SIMD %s" % (
        res.get("vgpr_count", "?"), res.get("sgpr_count", "?"), res.get("sgpr_spill_count", "?"), res.get("vgpr_spill_count", "?"),
        res.get("private_segment_fixed_size", "?"), res.get("group_segment_fixed_size", "?"), min(8, 512 // (-(-vg // 8) * 8)) if vg else "?"))

    rows, byline = collections.defaultdict(collections.Counter), collections.defaultdict(collections.Counter)
    noline = collections.Counter()
    for (a, op, args), (kind, ln) in zip(ins, where):
        for c in classify(op):
            rows[kind][c] += 1; rows["all"][c] += 1
            if isinstance(kind, int): rows["phys"][c] += 1
            byline[(kind if not isinstance(kind, int) else "phys", ln)][c] += 1
            if ln == 0: noline[c] += 1
    hdr = "  %-44s" % "where" + "".join("%10s" % c for c in COLS)
    print(hdr)
    fmt = lambda label, r: "  %-44s" % label + "".join("%10d" % r[c] for c in COLS)
    for k in sorted(k for k in rows if isinstance(k, int)):
        print(fmt("%2d %s" % (k, NAMES.get(k, "(no source line)")), rows[k]))
    print(fmt("phys_substep (the loop body, all phases)", rows["phys"]))
    print(fmt("k_substeps itself (actuator net, loads, logs)", rows["kern"]))
    print(fmt("post_body (epilogue, once per launch)", rows["post"]))
    print(fmt("whole kernel", rows["all"]))
    print(fmt("  of these without a source line", noline))

    if lines_rng or only_phase:
        print("  lines of kernels_physics.hpp" + (" in phase %d" % only_phase[0] if only_phase else "") + ":")
        print("    %5s" % "line" + "".join("%10s" % c for c in COLS))
        for (kind, ln) in sorted(k for k in byline if k[0] == "phys"):
            if ln <= 0 or byline[(kind, ln)]["valu"] < min_valu: continue
            if lines_rng and not (lines_rng[0] <= ln < lines_rng[1]): continue
            if only_phase and phase(ln) != only_phase[0]: continue
            print("    %5d" % ln + "".join("%10d" % byline[(kind, ln)][c] for c in COLS) + "  " + src[ln - 1].strip()[:110])
    if "--post" in argv:
        print("  lines of kernels_step.hpp (post_body):")
        for (kind, ln) in sorted(k for k in byline if k[0] == "post"):
            if ln <= 0 or byline[(kind, ln)]["valu"] < max(min_valu, 6): continue
            print("    %5d" % ln + "".join("%10d" % byline[(kind, ln)][c] for c in COLS) + "  " + src_step[ln - 1].strip()[:110])

    if "--spills" in argv:
        spill_v = {args[0] for _, op, args in ins if op.startswith("v_writelane_b32")}
        loop = substep_loop(ins)
        print("  spill VGPRs:", " ".join(sorted(spill_v)) or "none", "| substep loop:", "%#x .. %#x" % loop if loop else "not found")
        label = lambda i: ("%s:%d" % ({"post": "kernels_step.hpp", "kern": "kernels_physics.hpp"}.get(where[i][0], "kernels_physics.hpp"), where[i][1]))
        prod, cons, prod_line, cons_line, in_loop = collections.Counter(), collections.Counter(), collections.Counter(), collections.Counter(), 0
        slot_prod, loop_slots = {}, collections.defaultdict(list)         # (spill VGPR, lane) -> the producer of the value it holds at this address (slots are reused); the reloads inside the loop per slot
        for i, (a, op, args) in enumerate(ins):
            if op.startswith("v_writelane_b32") and args[0] in spill_v:
                want = sregs(args[1])
                for j in range(i - 1, -1, -1):
                    if ins[j][2] and not ins[j][1].startswith(("s_cmp", "s_cbranch", "s_branch", "s_waitcnt", "s_nop")) and sregs(ins[j][2][0]) & want:
                        prod[ins[j][1]] += 1; prod_line[label(j)] += 1; slot_prod[(args[0], args[2])] = "%s %s" % (ins[j][1], label(j)); break
                else:
                    prod["(kernel argument / live-in)"] += 1
            if op.startswith("v_readlane_b32") and len(args) > 1 and args[1] in spill_v:
                want = sregs(args[0])
                if loop and loop[0] <= a <= loop[1]: in_loop += 1; loop_slots[(args[1], args[2], slot_prod.get((args[1], args[2]), "?"))].append(label(i))
                for j in range(i + 1, len(ins)):
                    if any(sregs(t) & want for t in ins[j][2][1:] if not ins[j][1].startswith("v_writelane")) or (ins[j][1].startswith(("s_cmp", "s_bitcmp")) and any(sregs(t) & want for t in ins[j][2])):
                        cons[ins[j][1]] += 1; cons_line[label(i)] += 1; break
        nw, nr = sum(prod.values()), sum(cons.values())
        print("  spill stores (v_writelane into a spill VGPR): %d, by producer:" % nw, ", ".join("%s %d" % kv for kv in prod.most_common()))
        print("    by line:", ", ".join("%s x%d" % kv for kv in prod_line.most_common(24)))
        print("  spill reloads (v_readlane out of a spill VGPR): %d, inside the substep loop: %d, by consumer:" % (nr, in_loop), ", ".join("%s %d" % kv for kv in cons.most_common()))
        print("    by line:", ", ".join("%s x%d" % kv for kv in cons_line.most_common(32)))
        for slot in sorted(loop_slots):
            print("    in the loop: %s[%s] <- %-44s reloaded at %s" % (slot[0], slot[1], slot[2], " ".join(sorted(set(loop_slots[slot])))))


if __name__ == "__main__":
    main()

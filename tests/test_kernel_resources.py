"""Registers, spills and scratch of the k_substeps instances, read from the built library's gfx950 code object (no GPU needed).

k_substeps is bound by the vector ALU's issue slots.  A wave-uniform value that does not fit the scalar register file is
parked in a lane of a spill VGPR and costs a v_readlane -- a vector slot, plus hazard s_nops -- at every later use.  The parent of the
change that added this file spilled 145 SGPRs in the headline kernel k_substeps<2, 0, 1, false, false> and reloaded 81 of them inside
the substep loop; the kernel now reads its state pointers from the kernel arguments where it uses them and launders the model pointer
and the env index once per substep, spills 32, and reloads none inside the loop.  This file keeps it there:

  * every k_substeps instance: no VGPR spill, no scratch (private_segment_fixed_size == 0);
  * the 16-envs-per-CU class (one env per wavefront; robots only, + one link, or PS_F_FEW): at most 128 VGPRs = 4 wavefronts per SIMD;
  * the headline kernel: at most SGPR_SPILL_BOUND spilled SGPRs (the count reached, 32: a multiple of 8 as it is; the parent's
    was PARENT_SGPR_SPILLS), and no v_readlane out of a spill VGPR between the substep loop's back-edge target and its back edge.  The
    spill VGPRs are the destinations of the kernel's v_writelane; the substep loop is the one whose head carries the four s_setprio.

tools/dev/static_isa.py prints the same facts with their source lines."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "multiagent-quadruped-environment_amd", "csrc", "libmqe_hip.so")
LLVM = "/opt/rocm/lib/llvm/bin"
TOOLS = ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf", "llvm-objdump")
HEADLINE = "_Z10k_substepsILi2ELi0ELi1ELb0ELb0EE"
PARENT_SGPR_SPILLS = 145
SGPR_SPILL_BOUND = 32
PS_F_LINK, PS_F_FEW = 1, 16

pytestmark = pytest.mark.skipif(not (os.path.isfile(LIB) and all(os.path.isfile(os.path.join(LLVM, t)) for t in TOOLS)),
                                reason="needs the built HIP engine and the ROCm LLVM tools (no hipcc on this machine)")


@pytest.fixture(scope="module")
def code_object(tmp_path_factory):
    d = tmp_path_factory.mktemp("co")
    fat, co = str(d / "fat.bin"), str(d / "dev.co")
    subprocess.check_call([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", LIB, str(d / "stripped.so")])
    subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"])
    return co


@pytest.fixture(scope="module")
def kernels(code_object):
    """{mangled name: metadata fields} of every k_substeps instance"""
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", code_object], capture_output=True, text=True, check=True).stdout
    out = {}
    for blk in notes.split("- .agpr_count:")[1:]:
        f = dict(re.findall(r"\.(\w+):\s*(\S+)", ".agpr_count:" + blk))
        if f.get("name", "").startswith("_Z10k_substepsI"):
            out[f["name"]] = f
    assert len(out) >= 20, sorted(out)          # 12 shapes x 2 actuator forms, + the paired and the timed instances
    return out


def template_args(name):
    """(TA, TP, EPW, TIMED, ACT32) of a mangled k_substeps instance"""
    m = re.match(r"_Z10k_substepsILi(n?\d+)ELi(n?\d+)ELi(\d+)ELb([01])ELb([01])EE", name)
    assert m, name
    i = lambda t: -int(t[1:]) if t.startswith("n") else int(t)
    return i(m.group(1)), i(m.group(2)), int(m.group(3)), m.group(4) == "1", m.group(5) == "1"


def small_class(name):
    """kernels_physics.hpp ShapeClass<TP>::small, one env per wavefront: compiled for 4 wavefronts per SIMD"""
    ta, tp, epw, _, _ = template_args(name)
    return epw == 1 and (tp == 0 or tp == PS_F_LINK or (tp > 0 and tp & PS_F_FEW))


# <TA, TP> of the shape table in csrc/mqe_engine.hip (shape_row_of)
SHAPES = [(2, 0), (1, 0), (2, 16), (2, 1), (2, 18), (2, 22), (2, 24), (3, 34), (2, 2), (4, 2), (2, -1), (0, -1)]


def test_shape_list_is_complete(kernels):
    assert {template_args(n)[:2] for n in kernels} == set(SHAPES)


@pytest.mark.parametrize("ta,tp", SHAPES)
def test_no_vgpr_spill_no_scratch(kernels, ta, tp):
    """Every instance of the shape (actuator forms, paired, timed).  At the parent k_substeps<2, PS_F_LINK> (go1seesaw, door, tug) and
    k_substeps<2, PS_F_STATIC | PS_F_FEW> (bridge, wrestling) kept 2 VGPRs (12 bytes) in scratch, in both actuator forms; laundering
    the lane id in place gave them the register they lacked (kernels_physics.hpp, k_substeps)."""
    mine = {n: f for n, f in kernels.items() if template_args(n)[:2] == (ta, tp)}
    assert mine
    for n, f in sorted(mine.items()):
        print(n[:40], "vgpr", f["vgpr_count"], "sgpr spills", f["sgpr_spill_count"], "vgpr spills", f["vgpr_spill_count"], "scratch", f["private_segment_fixed_size"])
    bad = {n[:40]: (int(f["vgpr_spill_count"]), int(f["private_segment_fixed_size"])) for n, f in mine.items()
           if int(f["vgpr_spill_count"]) != 0 or int(f["private_segment_fixed_size"]) != 0}
    assert not bad, f"(VGPR spills, scratch bytes): {bad}"


def test_small_class_fits_four_waves(kernels):
    small = {n: int(f["vgpr_count"]) for n, f in kernels.items() if small_class(n)}
    assert len(small) >= 10, sorted(small)
    assert all(v <= 128 for v in small.values()), small


def disassemble(co, name):
    dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", f"--disassemble-symbols={name}", co], capture_output=True, text=True, check=True).stdout
    ins = []
    for line in dis.splitlines():
        m = re.match(r"\s+(\S+)\s*(.*?)\s*// ([0-9A-F]{12}):", line)
        if m:
            ins.append((int(m.group(3), 16), m.group(1), [t.strip() for t in m.group(2).split(",")] if m.group(2) else []))
    return ins


def test_headline_scalar_spills(kernels, code_object):
    name = next(n for n in kernels if n.startswith(HEADLINE))
    spills = int(kernels[name]["sgpr_spill_count"])
    print("SGPR spills", spills, "(parent:", PARENT_SGPR_SPILLS, ")")
    assert spills <= SGPR_SPILL_BOUND < PARENT_SGPR_SPILLS
    ins = disassemble(code_object, name)
    assert len(ins) > 5000
    spill_vgprs = {args[0] for _, op, args in ins if op.startswith("v_writelane_b32")}
    # the substep loop: the innermost backward branch around the four s_setprio
    prio = [a for a, op, _ in ins if op == "s_setprio"]
    assert len(prio) == 4, prio
    loop = None
    for a, op, args in ins:
        if op.startswith(("s_cbranch", "s_branch")) and args:
            imm = int(args[0], 0) & 0xFFFF
            tgt = a + 4 + 4 * (imm - 0x10000 if imm & 0x8000 else imm)
            if tgt <= min(prio) and a >= max(prio) and (loop is None or a - tgt < loop[1] - loop[0]):
                loop = (tgt, a)
    assert loop is not None, "no backward branch around the s_setprio"
    body = [(a, op, args) for a, op, args in ins if loop[0] <= a <= loop[1]]
    assert len(body) > 3000, len(body)          # the whole physics body is inside
    reloads = [hex(a) for a, op, args in body if op.startswith("v_readlane_b32") and len(args) > 1 and args[1] in spill_vgprs]
    print("spill VGPRs", sorted(spill_vgprs), "loop", hex(loop[0]), hex(loop[1]), "reloads inside", len(reloads))
    assert not reloads, f"{len(reloads)} v_readlane out of {sorted(spill_vgprs)} inside the substep loop: {reloads[:8]}"


def test_kernel_argument_offsets(code_object):
    """mqe_common.hpp MQE_KARG_STATE / LATE_ARG read k_substeps' arguments from the kernel-argument segment by byte offset: the state at
    8 (behind the model pointer), 52 pointers long, nsub and lag_pos right behind it."""
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", code_object], capture_output=True, text=True, check=True).stdout
    seen = 0
    for blk in notes.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s*(\S+)", blk).group(1)
        if not name.startswith("_Z10k_substepsI"):
            continue
        args = re.findall(r"\.offset:\s*(\d+)\s*\n\s*\.size:\s*(\d+)\s*\n\s*\.value_kind:\s*(\S+)", blk)[:4]
        assert args == [("0", "8", "global_buffer"), ("8", "416", "by_value"), ("424", "4", "by_value"), ("428", "4", "by_value")], (name, args)
        seen += 1
    assert seen >= 20

"""tools/isa_diff.py: the text comparison of two disassembly listings (a pure function; no hipcc, no GPU)."""

import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
import isa_diff  # noqa: E402

K1, K2, K3 = "_Z9kernel_onePf", "_ZN2tj16traj_step_kernelILi7ELb1EEEvNS_8StepArgsE", "_Z12added_kernelPf"


def listing(kernels, base=0x1000):
    """A listing in llvm-objdump -d's format: kernels = [(symbol, [instruction, ...])], laid out from `base` with fill behind each."""
    out, addr = ["", "k.co:\tfile format elf64-amdgpu", "", "Disassembly of section .text:", ""], base
    for sym, insts in kernels:
        out.append(f"{addr:016x} <{sym}>:")
        for inst in list(insts) + ["s_nop 0", "s_nop 0"]:
            out.append(f"\t{inst:58s} // {addr:012X}: BF800000" + (f" <{sym}+0x10>" if inst.startswith("s_branch") else ""))
            addr += 4
        out.append("")
    return "\n".join(out) + "\n"


A = [(K1, ["s_load_dwordx2 s[0:1], s[4:5], 0x0", "v_mov_b32_e32 v0, 0", "s_endpgm"]),
     (K2, ["v_fma_f32 v1, v2, v3, v1", "s_branch 65533", "s_endpgm"])]


def test_identical_code_at_other_addresses_compares_equal():
    r = isa_diff.compare_listings(listing(A), listing(A, base=0x7300))
    assert r["differ"] == [] and r["removed"] == [] and r["added"] == []
    assert r["hash"]["parent"] == r["hash"]["head"]
    assert list(isa_diff.split_listing(listing(A))) == [K1, K2]
    assert isa_diff.split_listing(listing(A))[K1].count("\n") == 2   # three instructions, the fill left out


def test_a_changed_instruction_is_found_in_its_symbol():
    B = [A[0], (K2, ["v_fma_f32 v1, v2, v4, v1", "s_branch 65533", "s_endpgm"])]
    r = isa_diff.compare_listings(listing(A), listing(B))
    assert r["differ"] == [K2] and r["removed"] == [] and r["added"] == []
    assert r["hash"]["parent"] != r["hash"]["head"]


def test_an_added_symbol_is_listed_and_leaves_the_common_hash_alone():
    B = [A[0], (K3, ["s_endpgm"]), A[1]]
    r = isa_diff.compare_listings(listing(A), listing(B))
    assert r["added"] == [K3] and r["removed"] == [] and r["differ"] == []
    assert r["hash"]["parent"] == r["hash"]["head"]
    back = isa_diff.compare_listings(listing(B), listing(A))
    assert back["removed"] == [K3] and back["added"] == []


def test_notes_are_split_per_kernel():
    notes = ("Displaying notes found in: .note\n    AMDGPU Metadata:\n        ---\namdhsa.kernels:\n"
             f"  - .agpr_count:     0\n    .name:           {K1}\n    .vgpr_count:     12\n"
             f"  - .agpr_count:     0\n    .name:           {K2}\n    .vgpr_count:     255\n"
             "amdhsa.target:   amdgcn-amd-amdhsa--gfx950\namdhsa.version:\n  - 1\n  - 2\n...\n")
    split = isa_diff.split_notes(notes)
    assert list(split) == [K1, K2] and ".vgpr_count:     255" in split[K2] and "255" not in split[K1] and "amdhsa.version" not in split[K2]
    r = isa_diff.compare(split, isa_diff.split_notes(notes.replace("255", "256")))
    assert r["differ"] == [K2]

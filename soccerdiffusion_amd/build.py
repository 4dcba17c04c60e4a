"""Builds the HIP shared library in-tree for gfx950 (hipcc cross-compiles without a GPU).

    python -m soccerdiffusion_amd.build [--force] [-v]
    python -m soccerdiffusion_amd.build --variant UNIT NAME [FLAG ...]

Output: soccerdiffusion_amd/lib/libsoccerdiffusion_hip.so (git-ignored; travels with gpurun).
"""

from __future__ import annotations

import os
import shutil
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
SRC = [os.path.join(CSRC, u + ".hip") for u in ("sd_kernels", "sd_traj", "sd_train", "sd_train_chain", "sd_conv", "sd_train_traj", "sd_trajg",
                                                "sd_conv_train", "sd_swin", "sd_frames", "sd_head", "sd_session", "sd_traj_draws", "sd_eval", "sd_traj_hold",
                                                "sd_traj_ms", "sd_traj_lim", "sd_traj_slew", "sd_traj_direct", "sd_traj_acc", "sd_train_shared")]
# The sampler's translation units are compiled WITHOUT packed fp32 vector instructions (v_pk_fma/mul/add_f32): they do not overlap with
# MFMAs - neither a wave's own nor its SIMD partner's - while plain fp32 instructions do (tools/exp/coissue3.hip; NOTEBOOK.md 5.11), and
# the trajectory kernel lives on that overlap: + 1.5 % sampler throughput.  The training units lose 0.6 % with the same flag: packed.
# Nothing is packed by hand in the vector-only phases (GELU, LayerNorm, softmax) either: the feature also governs the inline assembler
# (a v_pk_*_f32 wrapper does not assemble in these units), and with two waves per SIMD a packed instruction buys ~ 14 % on the
# instructions that pack, ~ 1 % of a step (NOTEBOOK.md, round 6 addendum).
NO_PACKED_FP32 = ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]
EXTRA_FLAGS = {"sd_traj.hip": NO_PACKED_FP32, "sd_trajg.hip": NO_PACKED_FP32, "sd_traj_draws.hip": NO_PACKED_FP32, "sd_traj_hold.hip": NO_PACKED_FP32,
               "sd_traj_ms.hip": NO_PACKED_FP32, "sd_traj_lim.hip": NO_PACKED_FP32, "sd_traj_slew.hip": NO_PACKED_FP32,
               "sd_traj_direct.hip": NO_PACKED_FP32, "sd_traj_acc.hip": NO_PACKED_FP32, "sd_kernels.hip": NO_PACKED_FP32}   # the row-panel sampler (modes 0 - 2) was tuned with the flag as well
# The units that own trajectory step kernels (traj_step*): build() checks their objects - no v_pk_{fma,mul,add}_f32 in a step kernel.
STEP_KERNEL_UNITS = ("sd_traj.hip", "sd_trajg.hip", "sd_traj_draws.hip", "sd_traj_hold.hip",   # (_draws / _hold / _ms / _lim: sd_traj.h's shared-context /
                     "sd_traj_ms.hip", "sd_traj_lim.hip", "sd_traj_slew.hip",             # hold / multistep / limits / slew instantiations;
                     "sd_traj_direct.hip", "sd_traj_acc.hip")                             # _direct: a one-step decoder's twins; _acc: acceleration)
LIB_DIR = os.path.join(PKG, "lib")
LIB = os.path.join(LIB_DIR, "libsoccerdiffusion_hip.so")
ARCH = "gfx950"


def hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (need ROCm >= 7.0 with gfx950 support)")


def _obj(src: str) -> str:
    return os.path.join(LIB_DIR, os.path.splitext(os.path.basename(src))[0] + ".o")


def _dep_file(src: str) -> str:
    return _obj(src) + ".d"


def _deps(src: str):
    """The project's files the unit's object was compiled from, as the compiler listed them (-MD -MF: the source and every header of the host
    and the device pass), or None where no usable list exists.  compile_cmd() names the project's files relative to csrc/, so the list holds
    for the tree wherever it lies; absolute entries are the toolchain's own headers and are left out.  A list without the unit's own source
    was not written by this build for this unit: None."""
    try:
        with open(_dep_file(src)) as f:
            words = f.read().replace("\\\n", " ").split()
    except OSError:
        return None
    paths = [os.path.normpath(os.path.join(CSRC, w)) for w in words if not w.endswith(":") and not os.path.isabs(w)]
    if os.path.normpath(src) not in paths:
        return None
    return paths + [os.path.abspath(__file__)]


def _newer_than(deps, t: float) -> bool:
    return deps is None or any(not os.path.exists(f) or os.path.getmtime(f) > t for f in deps)


def _obj_stale(src: str) -> bool:
    return not os.path.exists(_obj(src)) or _newer_than(_deps(src), os.path.getmtime(_obj(src)))


def is_stale() -> bool:
    """The library is older than a file one of its units was compiled from, or a unit has no dependency list.  Asks nothing of the
    objects themselves: a tree that travels with lib/'s library and *.o.d files but without the objects keeps its library; one that arrives
    without the *.o.d files compiles every unit."""
    return not os.path.exists(LIB) or any(_newer_than(_deps(s), os.path.getmtime(LIB)) for s in SRC)


def _run(cmd: list, what: str, verbose: bool) -> None:
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        sys.stderr.write(res.stdout + res.stderr)
        raise RuntimeError("hipcc failed " + what)
    if verbose:
        sys.stderr.write(res.stderr)


def count_packed_fp32(asm: str) -> dict:
    """{kernel symbol: number of v_pk_{fma,mul,add}_f32 instructions} for every trajectory step kernel (traj_step_kernel / traj_step_wide_kernel /
    the generic family) in a disassembly listing (llvm-objdump -d)."""
    import re

    counts, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\w+)>:", line)
        if m:
            cur = m.group(1) if "traj_step" in m.group(1) else None
            if cur:
                counts[cur] = 0
        elif cur and re.search(r"\bv_pk_(fma|mul|add)_f32\b", line):
            counts[cur] += 1
    return counts


def llvm_tool(name: str):
    """The toolchain's own llvm tool (clang-offload-bundler, llvm-objdump, llvm-readelf) beside the compiler, or None."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc()))), "lib", "llvm", "bin", name)
    return path if os.path.exists(path) else None


def unbundle(obj: str, co: str) -> bool:
    """Writes the gfx950 code object of a unit's object file to `co`; False where the tools that take the object apart (objcopy, the
    offload bundler) are missing."""
    bundler = llvm_tool("clang-offload-bundler")
    if not shutil.which("objcopy") or not bundler:
        return False
    fat = co + ".fatbin"
    subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat], check=True)
    subprocess.run([bundler, "--type=o", f"--targets=hipv4-amdgcn-amd-amdhsa--{ARCH}", f"--input={fat}", f"--output={co}", "--unbundle"],
                   check=True, capture_output=True)
    os.remove(fat)
    return True


def packed_fp32_in_traj_kernels(obj: str):
    """count_packed_fp32 of a unit's object file, or None where the tools that take the
    object apart (objcopy, the offload bundler, llvm-objdump) are missing.  EXTRA_FLAGS removes the packed fp32 operations from that
    translation unit's target features; the flag goes through -Xclang and a toolchain update could drop it silently, so build() checks its
    effect on the code of every unit in STEP_KERNEL_UNITS."""
    import tempfile

    objdump = llvm_tool("llvm-objdump")
    with tempfile.TemporaryDirectory() as tmp:
        co = os.path.join(tmp, "k.co")
        if not objdump or not unbundle(obj, co):
            return None
        asm = subprocess.run([objdump, "-d", co], check=True, capture_output=True, text=True).stdout
    return count_packed_fp32(asm)


def compile_cmd(src: str, out: str, verbose: bool = False) -> list:
    """The compiler call for one unit of SRC, to be run with cwd = CSRC: the source and the include directory are named relative to it, so
    that the dependency list (out + '.d') names the project's files the same way wherever the tree lies."""
    flags = ["-O3", "-std=c++17", f"--offload-arch={ARCH}", "-fPIC", "-Wno-unused-value", "-I", os.path.relpath(os.path.join(REPO, "include"), CSRC)]
    if verbose:
        flags.insert(0, "-Rpass-analysis=kernel-resource-usage")
    return [hipcc(), *flags, *EXTRA_FLAGS.get(os.path.basename(src), []), "-MD", "-MF", out + ".d", "-c", os.path.relpath(src, CSRC), "-o", out]


def build(force: bool = False, verbose: bool = False) -> str:
    """One object per translation unit (recompiled only when it or a file the compiler read for it changed; the stale ones compile in
    parallel), then one link.  The units share host functions only - no relocatable device code is needed."""
    if not force and not is_stale():
        return LIB
    os.makedirs(LIB_DIR, exist_ok=True)
    jobs = []
    for src in SRC:
        if force or _obj_stale(src):
            jobs.append((src, subprocess.Popen(compile_cmd(src, _obj(src) + ".tmp", verbose), cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                               text=True)))
    for src, proc in jobs:
        out, err = proc.communicate()
        if proc.returncode != 0:
            sys.stderr.write(out + err)
            raise RuntimeError("hipcc failed compiling " + src)
        os.replace(_obj(src) + ".tmp.d", _dep_file(src))
        os.replace(_obj(src) + ".tmp", _obj(src))
        if verbose:
            sys.stderr.write(err)
        if os.path.basename(src) in STEP_KERNEL_UNITS:
            counts = packed_fp32_in_traj_kernels(_obj(src))
            if counts is None:
                sys.stderr.write("warning: objcopy / clang-offload-bundler / llvm-objdump not found: the trajectory step kernels were not checked for "
                                 "packed fp32 instructions\n")
                continue
            bad = {k: v for k, v in counts.items() if v}
            if not counts or bad:
                os.remove(_obj(src))
                os.remove(_dep_file(src))   # no dependency list: the unit (and the library) count as stale
                raise RuntimeError(f"packed fp32 instructions in the trajectory step kernels (or none of them found): {bad or counts}; "
                                   f"EXTRA_FLAGS[{os.path.basename(src)!r}] no longer takes effect")
    _run([hipcc(), f"--offload-arch={ARCH}", "-shared", "-fPIC", *[_obj(s) for s in SRC], "-o", LIB + ".tmp"], "linking " + LIB, verbose)
    os.replace(LIB + ".tmp", LIB)
    return LIB


def build_variant(unit: str, name: str, flags: list) -> str:
    """lib/variants/lib_<name>.so for A/B runs (tools/ab_build.sh): unit (e.g. 'sd_traj') recompiled with the product's flags plus `flags`,
    linked with the other units' objects of the regular build, which must be current."""
    src = os.path.join(CSRC, unit + ".hip")
    if src not in SRC:
        raise ValueError(f"{unit}: not a translation unit of the library")
    vdir = os.path.join(LIB_DIR, "variants")
    os.makedirs(vdir, exist_ok=True)
    obj, lib = os.path.join(vdir, f"{unit}_{name}.o"), os.path.join(vdir, f"lib_{name}.so")
    res = subprocess.run(compile_cmd(src, obj) + list(flags), cwd=CSRC, capture_output=True, text=True)
    if res.returncode != 0:
        sys.stderr.write(res.stdout + res.stderr)
        raise RuntimeError("hipcc failed compiling " + src)
    _run([hipcc(), f"--offload-arch={ARCH}", "-shared", "-fPIC", *[obj if s == src else _obj(s) for s in SRC], "-o", lib], "linking " + lib, False)
    os.remove(obj)
    os.remove(obj + ".d")
    return lib


if __name__ == "__main__":
    if len(sys.argv) > 3 and sys.argv[1] == "--variant":   # --variant UNIT NAME [FLAG ...]
        print(build_variant(sys.argv[2], sys.argv[3], sys.argv[4:]))
    else:
        print(build(force="--force" in sys.argv, verbose="-v" in sys.argv))

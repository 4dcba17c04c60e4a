"""The gfx950 code of two builds of the library, compared symbol by symbol (no GPU needed): the check that a change touched no kernel.

usage: python tools/isa_diff.py PARENT_LIB_DIR HEAD_LIB_DIR     (two soccerdiffusion_amd/lib/ directories, each built with
       `python -m soccerdiffusion_amd.build --force` and the same hipcc)

Every unit's object is taken apart the way build() does (build.unbundle), then llvm-objdump -d and llvm-readelf --notes on the code object.
Per symbol present in both builds, compared as text: the disassembly with the address column removed, and the kernel's entry of
amdhsa.kernels (registers, spills, LDS, scratch, kernarg layout, workgroup size).  The fill between two symbols belongs to no kernel and is
left out.  Prints the table of profiles/draws_isa.txt - kernels = entries of amdhsa.kernels, lines = lines of the disassembly, sha256[:16]
over the common symbols' texts in the parent's order - and the removed and added symbols.  Exit status 1 where a common symbol differs."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def split_listing(asm: str) -> dict:
    """{symbol: its instructions, one per line, without the address column and without the fill behind its last instruction} of a
    disassembly listing (llvm-objdump -d), in the listing's order."""
    out, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r"^[0-9a-f]+ <([^>]+)>:", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line.startswith("\t") and line.strip() != "...":   # (...: zero fill behind the section's last symbol)
            cur.append(re.sub(r"// [0-9A-Fa-f]+: ", "// ", line.rstrip()))
    for lines in out.values():
        while lines and re.match(r"\s*(s_nop|s_code_end)\b", lines[-1]):
            lines.pop()
    return {k: "\n".join(v) for k, v in out.items()}


def split_notes(notes: str) -> dict:
    """{kernel symbol: its entry of amdhsa.kernels as text} of llvm-readelf --notes."""
    entries, inside = [], False
    for line in notes.splitlines():
        if re.match(r"^\S", line):
            inside = line.startswith("amdhsa.kernels:")
        elif inside and line.startswith("  - "):
            entries.append([line.rstrip()])
        elif inside and entries:
            entries[-1].append(line.rstrip())
    return {next(ln.split(":", 1)[1].strip() for ln in e if ln.strip().startswith(".name:")): "\n".join(e) for e in entries}


def compare(parent: dict, head: dict) -> dict:
    """Two {symbol: text} maps (split_listing / split_notes): the symbols only one side has, those whose text differs, and a hash over
    the common symbols' texts in the parent's order for either side."""
    common = [k for k in parent if k in head]
    digest = {}
    for side, texts in (("parent", parent), ("head", head)):
        h = hashlib.sha256()
        for k in common:
            h.update((k + "\n" + texts[k] + "\n").encode())
        digest[side] = h.hexdigest()[:16]
    return {"removed": [k for k in parent if k not in head], "added": [k for k in head if k not in parent],
            "differ": [k for k in common if parent[k] != head[k]], "hash": digest}


def compare_listings(parent_asm: str, head_asm: str) -> dict:
    return compare(split_listing(parent_asm), split_listing(head_asm))


def read_unit(obj: str):
    """(disassembly, notes) of a unit's object file, or None where it does not exist."""
    from soccerdiffusion_amd import build

    if not os.path.exists(obj):
        return None
    with tempfile.TemporaryDirectory() as tmp:
        co = os.path.join(tmp, "k.co")
        if not build.unbundle(obj, co):
            raise RuntimeError("objcopy / clang-offload-bundler not found")
        asm = subprocess.run([build.llvm_tool("llvm-objdump"), "-d", co], check=True, capture_output=True, text=True).stdout
        notes = subprocess.run([build.llvm_tool("llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    return asm, notes


def main(parent_dir: str, head_dir: str) -> int:
    from soccerdiffusion_amd import build

    print(f"{'unit':16s} {'kernels':14s} {'lines parent/head':24s} {'common: parent':18s} {'head':18s} differ asm/notes  removed  added")
    removed, added, bad = [], [], 0
    for unit in (os.path.splitext(os.path.basename(s))[0] for s in build.SRC):
        p, h = read_unit(os.path.join(parent_dir, unit + ".o")), read_unit(os.path.join(head_dir, unit + ".o"))
        if p is None or h is None:
            print(f"{unit:16s} " + ("(no such unit in the parent)" if p is None else "(no such unit in the head)"))
            bad += h is None
            continue
        pa, ha, pn, hn = split_listing(p[0]), split_listing(h[0]), split_notes(p[1]), split_notes(h[1])
        asm, notes = compare(pa, ha), compare(pn, hn)
        both = compare({k: pa[k] + "\n" + pn.get(k, "") for k in pa}, {k: ha[k] + "\n" + hn.get(k, "") for k in ha})
        print(f"{unit:16s} {f'{len(pn)} / {len(hn)}':14s} {f'{len(p[0].splitlines())} / {len(h[0].splitlines())}':24s} {both['hash']['parent']:18s} "
              f"{both['hash']['head']:18s} {f'''{len(asm['differ'])} / {len(notes['differ'])}''':16s} {len(asm['removed']):8d} {len(asm['added']):6d}")
        bad += len(asm["differ"]) + len(notes["differ"])
        removed += [f"{unit} {k}" for k in asm["removed"]]
        added += [f"{unit} {k}" for k in asm["added"]]
        for k in asm["differ"] + notes["differ"]:
            print(f"  differs: {k}")
    for title, names in (("Removed", removed), ("Added", added)):
        print(f"\n{title} symbols: " + ("none." if not names else str(len(names))))
        for n in names:
            print("  " + n)
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))

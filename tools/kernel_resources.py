"""Per-kernel register / scratch / occupancy table from hipcc's resource-usage remarks.
usage: python tools/kernel_resources.py [substring [unit ...]]   (compiles the named units, e.g. sd_traj sd_trajg - default: every unit of
the library - for gfx950 with the product's flags: soccerdiffusion_amd.build.SRC / compile_cmd)"""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from soccerdiffusion_amd import build as b  # noqa: E402

pat = sys.argv[1] if len(sys.argv) > 1 else ""
for src in [s for s in b.SRC if not sys.argv[2:] or os.path.splitext(os.path.basename(s))[0] in sys.argv[2:]]:
    with tempfile.TemporaryDirectory() as tmp:
        out = subprocess.run(b.compile_cmd(src, os.path.join(tmp, "unit.o"), verbose=True), cwd=b.CSRC, capture_output=True, text=True).stderr
    cur = None
    rows = {}
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line) or re.search(r" Name: (\S+)", line)
        if m:
            cur = m.group(1)
            rows[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur:
            rows[cur][m.group(1).strip()] = int(m.group(2))
    for name, r in rows.items():
        dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
        dem = dem.split("(")[0].replace("void ", "")
        if pat in dem:
            print(f"{dem:58s} vgpr {r.get('VGPRs', -1):4d} agpr {r.get('AGPRs', -1):4d} scratch {r.get('ScratchSize', -1):5d} "
                  f"vspill {r.get('VGPRs Spill', -1):4d} occ {r.get('Occupancy', -1)} lds {r.get('LDS Size', -1)}")

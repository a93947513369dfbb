"""Register / scratch / LDS / occupancy figures of every kernel of a tree, and the comparison of two trees.

    python tools/kernel_resources.py dump <tree> <out.json>      # cross-compiles <tree>/isaaclab_amd/csrc/*.hip for gfx950
    python tools/kernel_resources.py compare <a.json> <b.json>   # kernels of a that changed or are missing in b; exit status 1 if any

The figures are what ``-Rpass-analysis=kernel-resource-usage`` reports per kernel (device compile only: no GPU is needed).  A pull
request that moves shared device code runs ``dump`` on the parent and on the branch and ``compare``s: every existing kernel must keep
its line."""

from __future__ import annotations

import json
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wno-unused-function",
         "--cuda-device-only", "-c", "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
KEYS = {"SGPRs": "sgpr", "TotalSGPRs": "sgpr", "SGPRs Spill": "sgpr_spill", "VGPRs Spill": "vgpr_spill", "VGPRs": "vgpr", "AGPRs": "agpr", "ScratchSize [bytes/lane]": "scratch", "Occupancy [waves/SIMD]": "occupancy",
        "LDS Size [bytes/block]": "lds"}


def dump(tree: str) -> dict:
    csrc = os.path.join(tree, "isaaclab_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    sources = sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))

    def one(src):
        r = subprocess.run([hipcc, *FLAGS, src], cwd=csrc, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"{src}: {r.stderr[-2000:]}")
        return src, r.stderr

    out = {}
    with ThreadPoolExecutor(max_workers=8) as pool:
        for src, log in pool.map(one, sources):
            name = None
            for line in log.splitlines():
                m = re.search(r"remark: (.*)$", line)
                if not m:
                    continue
                text = m.group(1).replace("[-Rpass-analysis=kernel-resource-usage]", "").strip()
                if text.startswith("Function Name:"):
                    name = f"{src}:{text.split(':', 1)[1].strip()}"
                    out[name] = {}
                elif name is not None:
                    key, _, val = text.rpartition(":")
                    if key.strip() in KEYS:
                        out[name][KEYS[key.strip()]] = int(val)
    return out


def compare(a: dict, b: dict) -> list[str]:
    return [f"{k}: {a[k]} -> {b.get(k, 'missing')}" for k in sorted(a) if a[k] != b.get(k)]


def main(argv):
    if len(argv) == 4 and argv[1] == "dump":
        table = dump(argv[2])
        with open(argv[3], "w") as f:
            json.dump(table, f, indent=1, sort_keys=True)
        print(f"{len(table)} kernels")
        return 0
    if len(argv) == 4 and argv[1] == "compare":
        with open(argv[2]) as f:
            a = json.load(f)
        with open(argv[3]) as f:
            b = json.load(f)
        diff = compare(a, b)
        print("\n".join(diff) if diff else f"all {len(a)} kernels of {argv[2]} keep their figures; {len(set(b) - set(a))} new: "
              + ", ".join(f"{k} {b[k]}" for k in sorted(set(b) - set(a))))
        return 1 if diff else 0
    print(__doc__)
    return 2


if __name__ == "__main__":
    sys.exit(main(sys.argv))

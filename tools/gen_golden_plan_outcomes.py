"""tests/golden/plan_outcomes.npz: what the term compiler makes of the fixed case list of tests/_cfg_cases.py (``plan_outcomes``), one
uint64 per case.  It pins the compiler across a restructuring, so it is recorded with the package of the commit BEFORE the change:

    git worktree add /tmp/parent <commit>
    python tools/gen_golden_plan_outcomes.py --package-root /tmp/parent [--out FILE]

``--package-root DIR`` puts DIR first on ``sys.path``: ``isaaclab_amd`` (and its ``configs/``) come from there, the case list from this
tree.  Without it the script records this tree's own compiler -- for comparing (``--out``), not for committing."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--package-root", default=ROOT, help="directory whose isaaclab_amd/ is compiled (default: this tree)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "plan_outcomes.npz"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.abspath(args.package_root))
    import numpy as np

    import isaaclab_amd
    from _cfg_cases import plan_outcomes

    out = plan_outcomes()
    print(f"isaaclab_amd from {os.path.dirname(isaaclab_amd.__file__)}")
    for key in ("fuzz", "configs", "drop_param"):
        ok = out.pop(key + "_compiled")
        print(f"{key}: {len(ok)} cases, {int(ok.sum())} compiled, {int((~ok).sum())} refused")
    np.savez_compressed(args.out, **out)
    print(f"wrote {args.out}")

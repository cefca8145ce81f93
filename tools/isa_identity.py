"""Label-normalised ISA comparison of two builds of the same units (DESIGN.md §2a method): for every kernel of
<old_dir>/<unit>.s that <new_dir>/<unit>.s also holds, the instruction and directive lines (comments, alignment and
debug directives dropped, local labels renumbered in order of appearance) must be equal. The .s files come from

    hipcc --offload-arch=gfx950 <the unit's Makefile flags> --cuda-device-only -S csrc/<unit>.hip -o <dir>/<unit>.s

on each tree. --alias OLD=NEW rewrites a substring of the old build's lines first (a type that moved between
namespaces changes the mangled kernel names that mention it and nothing else). Prints a JSON summary; exit 1 if a
kernel differs or disappeared.

    python tools/isa_identity.py old/ new/ nrc_train16 nrc_train_dc nrc_frame --alias NS0_10FeistelKey=NS_10FeistelKey
"""
from __future__ import annotations

import argparse
import hashlib
import json
import re
import sys


def kernels(path: str, alias: list[tuple[str, str]]) -> dict[str, list[str]]:
    out, name, body = {}, None, []
    for line in open(path):
        s = line.split(";")[0].strip()
        for a, b in alias:
            s = s.replace(a, b)
        m = re.match(r"^(_Z\w+):$", s)
        if m and name is None:
            name, body = m.group(1), []
        elif name is not None and s.startswith(".Lfunc_end"):
            labels: dict[str, str] = {}
            out[name] = [re.sub(r"\.L[A-Za-z_]*\d+(_\d+)?", lambda m: labels.setdefault(m.group(0), f"L{len(labels)}"), x)
                         for x in body]
            name = None
        elif name is not None and s and not s.startswith((".p2align", ".loc", ".cfi", ".file")):
            body.append(s)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("old_dir")
    ap.add_argument("new_dir")
    ap.add_argument("units", nargs="+")
    ap.add_argument("--alias", action="append", default=[])
    args = ap.parse_args()
    alias = [tuple(a.split("=", 1)) for a in args.alias]
    res, ok = {}, True
    for unit in args.units:
        old, new = kernels(f"{args.old_dir}/{unit}.s", alias), kernels(f"{args.new_dir}/{unit}.s", [])
        ks = {k: {"lines": len(old[k]), "identical": old[k] == new[k],
                  "sha256": hashlib.sha256("\n".join(new[k]).encode()).hexdigest()[:16]} for k in sorted(old) if k in new}
        res[unit] = {"kernels_before": len(old), "kernels_added": sorted(set(new) - set(old)),
                     "kernels_missing": sorted(set(old) - set(new)), "kernels": ks,
                     "all_identical": all(v["identical"] for v in ks.values()) and not set(old) - set(new)}
        ok = ok and res[unit]["all_identical"]
    print(json.dumps(res, indent=1))
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()

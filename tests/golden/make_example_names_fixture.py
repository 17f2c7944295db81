#!/usr/bin/env python3
"""The `hoomd` names the reference's example script (examples/run.py) uses: the modules it imports and every attribute chain it
reads off `hoomd` (hoomd.md.integrate.mode_standard -> ["md", "integrate", "mode_standard"]).  Read from the script at run time,
where the reference tree is mounted; the fixture holds the names only, no text of the script.
tests/test_host_ui.py holds the stand-in package (compat/hoomd) to them.

  python3 tests/golden/make_example_names_fixture.py      # rewrites tests/golden/reference_example_names.json
"""
import ast
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_reference_fixture import REF  # noqa: E402

OUT = os.path.join(HERE, "reference_example_names.json")


def names(path):
    tree = ast.parse(open(path).read())
    chains, imports = set(), set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            imports.update(a.name for a in node.names if a.name.startswith("hoomd"))
        elif isinstance(node, ast.ImportFrom) and node.module and node.module.startswith("hoomd"):
            imports.update(node.module + "." + a.name for a in node.names)
        elif isinstance(node, ast.Attribute):
            parts, cur = [], node
            while isinstance(cur, ast.Attribute):
                parts.append(cur.attr); cur = cur.value
            if isinstance(cur, ast.Name) and cur.id == "hoomd":
                chains.add(tuple(reversed(parts)))
    return {"imports": sorted(imports), "chains": [list(c) for c in sorted(chains)]}


def main():
    with open(OUT, "w") as f:
        json.dump(names(os.path.join(REF, "examples", "run.py")), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

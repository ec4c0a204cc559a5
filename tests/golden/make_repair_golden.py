"""Make tests/golden/repair_snapshots.json: the reference's recorded listing of
``latest:home/thinkpad/data`` of repo-index-missing-blob after ``repair
snapshots``, copied as data so that no test reads the reference at run time.
Run where the reference's tree exists.

  crates/core/tests/integration/snapshots/
      integration__integration__repair_snapshots__repair-snapshots.snap
      the BTreeMap {path: Node} of ``ls``, as RON, with the fields that differ
      between machines redacted ("[some]", "[uid]", ...)
"""
import json
import os
import re

REF = "/root/reference/crates/core"
HERE = os.path.dirname(os.path.abspath(__file__))
SNAP = "tests/integration/snapshots/integration__integration__repair_snapshots__repair-snapshots.snap"


def value(v: str):
    v = v.strip().rstrip(",")
    m = re.fullmatch(r"Some\((.*)\)", v)
    if m:
        v = m.group(1)
    if v == "None":
        return None
    if v == "[]":
        return []
    if re.fullmatch(r"[0-9]+", v):
        return int(v)
    return json.loads(v)


def main():
    text = open(os.path.join(REF, SNAP)).read().split("---", 2)[2]
    nodes, cur = {}, None
    for line in text.splitlines():
        m = re.fullmatch(r'\s*("(?:[^"\\]|\\.)*"): \{', line)
        if m:
            cur = nodes.setdefault(json.loads(m.group(1)), {})
            continue
        m = re.fullmatch(r'\s*"(\w+)": (.*),', line)
        if m and cur is not None:
            cur[m.group(1)] = value(m.group(2))
    out = {"source": "rustic_core crates/core/tests/integration/snapshots (copied as data)",
           "repo": "repo-index-missing-blob.tar.gz", "path": "latest:home/thinkpad/data",
           "nodes": nodes}
    p = os.path.join(HERE, "repair_snapshots.json")
    json.dump(out, open(p, "w"), indent=1)
    print(p, os.path.getsize(p), nodes)


if __name__ == "__main__":
    main()

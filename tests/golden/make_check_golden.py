"""Make tests/golden/check_fixtures.json and tests/golden/check_n_m.json: the
reference's recorded results of ``check``, copied as data so that no test
reads the reference at run time.  Run where the reference's tree exists.

  crates/core/tests/fixtures/repo-*.tar.gz
      eight small repositories, password "geheim" (tests/integration.rs)
  crates/core/tests/integration/snapshots/integration__integration__check__*.snap
      the CheckResults of ``check --read-data`` for each, as Rust's Debug
      prints them; parsed here into {level, kind, fields} lists
  crates/core/src/commands/snapshots/*check__tests__n_m_*.snap
      parse_n_m(now, n, m) at seven dates for 18 spellings of n/m
"""
import base64
import glob
import json
import os
import re
import tarfile

REF = "/root/reference/crates/core"
HERE = os.path.dirname(os.path.abspath(__file__))
# the dates of the n/m snapshots, in the order of each recorded tuple
N_M_DATES = ["2024-10-11T12:00:00", "2024-10-11T13:00:00", "2024-10-12T12:00:00",
             "2024-10-18T12:00:00", "2024-11-11T12:00:00", "2025-10-11T12:00:00",
             "2020-02-02T12:00:00"]


def body(text: str) -> str:
    """A snapshot file without its front matter."""
    return text.split("---", 2)[2]


def balanced(s: str, at: int) -> int:
    """The index behind the bracket that closes the one at ``at``."""
    pairs = {"(": ")", "{": "}", "[": "]"}
    depth, i, quoted = 0, at, False
    while i < len(s):
        c = s[i]
        if quoted:
            if c == "\\":
                i += 1
            elif c == '"':
                quoted = False
        elif c == '"':
            quoted = True
        elif c in pairs:
            depth += 1
        elif c in pairs.values():
            depth -= 1
            if depth == 0:
                return i + 1
        i += 1
    raise ValueError("unbalanced")


def split_fields(s: str):
    """``name: value`` members at depth 0 of a struct body."""
    out, depth, start, quoted, i = [], 0, 0, False, 0
    while i < len(s):
        c = s[i]
        if quoted:
            if c == "\\":
                i += 1
            elif c == '"':
                quoted = False
        elif c == '"':
            quoted = True
        elif c in "({[":
            depth += 1
        elif c in ")}]":
            depth -= 1
        elif c == "," and depth == 0:
            out.append(s[start:i])
            start = i + 1
        i += 1
    out.append(s[start:])
    return [m.strip().split(":", 1) for m in out if m.strip()]


def value(v: str):
    v = v.strip()
    m = re.fullmatch(r"\w+\(\s*([0-9a-f]{64}),?\s*\)", v)  # PackId( <hex>, )
    if m:
        return m.group(1)
    if v.startswith("RusticError"):
        ctx = re.search(r"context:\s*\[(.*?)\],\s*source", v, re.S).group(1)
        return {"kind": re.search(r"kind:\s*(\w+)", v).group(1),
                "guidance": json.loads(re.search(r'guidance:\s*("(?:[^"\\]|\\.)*")', v).group(1)),
                "context": [[json.loads(a), json.loads(b)] for a, b in
                            re.findall(r'\(\s*("(?:[^"\\]|\\.)*"),\s*("(?:[^"\\]|\\.)*"),?\s*\)', ctx)]}
    if v.startswith('"'):
        return json.loads(v)
    if v in ("true", "false"):
        return v == "true"
    if re.fullmatch(r"[0-9]+", v):
        return int(v)
    return v  # an id printed bare, or an enum's variant (Tree, Data)


def findings(text: str):
    s, out = body(text), []
    for m in re.finditer(r"\(\s*(Warn|Error),\s*(\w+)\s*\{", s):
        end = balanced(s, m.end() - 1)
        out.append({"level": m.group(1), "kind": m.group(2),
                    "fields": {k.strip(): value(v) for k, v in split_fields(s[m.end():end - 1])}})
    return out


def main():
    repos = {}
    for path in sorted(glob.glob(os.path.join(REF, "tests/fixtures/repo-*.tar.gz"))):
        name = os.path.basename(path)
        snap = os.path.join(REF, "tests/integration/snapshots",
                            f"integration__integration__check__{name}.snap")
        t = tarfile.open(path)
        files = {m.name: base64.b64encode(t.extractfile(m).read()).decode()
                 for m in t.getmembers() if m.isfile()}
        repos[name] = {"files": files, "results": findings(open(snap).read())}
    out = {"source": "rustic_core crates/core/tests/fixtures and tests/integration/snapshots "
                     "(copied as data)",
           "password": "geheim", "repos": repos}
    p = os.path.join(HERE, "check_fixtures.json")
    json.dump(out, open(p, "w"), indent=1)
    print(p, os.path.getsize(p), {k: len(v["results"]) for k, v in repos.items()})

    cases = {}
    for path in sorted(glob.glob(os.path.join(REF, "src/commands/snapshots/*check__tests__n_m_*.snap"))):
        n, m = os.path.basename(path).split("n_m_", 1)[1][:-len(".snap")].split("_", 1)
        pairs = [[int(a), int(b)] for a, b in re.findall(r"\((\d+), (\d+)\)", body(open(path).read()))]
        assert len(pairs) == len(N_M_DATES), path
        cases[f"{n}/{m}"] = pairs
    p = os.path.join(HERE, "check_n_m.json")
    json.dump({"source": "rustic_core crates/core/src/commands/snapshots (copied as data)",
               "dates": N_M_DATES, "cases": cases}, open(p, "w"), indent=1)
    print(p, os.path.getsize(p), len(cases))


if __name__ == "__main__":
    main()

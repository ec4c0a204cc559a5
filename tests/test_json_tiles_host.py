"""CPU: the byte level of the device JSON parsers (csrc/rcdc_json_tiles.h and
the two grammars), run by tools/json_tiles_check, against a serial scan
written here: folding chunk functions equals scanning the bytes in order, the
counts and the emitted events are the scan's, and the strict primitives
accept and refuse what the units' own copies did."""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# RCDC_JSON_TILES_CHECK: another build of the same program (one compiled with
# -fsanitize=address,undefined, say) runs the same cases
TOOL = os.environ.get("RCDC_JSON_TILES_CHECK") or os.path.join(ROOT, "tools", "json_tiles_check")
ALPHABET = b'"\\{}[]a'
STRINGS = [bytes(s) for n in range(6) for s in itertools.product(ALPHABET, repeat=n)]
U32, U64 = 2**32 - 1, 2**64 - 1


def _hex(b):
    return b.hex() if b else "-"


@pytest.fixture(scope="module")
def check(rcdc_lib):
    """Feeds the check program cases (token lists); returns per case the
    result line's integers."""
    assert os.path.exists(TOOL), "tools/json_tiles_check not built (csrc/Makefile)"

    def run(cases):
        text = "\n".join(" ".join(str(t) for t in c) for c in cases) + "\n"
        r = subprocess.run([TOOL], input=text, capture_output=True, text=True, check=True)
        lines = r.stdout.splitlines()
        assert len(lines) == len(cases)
        out = []
        for c, ln in zip(cases, lines):
            w = ln.split()
            assert w[0] == c[0]
            out.append([int(v) for v in w[1:]])
        return out
    return run


# ---- the serial reference -------------------------------------------------------
def _event_ix(ch, depth):
    if ch == ord("{"):
        return {4: 0, 2: 1}.get(depth, -1)
    if ch == ord("]"):
        return {4: 2, 2: 3}.get(depth, -1)
    return -1


def _event_tr(ch, depth):
    if ch == ord("{"):
        return 0 if depth == 2 else -1
    if ch == ord('"'):
        return 1 if depth == 4 else -1
    if ch == ord("]"):
        return {4: 2, 2: 3}.get(depth, -1)
    return -1


def scan(text, esc_on, instr, depth, event_of=None):
    """The bytes in order: the state behind the last one, and the events as
    (kind, index, the counts of each kind before it)."""
    esc, counts, events = False, [0, 0, 0, 0], []
    for i, ch in enumerate(text):
        if esc_on and esc:
            esc = False
        elif esc_on and ch == ord("\\"):
            esc = True
        elif instr:
            instr = int(ch != ord('"'))
        else:
            e = event_of(ch, depth) if event_of else -1
            if e >= 0:
                events.append((e, i, *counts))
                counts[e] += 1
            instr = int(ch == ord('"'))
            depth += {ord("{"): 1, ord("["): 1, ord("}"): -1, ord("]"): -1}.get(ch, 0)
    return instr, depth, counts, events


def n_splits(n):
    return (n + 1) * (n + 2) // 2


# ---- folding ----------------------------------------------------------------------
@pytest.mark.parametrize("esc", [0, 1])
def test_folding_chunks_is_the_serial_scan(check, esc):
    got = check([["fold", esc, _hex(s)] for s in STRINGS])
    for s, g in zip(STRINGS, got):
        i0, d0, _, _ = scan(s, esc, 0, 0)
        i1, d1, _, _ = scan(s, esc, 1, 0)
        assert g == [n_splits(len(s)), n_splits(len(s)), i0, d0, i1, d1], (s, esc)


# ---- counts and emit ----------------------------------------------------------------
# the grammars as their units run them, and each under the other's ESC on the
# shorter strings; from depth 3, where one bracket reaches an event's depth
@pytest.mark.parametrize("grammar,esc,instr,depth,longest", [
    ("ix", 0, 0, 3, 5), ("tr", 1, 0, 3, 5), ("ix", 1, 0, 3, 4), ("tr", 0, 0, 3, 4),
    ("ix", 0, 1, 4, 4), ("tr", 1, 1, 4, 4), ("tr", 1, 0, 0, 5), ("ix", 0, 0, 0, 5),
])
def test_counts_and_emit_are_the_serial_scan(check, grammar, esc, instr, depth, longest):
    strings = [s for s in STRINGS if len(s) <= longest]
    event_of = _event_ix if grammar == "ix" else _event_tr
    got = check([["ev", grammar, esc, instr, depth, _hex(s)] for s in strings])
    seen = set()
    for s, g in zip(strings, got):
        _, _, counts, events = scan(s, esc, instr, depth, event_of)
        want = [n_splits(len(s)), n_splits(len(s)), *counts, len(events)]
        for ev in events:
            want += ev
            seen.add(ev[0])
        assert g == want, (s, grammar, esc)
    if depth == 3:
        assert seen == {0, 1, 2, 3}


def test_a_quote_that_is_an_event_opens_its_string(check):
    # tree grammar, depth 4: the first quote is an id open and opens the
    # string, the bracket inside it counts for nothing, the second closes it
    (g,) = check([["ev", "tr", 1, 0, 4, _hex(b'"]"]')]])
    assert g == [15, 15, 0, 1, 1, 0, 2, 1, 0, 0, 0, 0, 0, 2, 3, 0, 1, 0, 0]
    # an escaped quote inside it does not close it
    (g,) = check([["ev", "tr", 1, 0, 4, _hex(b'"\\""]')]])
    assert g[2:7] == [0, 1, 1, 0, 2] and g[7:9] == [1, 0] and g[13:15] == [2, 4]


# ---- the strict primitives ------------------------------------------------------------
def test_parse_uint(check):
    ok = [(U32, b"0,", 0), (U32, b"4294967295,", U32), (U64, b"18446744073709551615}", U64),
          (U32, b"7 ,", 7), (9, b"9,", 9)]
    bad = [(U32, b"4294967296,"), (U64, b"18446744073709551616,"), (U32, b"00,"), (U32, b"01,"),
           (U32, b""), (U32, b"-1,"), (U64, b"99999999999999999999,"), (9, b"10,")]
    got = check([["uint", m, _hex(t)] for m, t, _ in ok] + [["uint", m, _hex(t)] for m, t in bad])
    for (m, t, v), g in zip(ok, got):
        digits = len(t.rstrip(b" ,}"))
        assert g == [1, v, digits, 1], t
    for (m, t), g in zip(bad, got[len(ok):]):
        assert g[0] == 0, t
    # A digit run that ends at `end`: parse_uint itself stops there with the
    # value (what follows is the caller's to check, as in both units before),
    # and the check every caller makes behind a value refuses it.
    (g,) = check([["uint", U32, _hex(b"123")]])
    assert g == [1, 123, 3, 0]


ID = b'"00112233445566778899aAbBcCdDeEfF0123456789abcdefFEDCBA9876543210"'


def _words(hexdigits):
    raw = bytes.fromhex(hexdigits.decode())
    return [int.from_bytes(raw[4 * i:4 * i + 4], "little") for i in range(8)]


def test_parse_id(check):
    cases = [["id", len(ID), _hex(ID)], ["id", len(ID) + 1, _hex(ID + b",")]]
    short, long_ = ID[:64] + b'"', ID[:65] + b'0"'
    cases += [["id", len(short), _hex(short)], ["id", len(long_), _hex(long_)]]
    for at in (0, 1, 62, 63):
        t = bytearray(ID)
        t[1 + at] = ord("g")
        cases.append(["id", len(t), _hex(bytes(t))])
    cases += [["id", end, _hex(ID)] for end in range(66)]
    got = check(cases)
    assert got[0] == [1, 66, *_words(ID[1:65])]
    assert got[1] == [1, 66, *_words(ID[1:65])]
    for g in got[2:]:
        assert g[0] == 0 and g[2:] == [0] * 8


def test_skip_array(check):
    t = b'[ {"a":1} , {"b":2} ]x'
    close = t.index(b"]")
    base = dict(open=ord("{"), pos=0, end=len(t), k=2, n=3, ref=5, clpos=close, clref=5, clrank=9)

    def case(**kw):
        c = dict(base, **kw)
        return ["skip", c["open"], c["pos"], c["end"], c["k"], c["n"], c["ref"], c["clpos"],
                c["clref"], c["clrank"], _hex(t)]

    got = check([case(), case(clref=4), case(clpos=1), case(clpos=0), case(clpos=len(t)),
                 case(end=close), case(k=3), case(k=4), case(open=ord('"')), case(pos=1)])
    assert got[0] == [1, 9, close + 1]
    # the record is of another ref; lies before the cursor (which stands
    # behind "[ ", at 2); at or after `end` (behind the text, and at an `end`
    # that cuts the text there); k == n and k > n; the first element begins
    # with another byte; no '[' at the cursor
    for g in got[1:]:
        assert g[0] == 0

"""A model of rcdc_check_packs' rule (include/rcdc.h) in plain Python: what
the kernel is held against, and itself held against check.index_pass_host and
read.check_pack's sort (tests/test_check_host.py).

Entries are rows of numpy arrays: ids (n, 32) uint8, locs (n, 4) uint32
(pack, offset, length, uncompressed length), types n uint8 or None."""
import numpy as np

OK, HOST = 0, 1
NOT_COMPARED, EQUAL, DIFFERS = 0, 1, 2
TYPE, OFFSET = 0, 1
NO_HEADER = 0xFFFFFFFF


def pack_order(locs, first, count):
    """The entries of a pack by (offset, length, uncompressed length); equal
    locations keep input order."""
    rows = range(first, first + count)
    return sorted(rows, key=lambda e: (int(locs[e][1]), int(locs[e][2]), int(locs[e][3])))


def in_order(locs, first, count):
    keys = [(int(locs[e][1]), int(locs[e][2]), int(locs[e][3])) for e in range(first, first + count)]
    return all(a <= b for a, b in zip(keys, keys[1:]))


def model(ids, locs, types, ranges, sort_max, hdr=None):
    """(packs, findings, order): packs a list of dicts with the fields of
    rcdc_ckpack_pack, findings a list of (pack, entry, kind, got, expected) in
    the reference's order, order {row of d_order: entry}.  ``hdr``: (ids[2],
    locs[2], [(type, count, first)] per pack)."""
    packs, findings, order = [], [], {}
    for p, (first, count) in enumerate(ranges):
        if types is not None:
            ptype = int(types[first]) if count else 0
        elif hdr is not None and hdr[2][p][0] != NO_HEADER:
            ptype = hdr[2][p][0]
        else:
            ptype = 0
        rec = dict(status=OK, type=ptype, type_findings=0, offset_findings=0, end_offset=0,
                   header_verdict=NOT_COMPARED, header_diff=0, sorted=0, header_len=0,
                   first_finding=0)
        packs.append(rec)
        was = in_order(locs, first, count)
        if not was and count > sort_max:
            rec["status"] = HOST
            continue
        rec["sorted"] = int(was)
        rec["first_finding"] = len(findings)
        rows = pack_order(locs, first, count)
        expected = 0
        for k, e in enumerate(rows):
            order[first + k] = e
            t = int(types[e]) if types is not None else ptype
            if t != ptype:
                findings.append((p, e, TYPE, t, ptype))
                rec["type_findings"] += 1
            if int(locs[e][1]) != expected:
                findings.append((p, e, OFFSET, int(locs[e][1]), expected))
                rec["offset_findings"] += 1
            expected = (expected + int(locs[e][2])) & 0xFFFFFFFF
        rec["end_offset"] = expected
        rec["header_len"] = 32 + sum(41 if int(locs[e][3]) else 37 for e in rows)
        if hdr is None or hdr[2][p][0] == NO_HEADER:
            continue
        h_type, h_count, h_first = hdr[2][p]
        diff = None
        for k in range(min(count, h_count)):
            e, j = rows[k], h_first + k
            t = int(types[e]) if types is not None else ptype
            same = (bytes(ids[e]) == bytes(hdr[0][h_type][j]) and t == h_type
                    and all(int(locs[e][c]) == int(hdr[1][h_type][j][c]) for c in (1, 2, 3)))
            if not same:
                diff = k
                break
        if diff is None and count != h_count:
            diff = min(count, h_count)
        rec["header_verdict"] = EQUAL if diff is None else DIFFERS
        rec["header_diff"] = diff or 0
    return packs, findings, order


def random_pack(rng, count, shuffle=False, gap=False, types=None):
    """(ids, locs, types) of a pack as a packer writes it: blobs back to
    back, some with an uncompressed length."""
    ids = rng.integers(0, 256, (count, 32), dtype=np.uint8)
    lens = rng.integers(33, 5000, count, dtype=np.uint32)
    offs = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.uint64)]).astype(np.uint32) \
        if count else np.zeros(0, np.uint32)
    ulens = np.where(rng.random(count) < 0.5, lens * 2, 0).astype(np.uint32)
    locs = np.stack([np.zeros(count, np.uint32), offs, lens, ulens], 1) if count \
        else np.zeros((0, 4), np.uint32)
    if gap and count > 1:
        locs[count // 2:, 1] += 7
    tp = np.full(count, 0 if types is None else types, np.uint8)
    if shuffle and count > 1:
        perm = rng.permutation(count)
        while count > 1 and np.array_equal(perm, np.arange(count)):
            perm = rng.permutation(count)
        ids, locs, tp = ids[perm], locs[perm], tp[perm]
    return ids, locs, tp

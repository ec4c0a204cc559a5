"""Index files parsed on the device (rcdc_index_parse, DeviceIndex.extend_json
and DeviceIndex.load) against the plain-Python model of the grammar
(tests/index_json_model.py) and against today's host path
(IndexFile.from_json + DeviceIndex.from_index_files / extend)."""
import base64
import random

import numpy as np
import pytest

from tests import index_json_model as model
from tests.index_json_cases import (CASES, P1, P2, blob, compact, hid, random_index,
                                    random_text)

pytestmark = pytest.mark.gpu

GUARD = 256


def _arena(files, align=1, shift=0):
    """One device arena holding ``files``: each at a multiple of ``align``,
    the whole tensor starting ``shift`` bytes past a 16-byte boundary (0xFF
    between the files, so a read past a file's end does not look like
    whitespace).  Returns (tensor, offs, lens)."""
    import torch
    offs, o = [], 0
    for f in files:
        o = (o + align - 1) // align * align
        offs.append(o)
        o += len(f) + (1 if align == 1 else 0)
    host = np.full(o + shift + 1, 0xFF, np.uint8)
    for off, f in zip(offs, files):
        host[shift + off:shift + off + len(f)] = np.frombuffer(f, np.uint8)
    t = torch.from_numpy(host).to("cuda:0")
    return t[shift:shift + o], offs, [len(f) for f in files]


def _check(files, pack_base=(0, 0), align=1, shift=0, want=None):
    """Parse ``files`` in one call and compare every output with the model;
    nothing is written past the counts reported (0xA5 fill and guard)."""
    from rustic_core_amd.dindex import parse_json
    d, offs, lens = _arena(files, align, shift)
    res = parse_json(d, offs, lens, pack_base, guard=GUARD)
    m = want or model.collect(files, pack_base)
    assert res.files["status"].tolist() == m.status
    for i, (np_, ndel, ne) in enumerate(m.files):
        f = res.files[i]
        assert (tuple(f["packs"]), int(f["packs_to_delete"]), tuple(f["entries"])) == \
            (np_, ndel, ne), i
    assert [(p["id"].tobytes(), int(p["type"]), int(p["number"]), int(p["size"]))
            for p in res.packs] == m.packs
    for t in (0, 1):
        n = len(m.ids[t])
        assert res.entries[t] == n
        ids = res.ids[t].cpu().numpy()
        locs = res.locs[t].cpu().numpy().view(np.uint32)
        assert ids[:n].tobytes() == b"".join(m.ids[t]), t
        assert [tuple(r) for r in locs[:n].tolist()] == m.locs[t], t
        assert (ids[n:] == 0xA5).all() and (locs[n:] == 0xA5A5A5A5).all(), t
    for flat in res.raw:
        assert (flat[-GUARD:].cpu().numpy() == 0xA5).all()
    return res, m


def test_case_table(gpu_ctx):
    """The whole table in one batch, the files back to back at odd offsets in
    an arena that starts off a 16-byte boundary."""
    files = [c[1] for c in CASES]
    res, m = _check(files, (3, 5), align=1, shift=5)
    assert m.status == [0 if c[2] else 1 for c in CASES]
    # and one file at a time: a file's verdict does not depend on its neighbours
    _check(files[:1])
    _check([c[1] for c in CASES if not c[2]][:3])


def _three_tiles(tile):
    """A file of about three tiles, and its longest blob object."""
    packs, n = [], 0
    while len(compact({"packs": packs})) < 3 * tile - 400:
        blobs = []
        for j in range(1 + len(packs) % 4):
            n += 1
            blobs.append(blob(n % 256, "tree" if len(packs) % 3 == 0 else "data",
                              (n * 1000003) % (1 << 32), (n * 77) % 5000,
                              None if n % 2 else 4294967295 - n, keep_ulen=n % 5 != 0))
        p = {"id": hid(len(packs) % 256), "blobs": blobs}
        if len(packs) % 2:
            p["time"] = "2024-05-06T07:08:09.123456789+02:00"
        if len(packs) % 5 == 0:
            p["size"] = len(packs) * 1001
        packs.append(p)
    longest = max(len(compact(b)) for p in packs for b in p["blobs"])
    return compact({"supersedes": [hid(3)], "packs": packs, "packs_to_delete": [P1]}), longest


def test_tile_edges(gpu_ctx):
    """k spaces in front of a three-tile file, k = 0 .. 2 x the longest blob
    object: every byte of a blob object, of a quote pair and of a bracket
    meets a tile edge at some k.  Files start on tile boundaries."""
    from rustic_core_amd.dindex import parse_tile
    tile = parse_tile()
    text, longest = _three_tiles(tile)
    assert 2 * tile < len(text) < 4 * tile and 150 < longest < 250
    files = [b" " * k + text for k in range(2 * longest + 1)]
    small = compact({"packs": [P1, P2]})
    pad = lambda n: small[:-1] + b" " * (n - len(small)) + b"}"
    files += [pad(tile), pad(tile - 1), pad(tile + 1), b"{}", b'{"packs":[]}']
    assert [len(f) for f in files[-5:]] == [tile, tile - 1, tile + 1, 2, 12]
    one = model.collect([text])
    assert one.status == [0] and sum(one.files[0][0]) > 20
    res, m = _check(files, (0, 0), align=tile)
    assert m.status == [0] * (len(files) - 2) + [1, 0]
    # more tiles and more packs than a round of the two scans of one workgroup: the
    # counts' (rcdc_ix_count_scan_kernel) and the packs' (rcdc_ix_number_kernel)
    assert sum((len(f) + tile - 1) // tile for f in files) >= 1220 > 1024
    assert len(m.packs) > 2 * 1024
    # the same files at offsets that are no multiple of anything
    _check(files[::37] + files[-5:], (7, 9), align=1, shift=11)


def _pack(n_blobs, seed, tpe="data"):
    return {"id": hid(seed % 256), "blobs": [blob((seed + j) % 256, tpe, j, j + 1, (j % 3) or None)
                                             for j in range(n_blobs)]}


def test_counts_around_a_wave(gpu_ctx):
    sizes = compact({"packs": [_pack(n, i * 11, "tree" if i % 2 else "data")
                               for i, n in enumerate((0, 1, 63, 64, 65))]})
    many = [compact({"packs": [_pack(i % 3, i, "tree" if i % 4 == 0 else "data") for i in range(n)],
                     "packs_to_delete": [_pack(1, 5)] * (n % 3)}) for n in (63, 64, 65)]
    _check([sizes] + many, (1, 2))
    # 65 files, some outside G: the others' numbers and outputs are unchanged
    bad = [c[1] for c in CASES if not c[2]]
    good = [compact({"packs": [_pack(i % 5, i, "tree" if i % 3 == 0 else "data")]})
            for i in range(52)]
    files, k = [], 0
    for i in range(65):
        if i % 5 == 2:
            files.append(bad[(i * 7) % len(bad)])
        else:
            files.append(good[k])
            k += 1
    assert len(files) == 65 and k == 52
    res, m = _check(files, (10, 20))
    res2, m2 = _check(good, (10, 20))
    assert m.packs == m2.packs and m.locs == m2.locs and m.ids == m2.ids
    for t in (0, 1):
        n = res.entries[t]
        assert res2.entries[t] == n
        assert (res.ids[t][:n] == res2.ids[t][:n]).all() and (res.locs[t][:n] == res2.locs[t][:n]).all()


@pytest.mark.parametrize("index_type", ["FULL", "DATA_IDS", "ONLY_TREES"])
def test_extend_json_against_from_index_files(gpu_ctx, index_type):
    """The same random index through from_index_files / extend and through
    two extend_json calls, a file the device leaves to the host between two
    it parses."""
    import torch
    from rustic_core_amd import DeviceIndex, IndexType
    from rustic_core_amd.dindex import DATA, NOT_PARSED, PARSED, TREE
    from rustic_core_amd.index import IndexFile
    it = IndexType[index_type]
    rng = random.Random(77)
    pool = [rng.randbytes(32) for _ in range(200)]
    objs = [random_index(rng, 40, 90, pool) for _ in range(7)]
    texts = [random_text(f, rng) for f in objs]
    # file 1 and file 5: valid for from_json, outside G (an escape in "time")
    for k in (1, 5):
        o = objs[k].to_obj()
        o["packs"][0]["time"] = "a\\b"
        texts[k] = compact(o)
    files = [IndexFile.from_json(t) for t in texts]
    assert sum(len(p.blobs) for f in files for p in f.packs) > 2000
    want = DeviceIndex.from_index_files(files[:4], 0, it)
    want.extend(p for f in files[4:] for p in f.packs)
    got = DeviceIndex(0, it)
    d, offs, lens = _arena(texts[:4], 16)
    assert got.extend_json(d, offs, lens).tolist() == [PARSED, NOT_PARSED, PARSED, PARSED]
    d, offs, lens = _arena(texts[4:], 1, 3)
    assert got.extend_json(d, offs, lens).tolist() == [PARSED, NOT_PARSED, PARSED]
    ids = sorted({b.id for f in files for p in f.packs for b in p.blobs})
    ids += [rng.randbytes(32) for _ in range(50)]
    q = np.frombuffer(b"".join(ids), np.uint8).reshape(-1, 32)
    for t in (DATA, TREE):
        assert got.packs(t) == want.packs(t) and len(want.packs(t)) > 5
        assert got.total_size(t) == want.total_size(t)
        assert got.size(t) == want.size(t) and got.keys(t) == want.keys(t)
        assert torch.equal(got.lookup(t, q), want.lookup(t, q))
    assert want.size(TREE) > 500 and (want.size(DATA) > 500) == (it != IndexType.ONLY_TREES)
    mixed = np.concatenate([q[::3], q[::7],
                            np.frombuffer(rng.randbytes(32 * 9), np.uint8).reshape(-1, 32)])
    assert torch.equal(got.first_new(mixed), want.first_new(mixed))
    # a file from_json refuses raises as it does there
    d, offs, lens = _arena([b'{"packs":[{"id":"zz","blobs":[]}]}'])
    with pytest.raises(ValueError):
        got.extend_json(d, offs, lens)
    got.close()
    want.close()


def _fixture():
    from oracle import oracle
    from tests.test_crypto_oracle import GOLD
    from tests.test_pack_oracle import reference_pack
    key, _, _, _ = reference_pack(oracle)
    files = {k: base64.b64decode(v) for k, v in GOLD["repo_mixed"].items()}
    name = [k for k in files if k.startswith("repo/index/")][0]
    return key, files[name], oracle.open_(key, files[name])


def _same_index(dx, files):
    """dx holds what from_index_files(files) would."""
    from rustic_core_amd.dindex import DATA, TREE
    for t in (DATA, TREE):
        packs = [p for f in files for p in f.packs if (p.blobs[0].type if p.blobs else 0) == t]
        assert dx.packs(t) == [p.id for p in packs]
        assert dx.total_size(t) == sum(p.pack_size() for p in packs)
        blobs = [(p.id, b) for p in packs for b in p.blobs]
        assert dx.size(t) == len(blobs)
        got = dx.entries(t, [b.id for _, b in blobs])
        first = {}
        for pid, b in blobs:
            first.setdefault(b.id, (pid, b))
        for (pid, b), g in zip(blobs, got):
            wp, wb = first[b.id]
            assert g is not None and g[0] == wp
            assert (g[1].id, g[1].offset, g[1].length, g[1].uncompressed_length) == \
                (wb.id, wb.offset, wb.length, wb.uncompressed_length)


def test_load_reference_index_file(gpu_ctx):
    from rustic_core_amd import DeviceIndex
    from rustic_core_amd.crypto import Key
    from rustic_core_amd.dindex import PARSED, TREE
    from rustic_core_amd.index import IndexFile
    key, sealed, text = _fixture()
    f = IndexFile.from_json(text)
    dx = DeviceIndex(0)
    assert dx.load(Key(key), [sealed]).tolist() == [PARSED]
    _same_index(dx, [f])
    assert [b.type for b in f.packs[0].blobs] == [0, 1, 1, 1, 1]
    assert dx.size(TREE) == 0  # the pack goes to the type of its first blob
    dx.close()


def test_load_saved_files_and_errors(gpu_ctx):
    from rustic_core_amd import DeviceIndex
    from rustic_core_amd.compress import DECODE_MESSAGE
    from rustic_core_amd.crypto import Key
    from rustic_core_amd.dindex import PARSED, UNSUPPORTED_MESSAGE
    from rustic_core_amd.errors import ErrorKind, RusticError
    from rustic_core_amd.index import save_index_file
    from rustic_core_amd.read import MAC_MESSAGE
    rng = random.Random(9)
    key = Key(bytes(range(64)))
    files = [random_index(rng, 8, 60) for _ in range(3)]
    sealed = [save_index_file(key, f, version=v)[1] for f, v in zip(files, (2, 1, 2))]
    dx = DeviceIndex(0)
    assert dx.load(key, sealed).tolist() == [PARSED] * 3
    _same_index(dx, files)
    dx.close()

    def raises(batch, kind, message):
        d = DeviceIndex(0)
        with pytest.raises(RusticError) as e:
            d.load(key, batch)
        assert e.value.kind == kind and message in str(e.value)
        assert len(d) == 0
        d.close()
    flipped = bytearray(sealed[0])
    flipped[-1] ^= 1
    raises([sealed[1], bytes(flipped)], ErrorKind.Cryptography, MAC_MESSAGE)
    three = key.encrypt_data(b"3" + files[0].to_json())
    raises([three, sealed[1]], ErrorKind.Unsupported, UNSUPPORTED_MESSAGE)
    raises([key.encrypt_data(b"")], ErrorKind.Unsupported, UNSUPPORTED_MESSAGE)
    whole = key.decrypt_data(sealed[0])
    assert whole[0] == 2
    raises([key.encrypt_data(whole[:len(whole) // 2])], ErrorKind.Internal, DECODE_MESSAGE)
    raises([key.encrypt_data(whole[:3])], ErrorKind.Internal, DECODE_MESSAGE)
    # a frame without a content size in its header, decoded to many times its
    # length: the capacity is guessed and doubled until the text fits
    from oracle import zstd_ref as zr
    text = files[1].to_json() + b" " * 700_000
    frame = zr.compress_adv(text, content_size=False)
    assert zr.content_size(frame) is None and 8 * len(frame) + (128 << 10) < len(text)
    dx = DeviceIndex(0)
    assert dx.load(key, [sealed[0], key.encrypt_data(b"\x02" + frame)]).tolist() == [PARSED] * 2
    _same_index(dx, files[:2])
    dx.close()

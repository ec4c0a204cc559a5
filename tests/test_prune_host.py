"""CPU: prune's plan with the per-blob part on the host (``device=None``) --
the rule of commands/prune.rs as rustic_core_amd.prune states it, on cases
worked by hand."""
import datetime

import pytest

from rustic_core_amd.chunker import ConfigFile
from rustic_core_amd.errors import ErrorKind, RusticError
from rustic_core_amd.prune import (DATA, TREE, DeleteStats, LimitOption, PackStats, PackStatus,
                                   PackToDo, PruneOptions, SizeStats)
from rustic_core_amd.repack import plan_repack

from tests.prune_cases import (CASES, OLD, YOUNG, bid, case_files, existing_of, one_file,
                         pack, plan_of)

T = PackToDo
S = PackStatus


def todo(plan, name):
    return next(p for p in plan.packs if p.id == bid("pack:" + name))


@pytest.mark.parametrize("name", sorted(CASES))
def test_marking_cases(name):
    files, used, infos, flags = case_files(name)
    plan = plan_of(files, used)
    assert [p.info.sums() for p in plan.packs] == infos
    assert plan.used.tolist() == flags
    if name == "G":
        assert plan.counts.tolist() == [255]
        assert [i for i, p in enumerate(plan.packs) if p.info.used_blobs] == [254]


def test_options_and_limits():
    o = PruneOptions()
    assert LimitOption.parse(o.max_repack) == ("percent", 10)
    assert LimitOption.parse(o.max_unused) == ("percent", 5)
    assert o.keep_pack == datetime.timedelta(0) and o.keep_delete == datetime.timedelta(hours=23)
    assert not (o.instant_delete or o.fast_repack or o.repack_uncompressed or o.repack_all
                or o.no_resize) and o.repack_cacheable_only is None
    assert LimitOption.parse("unlimited") == ("unlimited", 0)
    assert LimitOption.parse("5b") == ("size", 5)
    assert LimitOption.parse("2 kB") == ("size", 2000)
    assert LimitOption.parse("4TiB") == ("size", 4 << 40)
    assert LimitOption.parse("1234") == ("size", 1234)
    for bad in ("x%", "12 parsecs", ""):
        with pytest.raises(RusticError) as e:
            LimitOption.parse(bad)
        assert e.value.kind == ErrorKind.InvalidInput


@pytest.mark.parametrize("time,want", [(OLD, T.Delete), (YOUNG, T.KeepMarked),
                                       (None, T.KeepMarkedAndCorrect)])
def test_case_h_marked_pack_first(time, want):
    f = one_file([pack("P", [("a", 10)])], [pack("M", [("a", 10)], time=time)])
    plan = plan_of([f], ["a"])
    assert plan.counts.tolist() == [2]
    assert [p.id for p in plan.packs] == [bid("pack:P"), bid("pack:M")]  # file order
    assert todo(plan, "M").info.sums() == (0, 1, 0, 10)  # scanned first: 2 -> 1
    assert todo(plan, "P").info.sums() == (1, 0, 10, 0)
    assert todo(plan, "M").to_do == want and todo(plan, "P").to_do == T.Keep
    assert S.Marked in todo(plan, "M").status


def test_missing_blob():
    with pytest.raises(RusticError) as e:
        plan_of([one_file([pack("P", [("a", 10)])])], ["a", "nowhere"])
    assert e.value.kind == ErrorKind.Internal and "missing in index files" in e.value.message
    assert bid("nowhere").hex() in e.value.message


def test_duplicate_packs_are_dropped():
    f0 = one_file([pack("P", [("a", 10)])])
    f1 = one_file([pack("P", [("a", 10)]), pack("Q", [("b", 5)])], [pack("Q", [("b", 5)], time=OLD)])
    f2 = one_file([pack("R", [("c", 5)])])
    plan = plan_of([f0, f1, f2], ["a", "b", "c"])
    assert [p.id for p in plan.packs] == [bid("pack:P"), bid("pack:Q"), bid("pack:R")]
    assert plan.counts.tolist() == [1, 1, 1]  # the dropped packs' entries are not counted
    mod = {f.id: f.modified for f in plan._files}
    assert [mod[bid("index:%d" % i)] for i in range(3)] == [False, True, False]
    assert bid("index:1") in [f.id for f in plan.index_files]


def test_decide_packs_branches():
    f = one_file([
        pack("unused_old", [("u1", 10)], time=OLD),
        pack("unused_young", [("u2", 10)], time=YOUNG),
        pack("used", [("a", 10)], time=OLD),
        pack("partly", [("b", 10), ("u3", 10)], time=OLD),
        pack("partly_young", [("c", 10), ("u4", 10)], time=YOUNG),
        pack("mismatch", [("d", 10)], time=OLD, size=10),
        pack("raw", [("e", 10)], time=OLD, raw=("e",)),
    ], [pack("marked_used", [("g", 10)], time=OLD)])
    used = ["a", "b", "c", "d", "e", "g"]
    keep1h = PruneOptions(keep_pack=datetime.timedelta(hours=1), max_unused="0%",
                          max_repack="unlimited")
    plan = plan_of([f], used, opts=keep1h)
    want = {"unused_old": T.MarkDelete, "unused_young": T.Keep, "used": T.Keep,
            "partly": T.Repack, "partly_young": T.Keep, "mismatch": T.Repack, "raw": T.Keep,
            "marked_used": T.Recover}
    assert {k: todo(plan, k).to_do for k in want} == want
    assert todo(plan, "unused_young").status == {S.HasUnusedBlobs, S.TooYoung}
    assert todo(plan, "mismatch").status == {S.HasUsedBlobs, S.TooSmall}
    assert todo(plan, "marked_used").status == {S.Marked, S.HasUsedBlobs}
    assert not todo(plan, "raw").compressed
    # repack_all: every used pack old enough; repack_uncompressed: the raw one
    plan = plan_of([f], used, opts=PruneOptions(keep_pack=datetime.timedelta(hours=1),
                                                repack_all=True, max_repack="unlimited"))
    assert todo(plan, "used").to_do == T.Repack and todo(plan, "partly_young").to_do == T.Keep
    plan = plan_of([f], used, opts=PruneOptions(repack_uncompressed=True, no_resize=True,
                                                max_repack="unlimited"))
    assert todo(plan, "raw").to_do == T.Repack and S.NotCompressed in todo(plan, "raw").status
    assert todo(plan, "used").to_do == T.Keep and todo(plan, "mismatch").to_do == T.Keep
    # repack_cacheable_only keeps data packs as they are
    plan = plan_of([f], used, opts=PruneOptions(repack_cacheable_only=True, max_unused="0%"))
    assert todo(plan, "partly").to_do == T.Keep and todo(plan, "mismatch").to_do == T.Keep
    with pytest.raises(RusticError) as e:
        plan_of([f], used, opts=PruneOptions(repack_uncompressed=True),
                config=ConfigFile(version=1))
    assert e.value.kind == ErrorKind.Unsupported


def test_decide_repack_limits_and_order():
    # candidates by unused / used: c1 30/10, c2 20/10 and c3 20/10 (a tie), c4 10/30
    f0 = one_file([pack("c4", [("d", 30), ("u4", 10)]), pack("c3", [("c", 10), ("u3", 20)])])
    f1 = one_file([pack("c2", [("b", 10), ("u2", 20)]), pack("c1", [("a", 10), ("u1", 30)]),
                   pack("t", [("t", 10), ("ut", 1)], tpe=TREE)])
    used = ["a", "b", "c", "d", "t"]
    plan = plan_of([f0, f1], used, opts=PruneOptions(max_unused="0%", max_repack="unlimited"))
    assert set(plan.repack_packs()) == {bid("pack:" + n) for n in ("c1", "c2", "c3", "c4", "t")}
    # a size that admits the tree pack, c1 and c3 (the tie goes to the lower
    # file number): 10 + 10 + 10 + 10 reaches 40 at c2
    plan = plan_of([f0, f1], used, opts=PruneOptions(max_unused="0%", max_repack="40b"))
    assert plan.repack_packs() == [bid("pack:c3"), bid("pack:c1"), bid("pack:t")]
    plan = plan_of([f0, f1], used, opts=PruneOptions(max_unused="0%", max_repack="11b"))
    assert plan.repack_packs() == [bid("pack:t")]
    # unlimited unused space keeps partly used data packs, not tree packs
    plan = plan_of([f0, f1], used, opts=PruneOptions(max_unused="unlimited",
                                                     max_repack="unlimited"))
    assert plan.repack_packs() == [bid("pack:t")]


def test_resize_packs():
    small = [pack("s%d" % i, [("s%d" % i, 40)], size=10) for i in range(3)]
    used = ["s0", "s1", "s2"]
    opts = PruneOptions(max_repack="unlimited")
    # 80 bytes of used blobs do not pass the pack size of 100: kept
    plan = plan_of([one_file(small[:2])], used[:2], opts=opts)
    assert plan.repack_packs() == []
    # 120 do
    plan = plan_of([one_file(small)], used, opts=opts)
    assert len(plan.repack_packs()) == 3
    # two, and the type is repacked anyway
    f = one_file(small[:2] + [pack("partly", [("b", 10), ("u", 10)])])
    plan = plan_of([f], used[:2] + ["b"], opts=PruneOptions(max_repack="unlimited",
                                                            max_unused="0%"))
    assert len(plan.repack_packs()) == 3
    plan = plan_of([one_file(small)], used, opts=PruneOptions(max_repack="unlimited",
                                                              no_resize=True))
    assert plan.repack_packs() == []


def six_packs():
    return [one_file([pack("P1", [("a", 100), ("b", 200)]), pack("P2", [("c", 50), ("d", 60)]),
                      pack("P3", [("e", 70)]), pack("T1", [("t", 30), ("u", 40)], tpe=TREE)],
                     [pack("M1", [("f", 10)], time=OLD), pack("M2", [("a", 100)], time=YOUNG)])]


def test_stats_six_packs():
    files = [(bid("index:0"), six_packs()[0])]
    existing = existing_of(files)
    existing[bid("pack:stray")] = 999
    plan = plan_of(files, ["a", "b", "c", "t"], existing=existing,
                   opts=PruneOptions(max_unused="0%", max_repack="unlimited", no_resize=True))
    assert {p.id: p.to_do for p in plan.packs} == {
        bid("pack:P1"): T.Keep, bid("pack:P2"): T.Repack, bid("pack:P3"): T.MarkDelete,
        bid("pack:T1"): T.Repack, bid("pack:M1"): T.Delete, bid("pack:M2"): T.KeepMarked}
    st = plan.stats
    assert st.blobs[DATA] == SizeStats(used=3, unused=4, remove=1, repack=2, repackrm=1)
    assert st.size[DATA] == SizeStats(used=350, unused=240, remove=70, repack=110, repackrm=60)
    assert st.blobs[TREE] == SizeStats(used=1, unused=1, remove=0, repack=2, repackrm=1)
    assert st.size[TREE] == SizeStats(used=30, unused=40, remove=0, repack=70, repackrm=40)
    assert st.packs == PackStats(used=1, partly_used=2, unused=1, repack=2, keep=1)
    assert st.packs_to_delete == DeleteStats(remove=1, recover=0, keep=1)
    assert st.size_to_delete == DeleteStats(remove=10 + 41 + 36, recover=0, keep=100 + 41 + 36)
    assert (st.packs_unref, st.size_unref) == (1, 999)
    assert (st.index_files, st.index_files_rebuild) == (1, 1)
    assert st.debug[(T.Repack, DATA, frozenset({S.HasUsedBlobs, S.HasUnusedBlobs}))] == \
        [1, 1, 60, 1, 50]
    assert st.debug[(T.Delete, DATA, frozenset({S.Marked, S.TooYoung}))] == [1, 1, 10, 0, 0]
    assert plan.size_after_prune() == {DATA: 460 + 5 * 41, TREE: 30 + 1 * 41}
    assert plan.pack_sizers()[DATA].pack_size() == 100


def test_check_existing_packs():
    files = [(bid("index:0"), one_file([pack("K", [("a", 10)]), pack("D", [("u", 10)])]))]
    ok = existing_of(files)
    for bad in ({k: v for k, v in ok.items() if k != bid("pack:K")},
                {**ok, bid("pack:K"): 5}):
        with pytest.raises(RusticError) as e:
            plan_of(files, ["a"], existing=bad)
        assert e.value.kind == ErrorKind.Internal
    assert "does not exist" in e.value.message or "does not match" in e.value.message
    # the same on a pack that is marked for deletion is no error
    plan = plan_of(files, ["a"], existing={bid("pack:K"): ok[bid("pack:K")]})
    assert plan.packs[1].to_do == T.MarkDelete
    plan = plan_of(files, ["a"], existing={**ok, bid("pack:D"): 5})
    assert (plan.stats.packs_unref, plan.stats.size_unref) == (0, 0)


def test_filter_index_files():
    # one file, nothing to do, too small: cleared
    plan = plan_of([one_file([pack("K", [("a", 10)])])], ["a"])
    assert plan.index_files == [] and plan.stats.index_files_rebuild == 0
    # two small files are rebuilt together
    plan = plan_of([one_file([pack("K", [("a", 10)])]), one_file([pack("L", [("b", 10)])])],
                   ["a", "b"])
    assert len(plan.index_files) == 2 and plan.stats.index_files == 2
    # KeepMarked needs no rewrite unless instant_delete
    f = one_file([pack("K", [("a", 10)])], [pack("M", [("u", 10)], time=YOUNG)])
    assert plan_of([f], ["a"]).index_files == []
    assert len(plan_of([f], ["a"], opts=PruneOptions(instant_delete=True)).index_files) == 1


def test_repack_pick():
    # d makes R1 needed, so that it takes a and b before R2 and K are scanned
    r1 = pack("R1", [("a", 10), ("b", 10), ("d", 10), ("u1", 10)])
    r2 = pack("R2", [("a", 10), ("c", 10), ("u2", 10)])
    k = pack("K", [("b", 10)], time=YOUNG)
    opts = PruneOptions(keep_pack=datetime.timedelta(hours=1), max_unused="0%",
                        max_repack="unlimited")
    plan = plan_of([one_file([r1, r2, k])], ["a", "b", "c", "d"], opts=opts)
    assert [p.to_do for p in plan.packs] == [T.Repack, T.Repack, T.Keep]
    assert plan.keep.tolist() == [1, 0, 1, 0, 0, 1, 0, 0]
    used = {bid("a"), bid("b"), bid("c"), bid("d")} - {bid("b")}  # the Keep pack's ids taken out
    want = [plan_repack(p, used) for p in (r1, r2)]
    assert [r for _, r in plan.repack_plans()] == want
    assert [[bl[1] for r in rs for bl in r.blobs] for rs in want] == \
        [[bid("a"), bid("d")], [bid("c")]]

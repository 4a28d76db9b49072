"""The cases of tests/basemerge.py are what they claim, by the C oracle alone (no GPU): the base
read holds exactly nb pairs, the read over the base holds the stated pairs and Count and equals the
fresh read at the same clock (where no TxId re-applies base ops), the pruned log of `unborn` reads
as the unpruned one, `txid_dup` holds duplicate pairs, `churn` has more groups than VGB; and the
Python restatement (randlog.ref_materialize) agrees with the C oracle on every case of at most 130
pairs.  The mirrored kernel constants appear verbatim in their sources."""
import os

import pytest

from tests import basemerge as bm
from tests import randlog
from tests.basemerge import AW, MV

N_DC = 3
NB = (1, 63, 64, 65, 119, 120, 121, 1024, 1025)
NS = (0, 1, 64, 119, 120, 121)


def test_mirrored_constants():
    """The mirrors agree with the sources they name (a changed kernel constant must change them)."""
    root = os.path.join(os.path.dirname(__file__), "..")
    src = lambda *p: open(os.path.join(root, *p)).read()  # noqa: E731
    grp = src("antidote_amd", "csrc", "am_group.h")
    assert "constexpr uint32_t KB = %d;" % bm.KB in grp
    assert "constexpr uint32_t VGB = VG / 2;" in grp and "constexpr uint32_t VG = AM_GRP_MAX_REC;" in grp
    hdr = src("include", "antidote_mat.h")
    assert "#define AM_GRP_MAX_REC %du" % bm.GRP_MAX_REC in hdr and bm.GRP_MAX_REC == 2 * bm.VGB
    assert "#define AM_BIG_MIN_OPS (AM_GRP_MAX_REC / 2)" in hdr and bm.AM_BIG_MIN_OPS == bm.GRP_MAX_REC // 2
    sets = src("antidote_amd", "csrc", "am_sets.hip")
    assert "KCAP = %d;" % bm.KCAP in sets and "BCAP = %d;" % bm.BCAP in sets
    assert "AM_SETS_BIG_OPS = %d;" % bm.AM_SETS_BIG_OPS in src("antidote_amd", "csrc", "am_internal.h")


def check_case(c, n_dc=N_DC):
    """The oracle's view of one case; returns the read over the base."""
    t = c["t"]
    base = bm.base_of(c, n_dc)  # asserts ok and exactly nb pairs
    assert len(c["ops"]) < bm.AM_SETS_BIG_OPS
    clock = bm.read_clock(c, n_dc)
    r = bm.oracle_read(n_dc, c["ops"], t, clock, c["nout"] + 8, base, c["txid"])
    assert r[0] == "ok", (c["name"], r)
    assert len(r[1]) == c["nout"] and r[5] == c["count"], (c["name"], len(r[1]), c["nout"], r[5], c["count"])
    assert bm.oracle_read(n_dc, c["ops"], t, clock, c["nout"], base, c["txid"])[0] == "ok"  # the exact room
    if c["nout"]:
        assert bm.oracle_read(n_dc, c["ops"], t, clock, c["nout"] - 1, base, c["txid"]) == ("error", bm.abi.AM_ERR_CAPACITY)
    if c["fresh"]:  # the closed form's claim: folding the new ops into the base = the fresh fold
        f = bm.oracle_read(n_dc, c["hist"], t, clock, c["nout"] + 8)
        assert f[0] == "ok" and f[1] == r[1], c["name"]
    if c["nb"] <= bm.KB and c["ns"] is not None and c["ns"] <= bm.KB and c["txid"] is None:
        # meant for the wave tier (base_merge): the key must be one that tier takes
        assert bm.wave_tier_key(t, c["ops"]) and bm.n_groups(t, c["ops"]) <= bm.GRP_MAX_REC, c["name"]
    if c["nout"] <= 130 and c["nb"] <= 130:
        py = randlog.ref_materialize(t, c["ops"], bm.read_of(c, 0, n_dc))
        assert py == r, (c["name"], py[:1], r[:1])
    return r


@pytest.mark.parametrize("t", [AW, MV])
def test_sizes_cases(t):
    """Every (nb, ns) around the lane split (64), KB (120) and BCAP (1024): the counts are exact, and
    the default kills leave holes at both ends and on both sides of position 64."""
    for nb in NB:
        for ns in NS:
            c = bm.sizes(t, nb, ns, N_DC)
            kills = bm.default_kills(nb)
            assert c["nout"] == nb - len(kills) + ns
            r = check_case(c)
            base, got, had = c["base"][2], set(r[1]), set(c["base"][2])
            gone = [j for j, p in enumerate(base) if p not in got]
            assert gone == kills, (nb, ns, gone)
            if nb >= 65:
                assert {0, 63, 64, nb - 1} <= set(gone)
            new = [p for p in r[1] if p not in had]
            assert len(new) == ns
            if ns > nb:  # new pairs below, between and above the base's
                assert new[0] < base[0] and new[-1] > base[-1]


@pytest.mark.parametrize("t", [AW, MV])
def test_sizes_padded(t):
    """The zone-skip keys: 600 + 500 ops (AW; MV 600 + 400, within AM_BIG_MIN_OPS), the base phase
    ends exactly at op 600, and the wave tier takes the key."""
    for ns in (1, 120):
        more = 500 if t == AW else 400
        c = bm.sizes(t, 120, ns, N_DC, base_ops=600, new_ops=more)
        assert (c["n_base"], c["n_read"], len(c["ops"])) == (600, 600 + more, 602 + more)
        check_case(c)
        assert bm.wave_tier_key(t, c["ops"])


def test_interleave_aw():
    c = bm.interleave(AW, N_DC)
    r = check_case(c)
    per = {}
    for e, x in r[1]:
        per.setdefault(e, []).append(x)
    base = {}
    for e, x in c["base"][2]:
        base.setdefault(e, []).append(x)
    # the new tokens first, the newest of them before the older; the base tokens behind, in base order
    assert per[45500] == [bm.NEW + 21, bm.NEW + 20] + base[45500] and len(base[45500]) == 2
    assert per[bm._elem(4)] == [bm.NEW + 22, bm.NEW + 23, bm.TOK + 4]  # one effect's tokens in its order
    assert len(base[31500]) == 4 and per[31500] == [x for x in base[31500] if x in (bm.TOK + 100, bm.TOK + 102)]
    assert 20500 in base and 20500 not in per  # every token killed, none added: the element is gone
    elems = sorted(per)
    assert elems[:3] == [1, 2, 3] and elems[-2:] == [10 ** 9 + 1, 10 ** 9 + 2]  # rank search at lo = 0 / lo = nb
    assert all(bm._elem(j) + 500 in per for j in bm.GAPS)
    assert all(bm._elem(j) not in per for j in (0, 63, 64, 69))


def test_interleave_mv():
    c = bm.interleave(MV, N_DC)
    r = check_case(c)
    base = c["base"][2]
    assert [x for v, x in r[1] if v == 5000] == [7, bm.TOK + 4, bm.TOK + 200, bm.TOK + 500, bm.TOK + 900]
    gone = [j for j, p in enumerate(base) if p not in set(r[1])]
    assert gone == [0, 62, 63, 64, 65, 70]  # one assign overrides base pairs on both sides of position 64
    assert r[1][0][0] == 1 and r[1][-1][0] == 10 ** 9 + 2


@pytest.mark.parametrize("t", [AW, MV])
def test_unborn(t):
    """The log holds no birth of any base token; its read over the base equals the read of the
    unpruned history (over the base, and fresh)."""
    c = bm.unborn(t, N_DC)
    r = check_case(c)  # (fresh: against the fresh read of the history)
    assert len(c["ops"]) == len(c["hist"]) - c["n_base"] and c["ops"][0].op_id == c["n_base"] + 1
    born = set()
    for op in c["ops"]:
        if t == AW:
            born |= {x for _, add, _ in op.effect for x in add}
        elif op.effect[0] == "assign":
            born.add(op.effect[2])
    assert not born & {x for _, x in c["base"][2]}
    full = bm.oracle_read(N_DC, c["hist"], t, bm.read_clock(c, N_DC), 256, c["base"])
    assert full == r  # every column: NewLastOp from the explicit ids
    assert len(r[1]) == (118 if t == AW else 117)
    if t == AW:
        assert [x for e, x in r[1] if e == bm._elem(10)] == [bm.NEW + 999, bm.TOK + 10]


@pytest.mark.parametrize("t", [AW, MV])
def test_churn(t):
    c = bm.churn(t, N_DC)
    check_case(c)
    assert bm.VGB < bm.n_groups(t, c["ops"]) <= bm.GRP_MAX_REC  # by_birth is off
    assert bm.wave_tier_key(t, c["ops"])  # and the key is still grouped
    assert 100 <= c["nb"] <= bm.KB and c["ns"] <= bm.KB and len(c["ops"]) == 1000
    assert len(set(c["base"][2]) & set(check_case(c)[1])) >= 10  # base pairs that stay


@pytest.mark.parametrize("t", [AW, MV])
def test_txid_cases(t):
    c = bm.txid_dup(t, N_DC)
    r = check_case(c)
    dups = [p for i, p in enumerate(r[1]) if i and r[1][i - 1] == p]
    assert dups == ([(1100, 1010), (2100, 1020)] if t == AW else [])  # insert_sorted drops an MV copy
    plain = check_case(bm.txid_dup(t, N_DC, txid=9))
    assert len(plain[1]) == 70 and len(set(plain[1])) == 70
    assert sum(op.txid == 5 for op in c["ops"][:c["n_base"]]) == 2 and not any(op.txid == 9 for op in c["ops"])


@pytest.mark.parametrize("t", [AW, MV])
def test_lds_edges(t):
    cs = bm.lds_edge(t, N_DC)
    assert [c["name"] for c in cs] == ["sum-1024", "sum-1025", "base-1024", "base-1025"]
    for c, total in zip(cs, (bm.BCAP, bm.BCAP + 1, bm.BCAP, bm.BCAP + 1)):
        check_case(c)
        assert c["nb"] > bm.KB and 300 <= len(c["ops"]) <= 2100
        births = 0  # of the ops past the base
        for op in c["ops"][c["n_base"]:c["n_read"]]:
            births += sum(len(add) for _, add, _ in op.effect) if t == AW else op.effect[0] == "assign"
        assert c["nb"] + births == total, (c["name"], c["nb"], births)

"""The HOST instantiation of mm355_regs.h -- the region type Reg / Extra of mm355_glue.h, glibc's logf and pow, caller-provided scratch; what
mm355_glue.cpp runs before and after extension -- against the oracle, on the CPU.  tests/host_harness/regs_finish_host.cpp is built as a
stand-alone program with g++ under AddressSanitizer and UBSan; its regions are held, field by field and in order, against the oracle's mmo_*
functions called one by one through ctypes.

(a) after extension: set_parent(sub_diff), select_sub(check_strand = 0), set_sam_pri, set_mapq(match_sc) and the inversion pass on constructed
    region sets with extension records -- the branches no end-to-end CPU test reaches.  A census, taken from the oracle's side alone, shows
    that every one of them is reached under every option set.
(b) before extension: gen_regs .. filter_strand_retained through Reg, on the world and option sets of tests/test_chain_only_host.py (which pin
    the device instantiation on the same inputs)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
import _capi
import _named_truth as T
from _tags_truth import Extra, f32_bits
from test_chain_only_host import CASES, world    # noqa: F401  (the fixture and the option sets of the device instantiation's test)

ALL_CHAINS, HARD_MLEVEL = T.ALL_CHAINS, T.HARD_MLEVEL
QLEN, N_CASES, SEED = 2000, 2000, 355
REG1 = np.dtype([(k, "<i4") for k in ("id", "cnt", "rid", "score", "qs", "qe", "rs", "re", "parent", "subsc", "as", "mlen", "blen", "n_sub",
                                      "score0")] + [("bits", "<u4"), ("hash", "<u4"), ("div", "<f4"), ("p", "<u8")])
assert REG1.itemsize == C.sizeof(T.Reg1) == 80
B_REV, B_INV, B_SAM_PRI, B_STRAND_RETAINED = 10, 11, 12, 26     # mmo_reg1_t's bit fields: mapq:8 split:2 rev inv sam_pri ... strand_retained
OPTION_SETS = [("map-ont", 0), ("map-hifi", 0), ("asm20", 0), ("map-ont", HARD_MLEVEL), ("map-ont", ALL_CHAINS)]
POST_OUT = ("id", "parent", "subsc", "n_sub", "mapq", "sam_pri", "strand_retained", "inv", "score", "dp_max2")
PRE_OUT = ("id", "parent", "cnt", "rid", "score", "score0", "qs", "qe", "rs", "re", "as", "mlen", "blen", "subsc", "n_sub", "hash", "rev",
           "strand_retained", "sam_pri", "div_bits")


@pytest.fixture(scope="module")
def harness(built, tmp_path_factory):
    """the program; run(words) -> per case, the list of its regions as tuples of int"""
    exe = str(tmp_path_factory.mktemp("regsfinish") / "regs_finish_host")
    # the sanitizer runtimes are linked statically: the program must not depend on what else the process that runs it has loaded
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-fno-omit-frame-pointer",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           os.path.join(_capi.HERE, "host_harness", "regs_finish_host.cpp"), "-o", exe])

    def run(words):
        r = subprocess.run([exe], input=np.concatenate(words).astype("<i8").tobytes(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 0, (r.returncode, r.stderr[-4000:].decode(errors="replace"))
        lines = [tuple(map(int, l.split())) for l in r.stdout.decode().splitlines()]
        out, i = [], 0
        while i < len(lines):
            n = lines[i][0]
            out.append(lines[i + 1:i + 1 + n])
            i += 1 + n
        return out
    return run


def _i64(*v):
    return np.array(v, np.int64)


# ================================================================ (a) after extension
def _opts(preset, extra):
    orc = O.OracleAligner(seqs=["ACGTTGCAAGCTTAGCCATGACGTAGCTAGGATCCAT" * 8], preset=preset)
    mo = orc.mo
    return dict(flag=(mo.flag | extra) & (ALL_CHAINS | HARD_MLEVEL), mask_level=mo.mask_level, mask_len=mo.mask_len, sub_diff=mo.a * 2 + mo.b,
                pri_ratio=mo.pri_ratio, min_diff=orc.k * 2, best_n=mo.best_n, min_strand_sc=int(mo.max_gap * 0.8), min_chain_sc=mo.min_chain_score,
                match_sc=mo.a)


def _gen_case(rng, o):
    """one region set, rows in descending order of hit_sort's key (dp_max with an extension record, else the chain score)"""
    n = int(rng.integers(1, 25))
    p_mode = rng.choice(3, p=[0.6, 0.2, 0.2])                  # every region has an extension record / none has / some have
    rows = []

    def fresh():
        ln = int(rng.integers(50, 900)); qs = int(rng.integers(0, QLEN - ln)); rs = int(rng.integers(0, 100000))
        return dict(qs=qs, qe=qs + ln, rid=int(rng.integers(0, 2)), rs=rs, re=rs + ln + int(rng.integers(-20, 20)), rev=int(rng.integers(0, 2)))

    def finish(r, base=None, inv=0):
        ln = r["qe"] - r["qs"]
        r["inv"] = inv
        r["cnt"] = 0 if inv else int(rng.integers(3, 21))          # both sides of 10
        r["score"] = 0 if inv else int(rng.integers(40, 300))      # both sides of 100
        if base is not None and not inv and rng.random() < 0.5:
            r["score"] = max(1, base["score"] - int(rng.integers(0, 40)))
        r["score0"] = r["score"] + int(rng.integers(0, 2)) * int(rng.integers(0, 30))
        r["blen"] = ln + int(rng.integers(0, 30)); r["mlen"] = max(1, int(r["blen"] * (0.7 + 0.3 * rng.random())))
        r["subsc"] = int(rng.integers(0, 2)) * int(rng.integers(0, max(1, r["score"]))); r["n_sub"] = int(rng.integers(0, 3))
        r["has_p"] = 1 if inv or p_mode == 0 else 0 if p_mode == 1 else int(rng.integers(0, 2))
        if base is not None and base["has_p"] and rng.random() < 0.8:   # dp_max differences on both sides of sub_diff
            r["dp_max"] = max(1, base["dp_max"] - int(rng.integers(0, 2 * o["sub_diff"] + 3)))
        else:
            r["dp_max"] = max(1, r["score"] * o["match_sc"] + int(rng.integers(-30, 30))) if not inv else int(rng.integers(40, 200))
        r["dp_max2"] = [0, int(rng.integers(1, r["dp_max"])) if r["dp_max"] > 1 else 0, r["dp_max"]][int(rng.integers(0, 3))]
        if not r["has_p"]:
            r["dp_max"] = r["dp_max2"] = 0
        rows.append(r)

    if n >= 3 and rng.random() < 0.3:        # an inversion between two primaries of one contig
        rs, rev = int(rng.integers(0, 50000)), int(rng.integers(0, 2))
        q0 = int(rng.integers(0, 400)); l1, li, l2 = int(rng.integers(300, 600)), int(rng.integers(60, 200)), int(rng.integers(300, 600))
        finish(dict(qs=q0, qe=q0 + l1, rid=0, rs=rs, re=rs + l1, rev=rev))
        finish(dict(qs=q0 + l1, qe=q0 + l1 + li, rid=0, rs=rs + l1, re=rs + l1 + li, rev=1 - rev), inv=1)
        finish(dict(qs=q0 + l1 + li, qe=q0 + l1 + li + l2, rid=0, rs=rs + l1 + li, re=rs + l1 + li + l2, rev=rev))
    while len(rows) < n:
        kind = int(rng.integers(0, 5)) if rows else 0
        if kind == 0:
            finish(fresh())
            continue
        b = rows[int(rng.integers(0, len(rows)))]
        r = {k: b[k] for k in ("qs", "qe", "rid", "rs", "re", "rev")}
        ln = b["qe"] - b["qs"]
        if kind == 1:                         # identical on the query, other target
            r.update(rid=int(rng.integers(0, 2)), rs=b["rs"] + int(rng.integers(0, 2)) * int(rng.integers(1, 5000)), rev=int(rng.integers(0, 2)))
            r["re"] = r["rs"] + (b["re"] - b["rs"])
        elif kind == 2:                       # identical coordinates: select_sub's equality rule
            r["rev"] = int(rng.integers(0, 2)) if rng.random() < 0.3 else b["rev"]
        elif kind == 3 and ln > 20:           # nested
            d0, d1 = int(rng.integers(0, ln // 4)), int(rng.integers(0, ln // 4))
            r.update(qs=b["qs"] + d0, qe=b["qe"] - d1, rs=b["rs"] + d0, re=b["re"] - d1)
        else:                                 # partly overlapping
            sh = int(rng.integers(1, ln)) * (1 if rng.random() < 0.5 else -1)
            qs = min(max(0, b["qs"] + sh), QLEN - ln)
            r.update(qs=qs, qe=qs + ln, rs=max(0, b["rs"] + sh)); r["re"] = r["rs"] + (b["re"] - b["rs"])
        finish(r, base=b if not b["inv"] else None)
    rows.sort(key=lambda r: -(r["dp_max"] if r["has_p"] else r["score"]))
    for i, r in enumerate(rows):
        r["hash"] = i                          # the row's tag: tells which regions select_sub dropped
        r["id"], r["parent"] = -1, -1          # set_parent numbers them
    if o["flag"] & ALL_CHAINS:                 # no set_parent: the ids and parents are the input's
        pri = []
        for i, r in enumerate(rows):
            r["id"] = i
            r["parent"] = -1 if r["inv"] or rng.random() < 0.15 else i if not pri or rng.random() < 0.5 else pri[int(rng.integers(0, len(pri)))]
            if r["parent"] == i:
                pri.append(i)
    return rows, int(rng.integers(0, 2)) * int(rng.integers(0, 400))


IN_FIELDS = ("id", "parent", "cnt", "rid", "score", "score0", "qs", "qe", "rs", "re", "mlen", "blen", "subsc", "n_sub", "hash", "rev", "inv",
             "has_p", "dp_max", "dp_max2")


def _case_words(o, rows, rep_len):
    return [_i64(1, o["flag"], f32_bits(o["mask_level"]), o["mask_len"], o["sub_diff"], f32_bits(o["pri_ratio"]), o["min_diff"], o["best_n"],
                 o["min_strand_sc"], o["min_chain_sc"], o["match_sc"], rep_len, len(rows)),
            np.array([[r[k] for k in IN_FIELDS] for r in rows], np.int64).reshape(-1)]


def _oracle_post(L, libc, o, rows, rep_len, census):
    """the case through mmo_set_parent, mmo_select_sub(check_strand = 0), mmo_set_sam_pri, mmo_set_mapq; returns POST_OUT tuples and adds
    the branches the case reached to `census`"""
    n0 = len(rows)
    a = np.zeros(n0, REG1)
    for k in ("id", "parent", "cnt", "rid", "score", "score0", "qs", "qe", "rs", "re", "mlen", "blen", "subsc", "n_sub", "hash"):
        a[k] = [r[k] for r in rows]
    a["bits"] = [r["rev"] << B_REV | r["inv"] << B_INV for r in rows]
    a["div"] = -1.0
    for i, r in enumerate(rows):
        if r["has_p"]:                         # mmo_select_sub frees a dropped region's record: libc's malloc
            ptr = libc.malloc(C.sizeof(Extra))
            C.memset(ptr, 0, C.sizeof(Extra))
            e = Extra.from_address(ptr)
            e.dp_max, e.dp_max2 = r["dp_max"], r["dp_max2"]
            a["p"][i] = ptr
    regs = C.cast(a.ctypes.data, C.POINTER(T.Reg1))
    n = C.c_int(n0)
    if not o["flag"] & ALL_CHAINS:
        L.mmo_set_parent(o["mask_level"], o["mask_len"], n0, regs, o["sub_diff"], int(bool(o["flag"] & HARD_MLEVEL)), 0.0)
        for i in range(n0):                    # census: n_sub raised by the sub_diff rule alone
            pa = int(a["parent"][i])
            if pa != i and rows[i]["has_p"] and rows[pa]["has_p"] and rows[i]["cnt"] < rows[pa]["cnt"]:
                ri, rp = rows[i], rows[pa]
                ol = min(ri["qe"], rp["qe"]) - max(ri["qs"], rp["qs"])
                same = (rp["rid"], rp["rs"], rp["re"]) == (ri["rid"], ri["rs"], ri["re"]) and ol == min(ri["qe"] - ri["qs"], rp["qe"] - rp["qs"])
                if not same and rp["dp_max"] - ri["dp_max"] <= o["sub_diff"]:
                    census["n_sub by sub_diff"] += 1
        parent0 = a["parent"].copy()
        L.mmo_select_sub(o["pri_ratio"], o["min_diff"], o["best_n"], 0, o["min_strand_sc"], C.byref(n), regs)
        kept = set(int(h) for h in a["hash"][:n.value])
        n_2nd = 0
        for i in range(n0):                    # census: a secondary dropped for identical coordinates (its score test passed: equal scores)
            pa = int(parent0[i])
            if pa == i or rows[i]["inv"]:
                continue
            ri, rp = rows[i], rows[pa]
            if i not in kept and n_2nd < o["best_n"] and ri["score"] == rp["score"] and \
                    all(ri[k] == rp[k] for k in ("qs", "qe", "rid", "rs", "re")):
                census["dropped identical"] += 1
            n_2nd += i in kept
        census["sync_regs"] += n.value != n0
        L.mmo_set_sam_pri(n.value, regs)
    L.mmo_set_mapq(n.value, regs, o["min_chain_sc"], o["match_sc"], rep_len, 0)
    out = []
    sum_sc = sum(int(a["score"][i]) for i in range(n.value) if a["parent"][i] == a["id"][i])
    for i in range(n.value):
        r = a[i]
        bits, mapq, dp_max, dp_max2 = int(r["bits"]), int(r["bits"]) & 0xff, 0, -1
        if r["p"]:
            e = Extra.from_address(int(r["p"]))
            dp_max, dp_max2 = e.dp_max, e.dp_max2
            libc.free(int(r["p"]))
        inv = bits >> B_INV & 1
        if inv:
            census["inv takes a neighbour's MAPQ"] += mapq > 0          # (set_mapq itself gives an inversion 0)
        elif r["parent"] == r["id"]:
            form = "dp_max2 form" if dp_max2 > 0 and dp_max > 0 else "p form" if dp_max2 >= 0 else "no-p form"
            census[form] += 1
            if dp_max2 >= 0 and dp_max > dp_max2 and mapq == 1:
                # the 0 -> 1 bump, not a MAPQ of 1: the first term of the formula, in double, stays clearly under 1, so its (int) is <= 0
                score, cnt, subsc = int(r["score"]), int(r["cnt"]), max(int(r["subsc"]), o["min_chain_sc"])
                pen = min((1.0 if score > 100 else 0.01 * score) * sum_sc / (sum_sc + rep_len), 1.0 if cnt > 10 else 0.1 * cnt)
                ident = int(r["mlen"]) / int(r["blen"])
                x = dp_max2 * subsc / dp_max / int(r["score0"]) if dp_max2 > 0 else subsc / int(r["score0"])
                first = ident * pen * 40.0 * (1.0 - (x * x if dp_max2 > 0 else x)) * math.log(dp_max / o["match_sc"])
                if dp_max2 > 0:
                    first = min(first, 6.02 * ident * ident * (dp_max - dp_max2) / o["match_sc"] + .499)
                census["0 -> 1 bump"] += first < 0.9
        out.append((int(r["id"]), int(r["parent"]), int(r["subsc"]), int(r["n_sub"]), mapq, bits >> B_SAM_PRI & 1, bits >> B_STRAND_RETAINED & 1, inv,
                    int(r["score"]), dp_max2))
    return out


@pytest.mark.parametrize("preset,extra", OPTION_SETS, ids=["%s-%#x" % s for s in OPTION_SETS])
def test_post_extension_sequence_equals_oracle(harness, preset, extra):
    L = T._lib()
    libc = C.CDLL(None)
    libc.malloc.restype = C.c_void_p; libc.malloc.argtypes = [C.c_size_t]; libc.free.argtypes = [C.c_void_p]
    o = _opts(preset, extra)
    rng = np.random.Generator(np.random.PCG64(SEED))
    census = {k: 0 for k in ("dp_max2 form", "p form", "no-p form", "0 -> 1 bump", "inv takes a neighbour's MAPQ", "n_sub by sub_diff",
                             "dropped identical", "sync_regs")}
    words, exp = [], []
    for _ in range(N_CASES):
        rows, rep_len = _gen_case(rng, o)
        words += _case_words(o, rows, rep_len)
        exp.append(_oracle_post(L, libc, o, rows, rep_len, census))
    print(preset, hex(extra), census)
    not_reachable = ("n_sub by sub_diff", "dropped identical", "sync_regs") if extra & ALL_CHAINS else ()
    assert all(v > 0 for k, v in census.items() if k not in not_reachable), census
    got = harness(words)
    assert len(got) == N_CASES
    for c, (g, e) in enumerate(zip(got, exp)):
        assert len(g) == len(e), (c, len(g), len(e))
        for i, (gr, er) in enumerate(zip(g, e)):
            assert gr == er, (c, i, dict(zip(POST_OUT, gr)), dict(zip(POST_OUT, er)))


# ================================================================ (b) before extension
def _pre_words(orc, qlen, u, ca, mp):
    mo = orc.mo
    sl = orc.seq_lens
    return [_i64(2, mo.flag, f32_bits(mo.mask_level), mo.mask_len, f32_bits(mo.pri_ratio), orc.k * 2, mo.best_n, int(mo.max_gap * 0.8), mo.seed, qlen,
                 len(u), len(ca), len(mp), len(sl)), u.view(np.int64), ca.reshape(-1).view(np.int64), mp.view(np.int64), np.array(sl, np.int64)]


def _oracle_pre(L, orc, qlen, u, ca, mp):
    """mmo_gen_regs, mmo_set_parent, mmo_select_sub(check_strand = 1), mmo_est_err, mmo_filter_strand_retained -> PRE_OUT tuples"""
    mo = orc.mo
    regs = L.mmo_gen_regs(T.read_hash(qlen, mo.seed, None), qlen, len(u), u.ctypes.data, ca.ctypes.data, 0)
    n = C.c_int(len(u))
    if not mo.flag & ALL_CHAINS:
        L.mmo_set_parent(mo.mask_level, mo.mask_len, n.value, regs, mo.a * 2 + mo.b, int(bool(mo.flag & HARD_MLEVEL)), mo.alt_drop)
        L.mmo_select_sub(mo.pri_ratio, orc.k * 2, mo.best_n, 1, int(mo.max_gap * 0.8), C.byref(n), regs)
    L.mmo_est_err(orc.idx, qlen, n.value, regs, ca.ctypes.data, len(mp), mp.ctypes.data)
    n.value = L.mmo_filter_strand_retained(n.value, regs)
    out = []
    for i in range(n.value):
        r = regs[i]
        out.append((r.id, r.parent, r.cnt, r.rid, r.score, r.score0, r.qs, r.qe, r.rs, r.re, r.as_, r.mlen, r.blen, r.subsc, r.n_sub, r.hash,
                    r.bits >> B_REV & 1, r.bits >> B_STRAND_RETAINED & 1, r.bits >> B_SAM_PRI & 1, f32_bits(r.div)))
    L.free(C.cast(regs, C.c_void_p))
    return out


def _chains(orc, seq):
    qlen = len(seq)
    if orc.mo.max_qlen > 0 and qlen > orc.mo.max_qlen:
        return None
    a, _rep_len, mini_pos, _ = orc.anchors(seq, sorted_=True)
    if len(a) == 0:
        return None
    u, ca, _ = orc.chains_final(a, qlen)
    if len(u) == 0:
        return None
    return np.ascontiguousarray(u, np.uint64), np.ascontiguousarray(ca, np.uint64), np.ascontiguousarray(mini_pos, np.uint64)


@pytest.mark.parametrize("preset,kw", CASES, ids=["%s-%s" % (p, "-".join("%s=%s" % i for i in kw.items()) or "default") for p, kw in CASES])
def test_pre_extension_sequence_equals_oracle(harness, world, preset, kw):
    """every region of the harness is marked div_unsure before filter_strand_retained: had the host instantiation a deferral, the reads of
    the inverted block (strand_retained regions) would come back short"""
    L = T._lib()
    orc = O.OracleAligner(world["fa"], preset=preset, **kw)
    orc.mo.flag &= ~4
    words, exp = [], []
    for rd in world["reads"]:
        c = _chains(orc, rd)
        if c is not None:
            words += _pre_words(orc, len(rd), *c)
            exp.append(_oracle_pre(L, orc, len(rd), *c))
    if preset == "map-ont" and kw.get("extra_flags") == ALL_CHAINS:      # test_chain_only_host's key tie: the later chain comes first
        span = 15
        a0 = [(100 + 10 * i, 50 + 10 * i) for i in range(6)]
        a1 = a0[:1] + [(100 + 12 * i, 50 + 10 * i) for i in range(1, 6)]
        ca = np.array([(x, span << 32 | y) for x, y in a0 + a1], np.uint64)
        u = np.array([(40 << 32) | 6, (40 << 32) | 6], np.uint64)
        mp = np.array(sorted(set((span << 32) | y for _, y in a0 + a1)), np.uint64)
        words += _pre_words(orc, 400, u, ca, mp)
        exp.append(_oracle_pre(L, orc, 400, u, ca, mp))
        assert [r[PRE_OUT.index("re")] for r in exp[-1]] == [a1[-1][0] + 1, a0[-1][0] + 1]
    got = harness(words)
    assert len(got) == len(exp) > 100
    for c, (g, e) in enumerate(zip(got, exp)):
        assert len(g) == len(e), (preset, kw, c, len(g), len(e))
        for i, (gr, er) in enumerate(zip(g, e)):
            assert gr == er, (preset, kw, c, i, dict(zip(PRE_OUT, gr)), dict(zip(PRE_OUT, er)))
    if preset == "map-ont" and not kw:                                   # the reads of the inverted block do reach select_sub's strand rule
        n_reached = 0
        for rd in world["reads"][180:184]:
            u, ca, _ = _chains(orc, rd)
            first = np.concatenate(([0], np.cumsum(u & np.uint64(0xffffffff))[:-1])).astype(np.int64)
            sc, rev = (u >> np.uint64(32)).astype(np.int64), (ca[first, 0] >> np.uint64(63)).astype(np.int64)
            top = int(np.argmax(sc))
            n_reached += int(((rev != rev[top]) & (sc > int(orc.mo.max_gap * 0.8)) & (sc < sc[top] * orc.mo.pri_ratio)).sum())
        assert n_reached >= 4

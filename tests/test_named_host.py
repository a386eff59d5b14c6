"""Query names (mm355_map_batch_named, Aligner.map(name=...)) on the CPU.

The truth helper tests/_named_truth.py proves itself: its composition of the oracle's stages equals mmo_map(qname) with the filter off, and
with the filter on its regions to other targets are mmo_map(qname)'s regions with qname < tname.  Then the host-side pieces, compiled with
g++ alone (tests/host_harness/named_host.cpp): mm355_regs.h with a name hash against mmo_map(qname), the MM_SEED_SELF clamp against a table
worked by hand, the name ranking against Python's bytes comparison.  GPU side: tests/test_gpu_named.py."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
import _capi
import _named_truth as T


@pytest.fixture(scope="module")
def named_lib(built):
    L = _capi.build_harness("named_host", ["-w", "-ffp-contract=off"], ["mm355_regs.h", "mm355_core.h", "mm355_names.h", "mm355_selfclamp.h"])
    L.named_regs_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int, C.c_void_p, C.c_void_p, C.c_int32,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_uint32]
    L.named_read_hash.restype = L.named_read_hash0.restype = L.named_x31.restype = C.c_uint32
    L.named_read_hash.argtypes = [C.c_int32, C.c_int32, C.c_uint32]
    L.named_read_hash0.argtypes = [C.c_int32, C.c_int32]
    L.named_x31.argtypes = [C.c_char_p]
    L.named_clamp.argtypes = [C.c_void_p]
    L.named_clamp.restype = None
    L.named_prepare.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.c_void_p]
    L.named_prepare.restype = None
    L.named_filter_applies.argtypes = [C.c_int, C.c_int64, C.c_int32]
    return L


# ------------------------------------------------------------------ the helper proves itself
@pytest.mark.parametrize("preset,xf,cigar", [("ava-ont", 0, False), ("map-ont", 3, False), ("map-ont", 3, True), ("ava-ont", 0, True)])
def test_truth_helper_self_proof(built, preset, xf, cigar):
    W = T.overlap_world()
    orc = O.OracleAligner(W["fa"], preset=preset, extra_flags=xf)
    if not cigar:
        orc.mo.flag &= ~4
    tn = [t.encode() for t in orc.seq_names]
    assert tn == [nm for nm, _ in W["targets"]]
    n_self = n_all = n_flt = 0
    for nm, s in W["queries"]:
        whole = T.oracle_named(orc, s, nm, with_cs=cigar)
        off, _ = T.compose_named(orc, s, nm, filter_on=False, with_cs=cigar)
        assert off == whole, nm                                   # the composition IS mmo_map when it filters nothing
        flt, ns = T.compose_named(orc, s, nm, filter_on=True, with_cs=cigar)
        n_self += ns; n_all += len(whole); n_flt += len(flt)
        if nm is None:
            assert flt == whole
        elif orc.mo.flag & T.ALL_CHAINS and not cigar:
            # regions are independent under ALL_CHAINS: what the filter leaves on OTHER names is what mmo_map reports for qname < tname
            assert [T.row_tuple(d) for d in flt if tn[d["rid"]] != nm] == [T.row_tuple(d) for d in whole if nm < tn[d["rid"]]], nm
    assert n_self > 100                                           # the read with the internal repeat, in every option set
    if orc.mo.flag & T.ALL_CHAINS:                                # (without ALL_CHAINS select_sub caps the rows: the filter frees slots for other targets)
        assert n_flt < n_all


def test_truth_world_shapes(built):
    """the inputs hold what the kernels can get wrong: > 1024 kept seeds, SELF anchors, a read that loses everything, the name shapes"""
    W = T.overlap_world()
    orc = O.OracleAligner(W["fa"], preset="ava-ont")
    names = [nm for nm, _ in W["targets"]]
    assert {b"rd1", b"rd10", b"rd1a", b""} <= set(names) and names.count(b"dup") == 2 and any(max(nm, default=0) >= 0x80 for nm in names)
    q = dict((nm, s) for nm, s in W["queries"] if nm is not None)
    assert orc.anchors(q[b"long8k"], sorted_=False)[2].shape[0] > 1024          # kept seeds (mini_pos) cross EX_TILE
    a, _, _, n_self = T.filtered_anchors(orc, q[b"selfrep"], b"selfrep")
    assert n_self > 100 and int((a[:, 1] >> np.uint64(43) & np.uint64(1)).sum()) == n_self
    gname, gseq = W["targets"][W["greatest"]]
    a0 = orc.anchors(gseq, sorted_=False)[0]
    a1 = T.filtered_anchors(orc, gseq, gname)[0]
    assert len(a0) > 1000 and len(a1) < len(a0) // 20                            # the greatest name: (nearly) everything dropped
    assert any(nm is None for nm, _ in W["queries"][1:-1])


# ------------------------------------------------------------------ mm355_regs.h with a name hash
def _harness_rows(L, orc, seq, name_hash):
    import mappy_rs
    mo = orc.mo
    qlen = len(seq)
    a, rep_len, mini_pos, _ = orc.anchors(seq, sorted_=True)
    u, ca, _ = orc.chains_final(a, qlen)
    if len(u) == 0:
        return []
    opt_i = np.array([mo.flag, mo.mask_len, mo.best_n, orc.k * 2, int(mo.max_gap * 0.8), mo.min_chain_score, mo.seed], np.int64)
    opt_f = np.array([mo.mask_level, mo.pri_ratio], np.float32)
    seq_len = np.array(orc.seq_lens, np.uint32)
    u = np.ascontiguousarray(u, np.uint64); ca = np.ascontiguousarray(ca, np.uint64); mp = np.ascontiguousarray(mini_pos, np.uint64)
    out = np.zeros(len(u), mappy_rs._HIT_DTYPE)
    tg = np.zeros(len(u), mappy_rs._TAG_DTYPE)
    n = L.named_regs_host(opt_i.ctypes.data, opt_f.ctypes.data, seq_len.ctypes.data, qlen, rep_len, len(u), u.ctypes.data, ca.ctypes.data,
                          len(mp), mp.ctypes.data, out.ctypes.data, tg.ctypes.data, 0 if name_hash is None else 1, name_hash or 0)
    assert n >= 0
    return [tuple(int(h[k]) for k in T.ROW_FIELDS) + (int(t["score"]), T.f32_bits(t["div"]), int(t["rep_len"])) for h, t in zip(out[:n], tg[:n])]


def _want(d):
    return T.row_tuple(d) + (d["score"], d["div_bits"], d["rep_len"])


def test_regs_header_with_name_hash(named_lib):
    W = T.dup_world()
    orc = O.OracleAligner(W["fa"], preset="map-ont")
    orc.mo.flag &= ~4
    n_dep = 0
    for s in W["reads"]:
        base = [_want(d) for d in T.oracle_named(orc, s, None)]
        assert _harness_rows(named_lib, orc, s, None) == base            # the form without the argument: today's result
        assert _harness_rows(named_lib, orc, s, 0) == base
        seen = {tuple(base)}
        for nm in W["names"]:
            want = [_want(d) for d in T.oracle_named(orc, s, nm)]
            assert _harness_rows(named_lib, orc, s, T.x31(nm)) == want, nm
            seen.add(tuple(want))
        n_dep += len(seen) > 1
    assert n_dep >= 2                                                     # the name does decide between the identical copies


def test_hash_and_x31(named_lib):
    for nm in (b"", b"a", b"rd1", b"read/1", b"q\xff", b"rd\xc3\xa9", b"a-long-read-name-0001"):
        assert named_lib.named_x31(nm) == T.x31(nm)
        for qlen, seed in ((1, 11), (3000, 11), (123457, 0)):
            assert named_lib.named_read_hash(qlen, seed, T.x31(nm)) == T.read_hash(qlen, seed, nm)
    assert named_lib.named_read_hash0(3000, 11) == named_lib.named_read_hash(3000, 11, 0) == T.read_hash(3000, 11, None)
    assert T.read_hash(3000, 11, b"rd1", T.NO_HASH_NAME) == T.read_hash(3000, 11, None)


# ------------------------------------------------------------------ the MM_SEED_SELF clamp
# rs, qs, re, qe | rs0, qs0, re0, qe0 -> expected rs0, qs0, re0, qe0; worked by hand from U:align.c::mm_align1:
#   max_ext = |qs - rs|: rs0 = max(rs0, rs - max_ext), qs0 = max(qs0, qs - max_ext);  max_ext = |qe - re|: re0 = min(re0, re + max_ext), qe0 likewise
CLAMP_CASES = [
    ((1000, 400, 1900, 1300, 0, 0, 3000, 3000), (400, 0, 2500, 1900)),        # both sides bind on the target; the query starts at 0 (400 - 600 < 0 stays 0)
    ((1000, 400, 1900, 1300, 900, 300, 2000, 1400), (900, 300, 2000, 1400)),  # neither binds: extensions of 100 < 600
    ((500, 500, 900, 900, 100, 200, 1500, 1400), (500, 500, 900, 900)),       # qs == rs and qe == re: no extension at all
    ((400, 1000, 1300, 1900, 0, 0, 3000, 3000), (0, 400, 1900, 2500)),        # the mirror image: the query side binds
    ((0, 700, 2300, 3000, 0, 0, 3000, 3000), (0, 0, 3000, 3000)),             # values at 0 and at the sequence end (3000): rs - rs0 = 0, qe0 - qe = 0
    ((1000, 400, 1900, 1350, 100, 0, 2600, 1900), (400, 0, 2450, 1900)),      # the two ends have their own distance (600 left, 550 right)
    ((1000, 400, 1900, 1300, 400, 0, 2500, 1900), (400, 0, 2500, 1900)),      # exactly at the limit: unchanged
]


@pytest.mark.parametrize("case", CLAMP_CASES)
def test_self_clamp_table(named_lib, case):
    c = np.array(case[0], np.int32)
    named_lib.named_clamp(c.ctypes.data)
    assert tuple(int(v) for v in c[4:]) == case[1] and tuple(int(v) for v in c[:4]) == case[0][:4]


# ------------------------------------------------------------------ name ranks, lb, eq
def test_name_preparation(named_lib):
    W = T.overlap_world()
    names = [nm for nm, _ in W["targets"]]
    qn = [nm for nm, _ in W["queries"]] + [b"rd", b"rd0", b"rd1\x01", b"zzz", b"\xff", b"Rd", b"dup", b"duq", b"rd\xc3", b"rd\xc3\xa9\x01"]
    narr = (C.c_char_p * len(names))(*names)
    qarr = (C.c_char_p * len(qn))(*qn)
    rank = np.zeros(len(names), np.uint32); key = np.zeros(len(qn), np.uint64)
    named_lib.named_prepare(len(names), narr, rank.ctypes.data, len(qn), qarr, key.ctypes.data)
    distinct = sorted(set(names))                                         # bytes: unsigned order, a proper prefix first (strcmp)
    assert [int(r) for r in rank] == [distinct.index(nm) for nm in names]
    for q, k in zip(qn, key):
        k = int(k)
        if q is None:
            assert k == 0
            continue
        lb, eq, named = k & 0xffffffff, k >> 32 & 1, k >> 33 & 1
        assert named == 1 and lb == sum(1 for d in distinct if d < q) and eq == int(q in distinct), q
        for nm, r in zip(names, rank):                                    # the device's two integer tests are the string comparison
            assert (int(r) < lb) == (q > nm) and (bool(eq) and int(r) == lb) == (q == nm)


def test_filter_applies_rule(named_lib):
    """the named seed kernels run only for a batch with a named read, NO_DIAG or NO_DUAL set, on an index that kept its names"""
    f = named_lib.named_filter_applies
    ava = 0x800403 & ~4                                                   # ava-ont's flags, chain-only
    for idx_flag in (0, 1, 2, 3):                                         # HPC / NO_SEQ do not matter
        assert f(1, ava, idx_flag) == 1 and f(1, 1, idx_flag) == 1 and f(1, 2, idx_flag) == 1 and f(1, 3 | T.FOR_ONLY, idx_flag) == 1
        assert f(0, ava, idx_flag) == 0                                   # no named read
        assert f(1, ava & ~3, idx_flag) == 0 and f(1, T.NO_HASH_NAME | 4, idx_flag) == 0   # neither flag
    for idx_flag in (4, 5, 6, 7):                                         # MM_I_NO_NAME: inert, only the hash applies
        assert f(1, ava, idx_flag) == 0 and f(1, 3, idx_flag) == 0


# ------------------------------------------------------------------ Python surface that needs no GPU
def test_python_name_arguments(built):
    import inspect
    import mappy_rs
    sig = inspect.signature(mappy_rs.Aligner.map)
    assert list(sig.parameters)[:5] == ["self", "seq", "seq2", "cs", "MD"] and sig.parameters["name"].kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(mappy_rs.Aligner.__init__).parameters["name_key"].kind is inspect.Parameter.KEYWORD_ONLY
    al = mappy_rs.Aligner(T.dup_world()["fa"], preset="map-ont")
    with pytest.raises(ValueError):
        al.map("ACGT" * 50, name=b"bytes-name")
    from mappy_rs import _ffi
    assert _ffi.pack_names(None) is None and _ffi.pack_names([None, None]) is None
    arr = _ffi.pack_names(["ré", None])
    assert arr[0] == b"r\xc3\xa9" and arr[1] is None

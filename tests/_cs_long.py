"""Inputs and truth for the long form of cs (minimap2 --cs=long, MM355_OUT_CS_LONG), shared by tests/test_cs_long_host.py (the carry rule of
mm355_extra.h replayed on the CPU) and tests/test_gpu_cs_long.py (k_extra_long through its stage entry and the whole mapping path).

Truth is the oracle's write_cs_core, mmo_cs_core(..., no_iden = 0, ...); cs_long_ref is a plain restatement of it, and truth() returns a
string only after the two agreed on the input.

A region is (name, t_st, ops, q): the target is G[t_st:], ops is [(op, len)] with BAM operation numbers, q the query codes (0..4)."""
import ctypes as C

import numpy as np

from oracle import oracle as O

SEG_OPS, SEG_COLS = 64, 2048          # MM355_EXTRA_SEG / MM355_EXTRA_SEG_COLS: where k_extra cuts a region


def cs_long_ref(ops, q, t):
    """U:format.c::write_cs_core with no_iden == 0, restated"""
    out, qo, to = [], 0, 0
    for op, ln in ops:
        if op in (0, 7, 8):
            run = ""
            for a, b in zip(q[qo:qo + ln].tolist(), t[to:to + ln].tolist()):
                if a == b: run += "ACGTN"[a]
                else: out.append(("=" + run if run else "") + "*" + "acgtn"[b] + "acgtn"[a]); run = ""
            out.append("=" + run if run else "")
            qo += ln; to += ln
        elif op == 1: out.append("+" + "".join("acgtn"[c] for c in q[qo:qo + ln].tolist())); qo += ln
        elif op == 2: out.append("-" + "".join("acgtn"[c] for c in t[to:to + ln].tolist())); to += ln
        else: to += ln
    return "".join(out)


def oracle_cs(ops, q, t, no_iden):
    """mmo_cs_core on code arrays: no_iden 1 = short form, 0 = long form"""
    L = O.lib()
    cig = np.array([ln << 4 | op for op, ln in ops] + [0], np.uint32)
    qc = np.ascontiguousarray(np.concatenate([q, np.zeros(8, np.uint8)]), np.uint8)
    tc = np.ascontiguousarray(np.concatenate([t, np.zeros(8, np.uint8)]), np.uint8)
    p = L.mmo_cs_core(cig.ctypes.data, len(ops), qc.ctypes.data, tc.ctypes.data, int(no_iden), None, None)
    s = C.string_at(p).decode()
    L.free(p)
    return s


def truth(ops, q, t):
    """the long form of a region; the oracle and the restatement must agree before either is used"""
    want = oracle_cs(ops, q, t, 0)
    assert want == cs_long_ref(ops, q, t), (ops[:8], want[:120])
    return want


def t_len(ops):
    return sum(ln for op, ln in ops if op != 1)


def n_run(G):
    """(first, end) of the first run of code 4 in G"""
    at = np.flatnonzero(G == 4)
    assert at.size, "the genome needs an N run"
    end = int(at[0])
    while end < len(G) and G[end] == 4: end += 1
    return int(at[0]), end


def _place(rng, G, n, clean=True):
    for _ in range(1000):
        st = int(rng.integers(0, len(G) - n - 16))
        if not clean or not (G[st:st + n] == 4).any(): return st
    raise AssertionError("no stretch of %d bases without N" % n)


def build(rng, G, t_st, ops, rate=0.0, marks=None):
    """the query of a region on G[t_st:]: match operations copy the target (code 4 included: N against N is equal) and get mismatches at
    `rate`, or exactly at marks[k] (positions, "all" or "alt") for operation k; 7 copies, 8 differs everywhere; insertions are random bases"""
    q, to = [], 0
    for k, (op, ln) in enumerate(ops):
        if op in (0, 7, 8):
            seg = G[t_st + to:t_st + to + ln].copy()
            assert len(seg) == ln
            mk = (marks or {}).get(k, "all" if op == 8 else None)
            mm = np.zeros(ln, bool)
            if mk is None: mm = rng.random(ln) < (rate if op == 0 else 0.0)
            elif isinstance(mk, str): mm[(0 if mk == "all" else 1)::(1 if mk == "all" else 2)] = True
            else: mm[list(mk)] = True
            seg[mm] = np.where(seg[mm] > 3, rng.integers(0, 4, int(mm.sum())), (seg[mm] + rng.integers(1, 4, int(mm.sum()))) % 4)
            q.append(seg); to += ln
        elif op == 1: q.append(rng.integers(0, 4, ln).astype(np.uint8))
        else: to += ln
    return np.concatenate(q).astype(np.uint8) if q else np.zeros(0, np.uint8)


def _mixed_ops(rng, n, first=None):
    ops = []
    for k in range(n):
        last = ops[-1][0] if ops else -1
        op = 0 if (k % 2 == 0 and last != 0) else int(rng.choice([1, 2]))
        if op == last: op = 0
        if k == 0 and first is not None: op = first
        ops.append((op, int(rng.integers(1, 40)) if op == 0 else int(rng.choice([1, 1, 2, 3, 10]))))
    return ops


ALL_MATCH = (255, 256, 2047, 2048, 2049, 2304, 4096, 4097, 12000)
N_OPS = (1, 63, 64, 65, 129)


def census(rng, G, eqx=True):
    """the smallest regions that reach each case of the carry rule (the names are what the tests count)"""
    out = []

    def add(name, ops, rate=0.0, marks=None, t_st=None, edit=None):
        st = _place(rng, G, t_len(ops) + 8) if t_st is None else t_st
        q = build(rng, G, st, ops, rate, marks)
        if edit is not None: edit(q)
        out.append((name, st, ops, q))

    add("empty", [])
    for n in N_OPS: add("ops_%d" % n, _mixed_ops(rng, n), rate=0.1)
    add("begins_I", [(1, 3), (0, 30), (2, 2), (0, 20)], marks={3: [4]})                 # the first match operation is one run: bytes before the first flush, lead > 0
    add("begins_D", [(2, 3), (0, 30), (1, 2), (0, 20)], marks={3: [0, 19]})
    add("begins_I_then_cut", [(1, 5), (0, 2500), (0, 4)])                               # the first segment never flushes and has gap text in front of its bases
    add("ends_gap", [(0, 30), (1, 4)], rate=0.1)
    add("ends_gap_D", [(0, 3000), (2, 7)])
    for n in ALL_MATCH: add("all_match_%d" % n, [(0, n)])
    add("all_match_inside", [(0, 7), (1, 2), (0, 4097), (2, 3), (0, 9)], marks={0: [3]})
    add("mm_last_before_cut", [(0, 5000)], marks={0: [SEG_COLS - 1]})                  # the run ends at the cut: the next segment's lead gets its own '='
    add("mm_first_behind_cut", [(0, 5000)], marks={0: [SEG_COLS]})                     # the next segment's lead is 0, the carry is printed by nobody
    add("mm_both_sides_of_cut", [(0, 5000)], marks={0: [SEG_COLS - 1, SEG_COLS, 2 * SEG_COLS - 1, 2 * SEG_COLS]})
    add("cut_all_mismatch", [(0, 5000)], marks={0: "all"})
    add("slot_worst_case", [(0, SEG_COLS)], marks={0: "alt"})                           # alternating match / mismatch over one segment
    n0, n1 = n_run(G)
    assert n0 >= 60 and n1 - n0 >= 8
    add("N_both", [(0, 60 + (n1 - n0) + 30)], t_st=n0 - 60)                             # code 4 against code 4: 'N' inside a run
    add("N_target_only", [(0, 60 + (n1 - n0) + 30)], t_st=n0 - 60, marks={0: range(60, 60 + n1 - n0)})
    add("N_query_only", [(0, 90), (1, 3), (0, 40)], edit=lambda q: q.__setitem__([5, 6, 40, 91, 100], 4))
    if eqx:
        add("eqx_adjacent", [(7, 5), (7, 3), (8, 2), (7, 4), (1, 2), (8, 1), (7, 2600), (7, 1), (8, 3)])
    return out


def random_regions(rng, G, n):
    """regions as tests/test_gpu_map.py::test_update_extra_and_cs_on_device draws them: many short operations, and HiFi-like ones with match
    operations longer than a segment"""
    out = []
    for i in range(n):
        hifi = i % 4 == 3
        n_ops = int(rng.integers(1, 12)) if hifi else int(rng.integers(1, 300))
        ops = _mixed_ops(rng, n_ops, first=int(rng.choice([1, 2])) if i % 7 == 3 else None)
        if hifi: ops = [(op, int(rng.choice([500, 1792, 2048, 2049, 2304, 4096, 7000])) if op == 0 else ln) for op, ln in ops]
        st = _place(rng, G, t_len(ops) + 8, clean=i % 3 != 0)
        q = build(rng, G, st, ops, rate=(0.0 if i % 8 == 3 else 0.002) if hifi else 0.08)
        if i % 6 == 2: q[rng.random(len(q)) < 0.05] = 4
        out.append(("random_%d" % i, st, ops, q))
    return out

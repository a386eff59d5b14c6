"""A plain model of where the seed stage's inputs go: the flat table's geometry (which lines fill, which lookups walk on, which cross from
the last line to line 0) and a census of mm_seed_select on a read (the streaks of high-occurrence hits and the branch each one takes).

Plain Python over the oracle (orc.sketch, orc.anchors(...)[3] for the minimizers after mm_seed_mz_flt, mmo_idx_get for the counts); the
product is not imported.  Its use: tests/test_seed_edges_host.py asserts, on the CPU, that the inputs of tests/test_gpu_seed_edges.py reach
the branches they are there for, so that the GPU tests cannot quietly stop reaching them.

Table geometry.  A key's home line is mm_table_hash(minimizer) & (n_lines - 1); an insert takes the first empty slot of the home line or of the
lines after it, the last line followed by line 0.  How many slots of each line end up taken does not depend on the order of the inserts
(the usual property of linear probing: a line's final load is min(8, keys homed there + keys carried in), and what is carried on is the
rest), which is what makes the model valid for the concurrent inserts of the device builders.  WHICH key sits where does depend on the
order, so per present key only `the home line is full` is known; the statements that hold for every order are about sets: of the keys homed
in the run of full lines that ends at the last line, exactly `carry into line 0` sit beyond the wrap.  For the host builder, which inserts
in ascending key order, place() gives every key's line exactly.

mm_seed_select census: seed.c::mm_seed_select restated (the heap included, so that the restatement can be checked against the oracle's
n_mini and rep_len), with every streak classified."""
import ctypes as C

import numpy as np

if __name__ == "__main__":      # run as a script (the census of the older inputs, at the end): the repository root is not on the path yet
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import oracle as O

M64 = (1 << 64) - 1
SLOTS = 8                      # MM355_SLOTS_PER_LINE
MAX_MAX_HIGH_OCC = 128
MZ_STAGE = 2048                # k_mzflt's LDS stage (reads with more minimizers sort through HBM)
CS_BUCKETS = 8192              # k_mzflt's count sketch
TILE = 64                      # hits per mask word of k_seed_select
SEL_MASK_HITS = 1024 * TILE    # SEL_MASK_TILES tiles are kept in LDS; hits from here on have their mask recomputed


# ------------------------------------------------------------------ table geometry
def table_hash(m):
    h = (m * 0x9E3779B97F4A7C15) & M64
    return h ^ (h >> 29)


def n_lines_for(n_keys):
    want = int(n_keys / 0.55) + SLOTS
    n = 1
    while n * SLOTS < want:
        n <<= 1
    return n


class Table:
    """the final load of every line of the table that holds `keys` (distinct minimizer values, already >> 8)"""

    def __init__(self, keys):
        self.keys = sorted(set(int(k) for k in keys))
        self.n_lines = n_lines_for(len(self.keys))
        self.mask = self.n_lines - 1
        home = [0] * self.n_lines
        for k in self.keys:
            home[table_hash(k) & self.mask] += 1
        self.home = home
        load, carry_in = [0] * self.n_lines, [0] * self.n_lines
        carry = 0
        while True:                                   # round the table until nothing changes (twice: a line that is not full carries nothing on)
            changed = False
            for i in range(self.n_lines):
                if carry_in[i] != carry:
                    carry_in[i] = carry; changed = True
                tot = home[i] + carry
                load[i] = min(SLOTS, tot)
                carry = tot - load[i]
            if not changed:
                break
        self.load, self.carry_in = load, carry_in
        self.wrap_carry = carry_in[0]                 # entries homed before the end of the table that sit in line 0 or after it
        self.present = set(self.keys)

    @property
    def load_factor(self):
        return len(self.keys) / float(self.n_lines * SLOTS)

    def full(self, line):
        return self.load[line & self.mask] == SLOTS

    def home_line(self, key):
        return table_hash(key) & self.mask

    def absent_probe(self, key):
        """(line fetches, crosses the wrap) of the lookup of a key that is not in the table: exact -- it walks the full lines from its home
        line and stops at the first line with an empty slot"""
        line, n, wrap = self.home_line(key), 1, False
        while self.full(line):
            wrap |= line == self.mask
            line = (line + 1) & self.mask
            n += 1
        return n, wrap

    def wrap_cluster(self):
        """the lines of the run of full lines that ends at the last line (empty list: the last line is not full)"""
        out, line = [], self.mask
        while self.full(line) and len(out) < self.n_lines:
            out.append(line); line -= 1
        return out[::-1]

    def must_cross(self, looked_up):
        """how many of the present keys in `looked_up` sit beyond the wrap whatever the insertion order was: the keys homed in the wrap
        cluster overflow it by wrap_carry (nothing is carried into the cluster's first line: the line before it is not full); those not
        looked up may be the ones that stayed"""
        lines = set(self.wrap_cluster())
        if not lines or self.wrap_carry == 0:
            return 0
        homed = [k for k in self.keys if self.home_line(k) in lines]
        assert len(homed) - SLOTS * len(lines) == self.wrap_carry
        lk = set(int(k) for k in looked_up)
        return max(0, self.wrap_carry - sum(1 for k in homed if k not in lk))

    def place(self, order=None):
        """key -> (line fetches of its lookup, crosses the wrap) when the keys are inserted in `order` (default ascending: the host builder)"""
        used = [0] * self.n_lines
        out = {}
        for k in (self.keys if order is None else order):
            line, n, wrap = self.home_line(k), 1, False
            while used[line] == SLOTS:
                wrap |= line == self.mask
                line = (line + 1) & self.mask
                n += 1
            used[line] += 1
            out[k] = (n, wrap)
        assert used == self.load                      # the order-free model and the literal fill agree
        return out


def genome_keys(orc, seqs):
    """the distinct minimizer values of the indexed sequences"""
    out = set()
    for rid, s in enumerate(seqs):
        mz = orc.sketch(s, rid)
        out.update((mz[:, 0] >> np.uint64(8)).tolist())
    return out


def idx_get(orc, minier):
    """mmo_idx_get: the position list of a minimizer value (empty: absent)"""
    n = C.c_int()
    p = O.lib().mmo_idx_get(orc.idx, int(minier), C.byref(n))
    return [p[i] for i in range(n.value)]


def idx_count(orc, minier, _n=C.c_int()):
    O.lib().mmo_idx_get(orc.idx, int(minier), C.byref(_n))
    return _n.value


def lookup_census(tab, looked_up):
    """what the lookups of the minimizer values `looked_up` meet in table `tab`"""
    lk = set(int(k) for k in looked_up)
    absent = [k for k in lk if k not in tab.present]
    probes = {k: tab.absent_probe(k) for k in absent}
    return dict(n_present=len(lk) - len(absent), n_absent=len(absent),
                present_must_cross=tab.must_cross(lk),
                present_home_full=sum(1 for k in lk if k in tab.present and tab.full(tab.home_line(k))),
                absent_in_full_last_line=[k for k in absent if tab.home_line(k) == tab.mask and tab.full(tab.mask)],
                absent_in_full_line=[k for k in absent if probes[k][0] >= 2],
                absent_cross=[k for k in absent if probes[k][1]],
                absent_3_fetches=[k for k in absent if probes[k][0] >= 3])


# ------------------------------------------------------------------ mm_seed_select
def _heapdown(i, n, l):
    k, tmp = i, l[i]
    while True:
        k = (k << 1) + 1
        if k >= n:
            break
        if k != n - 1 and l[k] < l[k + 1]:
            k += 1
        if l[k] < tmp:
            break
        l[i] = l[k]; i = k
    l[i] = tmp


def hit_list(orc, seq):
    """(counts, q_pos words, spans, minimizer values of the hits; n_mz after the filter, n_mz before it, minimizers after the filter)"""
    raw = orc.sketch(seq)
    mz = orc.anchors(seq, sorted_=False)[3]
    cnt, qp, sp, keys = [], [], [], []
    for x, y in mz.tolist():
        c = idx_count(orc, x >> 8)
        if c:
            cnt.append(c); qp.append(y & 0xffffffff); sp.append(x & 0xff); keys.append(x >> 8)
    return cnt, qp, sp, keys, len(mz), len(raw), mz


def count_sketch_max(mz):
    """the fullest bucket of k_mzflt's count sketch over the minimizer words of a read (the kernel skips the exact sort when it is <= mid_occ).
    This restates an implementation detail: whether the kernel went on to the sort cannot be seen from outside."""
    if len(mz) == 0:
        return 0
    b = np.array([(table_hash(int(x)) >> 20) & (CS_BUCKETS - 1) for x in mz[:, 0].tolist()])
    return int(np.bincount(b, minlength=CS_BUCKETS).max())


def select_census(orc, seq, mo=None):
    """the census of one read under MapOpt `mo` (default: the oracle's own).  Returns a dict: n_m0, streaks (list of dicts), flt / cnt / keys (per hit),
    n_mini, rep_len (what collect_matches would report -- compare with orc.anchors), and the minimizer figures."""
    mo = orc.mo if mo is None else mo
    cnt, qp, sp, keys, n_mz, n_raw, mz = hit_list(orc, seq)
    n, qlen = len(cnt), len(seq)
    mid, mmo, dist = mo.mid_occ, mo.max_max_occ, mo.occ_dist
    flt = [0] * n
    streaks = []
    selected = dist > 0 and mmo > mid
    if not selected:
        flt = [1 if c > mid else 0 for c in cnt]
    # the streaks are listed in either case (the `else` form filters them whole)
    i = 0
    while i < n:
        if cnt[i] <= mid:
            i += 1; continue
        st = i
        while i < n and cnt[i] > mid:
            i += 1
        en = i
        ps = 0 if st == 0 else qp[st - 1] >> 1
        pe = qlen if en == n else qp[en] >> 1
        L = en - st
        s = dict(st=st, en=en, L=L, ps=ps, pe=pe, at_start=st == 0, at_end=en == n, straddles_tile=st // TILE != (en - 1) // TILE,
                 past_mask=st >= SEL_MASK_HITS, across_mask=st < SEL_MASK_HITS < en, above_max_max=sum(1 for c in cnt[st:en] if c > mmo),
                 clamped=False, tie=False, cls="else", k=0)
        if selected and n >= 2:
            mho = int(float(pe - ps) / dist + .499)
            if mho > MAX_MAX_HIGH_OCC:
                mho = MAX_MAX_HIGH_OCC; s["clamped"] = True
            if mho > 0:
                k = min(mho, L)
                b = [cnt[j] << 32 | j for j in range(st, st + k)]
                for h in range((k >> 1) - 1, -1, -1):
                    _heapdown(h, k, b)
                for j in range(st + k, en):
                    if cnt[j] < b[0] >> 32:
                        b[0] = cnt[j] << 32 | j
                        _heapdown(0, k, b)
                for x in b:
                    flt[x & 0xffffffff] = 1
                s["k"] = k
                if L > k:
                    srt = sorted(cnt[st:en])
                    s["tie"] = srt[k - 1] == srt[k]
            for j in range(st, en):
                flt[j] ^= 1
            for j in range(st, en):
                if cnt[j] > mmo:
                    flt[j] = 1
            s["cls"] = "none" if mho <= 0 else "all" if L <= mho else "heap"
        elif selected:
            s["cls"] = "single"                      # n_m0 < 2: mm_seed_select returns at once, nothing is filtered
        streaks.append(s)
    rep_st = rep_en = rep_len = 0
    n_mini = 0
    for j in range(n):
        if flt[j]:
            en_ = (qp[j] >> 1) + 1; st_ = en_ - sp[j]
            if st_ > rep_en:
                rep_len += rep_en - rep_st; rep_st, rep_en = st_, en_
            else:
                rep_en = en_
        else:
            n_mini += 1
    rep_len += rep_en - rep_st
    return dict(n_m0=n, streaks=streaks, flt=flt, cnt=cnt, keys=keys, n_mini=n_mini, rep_len=rep_len, n_mz=n_mz, n_mz_raw=n_raw,
                mz_filtered=n_raw - n_mz, cs_max=count_sketch_max(orc.sketch(seq)), mid_occ=mid)


def summary(censuses):
    """the figures the tests assert, summed over the censuses of several reads"""
    S = [s for c in censuses for s in c["streaks"]]
    cls = lambda name: [s for s in S if s["cls"] == name]
    return dict(streaks=len(S), none=len(cls("none")), all=len(cls("all")), heap=len(cls("heap")), else_=len(cls("else")),
                clamp=sum(1 for s in S if s["clamped"] and s["L"] > MAX_MAX_HIGH_OCC and s["cls"] == "heap"),
                at_start=sum(1 for s in S if s["at_start"]), at_end=sum(1 for s in S if s["at_end"]),
                heap_straddles=sum(1 for s in cls("heap") if s["straddles_tile"]), heap_tie=sum(1 for s in cls("heap") if s["tie"]),
                all_cut=sum(1 for s in cls("all") if s["above_max_max"]), heap_cut=sum(1 for s in cls("heap") if s["above_max_max"]),
                above_max_max=sum(s["above_max_max"] for s in S),
                across_mask=sum(1 for s in S if s["across_mask"]), past_mask=sum(1 for s in S if s["past_mask"]),
                most_hits=max([c["n_m0"] for c in censuses] or [0]))


# ------------------------------------------------------------------ the census of the inputs the suite had before the seed-edge tests
def _old_inputs():
    """(label, FASTA contigs, names, reads) of four older tests, rebuilt from their seeds (tests/test_gpu_stages.py: world, _repeat_world;
    tests/test_gpu_map.py: test_map_parity_ultra_long_reads, the low-complexity reads of test_map_parity_adversarial_inputs)"""
    import synthdata as S
    comp = lambda c: np.where(c < 4, 3 - c, 4).astype(np.uint8)[::-1]
    g = S.make_genome(31, [400000, 250000], repeats=((4000, 6, 0.01), (900, 40, 0.02), (300, 120, 0.05)), n_runs=3)
    reads, _ = S.make_reads(32, g, 160, n50=5000, lo=200)
    rng = np.random.default_rng(7)
    unit = S.codes_to_str(g[0][1000:1037])
    reads += ["ACGT", "A", reads[0][:14], reads[1][:600] + "NNNNNNNNNN" + reads[1][600:1500], unit * 60,
              S.codes_to_str(S.random_codes(rng, 3000)), S.codes_to_str(g[1][5000:5400]), "N" * 50]
    yield "test_gpu_stages.py::world", g, ["chrA", "chrB"], reads
    rng = np.random.default_rng(77)
    g = S.random_codes(rng, 700000)
    unit = S.random_codes(rng, 1000)
    for _ in range(150):
        pos = int(rng.integers(0, len(g) - 1000))
        g[pos:pos + 1000] = S.mutate(unit, rng, 0.01, 0.0, 0.0)[:1000]
    reads = [S.codes_to_str(S.mutate(np.tile(unit, m), rng, 0.02, 0.01, 0.01)) for m in (2, 5, 9)]
    reads += [S.codes_to_str(g[5000:9000]), S.codes_to_str(S.mutate(np.tile(unit, 3)[::-1].copy(), rng, 0.02, 0.0, 0.0))]
    yield "test_gpu_stages.py::_repeat_world", [g], ["chrR"], reads
    g = S.make_genome(91, [1500000], repeats=((6000, 5, 0.01), (1500, 15, 0.02)), n_runs=2)
    rng = np.random.default_rng(92)
    reads = []
    for L in (150000, 300000, 650000, 1000000):
        a0 = int(rng.integers(0, 1500000 - L))
        reads.append(S.codes_to_str(S.mutate(g[0][a0:a0 + L], rng, 0.024, 0.016, 0.02)))
    c = np.concatenate([g[0][100000:260000], comp(g[0][700000:830000]), g[0][262000:400000]])
    reads.append(S.codes_to_str(S.mutate(c, rng, 0.03, 0.02, 0.02)))
    yield "test_gpu_map.py::test_map_parity_ultra_long_reads", g, ["chrU"], reads
    rng = np.random.default_rng(7)
    low = [S.random_codes(rng, 20000), np.zeros(30000, np.uint8), np.tile(np.array([0, 1], np.uint8), 10000),
           np.tile(np.array([0, 1, 2, 3, 3, 1, 0], np.uint8), 4000), S.random_codes(rng, 20000)]
    g = [np.concatenate(low), S.random_codes(rng, 200000)]
    lc = [S.codes_to_str(S.mutate(g[0][a:a + L], rng, 0.02, 0.01, 0.01))
          for a, L in ((15000, 12000), (19000, 25000), (45000, 15000), (55000, 20000), (60000, 30000), (70000, 40000), (0, 118000))]
    lc += ["A" * 50000, "AC" * 12000, "ACGTTCA" * 3000]
    yield "test_gpu_map.py::test_map_parity_adversarial_inputs (low-complexity reads)", g, ["lc", "rnd"], lc


if __name__ == "__main__":      # python tests/_seed_census.py: the table in the docstring of tests/test_seed_edges_host.py
    import synthdata as S
    print("| input | reads | mid_occ | table lines | load | carry into line 0 | streaks | none | all | heap | clamp | above max_max_occ | reads mz_flt filters | most hits |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for label, g, names, reads in _old_inputs():
        seqs = [S.codes_to_str(c) for c in g]
        orc = O.OracleAligner(seqs=seqs, names=names, preset="map-ont")
        tab = Table(genome_keys(orc, seqs))
        cs = [select_census(orc, rd) for rd in reads]
        s = summary(cs)
        print("| %s | %d | %d | %d | %.2f | %d | %d | %d | %d | %d | %d | %d | %d | %d |" % (
            label, len(reads), orc.mo.mid_occ, tab.n_lines, tab.load_factor, tab.wrap_carry, s["streaks"], s["none"], s["all"], s["heap"],
            s["clamp"], s["above_max_max"], sum(1 for c in cs if c["mz_filtered"]), s["most_hits"]), flush=True)

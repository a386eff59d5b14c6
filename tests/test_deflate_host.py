"""The deflate stage of the BAM writer on the host (mappy-rs_amd/csrc/mm355_deflate.h: the functions the kernel's lanes call, run serially),
built with g++ under AddressSanitizer and UBSan into a stand-alone program (tests/host_harness/deflate_host.cpp).  The oracle is Python's zlib
and gzip: every block inflates to its payload, carries the right CRC-32, ISIZE and BSIZE and is no longer than its stored form; random bytes
come out as the stored block of _bam.frame, level 0 is _bam.frame; the same input gives the same bytes; a bound from the optimal Huffman
code where that is at most 15 deep; a repeated string must show that matches are found.  GPU side: tests/test_gpu_deflate.py."""
import heapq
import os
import subprocess

import numpy as np
import pytest

import _bam
import _capi
import _deflate as D

P = D.P


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("deflate_host") / "deflate_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-w", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           os.path.join(_capi.HERE, "host_harness", "deflate_host.cpp"), "-o", exe, "-lz", "-lpthread"])
    return exe


def _run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout.splitlines()


@pytest.fixture(scope="module")
def coded(harness, tmp_path_factory):
    """name -> (the level-1 blocks, stored blocks as the program counted them), every payload coded once"""
    d = tmp_path_factory.mktemp("coded")
    out = {}
    for name, data in D.payloads().items():
        src, dst = d / "in.bin", d / "out.bgzf"
        src.write_bytes(data)
        line, = _run(harness, "wrap", 1, src, dst)
        got = dst.read_bytes()
        f = line.split()
        assert (int(f[1]), int(f[5])) == ((len(data) + P - 1) // P, len(got)), name
        out[name] = got, int(f[3])
    return out


def test_every_block_inflates_to_its_payload(coded):
    for name, data in D.payloads().items():
        got, n_stored = coded[name]
        stored = D.check(got, data)
        assert sum(stored) == n_stored, name
        print(name, len(data), len(got), n_stored)


def test_random_bytes_are_stored_and_level_0_is_frame(harness, coded, tmp_path):
    pl = D.payloads()
    for name, data in pl.items():
        if name.startswith("random_") or name == "equal_shuffled":
            assert coded[name][0] == _bam.frame(data), name
    # below the minimum match nothing can be shorter than stored: 1 .. 4 bytes of anything
    for name in ("zeros_1", "zeros_2", "zeros_3", "zeros_4", "text_4"):
        assert coded[name][0] == _bam.frame(pl[name]), name
    for name in ("random_0", "random_1", "zeros_%d" % P, "text_%d" % (P + 1), "records"):
        src, dst = tmp_path / "in.bin", tmp_path / "out.bgzf"
        src.write_bytes(pl[name])
        _run(harness, "wrap", 0, src, dst)
        assert dst.read_bytes() == _bam.frame(pl[name]), name


def test_same_input_same_bytes(harness, coded, tmp_path):
    pl = D.payloads()
    for name in ("records", "text_%d" % (3 * P + 77), "fibonacci", "period_32768"):
        src, dst = tmp_path / "in.bin", tmp_path / "again.bgzf"
        src.write_bytes(pl[name])
        _run(harness, "wrap", 1, src, dst)
        assert dst.read_bytes() == coded[name][0], name


def test_no_more_than_the_optimal_huffman_code_and_a_header(coded):
    """for a payload whose optimal unlimited Huffman code (end-of-block counted once) is at most 15 deep, the deflate stream may not exceed that
    code's cost plus 1880 bits of header plus 7 bits of padding: matches can only lower the size.  The length limit acts on the Fibonacci
    payloads, whose trees are or may be deeper, so the bound is not claimed there"""
    pl = D.payloads()
    n_checked = 0
    for name in ("equal_in_order", "equal_shuffled", "zeros_1", "zeros_4", "zeros_257", "zeros_%d" % P, "ff_%d" % P, "ff_259", "zeros_%d" % (P - 1)):
        bits, depth = D.huffman(pl[name])
        assert depth <= 15, name
        blk, = D.blocks(coded[name][0])
        assert (len(blk) - 26) * 8 <= bits + D.HEADER_BITS + 7, (name, len(blk), bits)
        n_checked += 1
    assert n_checked == 9
    # the length limit: every Huffman tree of fibonacci_deep is 21 deep (tests/_deflate.py), so its code was cut at 15 bits, and zlib read the
    # block in test_every_block_inflates_to_its_payload.  A code of k bits for the k-th most frequent value, cut at 15, costs 2.6 bits per
    # byte of either payload: under half the stored size
    assert D.huffman(pl["fibonacci_deep"])[1] == 21
    for name in ("fibonacci", "fibonacci_deep"):
        blk, = D.blocks(coded[name][0])
        assert len(blk) < len(pl[name]) // 2, (name, len(blk))


def test_matches_are_found(coded):
    pl = D.payloads()
    assert len(coded["repeat_1000"][0]) < len(pl["repeat_1000"]) // 4          # a literals-only coder cannot do that
    # a distance of 32768 is legal and used; 32769 is not: that payload has no match and is stored
    assert len(coded["period_32768"][0]) < P * 3 // 4
    assert coded["period_32769"][0] == _bam.frame(pl["period_32769"])
    assert len(coded["records"][0]) < len(pl["records"])


def _optimal_bits(counts):
    heap = [c for c in counts if c]
    heapq.heapify(heap)
    bits = 0
    while len(heap) > 1:
        m = heapq.heappop(heap) + heapq.heappop(heap)
        bits += m
        heapq.heappush(heap, m)
    return bits


def test_codes_are_optimal_complete_and_limited(harness):
    """dfl_make_code: the cost of an optimal Huffman code where the limit does not act (any optimal tree of these counts is under the limit:
    the largest count is below twice the smallest, or the counts are few); complete and prefix-free always; at most max_bits when the
    unlimited tree is a chain (the strict Fibonacci row: 23 deep at 24 symbols) and for the code-length code's 7 bits; ties by symbol number:
    equal counts give canonical codes in symbol order"""
    rng = np.random.default_rng(44)
    cases = [(15, [int(x) for x in rng.integers(100, 200, 286)]), (15, [0, 5, 0, 0, 9, 1] + [0] * 20 + [7, 7]), (15, [3, 1]), (7, [int(x) for x in rng.integers(50, 99, 19)]),
             (15, [0] * 7 + [4]), (15, [2] * 8)]
    fib = [1, 1]
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    limited = [(15, fib), (15, fib[::-1]), (7, fib[:19]), (7, [1, 0, 1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024])]
    for k, (max_bits, counts) in enumerate(cases + limited):
        lines = [tuple(map(int, ln.split())) for ln in _run(harness, "code", max_bits, *counts)]
        lens = [l for l, _ in lines]
        used = [s for s, c in enumerate(counts) if c]
        assert [s for s, l in enumerate(lens) if l] == used and max(lens) <= max_bits, k
        if len(used) == 1:
            assert lines[used[0]] == (1, 0)
            continue
        assert sum(2 ** (max_bits - lens[s]) for s in used) == 2 ** max_bits, k                # complete
        words = sorted(format(c, "0%db" % l)[::-1] for l, c in (lines[s] for s in used))      # as the stream carries them: first bit first
        assert all(not b.startswith(a) for a, b in zip(words, words[1:])), k                   # prefix-free
        # canonical: by (length, symbol) the codes count up
        by_len = sorted(used, key=lambda s: (lens[s], s))
        assert [format(lines[s][1], "0%db" % lens[s])[::-1] for s in by_len] == sorted(words, key=lambda w: (len(w), w)), k
        cost = sum(counts[s] * lens[s] for s in used)
        if k < len(cases):
            assert cost == _optimal_bits(counts), k
        else:
            assert cost > _optimal_bits(counts) and all(lens[a] >= lens[b] for a in used for b in used if counts[a] < counts[b]), k
    assert [l for l, _ in (tuple(map(int, ln.split())) for ln in _run(harness, "code", 15, *([2] * 8)))] == [3] * 8


def test_symbols_of_lengths_and_distances(harness):
    """the closed forms of dfl_len_sym and dfl_dist_sym against the tables of RFC 1951 3.2.5"""
    lines = [tuple(map(int, ln.split())) for ln in _run(harness, "syms")]
    assert len(lines) == 256 + 32768
    len_base = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
    len_extra = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
    dist_base = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
    dist_extra = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
    for l, (sym, eb, ev) in zip(range(3, 259), lines[:256]):
        k = sym - 257
        assert 0 <= k < 29 and eb == len_extra[k] and len_base[k] + ev == l and ev < 1 << eb, l
        assert l != 258 or sym == 285
    for d, (sym, eb, ev) in zip(range(1, 32769), lines[256:]):
        assert 0 <= sym < 30 and eb == dist_extra[sym] and dist_base[sym] + ev == d and ev < 1 << eb, d


def test_library_host_path_equals_the_program(built, coded):
    """mappy_rs.bgzf_wrap: compress=False is the stored framing, compress=True the bytes of the stand-alone coder (no GPU is touched)"""
    import mappy_rs
    pl = D.payloads()
    for name in ("random_0", "zeros_4", "text_259", "text_%d" % (3 * P + 77), "records", "random_%d" % (P + 1)):
        assert mappy_rs.bgzf_wrap(pl[name], compress=True) == coded[name][0], name
        assert mappy_rs.bgzf_wrap(pl[name], compress=False) == mappy_rs.bgzf_wrap(pl[name]) == _bam.frame(pl[name]), name

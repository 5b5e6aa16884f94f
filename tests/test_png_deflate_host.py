"""The deflate of the PNG encode without a GPU (include/dspn_png_encode.h, "The device deflate"): the host encoder
dspn_png_deflate_host, which runs the rule text the device kernels run, over the case list of tests/png_deflate_cases.py --
zlib inflates every stream to its input and checks the Adler-32, the sizes stay within the declared bound and near zlib's own
Z_RLE stream, noise blocks come out stored and all others dynamic; the length-limited code lengths alone against a heapq
Huffman; the argument checks of the device entry point (they return before any HIP call, so stand-in pointers do) and the
pure size queries."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytest.importorskip("PIL.Image")
import png_deflate_cases as pc  # noqa: E402

from dspnet_amd import _lib  # noqa: E402
from dspnet_amd.dataset import png_encode as pe  # noqa: E402

CASES = pc.cases()
NAMES = [n for n, _ in CASES]
# Size against zlib's own stream for the same strategy, zlib.compressobj(6, DEFLATED, 15, 8, Z_RLE), over this case list with
# the finished host encoder (deterministic; DESIGN.md has the table).  The worst ratio is WORST_RATIO, at length_285: 23
# bytes against 12, because zlib writes a stream that short with the fixed codes and this rule has none.  The bound adds 0.01
# for zlib builds that differ between machines and 16 bytes for streams of a few dozen bytes.  That ratio comes from streams
# the 16 bytes already cover, so a second, tighter bound holds beside it: with the 16 bytes taken off first the worst ratio
# is WORST_RATIO_BEYOND_SLACK, at all_zeros (113 bytes against 86: three blocks with a header each against zlib's one);
# the other streams of a block or more stay below 1.03 when they are label-like and at 1.00 when they are photo-like.
WORST_RATIO = 1.9167
WORST_RATIO_BEYOND_SLACK = 1.1279
SIZE_SLACK_BYTES = 16


@pytest.fixture(scope="module")
def streams():
    return {n: pe.deflate_host(d) for n, d in CASES}


def test_case_list_covers_what_it_names():
    assert len(set(NAMES)) == len(NAMES)
    sizes = {len(d) for _, d in CASES}
    assert {1, 2, pc.BLOCK - 1, pc.BLOCK, pc.BLOCK + 1} <= sizes and any(s > 3 * pc.BLOCK and s % pc.BLOCK for s in sizes)
    assert sum(n.startswith("png_") for n in NAMES) == len(pc.ref_png_encode.cases())
    d = dict(CASES)
    for over in (1, 2, 3, 300):
        run = d["run_over_edge_%d" % over]
        assert run[pc.BLOCK - 500:pc.BLOCK + over] == b"\x07" * (500 + over) and run[pc.BLOCK - 501] != 7 and run[pc.BLOCK + over] != 7
    assert sorted(set(d["all_256_values"])) == list(range(256))


@pytest.mark.parametrize("name", NAMES)
def test_stream_inflates_to_its_input_within_the_bound(name, streams):
    data, z = dict(CASES)[name], streams[name]
    assert z[:2] == b"\x78\x01"
    assert pc.inflate_strictly(z) == data
    assert len(z) <= pe.deflate_bound(len(data))


def test_block_types(streams):
    for name, data in CASES:
        types = pc.block_types(streams[name], len(data))
        assert len(types) == -(-len(data) // pc.BLOCK), name
        stored = {i for i, t in enumerate(types) if t == 0}
        if name in pc.STORED:
            assert stored == pc.STORED[name], name
        elif not name.startswith("png_") and not name.startswith("run_over_edge"):
            assert stored == set(), name


@pytest.mark.parametrize("name", ["runs_1_to_7", "runs_257_to_263", "runs_two_pieces_and_more", "length_285", "all_256_values_skewed",
                                  "fibonacci", "block_exact"])
def test_tokens_follow_the_rule(name, streams):
    """the decoded literal and match sequence of one-block streams against a restatement of the token rule"""
    data, tokens = dict(CASES)[name], []
    assert pc.block_types(streams[name], len(data), tokens) == [2]
    assert tokens == pc.rule_tokens(data)
    if name == "length_285":
        assert tokens == [1, 9, ("match", 258), 2]
    if name == "runs_1_to_7":                                   # runs of 1, 2, 3 stay literals; 4 is a literal and a match of 3
        assert [t for t in tokens if isinstance(t, tuple)] == [("match", 3), ("match", 4), ("match", 5), ("match", 6)]
    if name == "all_256_values_skewed":
        assert not any(isinstance(t, tuple) for t in tokens)


def test_sizes_against_zlib_rle(streams):
    worst, at = 0.0, None
    for name, data in CASES:
        mine, theirs = len(streams[name]), len(pc.zlib_rle(data))
        print("size %-28s %8d %8d %8d %.4f" % (name, len(data), mine, theirs, mine / theirs))
        if mine / theirs > worst:
            worst, at = mine / theirs, name
    print("worst ratio %.4f at %s" % (worst, at))
    tight = max(((len(streams[n]) - SIZE_SLACK_BYTES) / len(pc.zlib_rle(d)), n) for n, d in CASES)
    print("worst ratio with %d bytes taken off %.4f at %s" % ((SIZE_SLACK_BYTES,) + tight))
    for name, data in CASES:
        assert len(streams[name]) <= (WORST_RATIO + 0.01) * len(pc.zlib_rle(data)) + SIZE_SLACK_BYTES, name
        assert len(streams[name]) <= (WORST_RATIO_BEYOND_SLACK + 0.01) * len(pc.zlib_rle(data)) + SIZE_SLACK_BYTES, name


def code_lengths(counts, limit):
    counts = np.ascontiguousarray(counts, np.uint32)
    lengths = np.zeros(len(counts), np.uint8)
    _lib.check(_lib.lib().dspn_png_deflate_code_lengths(counts.ctypes.data, len(counts), limit, lengths.ctypes.data), "code_lengths")
    return lengths.tolist()


def count_sets(n, limit):
    g = np.random.Generator(np.random.PCG64(n * 100 + limit))
    yield "two", [0] * (n - 2) + [5, 9]
    yield "all_equal", [3] * n
    yield "all_ones", [1] * n
    for k in range(8):
        c = g.integers(0, [2, 10, 1000, 40000][k % 4], n)
        c[g.integers(0, n)] += 1
        yield "uniform%d" % k, c.tolist()
    for k in range(6):                                          # steep: geometric counts reach the limiter
        c = (g.random(n) ** (8 + 4 * k) * 3e6).astype(np.int64)
        c[g.integers(0, n)] += 1
        yield "steep%d" % k, c.tolist()
    fib = [1, 1]
    while len(fib) < min(n, 40):
        fib.append(fib[-1] + fib[-2])
    yield "fibonacci", fib + [0] * (n - len(fib))
    yield "fibonacci_reversed", [0] * (n - len(fib)) + fib[::-1]
    yield "fibonacci_block", [pc.FIB[v] if v < len(pc.FIB) else 0 for v in range(n)]


@pytest.mark.parametrize("n,limit", [(286, 15), (19, 7)])
def test_code_lengths(n, limit):
    reached = 0
    for name, counts in count_sets(n, limit):
        lengths = code_lengths(counts, limit)
        used = [s for s in range(n) if counts[s]]
        assert all((lengths[s] == 0) == (counts[s] == 0) for s in range(n)), name
        assert all(1 <= lengths[s] <= limit for s in used), name
        kraft = sum(1 << (limit - lengths[s]) for s in used)
        assert kraft == 1 << limit, name                        # a complete prefix code, exactly
        cost = sum(counts[s] * lengths[s] for s in used)
        free = pc.huffman_lengths(counts)
        if max(free.values()) <= limit:
            assert cost == pc.huffman_cost(counts), name
        else:
            reached += 1
            assert cost > pc.huffman_cost(counts), name
        assert code_lengths(counts, limit) == lengths           # deterministic
    assert reached >= 3                                         # the limiter was at work
    one = [0] * n
    one[n // 2] = 7
    assert code_lengths(one, limit) == [1 if s == n // 2 else 0 for s in range(n)]
    assert code_lengths([0] * n, limit) == [0] * n


def test_code_lengths_refusals():
    lib = _lib.lib()
    c, l = np.ones(300, np.uint32), np.zeros(300, np.uint8)
    for args in ((None, 19, 7, l.ctypes.data), (c.ctypes.data, 19, 7, None), (c.ctypes.data, 0, 7, l.ctypes.data),
                 (c.ctypes.data, 287, 15, l.ctypes.data), (c.ctypes.data, 19, 0, l.ctypes.data), (c.ctypes.data, 19, 16, l.ctypes.data),
                 (c.ctypes.data, 19, 4, l.ctypes.data)):          # 19 symbols do not fit 4 bits
        assert lib.dspn_png_deflate_code_lengths(*args) == -1, args
    big = np.full(4, 0x7FFFFFFF, np.uint32)
    assert lib.dspn_png_deflate_code_lengths(big.ctypes.data, 4, 7, l.ctypes.data) == -1
    assert b"2^32" in lib.dspn_last_error()


def test_argument_validation_without_gpu():
    lib = _lib.lib()
    p = ctypes.c_void_p(256)                # never dereferenced: every call below fails its checks first

    def call(n=1, offsets=(0,), sizes=(1000,), src=p, in_bytes=1000, out=p, out_bytes=1013, result=p, ws=p, ws_bytes=1 << 20, tables=True):
        o, s = np.ascontiguousarray(offsets, np.int64), np.ascontiguousarray(sizes, np.int64)
        rc = lib.dspn_png_deflate_batch(o.ctypes.data if tables else None, s.ctypes.data if tables else None, n, src, in_bytes, out,
                                        out_bytes, result, ws, ws_bytes, None)
        return rc, lib.dspn_last_error()

    assert call(n=-1) == (-1, b"png_deflate: negative count (n -1)")
    assert call(n=0)[0] == 0                                                    # a no-op, before anything is looked at
    for kw in (dict(src=None), dict(out=None), dict(ws=None), dict(result=None), dict(tables=False)):
        rc, text = call(**kw)
        assert rc == -1 and b"null argument" in text, kw
    for kw in (dict(in_bytes=0), dict(out_bytes=0), dict(in_bytes=-5)):
        rc, text = call(**kw)
        assert rc == -1 and b"empty pool" in text, kw
    for size in (0, -1):
        rc, text = call(sizes=(size,))
        assert rc == -1 and b"a stream of %d bytes" % size in text
    for kw in (dict(in_bytes=999), dict(offsets=(1,)), dict(offsets=(-1,)), dict(offsets=(1 << 62,)), dict(sizes=(1 << 62,))):
        rc, text = call(**kw)
        assert rc == -1 and b"run past in_bytes" in text, kw
    rc, text = call(out_bytes=1012)
    assert rc == -1 and b"out_bytes 1012 below the sum of the bounds 1013" in text
    need = lib.dspn_png_deflate_workspace_bytes(1, 1000)
    rc, text = call(ws_bytes=need - 1)
    assert rc == -2 and b"workspace of %d bytes, %d needed" % (need - 1, need) in text
    for kw in (dict(ws=ctypes.c_void_p(260)), dict(result=ctypes.c_void_p(260))):
        rc, text = call(**kw)
        assert rc == -1 and b"8-byte aligned" in text
    # the second stream of a table is checked like the first; the bounds add up
    rc, text = call(n=2, offsets=(0, 500), sizes=(500, 501))
    assert rc == -1 and b"image 1: 501 bytes from offset 500 run past in_bytes 1000" in text
    rc, text = call(n=2, offsets=(0, 500), sizes=(500, 500), out_bytes=2 * 513 - 1)
    assert rc == -1 and b"below the sum of the bounds 1026" in text
    # the host encoder's own checks
    buf, length = np.zeros(64, np.uint8), ctypes.c_longlong(0)
    assert lib.dspn_png_deflate_host(buf.ctypes.data, 0, buf.ctypes.data, 64, ctypes.addressof(length)) == -1
    assert lib.dspn_png_deflate_host(buf.ctypes.data, 10, buf.ctypes.data, 22, ctypes.addressof(length)) == -1
    assert b"below the bound 23" in lib.dspn_last_error()
    assert lib.dspn_png_deflate_host(None, 10, buf.ctypes.data, 64, ctypes.addressof(length)) == -1
    with pytest.raises(_lib.DspnError, match="0 bytes"):
        pe.deflate_host(b"")


def test_size_queries():
    lib = _lib.lib()
    B = pc.BLOCK
    assert [pe.deflate_bound(n) for n in (1, B, B + 1, 3 * B, 3 * B + 1)] == [14, B + 13, B + 20, 3 * B + 25, 3 * B + 32]
    assert pe.deflate_bound(0) == 0 and pe.deflate_bound(-4) == 0
    assert pe.deflate_bound(1 << 40) == (1 << 40) + 6 * (1 << 25) + 7
    assert lib.dspn_png_deflate_workspace_bytes(0, 10) == 0 and lib.dspn_png_deflate_workspace_bytes(-1, 10) == 0
    assert lib.dspn_png_deflate_workspace_bytes(3, 2) == 0                      # fewer bytes than streams
    # the table (3 n + 1), per image size, checksum and start (3 n + 1), per block a 920-byte plan and an offset
    for n, total in ((1, 1), (1, B), (2, 5 * B + 3), (32, 32 * 1024 * 2049)):
        blocks = total // B + n
        assert lib.dspn_png_deflate_workspace_bytes(n, total) == 8 * (6 * n + 2) + 928 * blocks

"""The byte streams the tests of the PNG encoder's deflate share (include/dspn_png_encode.h, "The device deflate"): block
edges, run-length edges, both limiters and the stored fallback, seeded; plus the filtered streams of every case of
tests/ref_png_encode.py, taken from Pillow's files.  Also the plain helpers both test files use: an unlimited Huffman by heapq,
zlib's own Z_RLE stream as the size yardstick, and a walk over the block headers of a stream."""
import heapq
import zlib

import numpy as np

import ref_png_encode

BLOCK = 32768                     # DSPN_PNG_DEFLATE_BLOCK
# 18 Fibonacci numbers from 1, 2: with the end-of-block symbol's single count in front they are 1, 1, 2, 3, ..., one chain
FIB = [1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597, 2584, 4181]


def huffman_lengths(counts):
    """unlimited Huffman code lengths {symbol: length} of the non-zero counts (one used symbol: length 1)"""
    used = [(c, s) for s, c in enumerate(counts) if c]
    if len(used) == 1:
        return {used[0][1]: 1}
    heap = [(c, s, (s,)) for c, s in used]
    heapq.heapify(heap)
    depth = dict.fromkeys((s for _, s in used), 0)
    tick = len(counts)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for s in a[2] + b[2]:
            depth[s] += 1
        heapq.heappush(heap, (a[0] + b[0], tick, a[2] + b[2]))
        tick += 1
    return depth


def huffman_cost(counts):
    depth = huffman_lengths(counts)
    return sum(counts[s] * d for s, d in depth.items())


def no_adjacent_equal(counts):
    """a byte string in which value v occurs counts[v] times and no two neighbours are equal (the most frequent value takes
    every other place first)"""
    values = [v for v, c in sorted(enumerate(counts), key=lambda vc: -vc[1]) for _ in range(c)]
    n = len(values)
    out = [0] * n
    for place, v in zip(list(range(0, n, 2)) + list(range(1, n, 2)), values):
        out[place] = v
    assert all(a != b for a, b in zip(out, out[1:]))
    return bytes(out)


def fibonacci_block():
    data = no_adjacent_equal(FIB)
    counts = [0] * 286
    for v in data:
        counts[v] += 1
    counts[256] = 1               # end of block
    assert max(huffman_lengths(counts).values()) > 15          # the unlimited code does not fit: the limiter is reached
    return data


def runs(lengths, first=1):
    """runs of the given lengths, neighbours with different values"""
    return b"".join(bytes([(first + 7 * i) % 251 + 1]) * r for i, r in enumerate(lengths))


def cases():
    """[(name, bytes)]"""
    g = np.random.Generator(np.random.PCG64(77))

    def noise(n):
        return g.integers(0, 256, n, dtype=np.uint8).tobytes()

    def label(n):
        """long runs of a few values, as a filtered label map has them"""
        return np.repeat(g.integers(0, 34, n // 40 + 2, dtype=np.uint8), g.integers(1, 120, n // 40 + 2))[:n].tobytes()

    out = [("one_byte", b"\x05"), ("two_equal", b"\x05\x05"), ("two_different", b"\x05\x06"),
           ("block_minus_1", label(BLOCK - 1)), ("block_exact", label(BLOCK)), ("block_plus_1", label(BLOCK + 1)),
           ("three_blocks_and_tail", label(3 * BLOCK + 777)),
           ("runs_1_to_7", runs(range(1, 8))), ("runs_257_to_263", runs(range(257, 264))),
           ("runs_two_pieces_and_more", runs([2 * 258 + 1 + k for k in range(4)]))]
    for over in (1, 2, 3, 300):                                 # a run that crosses a block edge by `over` bytes
        out.append(("run_over_edge_%d" % over, noise(BLOCK - 500)[:BLOCK - 500 - 1] + b"\xfe" + b"\x07" * (500 + over) + noise(40)))
    out.append(("all_zeros", bytes(2 * BLOCK + 300)))
    out.append(("all_256_values", bytes(range(256))))           # HLIT = 257 and no match
    out.append(("all_256_values_skewed", bytes(range(256)) + bytes([1, 2] * 600)))     # ... in a block that stays dynamic
    out.append(("length_285", b"\x01" + b"\x09" * 259 + b"\x02"))
    out.append(("noise_block", noise(BLOCK)))
    out.append(("noise_odd", noise(BLOCK + 4097)))
    out.append(("zeros_noise_zeros", bytes(BLOCK) + noise(BLOCK) + bytes(BLOCK)))       # a stored block in mid-stream
    out.append(("fibonacci", fibonacci_block()))
    out.append(("fibonacci_then_label", fibonacci_block() + label(BLOCK)))
    for name, a in ref_png_encode.cases():
        out.append(("png_" + name, ref_png_encode.pillow_filtered(a)))
    return out


# the blocks that must come out stored, by case (index of the block in the stream): the noise blocks, and the streams whose
# dynamic header alone (17 bits and the code lengths) is longer than they are (the one-byte block of block_plus_1 too); 256 different bytes gain nothing either
STORED = {"noise_block": {0}, "noise_odd": {0, 1}, "zeros_noise_zeros": {1}, "one_byte": {0}, "two_equal": {0},
          "two_different": {0}, "all_256_values": {0}, "block_plus_1": {1}}


def zlib_rle(data):
    """zlib's own stream for the same strategy: the size yardstick"""
    z = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    return z.compress(data) + z.flush()


def inflate_strictly(stream):
    """the inflated bytes; the stream must end exactly at its last byte (zlib checks the Adler-32 itself)"""
    d = zlib.decompressobj()
    data = d.decompress(stream)
    assert d.eof and d.unused_data == b"" and d.unconsumed_tail == b""
    return data


def _bits(stream, pos, n):
    """n <= 24 bits of the stream from bit position pos, the first one lowest"""
    return (int.from_bytes(stream[pos >> 3:(pos >> 3) + 4], "little") >> (pos & 7)) & ((1 << n) - 1)


def block_types(stream, nbytes, tokens=None):
    """BTYPE of every block of a zlib stream of this encoder over nbytes input bytes, from a walk over the block headers: a
    stored block is skipped by its LEN, a dynamic one by reading its symbols up to the end-of-block symbol.  tokens: a list
    that receives a dynamic block's tokens, a byte value for a literal, ("match", length) for a match"""
    pos, types, done = 16, [], 0
    while True:
        final, btype = _bits(stream, pos, 1), _bits(stream, pos + 1, 2)
        size = min(BLOCK, nbytes - done)
        types.append(btype)
        if btype == 0:
            at = (pos + 3 + 7) // 8 * 8
            length = _bits(stream, at, 16)
            assert length == size and _bits(stream, at + 16, 16) == length ^ 0xFFFF
            pos = at + 32 + 8 * length
        else:
            assert btype == 2
            pos = _dynamic_end(stream, pos, tokens)
        done += size
        if final:
            assert done == nbytes and (pos + 7) // 8 + 4 == len(stream)
            return types


_CLEN_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
_LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]


def rule_tokens(data):
    """the tokens the rule of include/dspn_png_encode.h gives a block, restated: per maximal run a literal, then pieces of 258
    while 3 or more bytes remain, then the remaining 1 or 2 bytes as literals"""
    out, i = [], 0
    while i < len(data):
        r = 1
        while i + r < len(data) and data[i + r] == data[i]:
            r += 1
        out.append(data[i])
        left = r - 1
        while left >= 3:
            out.append(("match", min(258, left)))
            left -= min(258, left)
        out += [data[i]] * left
        i += r
    return out


def _decoder(lengths):
    """{(length, code read bit by bit, first bit highest): symbol} of a canonical code"""
    table, code = {}, 0
    for n in range(1, 16):
        for s, l in enumerate(lengths):
            if l == n:
                table[(n, code)] = s
                code += 1
        code <<= 1
    return table


def _dynamic_end(stream, pos, tokens=None):
    """the bit position behind the dynamic block whose header starts at pos (distance 1 only, HDIST = 0)"""
    def take(n):
        nonlocal pos
        v = _bits(stream, pos, n)
        pos += n
        return v

    def symbol(table):
        code = n = 0
        while True:
            code, n = code << 1 | take(1), n + 1
            if (n, code) in table:
                return table[(n, code)]
            assert n < 15

    take(3)
    hlit, hdist, hclen = take(5) + 257, take(5) + 1, take(4) + 4
    assert hdist == 1
    cl = [0] * 19
    for i in range(hclen):
        cl[_CLEN_ORDER[i]] = take(3)
    table, lengths = _decoder(cl), []
    while len(lengths) < hlit + hdist:
        s = symbol(table)
        if s < 16:
            lengths.append(s)
        elif s == 16:
            lengths += [lengths[-1]] * (3 + take(2))
        else:
            lengths += [0] * ((3 + take(3)) if s == 17 else (11 + take(7)))
    assert len(lengths) == hlit + 1 and lengths[hlit] == 1
    table = _decoder(lengths[:hlit])
    while True:
        s = symbol(table)
        if s == 256:
            return pos
        if s > 256:
            extra = take(_LEN_EXTRA[s - 257])
            assert take(1) == 0                                 # the distance code's one symbol
        if tokens is not None:
            tokens.append(s if s < 256 else ("match", _LEN_BASE[s - 257] + extra))

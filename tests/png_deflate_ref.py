"""What a compressed PNG of the library must be, checked from the format alone
with struct, zlib and numpy (the library is not used): the chunks and their
CRCs, a zlib stream that inflates to H rows of 3W + 1 bytes, on every row the
filter type with the least sum of min(b, 256 - b) over its filtered bytes (ties
to the lowest type, bpp 3, zeros above row 0), the pixels PIL reads back, and
the size against zlib's Z_RLE strategy over the same filtered bytes.

With `blocks=True` the checker also looks inside every block, from RFC 1951
alone (a bit reader of its own: `read_block`, `parse_segments`): the file's
block structure is the one rt_png_deflate.hpp's header comment states, every
dynamic segment carries exactly the `deflate_rle` tokens of its rows
(`tokens`), and its two codes cost what a minimum-redundancy code costs
(`huffman_cost_and_depth`), so that the file is one fixed file per canvas up
to the order of equal-cost codes, which "host == device" holds.
"""
import functools
import heapq
import struct
import zlib

import numpy as np

import png_ref

SEGMENT = 16384  # RT_PNG_DEFLATE_SEGMENT


def rows_per_segment(w):
    return max(1, SEGMENT // (3 * w + 1))


def n_segments(w, h):
    return -(-h // rows_per_segment(w))


def stored_len(n):
    return n + 5 * (-(-n // png_ref.STORED))


def bound(w, h):
    """Every segment in stored blocks: 63 bytes around them."""
    rps, row = rows_per_segment(w), 3 * w + 1
    full, rest = divmod(h, rps)
    return 63 + full * stored_len(rps * row) + (stored_len(rest * row) if rest else 0)


def chunks(png):
    """[(type, payload)] of a file whose signature and chunk CRCs hold."""
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
    out, at = [], 8
    while at < len(png):
        n, = struct.unpack(">I", png[at:at + 4])
        kind, payload = png[at + 4:at + 8], png[at + 8:at + 8 + n]
        assert len(payload) == n, "a chunk runs past the file"
        crc, = struct.unpack(">I", png[at + 8 + n:at + 12 + n])
        assert crc == zlib.crc32(kind + payload), f"CRC of {kind!r}"
        out.append((kind, payload))
        at += 12 + n
    assert at == len(png)
    return out


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filtered_image(px):
    """(types, F): the filter type of every row by the minimum-sum rule, and the H x (3W + 1) filtered bytes."""
    h, w = px.shape[0], px.shape[1]
    x = px.reshape(h, 3 * w).astype(np.int64)
    a = np.concatenate([np.zeros((h, 3), np.int64), x[:, :-3]], axis=1)
    b = np.concatenate([np.zeros((1, 3 * w), np.int64), x[:-1]], axis=0)
    c = np.concatenate([np.zeros((h, 3), np.int64), b[:, :-3]], axis=1)
    cand = np.stack([x, x - a, x - b, x - (a + b) // 2, x - _paeth(a, b, c)]) & 0xFF  # (5, H, 3W)
    cost = np.minimum(cand, 256 - cand).sum(axis=2)  # (5, H)
    types = np.argmin(cost, axis=0)  # (the first least one: ties to the lowest type)
    rows = cand[types, np.arange(h)]
    return types, np.concatenate([types[:, None], rows], axis=1).astype(np.uint8)


def check_file(png, px, size_against_rle=False, bound_of=bound, blocks=False, sample=None):
    """`png` holds `px` in this format; returns (IDAT payload length, the filtered bytes), and with
    `blocks` (check_blocks: every block's structure, tokens and codes) the segments as well."""
    png = bytes(png)
    h, w = px.shape[0], px.shape[1]
    parts = chunks(png)
    assert [k for k, _ in parts] == [b"IHDR", b"IDAT", b"IEND"]
    assert parts[0][1] == struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0) and parts[2][1] == b""
    idat = parts[1][1]
    F = zlib.decompress(idat)  # (rejects a bad code, a bad stored length, a wrong Adler-32)
    assert len(F) == h * (3 * w + 1)
    types, want = filtered_image(px)
    got = np.frombuffer(F, np.uint8).reshape(h, 3 * w + 1)
    assert np.array_equal(got[:, 0], types), "filter types"
    assert np.array_equal(got, want), "filtered rows"
    mode, size, pixels = png_ref.decoded(png)
    assert mode == "RGB" and size == (w, h)
    assert np.array_equal(pixels, px)
    assert len(png) <= bound_of(w, h)
    if size_against_rle:
        co = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
        z = len(co.compress(F) + co.flush())
        print(f"{w}x{h}: IDAT {len(idat)}, Z_RLE {z}, blocks {n_segments(w, h)}, file {len(png)}, bound {bound_of(w, h)}")
        assert len(idat) <= z + 64 * n_segments(w, h)
    if blocks:
        return len(idat), F, check_blocks(idat, F, w, h, sample)
    return len(idat), F


def longest_run(F):
    """The longest run of one byte value in F."""
    a = np.frombuffer(bytes(F), np.uint8)
    cuts = np.flatnonzero(np.diff(a) != 0) + 1
    return int(np.diff(np.concatenate([[0], cuts, [a.size]])).max())


# ---- inside the blocks (RFC 1951). A token is a literal's byte value or a match's (length, distance).
_LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
             227, 258)
_LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
_DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
              4097, 6145, 8193, 12289, 16385, 24577)
_DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)  # 3.2.7
_FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8  # 3.2.6
_FIXED_DIST = [5] * 30


def length_symbol(length):
    """The length symbol of a match of `length` bytes and the number of its extra bits."""
    s = max(i for i in range(29) if _LEN_BASE[i] <= length)  # (258 has a symbol of its own, the last)
    assert 3 <= length <= 258 and length - _LEN_BASE[s] < 1 << _LEN_EXTRA[s]
    return 257 + s, _LEN_EXTRA[s]


def tokens(F):
    """The deflate_rle tokens of the bytes F: every maximal run of one value on its own; a run
    of at most 3 bytes is literals; a longer one is a literal, then matches at distance 1 of 258
    bytes while at least 3 bytes are left, one shorter match of what is left if that is at
    least 3 bytes, else 1-2 literals."""
    a = np.frombuffer(bytes(F), np.uint8)
    if a.size == 0:
        return []
    cuts = np.concatenate([[0], np.flatnonzero(np.diff(a) != 0) + 1, [a.size]])
    out = []
    for byte, run in zip(a[cuts[:-1]].tolist(), np.diff(cuts).tolist()):
        if run <= 3:
            out.extend([byte] * run)
            continue
        out.append(byte)
        left = run - 1
        while left >= 3:
            m = min(left, 258)
            out.append((m, 1))
            left -= m
        out.extend([byte] * left)
    return out


def expand(toks):
    """The bytes a token list stands for."""
    out = bytearray()
    for t in toks:
        if isinstance(t, tuple):
            length, dist = t
            assert 0 < dist <= len(out), "a match that reaches before the data"
            for _ in range(length):
                out.append(out[-dist])
        else:
            out.append(t)
    return bytes(out)


def huffman_cost_and_depth(counts):
    """(Σ count·length, the deepest length) of a Huffman code without a length limit for the
    symbols with a non-zero count. Every minimum-redundancy code has this cost; among them the
    one built here (ties to the shallower subtree) is the least deep. A lone symbol takes one bit."""
    heap = [(c, 0) for c in counts if c]
    if len(heap) == 1:
        return heap[0][0], 1
    heapq.heapify(heap)
    cost = 0
    while len(heap) > 1:
        a, da = heapq.heappop(heap)
        b, db = heapq.heappop(heap)
        cost += a + b
        heapq.heappush(heap, (a + b, max(da, db) + 1))
    return cost, heap[0][1]


class Bits:
    """A deflate stream's bits, least significant first (3.1.1)."""

    def __init__(self, data, pos=0):
        self.data, self.pos = bytes(data), pos

    def take(self, n):
        v, data, pos = 0, self.data, self.pos
        for i in range(n):
            v |= ((data[(pos + i) >> 3] >> ((pos + i) & 7)) & 1) << i
        self.pos = pos + n
        return v


def _decoder(lengths):
    """A canonical code from its lengths (3.2.2): per length the first code, the number of codes
    and where its symbols start in `syms` (symbol order within a length)."""
    n = max(lengths) if len(lengths) else 0
    count = [0] * (n + 2)
    for l in lengths:
        count[l] += 1
    count[0] = 0
    assert sum(c << (n - l) for l, c in enumerate(count[:n + 1]) if l) <= 1 << n, "an over-subscribed code"
    first, offset, code, at = [0] * (n + 2), [0] * (n + 2), 0, 0
    for l in range(1, n + 1):
        code = (code + count[l - 1]) << 1
        first[l], offset[l] = code, at
        at += count[l]
    syms = sorted((s for s, l in enumerate(lengths) if l), key=lambda s: (lengths[s], s))
    return n, first, count, offset, syms


def _decode(b, dec):
    n, first, count, offset, syms = dec
    data, pos, code = b.data, b.pos, 0
    for l in range(1, n + 1):
        code = code << 1 | ((data[pos >> 3] >> (pos & 7)) & 1)  # (Huffman codes go most significant bit first)
        pos += 1
        k = code - first[l]
        if 0 <= k < count[l]:
            b.pos = pos
            return syms[offset[l] + k]
    raise AssertionError("bits that are no code")


def read_block(b):
    """One deflate block of any kind at b.pos (3.2.3-3.2.7), as a dict:
    final, type, bits (its first bit and the bit after it) and
      stored   pad (the bits skipped to the byte boundary), raw
      fixed    tokens
      dynamic  hlit, hdist, hclen, cl_lens (by symbol, 19), sent (the code-length symbols as sent),
               ll_lens, dist_lens, tokens, token_bits (literal/length code bits, end-of-block included)."""
    start = b.pos
    out = {"final": b.take(1), "type": b.take(2)}
    if out["type"] == 0:
        out["pad"] = b.take(-b.pos % 8)
        n, nn = b.take(16), b.take(16)
        assert n ^ nn == 0xFFFF, "a stored block's LEN and NLEN"
        at = b.pos >> 3
        assert at + n <= len(b.data), "a stored block runs past the stream"
        out["raw"] = b.data[at:at + n]
        b.pos += 8 * n
    else:
        assert out["type"] != 3, "block type 11"
        if out["type"] == 1:
            ll_lens, dist_lens = _FIXED_LL, _FIXED_DIST
        else:
            out["hlit"], out["hdist"], out["hclen"] = b.take(5) + 257, b.take(5) + 1, b.take(4) + 4
            cl = [0] * 19
            for i in range(out["hclen"]):
                cl[CL_ORDER[i]] = b.take(3)
            cl_dec, sent, lens = _decoder(cl), [], []
            while len(lens) < out["hlit"] + out["hdist"]:
                s = _decode(b, cl_dec)
                sent.append(s)
                if s < 16:
                    lens.append(s)
                elif s == 16:
                    assert lens, "a repeat with nothing before it"
                    lens.extend([lens[-1]] * (3 + b.take(2)))
                else:
                    lens.extend([0] * (3 + b.take(3) if s == 17 else 11 + b.take(7)))
            assert len(lens) == out["hlit"] + out["hdist"], "code lengths run past HLIT + HDIST"
            ll_lens, dist_lens = lens[:out["hlit"]], lens[out["hlit"]:]
            assert ll_lens[256], "no code for end-of-block"
            out.update(cl_lens=cl, sent=sent, ll_lens=ll_lens, dist_lens=dist_lens)
        ll_dec, dist_dec = _decoder(ll_lens), _decoder(dist_lens)
        toks, code_bits = [], 0
        while True:
            s = _decode(b, ll_dec)
            code_bits += ll_lens[s]
            if s == 256:
                break
            if s < 256:
                toks.append(s)
                continue
            assert s < 286, "length symbols 286 and 287"
            length = _LEN_BASE[s - 257] + b.take(_LEN_EXTRA[s - 257])
            d = _decode(b, dist_dec)
            assert d < 30, "distance symbols 30 and 31"
            toks.append((length, _DIST_BASE[d] + b.take(_DIST_EXTRA[d])))
        out.update(tokens=toks, token_bits=code_bits)
    out["bits"] = (start, b.pos)
    return out


def inflate_tokens(deflate):
    """The tokens of a raw deflate stream of any valid shape (stored bytes count as literals)."""
    b, toks = Bits(deflate), []
    while True:
        blk = read_block(b)
        toks.extend(blk["raw"] if blk["type"] == 0 else blk["tokens"])
        if blk["final"]:
            return toks


def parse_segments(idat, w, h):
    """The segments of a compressed PNG's zlib payload, walked along the file's own blocks, as
    rt_png_deflate.hpp's header comment lays them out. Every segment starts on a byte boundary,
    holds rows_per_segment(w) whole rows, and is either
      dynamic  one block, not final, then an empty stored block (zero padding, 00 00 FF FF); or
      stored   blocks of 65535 bytes and a last, shorter or equal, non-empty one.
    BFINAL sits on the last block of the last segment alone; the Adler-32 follows it. A segment is
    read_block's dict of its first block with: kind, bytes (its file bytes: start, end), raw, and
    for a stored segment blocks (each block's length)."""
    idat = bytes(idat)
    assert idat[:2] == b"\x78\x01"
    b, row, rps, segs = Bits(idat, 16), 3 * w + 1, rows_per_segment(w), []
    n_seg = n_segments(w, h)
    for k in range(n_seg):
        n, last = (min(h, (k + 1) * rps) - k * rps) * row, k == n_seg - 1
        assert b.pos % 8 == 0
        start = b.pos >> 3
        seg = read_block(b)
        if seg["type"] == 2:
            seg["kind"] = "dynamic"
            assert seg["final"] == 0, "BFINAL on a dynamic block"
            seg["raw"] = expand(seg["tokens"])
            close = read_block(b)
            assert close["type"] == 0 and close["pad"] == 0 and close["raw"] == b"", "the closing empty stored block"
            assert close["final"] == (1 if last else 0), "BFINAL on the closing block of the last segment alone"
        else:
            assert seg["type"] == 0, "a fixed-Huffman block"
            seg["kind"] = "stored"
            parts, blk, left = [], seg, n
            while True:
                assert blk["type"] == 0 and blk["pad"] == 0
                assert len(blk["raw"]) == min(png_ref.STORED, left), "stored blocks of <= 65535 bytes"
                parts.append(blk["raw"])
                left -= len(blk["raw"])
                assert blk["final"] == (1 if last and left == 0 else 0), "BFINAL on the file's last block alone"
                if left == 0:
                    break
                blk = read_block(b)
            seg["blocks"] = [len(p) for p in parts]
            seg["raw"] = b"".join(parts)
        assert len(seg["raw"]) == n, f"segment {k} holds {len(seg['raw'])} bytes of {n}"
        seg["bytes"] = (start, b.pos >> 3)
        segs.append(seg)
    assert b.pos % 8 == 0 and (b.pos >> 3) + 4 == len(idat), "the Adler-32 ends the stream"
    return segs


def _code_is_least(what, counts, lens, limit):
    """`lens` is a complete code of at most `limit` bits for the symbols with a count, none for the
    others, and costs what a minimum-redundancy code costs: exactly, when one fits the limit; with
    a deeper unlimited code, not less, and then the limit is reached."""
    assert sum(1 for c in counts if c) >= 2  # (a literal and end-of-block; a length in use and the zeros)
    for s, (c, l) in enumerate(zip(counts, lens)):
        assert l <= limit, f"{what}: symbol {s} has {l} bits"
        assert (l > 0) == (c > 0), f"{what}: symbol {s}, count {c}, {l} bits"
    assert sum(1 << (limit - l) for l in lens if l) == 1 << limit, f"{what}: the code is not complete"
    cost = sum(c * l for c, l in zip(counts, lens))
    least, depth = huffman_cost_and_depth(counts)
    if depth <= limit:
        assert cost == least, f"{what}: {cost} bits, a minimum-redundancy code takes {least}"
    else:
        assert cost >= least and max(lens) == limit, f"{what}: {cost} bits of at most {max(lens)} against {least}"
    return depth


def check_segment(seg, F_seg):
    """A dynamic segment (parse_segments) of the filtered bytes F_seg is the one the format fixes,
    up to the order of codes of equal cost. Returns the depths of the unlimited codes: (literal/
    length, code-length)."""
    assert seg["kind"] == "dynamic"
    want = tokens(F_seg)
    assert seg["tokens"] == want, "the tokens are not deflate_rle's"
    assert seg["raw"] == bytes(F_seg)
    matches = [t for t in want if isinstance(t, tuple)]
    assert seg["hdist"] == 1, "HDIST"
    assert seg["dist_lens"] == [1 if matches else 0], "one distance code of one bit exactly when something matches"
    assert all(s < 16 for s in seg["sent"]), "a run code (16-18) in the header"
    ll, cl = seg["ll_lens"], seg["cl_lens"]
    assert seg["hlit"] == max([257] + [s + 1 for s in range(257, len(ll)) if ll[s]]), "HLIT is not the least"
    assert seg["hclen"] == max([4] + [i + 1 for i in range(19) if cl[CL_ORDER[i]]]), "HCLEN is not the least"
    counts = [0] * 286
    for t in want:
        counts[length_symbol(t[0])[0] if isinstance(t, tuple) else t] += 1
    counts[256] = 1
    ll_depth = _code_is_least("literal/length code", counts, ll + [0] * (286 - len(ll)), 15)
    assert seg["token_bits"] == sum(c * l for c, l in zip(counts, ll))
    cl_counts = [0] * 19
    for s in seg["sent"]:
        cl_counts[s] += 1
    cl_depth = _code_is_least("code-length code", cl_counts, cl, 7)
    return ll_depth, cl_depth


def check_blocks(idat, F, w, h, sample=None):
    """parse_segments, with check_segment on every dynamic segment (on those in `sample` alone, if
    given); every segment's bytes are F's. Returns the segments."""
    segs, at = parse_segments(idat, w, h), 0
    for k, seg in enumerate(segs):
        F_seg = F[at:at + len(seg["raw"])]
        at += len(F_seg)
        assert seg["raw"] == F_seg, f"segment {k}"
        if seg["kind"] == "dynamic" and (sample is None or k in sample):
            check_segment(seg, F_seg)
    assert at == len(F)
    return segs


def _row(first, w):  # one row: `first` components of 1.0, then zeros (filter None wins: see the tests)
    c = np.zeros((1, w, 3))
    c.reshape(-1)[:first] = 1.0
    return c


def _byte_row(hex_bytes):  # one row of these component bytes
    row = np.frombuffer(bytes.fromhex(hex_bytes), np.uint8)
    return (row / 255.0).reshape(1, row.size // 3, 3)


def _counted_row(counts):
    """One row whose 3W bytes hold the k-th of the values 0, 255, 1, 254, ... counts[k] times
    (`counts` descending). The values are small under min(b, 256 - b) and jump about, so the filter
    None wins; the filter byte is one more 0. The bytes in descending count order fill the even
    positions and then the odd ones, so that no value stands three times in a row: nothing matches."""
    assert list(counts) == sorted(counts, reverse=True) and sum(counts) % 3 == 0 and len(counts) <= 256
    values = [k // 2 if k % 2 == 0 else 255 - k // 2 for k in range(len(counts))]
    seq = np.repeat(np.array(values, np.uint8), counts)
    row, half = np.empty(seq.size, np.uint8), (seq.size + 1) // 2
    row[0::2], row[1::2] = seq[:half], seq[half:]
    return (row / 255.0).reshape(1, seq.size // 3, 3)


def _lit_limit_row(n):
    """n byte values with the counts 1, 2, 3, 5, 8, ... and end-of-block's 1 before them: a
    minimum-redundancy code is a chain n deep. (The filter byte adds one to the largest count.)"""
    fib = [1, 2]
    while len(fib) < n:
        fib.append(fib[-1] + fib[-2])
    return _counted_row(fib[::-1])


CL_LIMIT_LENGTHS = {3: 1, 4: 3, 5: 1, 6: 34, 7: 5, 8: 8, 9: 21, 10: 13, 11: 2}  # length -> symbols


def _cl_limit_row():
    """Literal counts that are powers of two, 2^(11 - length), for CL_LIMIT_LENGTHS' symbols per
    length (end-of-block is one of the two at 11 bits, the filter byte one of the 256 zeros): the
    sums are 2048 tokens, so the literal/length lengths are forced, and the header sends each
    length CL_LIMIT_LENGTHS[length] times beside 170 zeros, which wants a code 9 deep."""
    counts = [1 << (11 - l) for l, k in sorted(CL_LIMIT_LENGTHS.items()) for _ in range(k)][:-1]
    counts[0] -= 1
    return _counted_row(counts)


def _spans(rng, n, lo, hi):
    """Lengths between lo and hi (the last one shorter) that add up to n."""
    out = []
    while sum(out) < n:
        out.append(min(int(rng.integers(lo, hi + 1)), n - sum(out)))
    return out


def mixed_rows(rng, h, w, kinds):
    """h rows of w pixels, each of one kind of kinds[y % len(kinds)]: 'flat' spans of one colour,
    'ramp's (every component a line in x, modulo 256: the filter Sub leaves runs), 'noise', or
    'mix': spans of the three. Values are k/255, so every row holds what is said."""
    px = np.zeros((h, w, 3), np.int64)
    x = np.arange(w)[:, None]
    for y in range(h):
        kind, at = kinds[y % len(kinds)], 0
        for n in _spans(rng, w, 1, max(1, w if kind in ("ramp", "noise") else w // 2)):
            k = kind if kind != "mix" else ("flat", "ramp", "noise")[int(rng.integers(3))]
            if k == "flat":
                px[y, at:at + n] = rng.integers(0, 256, 3)
            elif k == "ramp":
                px[y, at:at + n] = rng.integers(0, 256, 3) + x[:n] * rng.integers(0, 4, 3)
            else:
                px[y, at:at + n] = rng.integers(0, 256, (n, 3))
            at += n
    return (px % 256) / 255.0


# ---- the device's thread geometry (rt_png_deflate_dev.hip, pngz_encode_device)
DEVICE_MAX_WIDTH = 8533  # a row of 25600 bytes: 256 threads of 100


def device_chunk(w):
    """Bytes of a segment per thread: whole words, an odd number of them."""
    chunk = (-(-rows_per_segment(w) * (3 * w + 1) // 256) + 3) & ~3
    return chunk + 4 if chunk % 8 == 0 else chunk


@functools.lru_cache(maxsize=None)
def sweep_widths():
    """The width sweep: 1..48, the widths at which a row crosses 256, 512 and 1024 bytes, and the
    first width of every chunk size the device can reach."""
    first = {}
    for w in range(1, DEVICE_MAX_WIDTH + 1):
        first.setdefault(device_chunk(w), w)
    # a full segment holds more than half of 16384 bytes (a row of at most that; a longer one is a
    # segment of its own, at most 25600 bytes): 33 to 100 bytes a thread, rounded up to 4k + 4
    assert sorted(first) == list(range(36, 101, 8))
    return sorted(set(range(1, 49)) | {84, 85, 86, 170, 171, 341, 342} | set(first.values()))


SWEEP_H = 5


@functools.lru_cache(maxsize=None)
def sweep_canvas(w):
    """Five rows of a seeded mix of flat spans, ramps and noise patches, one row of them noise."""
    return mixed_rows(np.random.default_rng(7000 + w), SWEEP_H, w, ("mix", "flat", "noise", "ramp", "mix"))


@functools.lru_cache(maxsize=None)
def edge_canvases():
    """name -> canvas: the format's edges, shared by the host and the device tests."""
    wide = (SEGMENT + 2) // 3  # 5462: a row of 16387 bytes, one row per segment
    rps = rows_per_segment(100)  # 54 rows of 301 bytes
    alt = np.tile(np.array([[0.6, 0.8, 1.0], [0.0, 0.2, 0.4]]), (20, 1)).reshape(1, 40, 3)
    out = {f"edge_{h}x{w}": png_ref.edge_canvas(h, w) for h, w in [(1, 1), (1, 2), (2, 1), (3, 258)]}
    out.update({
        "run_258": _row(3, 87),   # 00 | ff ff ff | 258 zeros
        "run_259": _row(0, 86),   # 00 and 258 zeros
        "run_260": _row(1, 87),   # 00 | ff | 260 zeros
        "all_ones": png_ref.sized_canvas("all_ones"),
        "row_over_segment": png_ref.edge_canvas(3, wide),
        "rows_minus_1": png_ref.edge_canvas(rps - 1, 100),
        "rows_exact": png_ref.edge_canvas(rps, 100),
        "rows_plus_1": png_ref.edge_canvas(rps + 1, 100),
        "noise_64x64": np.random.default_rng(64).uniform(0.0, 1.0, size=(64, 64, 3)),
        "no_match": alt,
        "lit_limit_16": _lit_limit_row(16),  # W 1393
        "lit_limit_18": _lit_limit_row(18),  # W 3648
        "cl_limit": _cl_limit_row(),         # W 682
        # a row of 8194 bytes: one row per segment, three rounds of the device's scan over the segments
        "segments_513": mixed_rows(np.random.default_rng(513), 513, 2731, ("flat", "noise", "ramp", "mix", "noise")),
        # the widest row the device takes, the one before, and a row of exactly one segment
        "max_width": mixed_rows(np.random.default_rng(8533), 2, DEVICE_MAX_WIDTH, ("noise", "mix")),
        "max_width_minus_1": mixed_rows(np.random.default_rng(8532), 2, DEVICE_MAX_WIDTH - 1, ("noise", "mix")),
        "row_of_a_segment": mixed_rows(np.random.default_rng(5461), 2, (SEGMENT - 1) // 3, ("noise", "mix")),
        # next to the encoders' decision (dynamic_len < stored_len): a dynamic segment one byte below its
        # stored form, and one exactly as long, which is stored (rows of two byte values from a seeded
        # search through the host encoder: 10^5 rows of 4..64 pixels over 2..6 values gave 1028 and 864)
        "wins_by_one": _byte_row("f821212121f8212121f8f821f8f821f8f8f8f8f8f821212121f821f8f8f8f8212121f8f8f82121f8f8f8f8"
                                 "f821f8f8f8212121f82121"),
        "tie": _byte_row("47e747e747e747e7474747e7474747e7e7e747e747e7e7e74747e7e747e7e747e747e747e7e7e747e7474747e747"
                         "e747e74747"),
        # (host only) a row of 65539 bytes: a stored segment of two blocks, a dynamic block over more than one
        "row_over_stored_block": mixed_rows(np.random.default_rng(21846), 2, 21846, ("noise", "flat")),
    })
    return out


EDGE_NAMES = ["edge_1x1", "edge_1x2", "edge_2x1", "edge_3x258", "run_258", "run_259", "run_260", "all_ones",
              "row_over_segment", "rows_minus_1", "rows_exact", "rows_plus_1", "noise_64x64", "no_match",
              "lit_limit_16", "lit_limit_18", "cl_limit", "segments_513", "max_width", "max_width_minus_1",
              "row_of_a_segment", "wins_by_one", "tie"]
HOST_NAMES = EDGE_NAMES + ["row_over_stored_block"]  # (the device refuses a row of more than 25600 bytes)
# the segments of segments_513 whose blocks are checked: the first, the last, both sides of every 256th
SEGMENTS_513_SAMPLE = frozenset({0, 255, 256, 511, 512})
GOLDEN_HALF = ("c1", "first_scene_96x54", "yaml_cover_80x80")  # below half of the stored file

"""What a compressed PNG of the library must be, checked from the format alone
with struct, zlib and numpy (the library is not used): the chunks and their
CRCs, a zlib stream that inflates to H rows of 3W + 1 bytes, on every row the
filter type with the least sum of min(b, 256 - b) over its filtered bytes (ties
to the lowest type, bpp 3, zeros above row 0), the pixels PIL reads back, and
the size against zlib's Z_RLE strategy over the same filtered bytes.
"""
import functools
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


def check_file(png, px, size_against_rle=False, bound_of=bound):
    """`png` holds `px` in this format; returns (IDAT payload length, the filtered bytes)."""
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
    return len(idat), F


def longest_run(F):
    """The longest run of one byte value in F."""
    a = np.frombuffer(bytes(F), np.uint8)
    cuts = np.flatnonzero(np.diff(a) != 0) + 1
    return int(np.diff(np.concatenate([[0], cuts, [a.size]])).max())


def _row(first, w):  # one row: `first` components of 1.0, then zeros (filter None wins: see the tests)
    c = np.zeros((1, w, 3))
    c.reshape(-1)[:first] = 1.0
    return c


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
    })
    return out


EDGE_NAMES = ["edge_1x1", "edge_1x2", "edge_2x1", "edge_3x258", "run_258", "run_259", "run_260", "all_ones",
              "row_over_segment", "rows_minus_1", "rows_exact", "rows_plus_1", "noise_64x64", "no_match"]
GOLDEN_HALF = ("c1", "first_scene_96x54", "yaml_cover_80x80")  # below half of the stored file

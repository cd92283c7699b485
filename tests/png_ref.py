"""The PNG the writers must produce (image/png.rs:13-31), built here from the
format alone with struct and zlib's checksums, so that it does not depend on
the library: signature, IHDR, one IDAT whose zlib stream (78 01) holds stored
deflate blocks of at most 65535 raw bytes, the Adler-32 of the raw image, IEND.

The pixels are the reference writer's: the tokens of the oracle's
`canvas_to_ppm` (pinned by the reference's PPM tests) parsed back to uint8;
png.rs:29-31 and ppm.rs:73-75 quantise alike (half away from zero, unlike
numpy.round).
"""
import functools
import io
import struct
import zlib

import numpy as np

STORED = 65535


def quantised(oracle, canvas):
    ppm = oracle.canvas_to_ppm(canvas)
    ppm = ppm.encode() if isinstance(ppm, str) else bytes(ppm)
    body = ppm.split(b"\n", 3)[3]
    h, w = canvas.shape[0], canvas.shape[1]
    return np.array(body.split(), dtype=np.int64).astype(np.uint8).reshape(h, w, 3)


def _chunk(kind, payload):
    return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", zlib.crc32(kind + payload))


def expected_png(px):
    h, w = px.shape[0], px.shape[1]
    raw = np.concatenate([np.zeros((h, 1), np.uint8), px.reshape(h, 3 * w)], axis=1).tobytes()
    n = -(-len(raw) // STORED)
    z = [b"\x78\x01"]
    for b in range(n):
        part = raw[b * STORED:(b + 1) * STORED]
        z.append(struct.pack("<BHH", 1 if b == n - 1 else 0, len(part), len(part) ^ 0xFFFF) + part)
    z.append(struct.pack(">I", zlib.adler32(raw)))
    out = (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))
           + _chunk(b"IDAT", b"".join(z)) + _chunk(b"IEND", b""))
    assert len(out) == predicted_size(w, h)
    return out


def predicted_size(w, h):
    r = h * (3 * w + 1)
    return 63 + 5 * (-(-r // STORED)) + r


def decoded(png):
    from PIL import Image
    img = Image.open(io.BytesIO(png))
    img.load()
    return img.mode, img.size, np.asarray(img)


def check_file(png, px):
    """`png` is the hand-built file of `px`, and PIL reads `px` back from it."""
    png = bytes(png)
    want = expected_png(px)
    assert len(png) == len(want)
    if png != want:
        bad = np.flatnonzero(np.frombuffer(png, np.uint8) != np.frombuffer(want, np.uint8))
        raise AssertionError(f"{bad.size} bytes differ, the first at offset {bad[0]} of {len(want)}")
    mode, size, pixels = decoded(png)
    assert mode == "RGB" and size == (px.shape[1], px.shape[0])
    assert np.array_equal(pixels, px)


def edge_values(rng, n):  # test_gpu_ppm.py's: halves and their neighbours, negatives, NaN, infinities, above 1
    halves = (np.arange(256) + 0.5) / 255.0
    return np.concatenate([halves, np.nextafter(halves, 0), np.nextafter(halves, 2), np.arange(256) / 255.0,
                           [0.0, -0.0, -1e-300, -0.5, 1.0, 1.0000001, 2.0, 1e300, np.inf, -np.inf, np.nan],
                           rng.uniform(-0.2, 1.2, n)])


def edge_canvas(h, w, seed=None):
    rng = np.random.default_rng(w * 100003 + h if seed is None else seed)
    return rng.choice(edge_values(rng, 3 * w * h), size=(h, w, 3))


# (name, H, W): the stored-block boundaries with W = 28 (a row is 85 raw bytes, 65535 = 85 * 771),
# rows that straddle blocks, R = 65533, the Adler worst case, one frame
SIZES = [("one_block", 771, 28), ("block_plus_row", 772, 28), ("two_blocks", 1542, 28), ("two_blocks_plus_row", 1543, 28),
         ("row_65536", 2, 21845), ("r_65533", 1, 21844), ("all_ones", 300, 300), ("frame_640x360", 360, 640)]


@functools.lru_cache(maxsize=None)
def sized_canvas(name):
    h, w = next((h, w) for n, h, w in SIZES if n == name)
    if name == "all_ones":
        return np.ones((h, w, 3))
    if name == "frame_640x360":
        return np.random.default_rng(640).uniform(-0.1, 1.1, size=(h, w, 3))
    return edge_canvas(h, w)

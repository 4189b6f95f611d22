"""CPU: the host side of the step-7 video (vistracker_amd/video.py): JFIF header tables pinned to Pillow / libjpeg and Annex K, the AVI writer's RIFF
tree, and its 32-bit overflow guard."""
import io
import os
import struct

import numpy as np
import pytest

import jpeg_model as M
from vistracker_amd import video as V

QUALITIES = (1, 10, 50, 75, 90, 95, 100)


def _pillow_jpeg(q, subsampling=2):
    PIL = pytest.importorskip("PIL.Image")
    img = np.random.default_rng(q).integers(0, 256, (24, 40, 3), dtype=np.uint8)
    b = io.BytesIO()
    PIL.fromarray(img).save(b, "JPEG", quality=q, subsampling=subsampling)
    return b.getvalue()


@pytest.mark.parametrize("q", QUALITIES)
def test_quant_tables_equal_libjpeg(q):
    """Pillow's quantization property is in natural order; so are quant_tables and the model's tables (the header holds them in zig-zag order)"""
    PIL = pytest.importorskip("PIL.Image")
    qt = PIL.open(io.BytesIO(_pillow_jpeg(q))).quantization
    lum, chr_ = V.quant_tables(q)
    assert list(qt[0]) == list(lum) and list(qt[1]) == list(chr_)
    ml, mc = M.quality_tables(q)
    assert list(ml) == list(lum) and list(mc) == list(chr_)
    info = M.parse(V.jfif_header(16, 16, q, "420"), decode=False)
    assert list(info["dqt"][0]) == list(lum) and list(info["dqt"][1]) == list(chr_)


def test_huffman_tables_are_annex_k():
    """the DHT of the header equals the tables libjpeg writes by default (Annex K), read from a Pillow file by the model's parser"""
    ref = M.parse(_pillow_jpeg(75))["dht"]
    ours = M.parse(V.jfif_header(8, 8, 75, "444"), decode=False)["dht"]
    assert ours == ref and len(ours) == 4
    # and Annex K's counts: 12 DC symbols, 162 AC symbols per table
    assert [sum(ours[k][0]) for k in ((0, 0), (0, 1), (1, 0), (1, 1))] == [12, 12, 162, 162]


@pytest.mark.parametrize("sub,f", [("420", 2), ("444", 1)])
@pytest.mark.parametrize("H,W", [(1, 1), (900, 2160), (17, 33)])
def test_header_parses(sub, f, H, W):
    hdr = V.jfif_header(H, W, 90, sub)
    assert hdr[:2] == b"\xff\xd8" and hdr[2:4] == b"\xff\xe0" and hdr[6:11] == b"JFIF\x00"
    info = M.parse(hdr, decode=False)
    assert info["header_bytes"] == len(hdr)
    assert (info["H"], info["W"], info["P"]) == (H, W, 8)
    assert info["comps"] == [(1, f, f, 0), (2, 1, 1, 1), (3, 1, 1, 1)]
    assert info["scan"] == [(1, 0, 0), (2, 1, 1), (3, 1, 1)]
    assert info["dri"] == -(-W // (8 * f))                      # restart interval: one MCU row


def test_bad_arguments():
    for q in (0, 101, 50.0, True):
        with pytest.raises(ValueError):
            V.jfif_header(8, 8, q)
    with pytest.raises(ValueError):
        V.jfif_header(8, 8, 90, "422")
    with pytest.raises(ValueError):
        V.jfif_header(0, 8, 90)
    with pytest.raises(ValueError):
        V.JpegEncoder(8, 8, quality=0)
    with pytest.raises(ValueError):
        V.JpegEncoder(8, 8, quality=101)


# ---- AVI ------------------------------------------------------------------------------------------------------------------------------------------
def walk_riff(data):
    """RIFF tree -> nested list of (fourcc, payload offset, size, children or None); asserts every size fits its parent and pads are even"""
    def chunks(lo, hi):
        out, p = [], lo
        while p < hi:
            cid, n = data[p:p + 4], struct.unpack("<I", data[p + 4:p + 8])[0]
            assert p + 8 + n <= hi, (cid, p, n, hi)
            if cid in (b"RIFF", b"LIST"):
                out.append((data[p + 8:p + 12], p + 12, n - 4, chunks(p + 12, p + 8 + n)))
            else:
                out.append((cid, p + 8, n, None))
            p += 8 + n + (n & 1)
        assert p == hi, (p, hi)
        return out
    return chunks(0, len(data))


def test_avi_writer_riff_tree(tmp_path):
    frames = [b"\xff\xd8" + bytes(range(7)) + b"\xff\xd9", b"\xff\xd8" + b"\x11" * 100 + b"\xff\xd9", b"\xff\xd8\x00\xff\xd9"]
    path = str(tmp_path / "a.avi")
    with V.AviMjpegWriter(path, 640, 480, fps=30) as w:
        for f in frames:
            w.write(f)
    data = open(path, "rb").read()
    top = walk_riff(data)
    assert len(top) == 1 and top[0][0] == b"AVI " and data[:4] == b"RIFF"
    assert struct.unpack("<I", data[4:8])[0] == len(data) - 8
    kids = top[0][3]
    assert [k[0] for k in kids] == [b"hdrl", b"movi", b"idx1"]
    hdrl = kids[0][3]
    assert hdrl[0][0] == b"avih" and hdrl[0][2] == 56
    avih = struct.unpack("<14I", data[hdrl[0][1]:hdrl[0][1] + 56])
    assert avih[0] == 33333 and avih[4] == len(frames) and avih[6] == 1 and (avih[8], avih[9]) == (640, 480)
    assert avih[3] & 0x10 and avih[7] == max(len(f) for f in frames)
    strl = hdrl[1]
    assert strl[0] == b"strl"
    strh, strf = strl[3]
    assert strh[0] == b"strh" and strh[2] == 56 and strf[0] == b"strf" and strf[2] == 40
    sh = data[strh[1]:strh[1] + 56]
    assert sh[:8] == b"vidsMJPG"
    scale, rate, start, length = struct.unpack("<4I", sh[20:36])
    assert (scale, rate, start, length) == (1, 30, 0, len(frames))
    bi = struct.unpack("<IiiHH4sIiiII", data[strf[1]:strf[1] + 40])
    assert bi[:6] == (40, 640, 480, 1, 24, b"MJPG")
    movi = kids[1]
    chunks = movi[3]
    assert [c[0] for c in chunks] == [b"00dc"] * len(frames)
    assert [data[c[1]:c[1] + c[2]] for c in chunks] == frames               # the bytes come back unchanged
    assert all((c[1] - movi[1]) % 2 == 0 for c in chunks)                  # every chunk starts on an even offset (odd frames are padded)
    idx = kids[2]
    assert idx[2] == 16 * len(frames)
    for k, c in enumerate(chunks):
        cid, flags, off, size = struct.unpack("<4sIII", data[idx[1] + 16 * k:idx[1] + 16 * k + 16])
        movi_fourcc = movi[1] - 4
        assert cid == b"00dc" and flags & 0x10 and size == len(frames[k])
        assert data[movi_fourcc + off:movi_fourcc + off + 4] == b"00dc" and movi_fourcc + off + 8 == c[1]


def test_avi_writer_fractional_fps(tmp_path):
    path = str(tmp_path / "b.avi")
    with V.AviMjpegWriter(path, 8, 8, fps=29.97) as w:
        w.write(b"\xff\xd8\xff\xd9")
    data = open(path, "rb").read()
    p = data.index(b"strh") + 8
    scale, rate = struct.unpack("<2I", data[p + 20:p + 28])
    assert rate / scale == pytest.approx(29.97) and (rate, scale) == (2997, 100)


def test_avi_overflow_guard(tmp_path):
    """before a frame would take the file past the 32-bit RIFF size, write() raises and writes nothing; the file closes valid"""
    path = str(tmp_path / "c.avi")
    w = V.AviMjpegWriter(path, 8, 8)
    w.write(b"\xff\xd8ab\xff\xd9")
    real = w.size
    w.size = 0xFFFFFFFF - 100                 # as if ~4 GiB had been written
    with pytest.raises(OverflowError):
        w.write(b"x" * 200)
    assert w.frames == 1
    w.size = real
    w.close()
    data = open(path, "rb").read()
    kids = walk_riff(data)[0][3]
    assert [k[0] for k in kids] == [b"hdrl", b"movi", b"idx1"] and len(kids[1][3]) == 1
    # the same frame just fits below the limit
    w2 = V.AviMjpegWriter(str(tmp_path / "d.avi"), 8, 8)
    w2.size = 0xFFFFFFFF + 8 - (8 + 200 + 8 + 16) - 1000
    w2.write(b"x" * 200)
    w2.f.close()

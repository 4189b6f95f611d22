"""Step 7's video (render/render_recon.py:113-115, 169, 188: ``imageio.get_writer(..., format='FFMPEG', fps)`` + ``append_data``): Motion-JPEG in an AVI
file, encoded on the GPU.

``JpegEncoder`` turns uint8 frames already in device memory into complete JPEG files through ``vt_jpeg_encode`` (``csrc/jpeg.hip``, whose header states
the contract); only the compressed bytes cross to the host.  ``jfif_header`` builds the per-size header (SOI, APP0, DQT, SOF0, DHT, DRI, SOS) once: every
frame carries its own Huffman tables, so each frame decodes on its own.  ``AviMjpegWriter`` is a pure-Python RIFF AVI 1.0 writer (no OpenDML: it refuses
to grow past the 32-bit RIFF size).  No cv2 / imageio / ffmpeg is needed; H.264 / mp4 are out of scope.  There is no CPU encoder: host frames are uploaded.
"""
from __future__ import annotations

import ctypes as C
import struct
from fractions import Fraction

import numpy as np
import torch

from . import _lib as L

# ITU T.81 Annex K: quantisation tables in natural (row-major) order, Huffman tables as (BITS, HUFFVAL)
LUM_QUANT = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
             18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
CHR_QUANT = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32
DC_LUM = ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12)))
DC_CHR = ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12)))
AC_LUM = ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d), (
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
    0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
    0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa))
AC_CHR = ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77), (
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
    0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
    0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa))
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43,
          36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
SUBSAMPLING = {"420": (420, 2), "444": (444, 1)}       # name -> (ABI code, horizontal = vertical sampling factor of luminance)


def _check_quality(quality):
    if isinstance(quality, bool) or not isinstance(quality, (int, np.integer)) or not 1 <= int(quality) <= 100:
        raise ValueError(f"JPEG quality must be an integer 1..100, got {quality!r}")
    return int(quality)


def _check_subsampling(subsampling):
    if subsampling not in SUBSAMPLING:
        raise ValueError(f"subsampling must be one of {sorted(SUBSAMPLING)}, got {subsampling!r}")
    return SUBSAMPLING[subsampling]


def quant_tables(quality):
    """libjpeg's jpeg_set_quality(quality, force_baseline=TRUE): the Annex K tables scaled, natural order -> (luminance, chrominance)"""
    q = _check_quality(quality)
    s = 5000 // q if q < 50 else 200 - 2 * q
    scale = lambda base: tuple(min(255, max(1, (b * s + 50) // 100)) for b in base)
    return scale(LUM_QUANT), scale(CHR_QUANT)


def _segment(marker, payload):
    return struct.pack(">BBH", 0xFF, marker, len(payload) + 2) + payload


def jfif_header(H, W, quality=90, subsampling="420"):
    """SOI, APP0 (JFIF 1.01), DQT (both tables, zig-zag order), SOF0, DHT (the four Annex K tables), DRI (one MCU row), SOS: everything in front of
    the entropy-coded data ``vt_jpeg_encode`` writes"""
    if not (1 <= H <= 65535 and 1 <= W <= 65535):
        raise ValueError(f"JPEG frames are 1..65535 pixels per side, got {H} x {W}")
    _, f = _check_subsampling(subsampling)
    lum, chr_ = quant_tables(quality)
    out = bytearray(b"\xff\xd8")
    out += _segment(0xE0, b"JFIF\x00" + struct.pack(">BBBHHBB", 1, 1, 0, 1, 1, 0, 0))
    out += _segment(0xDB, bytes([0x00]) + bytes(lum[z] for z in ZIGZAG) + bytes([0x01]) + bytes(chr_[z] for z in ZIGZAG))
    out += _segment(0xC0, struct.pack(">BHHB", 8, H, W, 3) + bytes([1, (f << 4) | f, 0, 2, 0x11, 1, 3, 0x11, 1]))
    dht = bytearray()
    for tc_th, (bits, vals) in ((0x00, DC_LUM), (0x10, AC_LUM), (0x01, DC_CHR), (0x11, AC_CHR)):
        dht += bytes([tc_th]) + bytes(bits) + bytes(vals)
    out += _segment(0xC4, bytes(dht))
    mcus_x = -(-W // (8 * f))
    out += _segment(0xDD, struct.pack(">H", mcus_x))
    out += _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return bytes(out)


class JpegEncoder:
    """GPU JPEG encoder for (n, H, W, 3) uint8 device frames (``vt_jpeg_encode``).  The device workspace and the pinned host buffer of the compressed
    bytes are cached and grow as needed (as ``visualize.ShadedRasterizer`` does); batches larger than ``batch`` frames are encoded ``batch`` at a time
    (the bytes do not depend on the batching)."""

    def __init__(self, H, W, quality=90, subsampling="420", device="cuda:0", batch=8):
        self.quality = _check_quality(quality)
        self.sub_code, _ = _check_subsampling(subsampling)
        self.H, self.W, self.subsampling = int(H), int(W), subsampling
        self.header = jfif_header(self.H, self.W, self.quality, subsampling)
        self.device = torch.device(device)
        self.batch = int(batch)
        self.ws = None
        self.host = None

    def _buffers(self, n):
        max_out = C.c_longlong(0)
        nbytes = L.lib().vt_jpeg_workspace_bytes(n, self.H, self.W, self.sub_code, C.byref(max_out))
        if nbytes < 0:
            L.check(L.VT_ERR_ARG)
        if self.ws is None or self.ws.numel() < nbytes:
            self.ws = None
            self.ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        if self.host is None or self.host.numel() < max_out.value:
            self.host = None
            self.host = torch.empty(max_out.value, dtype=torch.uint8, pin_memory=True)
        return self.ws, self.host

    def encode_raw(self, frames, ws=None, ws_bytes=None):
        """entropy-coded data of each frame of ``frames`` (one vt_jpeg_encode call, no batching) -> (host uint8 array, offsets (n + 1,))"""
        fr = self._check(frames)
        n = fr.shape[0]
        cache_ws, host = self._buffers(n)
        ws = cache_ws if ws is None else ws
        ws_bytes = ws.numel() if ws_bytes is None else int(ws_bytes)
        offs = np.zeros(n + 1, np.int64)
        with torch.cuda.device(self.device):
            L.check(L.lib().vt_jpeg_encode(fr.data_ptr(), n, self.H, self.W, fr.stride(0), fr.stride(1), self.quality, self.sub_code, L.dptr(ws), ws_bytes,
                                           host.data_ptr(), host.numel(), offs.ctypes.data_as(C.POINTER(C.c_longlong)), L.stream_ptr()))
        return host.numpy(), offs

    def encode(self, frames):
        """(n, H, W, 3) uint8 device tensor, or a view of one with packed pixels (stride 3, 1 on the last two axes) -> list of n complete JPEG files"""
        fr = self._check(frames)
        out = []
        for s in range(0, fr.shape[0], self.batch):
            data, offs = self.encode_raw(fr[s:s + self.batch])
            out.extend(self.header + data[offs[i]:offs[i + 1]].tobytes() for i in range(len(offs) - 1))
        return out

    def _check(self, frames):
        if not isinstance(frames, torch.Tensor):
            raise TypeError(f"JpegEncoder.encode takes a uint8 CUDA (HIP) tensor, got {type(frames).__name__}; there is no CPU encoder")
        if not frames.is_cuda:
            raise L.VtError("JpegEncoder.encode needs frames in device memory (a CUDA tensor); there is no CPU fallback")
        if frames.dtype != torch.uint8:
            raise TypeError(f"JpegEncoder.encode takes uint8 frames, got {frames.dtype}")
        if frames.dim() == 3:
            frames = frames[None]
        if frames.dim() != 4 or tuple(frames.shape[1:]) != (self.H, self.W, 3):
            raise ValueError(f"frames must be (n, {self.H}, {self.W}, 3), got {tuple(frames.shape)}")
        if frames.device != self.device:
            raise ValueError(f"frames on {frames.device}, encoder on {self.device}")
        if frames.stride(3) != 1 or frames.stride(2) != 3 or frames.stride(1) < 3 * self.W or frames.stride(0) < 0:
            raise ValueError(f"frames need packed pixels (strides (., >= {3 * self.W}, 3, 1)), got {frames.stride()}")
        return frames


# ---- AVI 1.0 (RIFF) ------------------------------------------------------------------------------------------------------------------------------
_AVIF_HASINDEX, _AVIIF_KEYFRAME = 0x10, 0x10
_RIFF_MAX = 0xFFFFFFFF


class AviMjpegWriter:
    """RIFF AVI 1.0 with one Motion-JPEG video stream: hdrl (avih, strl: strh 'vids' / 'MJPG', strf BITMAPINFOHEADER), movi ('00dc' chunks, padded to
    even length), idx1.  Frame counts and sizes are patched on close.  ``write`` raises OverflowError (and writes nothing) before the file would pass
    the 32-bit RIFF size; the file stays valid with the frames written so far."""

    def __init__(self, path, W, H, fps=30):
        if not (W > 0 and H > 0):
            raise ValueError(f"bad frame size {W} x {H}")
        fr = Fraction(fps).limit_denominator(1001)
        if fr <= 0:
            raise ValueError(f"fps must be positive, got {fps}")
        self.path, self.W, self.H, self.rate, self.scale = path, int(W), int(H), fr.numerator, fr.denominator
        self.index = []              # (offset from the 'movi' fourcc, size)
        self.max_frame = 0
        self.f = open(path, "wb")
        self._closed = False
        self._write_headers()

    def _write_headers(self):
        f = self.f
        us_per_frame = int(round(1e6 * self.scale / self.rate))
        avih = struct.pack("<14I", us_per_frame, 0, 0, _AVIF_HASINDEX, 0, 0, 1, 0, self.W, self.H, 0, 0, 0, 0)
        strh = (b"vids" + b"MJPG" + struct.pack("<IHHIIIIIIiI", 0, 0, 0, 0, self.scale, self.rate, 0, 0, 0, -1, 0)
                + struct.pack("<4h", 0, 0, min(self.W, 32767), min(self.H, 32767)))
        strf = struct.pack("<IiiHH4sIiiII", 40, self.W, self.H, 1, 24, b"MJPG", self.W * self.H * 3, 0, 0, 0, 0)
        strl = b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + b"strf" + struct.pack("<I", len(strf)) + strf
        hdrl = b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + b"LIST" + struct.pack("<I", len(strl)) + strl
        f.write(b"RIFF" + struct.pack("<I", 0) + b"AVI ")
        self._hdrl_pos = f.tell()
        f.write(b"LIST" + struct.pack("<I", len(hdrl)) + hdrl)
        # file positions of the fields patched on close
        self._avih_frames = self._hdrl_pos + 12 + 8 + 16
        self._avih_bufsize = self._hdrl_pos + 12 + 8 + 28
        strh_pos = self._hdrl_pos + 12 + 8 + len(avih) + 12 + 8
        self._strh_length = strh_pos + 32
        self._strh_bufsize = strh_pos + 36
        self._movi_pos = f.tell()
        f.write(b"LIST" + struct.pack("<I", 0) + b"movi")
        self.size = f.tell()          # bytes written so far

    def _bytes_after(self, nbytes):
        """file size once one more frame of nbytes and the index are written"""
        return self.size + 8 + nbytes + (nbytes & 1) + 8 + 16 * (len(self.index) + 1)

    def write(self, jpeg):
        if self._closed:
            raise ValueError("AviMjpegWriter is closed")
        jpeg = bytes(jpeg)
        if self._bytes_after(len(jpeg)) - 8 > _RIFF_MAX:
            raise OverflowError(f"{self.path}: frame {len(self.index)} would take the AVI past the 32-bit RIFF size (4 GiB); AVI 2.0 (OpenDML) "
                                "is not supported -- split the video")
        off = self.size - (self._movi_pos + 8)              # from the 'movi' fourcc, as idx1 counts
        self.f.write(b"00dc" + struct.pack("<I", len(jpeg)) + jpeg + (b"\x00" if len(jpeg) & 1 else b""))
        self.size += 8 + len(jpeg) + (len(jpeg) & 1)
        self.index.append((off, len(jpeg)))
        self.max_frame = max(self.max_frame, len(jpeg))

    def close(self):
        if self._closed:
            return
        self._closed = True
        f = self.f
        try:
            f.write(b"idx1" + struct.pack("<I", 16 * len(self.index)))
            f.write(b"".join(b"00dc" + struct.pack("<III", _AVIIF_KEYFRAME, o, n) for o, n in self.index))
            end = f.tell()
            n = len(self.index)
            for pos, val in ((4, end - 8), (self._movi_pos + 4, self.size - self._movi_pos - 8), (self._avih_frames, n), (self._strh_length, n),
                             (self._avih_bufsize, self.max_frame), (self._strh_bufsize, self.max_frame)):
                f.seek(pos); f.write(struct.pack("<I", val))
        finally:
            f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    @property
    def frames(self):
        return len(self.index)


def write_video(chunks, path, fps=30, quality=90, subsampling="420", device=None):
    """Motion-JPEG AVI of ``chunks``: an iterable of uint8 (n, H, W, 3) frame chunks (device tensors, host tensors or numpy arrays; host chunks are
    uploaded, the encoder runs on the GPU) -> (path, frame count)"""
    _check_quality(quality); _check_subsampling(subsampling)
    enc = writer = None
    count = 0
    try:
        for ch in chunks:
            if not isinstance(ch, torch.Tensor):
                ch = torch.as_tensor(np.ascontiguousarray(ch))
            if ch.dim() == 3:
                ch = ch[None]
            if not ch.is_cuda:
                ch = ch.to(device if device is not None else torch.device("cuda", torch.cuda.current_device()))
            if enc is None:
                enc = JpegEncoder(int(ch.shape[1]), int(ch.shape[2]), quality=quality, subsampling=subsampling, device=ch.device)
            jpgs = enc.encode(ch)                    # before the file is created: bad input leaves nothing behind
            if writer is None:
                writer = AviMjpegWriter(path, enc.W, enc.H, fps=fps)
            for jpg in jpgs:
                writer.write(jpg)
                count += 1
        if writer is None:
            raise ValueError("write_video: no frames")
    finally:
        if writer is not None:
            writer.close()
    return path, count


def write_videos(chunk_tuples, paths, fps=30, quality=90, subsampling="420", device=None):
    """``write_video`` for k videos fed together: ``chunk_tuples`` yields k-tuples of frame chunks, chunk j of every tuple goes to ``paths[j]`` (sizes may
    differ from video to video), so no video's frames have to be kept while another is written -> list of (path, frame count)"""
    _check_quality(quality); _check_subsampling(subsampling)
    k = len(paths)
    encs, writers, counts = [None] * k, [None] * k, [0] * k
    try:
        for chs in chunk_tuples:
            if len(chs) != k:
                raise ValueError(f"write_videos: {len(chs)} chunks for {k} videos")
            for j, ch in enumerate(chs):
                if not isinstance(ch, torch.Tensor):
                    ch = torch.as_tensor(np.ascontiguousarray(ch))
                if ch.dim() == 3:
                    ch = ch[None]
                if not ch.is_cuda:
                    ch = ch.to(device if device is not None else torch.device("cuda", torch.cuda.current_device()))
                if encs[j] is None:
                    encs[j] = JpegEncoder(int(ch.shape[1]), int(ch.shape[2]), quality=quality, subsampling=subsampling, device=ch.device)
                jpgs = encs[j].encode(ch)
                if writers[j] is None:
                    writers[j] = AviMjpegWriter(paths[j], encs[j].W, encs[j].H, fps=fps)
                for jpg in jpgs:
                    writers[j].write(jpg)
                    counts[j] += 1
        if any(w is None for w in writers):
            raise ValueError("write_videos: no frames")
    finally:
        for w in writers:
            if w is not None:
                w.close()
    return list(zip(paths, counts))

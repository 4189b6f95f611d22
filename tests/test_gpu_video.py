"""GPU: the step-7 Motion-JPEG video (csrc/jpeg.hip vt_jpeg_encode, vistracker_amd/video.py).

The GPU's streams are parsed by tests/jpeg_model.py (written from T.81 and the contract in jpeg.hip's header, no code shared with the kernel) and their
coefficients compared with the float64 model; the entropy-coded bytes must equal the model's re-encoding of those coefficients byte for byte (Huffman
codes, padding, stuffing, restart markers).  libjpeg (through Pillow) must decode every file."""
import io
import struct
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import jpeg_model as M
from vistracker_amd import _lib as L
from vistracker_amd import video as VID
from vistracker_amd import visualize as V

pytestmark = pytest.mark.gpu
# coefficients within 1e-3 of a rounding half-way point may differ by one (fp32 vs float64); their number is bounded per image
MAX_AMBIGUOUS_SHARE = 2e-3
# PSNR of step-7 frames (rendered panels + a photo-like rgb panel) at q90 4:2:0, decoded by libjpeg: worst frame measured 38.68 dB on an MI355X
PSNR_BAR = 38.0


def photo(H, W, seed=0, noise=6.0):
    """smooth colour gradients + blobs + sensor-like noise: a stand-in for the camera panel"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.stack([120 + 80 * np.sin(x / 97 + c) * np.cos(y / 71 - c) for c in range(3)], -1)
    for _ in range(6):
        cy, cx, r = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(10, 120)
        img += rng.uniform(-60, 60, 3) * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * r * r))[..., None]
    img += rng.normal(0, noise, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def encode(frames, q=90, sub="420"):
    fr = torch.as_tensor(np.ascontiguousarray(frames), device="cuda")
    if fr.dim() == 3:
        fr = fr[None]
    return VID.JpegEncoder(fr.shape[1], fr.shape[2], quality=q, subsampling=sub).encode(fr)


def check_stream(jpg, rgb, q, sub, exact_bytes=True):
    """parse jpg; its coefficients against the model; its entropy-coded data against the re-encoding -> (info, number of ambiguous flips)"""
    info = M.parse(jpg)
    H, W = rgb.shape[:2]
    assert (info["H"], info["W"]) == (H, W)
    f = 2 if sub == "420" else 1
    assert len(info["rst"]) == -(-H // (8 * f)) - 1
    model = M.model_coefficients(rgb, q, sub)
    flips = 0
    for c, (mc, amb) in enumerate(model):
        got = info["coef"][c]
        assert got.shape == mc.shape, (c, got.shape, mc.shape)
        d = got != mc
        assert not (d & ~amb).any(), (c, int((d & ~amb).sum()), np.argwhere(d & ~amb)[:5])
        assert np.abs(got - mc)[d].max(initial=0) <= 1
        flips += int(d.sum())
    assert flips <= MAX_AMBIGUOUS_SHARE * sum(m[0].size for m in model) + 2, flips
    data = jpg[info["header_bytes"]:]
    if exact_bytes:
        assert data == M.entropy_encode(info["coef"], info)
    return info, flips


def psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 10 * np.log10(255.0 ** 2 / max(mse, 1e-12))


def pil_decode(jpg):
    from PIL import Image
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        im = Image.open(io.BytesIO(jpg))
        im.load()
    return np.asarray(im.convert("RGB"))


# ---- coefficient exactness -----------------------------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (7, 9), (8, 8), (16, 16), (17, 33), (64, 48)]


@pytest.mark.parametrize("sub", ["420", "444"])
@pytest.mark.parametrize("q", [1, 50, 90, 100])
def test_coefficients_small_sizes(sub, q):
    for k, (H, W) in enumerate(SIZES):
        rgb = np.random.default_rng(100 + k).integers(0, 256, (H, W, 3), dtype=np.uint8) if k % 2 else photo(H, W, seed=k)
        jpg = encode(rgb, q, sub)[0]
        check_stream(jpg, rgb, q, sub)


@pytest.mark.parametrize("sub", ["420", "444"])
@pytest.mark.parametrize("q", [1, 50, 90, 100])
def test_coefficients_step7_size(sub, q):
    rgb = photo(900, 2160, seed=3, noise=2.0)
    jpg = encode(rgb, q, sub)[0]
    _, flips = check_stream(jpg, rgb, q, sub)
    print(f"900x2160 {sub} q{q}: {len(jpg)} bytes, {flips} half-way flips")


# ---- libjpeg decodes it ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub,pil_sub", [("420", 2), ("444", 0)])
def test_libjpeg_decodes_and_psnr_matches_pillow(sub, pil_sub):
    pytest.importorskip("PIL")
    from PIL import Image
    rgb = photo(900, 2160, seed=5)
    for q in (50, 90):
        ours = pil_decode(encode(rgb, q, sub)[0])
        assert ours.shape == rgb.shape
        b = io.BytesIO(); Image.fromarray(rgb).save(b, "JPEG", quality=q, subsampling=pil_sub)
        ref = pil_decode(b.getvalue())
        p_ours, p_ref = psnr(ours, rgb), psnr(ref, rgb)
        print(f"{sub} q{q}: PSNR ours {p_ours:.2f} dB, Pillow {p_ref:.2f} dB")
        assert abs(p_ours - p_ref) <= 0.5, (p_ours, p_ref)


# ---- stuffing and the largest categories -----------------------------------------------------------------------------------------------------
def test_stuffing_and_extreme_frames():
    H, W = 48, 64
    rng = np.random.default_rng(9)
    y, x = np.mgrid[0:H, 0:W]
    cases = {"noise": rng.integers(0, 256, (H, W, 3), dtype=np.uint8), "white": np.full((H, W, 3), 255, np.uint8),
             "black": np.zeros((H, W, 3), np.uint8), "checker": (((y + x) % 2) * 255).astype(np.uint8)[..., None].repeat(3, -1)}
    stuffed = {}
    for sub in ("420", "444"):
        for name, rgb in cases.items():
            jpg = encode(rgb, 100, sub)[0]
            info, flips = check_stream(jpg, rgb, 100, sub)
            model = M.model_coefficients(rgb, 100, sub)
            if not any(a.any() for _, a in model):
                # no half-way coefficient: the model's own stream is THE stream, stuffing included
                ref = M.entropy_encode([m for m, _ in model], info)
                assert jpg[info["header_bytes"]:] == ref
                assert info["stuffed"] == ref.count(b"\xff\x00"), name
            stuffed[(sub, name)] = info["stuffed"]
            dec = pil_decode(jpg)
            assert dec.shape == rgb.shape
            if name in ("white", "black"):
                assert np.abs(dec.astype(int) - rgb).max() <= 1, name
    assert stuffed[("420", "noise")] > 0 and stuffed[("444", "noise")] > 0, stuffed
    # DC category 11 (|diff| >= 1024) and AC categories up to 10 occur in the checkerboard / black frames at q100
    info = M.parse(encode(cases["black"], 100, "444")[0])
    assert info["coef"][0][0, 0, 0] == -1024


# ---- determinism and batch invariance ----------------------------------------------------------------------------------------------------------
def test_deterministic_and_batch_invariant():
    H, W = 120, 200
    frames = np.stack([photo(H, W, seed=20 + k) for k in range(8)])
    big = torch.zeros(11, H + 5, W + 7, 3, dtype=torch.uint8, device="cuda")
    big[2:10, 3:3 + H, 1:1 + W] = torch.as_tensor(frames, device="cuda")
    view = big[2:10, 3:3 + H, 1:1 + W]
    assert not view.is_contiguous()
    for sub in ("420", "444"):
        enc = VID.JpegEncoder(H, W, 90, sub)
        dev = torch.as_tensor(frames, device="cuda")
        a, b = enc.encode(dev), enc.encode(dev)
        assert a == b
        singles = [enc.encode(dev[k:k + 1])[0] for k in range(8)]
        assert singles == a
        assert enc.encode(view) == a
        enc3 = VID.JpegEncoder(H, W, 90, sub, batch=3)                 # batches of 3, 3, 2: every frame elsewhere in its batch
        assert enc3.encode(dev) == a


# ---- end to end: step-7 frames -> AVI ----------------------------------------------------------------------------------------------------------
def _walk(data, lo, hi):
    out, p = [], lo
    while p < hi:
        cid, n = data[p:p + 4], struct.unpack("<I", data[p + 4:p + 8])[0]
        out.append((cid, p + 8, n)); p += 8 + n + (n & 1)
    return out


def avi_frames(path):
    data = open(path, "rb").read()
    assert data[:4] == b"RIFF" and data[8:12] == b"AVI " and struct.unpack("<I", data[4:8])[0] == len(data) - 8
    top = _walk(data, 12, len(data))
    movi = [t for t in top if t[0] == b"LIST" and data[t[1]:t[1] + 4] == b"movi"][0]
    frames = [data[o:o + n] for cid, o, n in _walk(data, movi[1] + 4, movi[1] + movi[2]) if cid == b"00dc"]
    hdrl = [t for t in top if t[0] == b"LIST" and data[t[1]:t[1] + 4] == b"hdrl"][0]
    avih = struct.unpack("<14I", data[hdrl[1] + 12:hdrl[1] + 12 + 56])
    assert avih[4] == len(frames)
    return frames


def test_render_frames_to_video_end_to_end(tmp_path):
    from test_gpu_render import smpl_scene
    n_frames = 8
    _, faces, colors, h, model, sp, tv, tf = smpl_scene(n_frames)
    recon = {"poses": sp["pose"], "betas": sp["betas"], "trans": sp["trans"], "obj_angles": sp["obj_R"].transpose(0, 2, 1),
             "obj_trans": sp["obj_t"], "obj_scales": np.ones(n_frames, np.float32)}
    c, s = np.cos(0.35), np.sin(0.35)
    R2 = np.array([[c, 0, -s], [0, 1, 0], [s, 0, c]])
    kin = V.KinectTransform(world2local_R=[np.eye(3), np.eye(3), R2], world2local_t=[np.zeros(3), np.zeros(3), np.array([0.8, 0, 0.3])])
    r = V.RendererSide2side(image_size=1200)
    rgb_img = photo(1536, 2048, seed=11)
    host = np.concatenate(list(r.render_frames([recon], tv, tf, h, kin, rgb=lambda i: rgb_img, chunk=5)))
    assert host.shape == (n_frames, 900, 2160, 3)
    dev_chunks = list(r.render_frames([recon], tv, tf, h, kin, rgb=lambda i: rgb_img, chunk=5, on_device=True))
    assert all(isinstance(ch, torch.Tensor) and ch.is_cuda and ch.dtype == torch.uint8 for ch in dev_chunks)
    assert np.array_equal(torch.cat(dev_chunks).cpu().numpy(), host)
    p1, n1 = VID.write_video(iter(dev_chunks), str(tmp_path / "dev.avi"), fps=30, quality=90)
    assert n1 == n_frames
    frames = avi_frames(p1)
    assert len(frames) == n_frames
    worst = 1e9
    for k, jpg in enumerate(frames):
        dec = pil_decode(jpg)
        assert dec.shape == (900, 2160, 3)
        worst = min(worst, psnr(dec, host[k]))
    print(f"step-7 frames at q90 4:2:0: worst PSNR {worst:.2f} dB, {np.mean([len(f) for f in frames]) / 1e3:.0f} kB per frame")
    assert worst >= PSNR_BAR, worst
    check_stream(frames[3], host[3], 90, "420")
    # the host chunks give the same file; so does SequencePipeline.render(video=...)
    p2, _ = VID.write_video([host[:5], host[5:]], str(tmp_path / "host.avi"), fps=30, quality=90)
    assert open(p1, "rb").read() == open(p2, "rb").read()
    from vistracker_amd.pipeline import SequencePipeline
    fake = SimpleNamespace(device="cuda:0", ctx=SimpleNamespace(smpl=h))
    p3 = SequencePipeline.render(fake, {"recon": recon}, kin, rgb=lambda i: rgb_img, template=(tv, tf), chunk=5, video=str(tmp_path / "pipe.avi"))
    assert p3 == str(tmp_path / "pipe.avi") and open(p3, "rb").read() == open(p1, "rb").read()


# ---- errors ------------------------------------------------------------------------------------------------------------------------------------
def test_errors(tmp_path):
    enc = VID.JpegEncoder(16, 24, 90)
    with pytest.raises(L.VtError):
        enc.encode(torch.zeros(1, 16, 24, 3, dtype=torch.uint8))               # CPU tensor
    with pytest.raises(TypeError):
        enc.encode(torch.zeros(1, 16, 24, 3, device="cuda"))                   # float
    with pytest.raises(ValueError):
        enc.encode(torch.zeros(1, 16, 25, 3, dtype=torch.uint8, device="cuda"))
    for q in (0, 101):
        with pytest.raises(ValueError):
            VID.JpegEncoder(16, 24, q)
        with pytest.raises(ValueError):
            VID.write_video([np.zeros((1, 16, 24, 3), np.uint8)], str(tmp_path / "q.avi"), quality=q)
    assert not (tmp_path / "q.avi").exists()
    with pytest.raises(TypeError):
        VID.write_video([np.zeros((1, 16, 24, 3), np.float32)], str(tmp_path / "f.avi"))
    assert not (tmp_path / "f.avi").exists()
    # a workspace one byte short: VT_ERR_ARG before anything runs, the host buffer and the offsets untouched
    fr = torch.full((2, 16, 24, 3), 7, dtype=torch.uint8, device="cuda")
    enc._buffers(2)
    need = enc.ws.numel()
    full = L.lib().vt_jpeg_workspace_bytes(2, 16, 24, 420, None)
    enc.host.fill_(0xAB)
    import ctypes as C
    offs = np.full(3, -5, np.int64)
    rc = L.lib().vt_jpeg_encode(fr.data_ptr(), 2, 16, 24, fr.stride(0), fr.stride(1), 90, 420, L.dptr(enc.ws), full - 1, enc.host.data_ptr(),
                                enc.host.numel(), offs.ctypes.data_as(C.POINTER(C.c_longlong)), L.stream_ptr())
    assert rc == L.VT_ERR_ARG and b"workspace" in L.lib().vt_last_error()
    assert (offs == -5).all() and bool((enc.host == 0xAB).all())
    rc = L.lib().vt_jpeg_encode(fr.data_ptr(), 2, 16, 24, fr.stride(0), fr.stride(1), 90, 420, L.dptr(enc.ws), need, enc.host.data_ptr(),
                                10, offs.ctypes.data_as(C.POINTER(C.c_longlong)), L.stream_ptr())
    assert rc == L.VT_ERR_ARG and b"output buffer" in L.lib().vt_last_error()
    with pytest.raises(L.VtError):
        enc.encode_raw(fr, ws_bytes=full - 1)
    assert L.lib().vt_jpeg_workspace_bytes(1, 0, 8, 420, None) < 0
    assert L.lib().vt_jpeg_workspace_bytes(1, 8, 8, 422, None) < 0

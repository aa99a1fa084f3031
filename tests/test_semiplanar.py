"""Semi-planar front end: nv12 / nv21 / p010le / nv16 / nv24 / nv42 sources.  What the reference tool chain does with
them before encode2(): libavutil/pixdesc.c:2838-2873 picks yuv444p* of the same depth; libswscale's input readers
de-interleave the chroma pairs (input.c:686-698) and for P010 shift every sample right by 6 (input.c:700-726); then
the yuv420p* / yuv422p* path runs, or for nv24 / nv42 the exact unscaled de-interleave (swscale_unscaled.c:1926-1930).
PARITY UNPINNED: no libswscale binary or vector exists in this environment; the HIP kernels are held to the numpy
restatement below, which reduces every format to the planar 4:2:0 oracle / tests/sws422.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.sws422 import sws_422_to_444

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAME_PINNED, FRAME_YUV420, FRAME_REGISTER, FRAME_YUV422, FRAME_NV, FRAME_NV_VU = 1, 2, 4, 8, 16, 32
# name -> (flags, depth, subsampling, V first)
FMTS = {
    "nv12": (FRAME_NV | FRAME_YUV420, 8, 420, False), "nv21": (FRAME_NV | FRAME_NV_VU | FRAME_YUV420, 8, 420, True),
    "p010le": (FRAME_NV | FRAME_YUV420, 10, 420, False), "nv16": (FRAME_NV | FRAME_YUV422, 8, 422, False),
    "nv24": (FRAME_NV, 8, 444, False), "nv42": (FRAME_NV | FRAME_NV_VU, 8, 444, True),
}
FMT444 = {8: "yuv444p", 10: "yuv444p10le"}
PIX444 = {8: 5, 10: 70}


def chroma_shape(fmt, h, w):
    sub = FMTS[fmt][2]
    cw = w if sub == 444 else (w + 1) // 2
    ch = (h + 1) // 2 if sub == 420 else h
    return ch, cw


def nv_frame(fmt, seed, h, w, kind="noise"):
    """(Y (h, w), chroma (ch, 2 * cw)) of a semi-planar frame.  p010le samples carry random low 6 bits."""
    rng = np.random.default_rng(seed)
    depth = FMTS[fmt][1]
    dt = np.uint8 if depth == 8 else np.dtype("<u2")
    ch, cw = chroma_shape(fmt, h, w)
    if kind == "noise":
        y = rng.integers(0, 1 << depth, (h, w))
        uv = rng.integers(0, 1 << depth, (ch, 2 * cw))
    else:
        yy, xx = np.mgrid[0:ch, 0:2 * cw]
        y = rng.integers(0, 1 << depth, (h, w))
        uv = (3 * (xx >> 1) + 5 * yy + 97 * (xx & 1) + seed) % (1 << depth)
    if depth == 10:                                                # P010: 10 bits at the top, garbage below
        y = (y << 6) | rng.integers(0, 64, y.shape)
        uv = (uv << 6) | rng.integers(0, 64, uv.shape)
    return y.astype(dt), uv.astype(dt)


def restate(oracle, y, uv, fmt):
    """numpy restatement: de-interleave (plus >> 6 for P010), then the planar path -> (3, h, w) yuv444p* samples."""
    _, depth, sub, vu = FMTS[fmt]
    y, uv = np.asarray(y), np.asarray(uv)
    u, v = uv[:, 0::2], uv[:, 1::2]
    if vu:
        u, v = v, u
    if fmt == "p010le":
        y, u, v = y >> 6, u >> 6, v >> 6
    if sub == 420:
        return oracle.sws_420_to_444(y, u, v, depth)
    if sub == 422:
        return sws_422_to_444(oracle, y, u, v, depth)
    return np.stack([y, u, v])


@pytest.fixture(scope="module")
def lib():
    from ffmpeg_ffv2_amd import _lib, build
    build.build()
    lib = _lib.load()
    lib.ffv2amd_codec_encode_nv.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint, C.c_void_p]
    lib.ffv2amd_ring_send.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_ssize_t), C.c_void_p, C.c_int64, C.c_uint]
    lib.ffv2amd_qpring_send.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_ssize_t), C.c_void_p, C.c_int64, C.c_uint]
    return lib


# ---- CPU ----
BAD_FLAGS = [0, FRAME_NV_VU, FRAME_NV_VU | FRAME_YUV420, FRAME_NV | FRAME_YUV420 | FRAME_YUV422,
             FRAME_NV | FRAME_NV_VU | FRAME_YUV420 | FRAME_YUV422]


def test_library_exports_and_argument_checks(lib):
    """The semi-planar entry points exist and refuse NULL, bad arguments and bad flag combinations before touching
    a device."""
    for name in ("ffv2amd_frame_bytes_nv", "ffv2amd_convert_nv_device", "ffv2amd_encode_frame_nv",
                 "ffv2amd_qp_send_frame_nv", "ffv2amd_debug_nv_time", "ffv2amd_codec_encode_nv"):
        assert hasattr(lib, name), name
    buf = (C.c_uint8 * 64)()
    data = (C.c_void_p * 4)(C.addressof(buf), C.addressof(buf), None, None)
    ls = (C.c_ssize_t * 4)(8, 8, 0, 0)
    n = C.c_size_t(0)
    ms = C.c_float(0)
    p = C.addressof(buf)
    for flags in [f for f, *_ in FMTS.values()] + BAD_FLAGS:
        assert lib.ffv2amd_frame_bytes_nv(None, flags) == 0
        assert lib.ffv2amd_convert_nv_device(None, 1, p, 8, p, 8, 0, flags, p, None) == -22
        assert lib.ffv2amd_encode_frame_nv(None, data, ls, flags, 0, p, 64, C.byref(n)) == -22
        assert lib.ffv2amd_qp_send_frame_nv(None, data, ls, flags, 16, 0) == -22
        assert lib.ffv2amd_debug_nv_time(None, 1, p, 8, p, 8, 0, flags, p, 1, C.byref(ms)) == -22
        assert lib.ffv2amd_ring_send(None, data, ls, None, 0, flags) == -22
        assert lib.ffv2amd_qpring_send(None, data, ls, None, 0, flags) == -22
        assert lib.ffv2amd_codec_encode_nv(None, None, None, flags, None) == -22
    assert lib.ffv2amd_encode_frame_nv(None, None, None, FRAME_NV, 0, None, 0, None) == -22
    assert lib.ffv2amd_convert_nv_device(None, 0, None, 0, None, 0, 0, FRAME_NV, None, None) == -22
    # the shim refuses the bad combinations before looking at its context
    from tests.codec_ctypes import Ctx
    ctx = Ctx()
    for flags in (FRAME_NV_VU, FRAME_NV | FRAME_YUV420 | FRAME_YUV422):
        assert lib.ffv2amd_codec_send_frame(C.byref(ctx), None, flags) == -22


def test_python_format_names_map_to_flags():
    from ffmpeg_ffv2_amd.encoder import NV_FORMATS
    assert set(NV_FORMATS) == set(FMTS)
    for name, (flags, depth, _, _) in FMTS.items():
        assert NV_FORMATS[name] == (flags, depth), name


@pytest.mark.parametrize("fmt", ["nv12", "nv21", "p010le", "nv16"])
def test_restatement_is_the_planar_path_on_deinterleaved_planes(oracle, fmt):
    _, depth, sub, vu = FMTS[fmt]
    h, w = 37, 51
    y, uv = nv_frame(fmt, 3, h, w)
    got = restate(oracle, y, uv, fmt)
    sh = 6 if fmt == "p010le" else 0
    a, b = (uv[:, 0::2] >> sh), (uv[:, 1::2] >> sh)
    u, v = (b, a) if vu else (a, b)
    want = oracle.sws_420_to_444(y >> sh, u, v, depth) if sub == 420 else sws_422_to_444(oracle, y, u, v, depth)
    assert (got == want).all()
    assert got.max() < (1 << depth)


def test_restatement_ignores_p010_low_bits(oracle):
    y, uv = nv_frame("p010le", 9, 30, 44)
    base = restate(oracle, y, uv, "p010le")
    rng = np.random.default_rng(1)
    y2 = (y & 0xffc0) | rng.integers(0, 64, y.shape).astype(y.dtype)
    uv2 = (uv & 0xffc0) | rng.integers(0, 64, uv.shape).astype(uv.dtype)
    assert (y2 != y).any() and (uv2 != uv).any()
    assert (restate(oracle, y2, uv2, "p010le") == base).all()
    assert (restate(oracle, y & 0xffc0, uv & 0xffc0, "p010le") == base).all()


@pytest.mark.parametrize("fmt", ["nv24", "nv42"])
def test_nv24_is_an_exact_deinterleave(oracle, fmt):
    y, uv = nv_frame(fmt, 4, 9, 13)
    out = restate(oracle, y, uv, fmt)
    first, second = (2, 1) if fmt == "nv42" else (1, 2)
    assert (out[0] == y).all()
    for x in range(13):
        assert (out[first][:, x] == uv[:, 2 * x]).all() and (out[second][:, x] == uv[:, 2 * x + 1]).all()


# ---- GPU ----
def _enc(w, h, depth, **kw):
    from ffmpeg_ffv2_amd import FFV2Encoder
    return FFV2Encoder(w, h, FMT444[depth], device=0, **kw)


CASES = [(240, 320), (128, 192), (130, 200), (65, 129), (37, 51), (16, 16), (1080, 1920)]
NARROW = [(1 + w % 7, w) for w in range(1, 17)] + [(1, 40), (7, 3), (2, 1), (5, 33)]


def _pitched(torch, y, uv, nframes_src, pad_y, pad_uv, sentinel):
    """nframes_src frames in ONE device allocation per frame slot: [Y rows (pitch y_pitch)][chroma rows (uv_pitch)]
    [tail], every padding byte the sentinel; returns (y view (F,h,w), uv view (F,ch,2cw), the whole buffer)."""
    F = len(nframes_src)
    isz = y.dtype.itemsize
    h, w = y.shape
    ch, c2 = uv.shape
    yp, up = w + pad_y, c2 + pad_uv                                 # samples per row
    per = yp * h + up * ch + 24                                     # samples per frame (tail padding too)
    host = np.full((F, per), sentinel, y.dtype)
    for f, (yy, cc) in enumerate(nframes_src):
        host[f, : yp * h].reshape(h, yp)[:, :w] = yy
        host[f, yp * h: yp * h + up * ch].reshape(ch, up)[:, :c2] = cc
    tdt = torch.uint8 if isz == 1 else torch.int16
    buf = torch.from_numpy(host.view(np.uint8 if isz == 1 else np.int16)).to("cuda:0")
    yv = buf[:, : yp * h].unflatten(1, (h, yp))[:, :, :w]
    uvv = buf[:, yp * h: yp * h + up * ch].unflatten(1, (ch, up))[:, :, :c2]
    assert yv.dtype == tdt
    return yv, uvv, buf


@pytest.mark.gpu
@pytest.mark.parametrize("fmt,naive", [(f, False) for f in FMTS] + [("nv16", True)])
def test_convert_nv_device_matches_restatement(oracle, monkeypatch, fmt, naive):
    """Pitched sources (padding full of a sentinel that must not leak), batches of 3 frames with a frame stride,
    P010 with random low bits, the geometries of test_upconv422, narrow widths and heights below 8.  naive: nv16
    through the 4:2:2 per-sample fallback (the 4:2:0 one: test_convert_nv420_fallback_kernel_in_a_child)."""
    import torch
    if naive:
        monkeypatch.setenv("FFV2AMD_UPCONV422_NAIVE", "1")        # read per launch
    depth = FMTS[fmt][1]
    for h, w in CASES + NARROW:
        enc = _enc(w, h, depth)
        src = [nv_frame(fmt, h * w + f, h, w, "noise" if f % 2 else "ramp") for f in range(3)]
        sentinel = 0xA5 if depth == 8 else 0xFFFF
        yv, uvv, _ = _pitched(torch, src[0][0], src[0][1], src, 13, 70, sentinel)
        got = enc.unpack_frames(enc.convert_nv(yv, uvv, fmt).cpu().numpy())
        for f in range(3):
            want = restate(oracle, *src[f], fmt)
            bad = np.argwhere(got[f] != want)
            assert len(bad) == 0, "%s %s frame %d: first mismatch at (plane, y, x) = %s: %d vs %d" % (
                fmt, (h, w), f, bad[0], got[f][tuple(bad[0])], want[tuple(bad[0])])
        enc.close()


@pytest.mark.gpu
def test_convert_nv420_fallback_kernel_in_a_child():
    """FFV2AMD_UPCONV_NAIVE=1 (read once per process) sends nv12 / nv21 / p010le through the per-sample kernel."""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from tests import oracle_lib\n"
            "from tests.test_semiplanar import _check_small\n"
            "_check_small(oracle_lib.load())\n") % ROOT
    env = dict(os.environ, FFV2AMD_UPCONV_NAIVE="1")
    r = subprocess.run(["timeout", "-k", "10", "600", os.sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "checked" in r.stdout


def _check_small(oracle):
    import torch
    for fmt in ("nv12", "nv21", "p010le"):
        depth = FMTS[fmt][1]
        for h, w in [(65, 129), (37, 51), (16, 16)] + NARROW[::3]:
            enc = _enc(w, h, depth)
            src = [nv_frame(fmt, h + w + f, h, w) for f in range(3)]
            yv, uvv, _ = _pitched(torch, src[0][0], src[0][1], src, 5, 18, 0x5A if depth == 8 else 0xFFC0)
            got = enc.unpack_frames(enc.convert_nv(yv, uvv, fmt).cpu().numpy())
            for f in range(3):
                assert (got[f] == restate(oracle, *src[f], fmt)).all(), (fmt, h, w, f)
            enc.close()
    print("checked")


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", list(FMTS))
def test_encode_frame_nv_equals_convert_then_encode(oracle, fmt):
    depth = FMTS[fmt][1]
    h, w = 136, 200
    enc = _enc(w, h, depth)
    # a strided host frame (rows of a larger buffer)
    y, uv = nv_frame(fmt, 2, h, w)
    want = oracle.encode(restate(oracle, y, uv, fmt), FMT444[depth])
    big_y = np.zeros((h, w + 40), y.dtype); big_y[:, :w] = y
    big_uv = np.zeros((uv.shape[0], uv.shape[1] + 20), uv.dtype); big_uv[:, : uv.shape[1]] = uv
    assert enc.encode2_nv(big_y[:, :w], big_uv[:, : uv.shape[1]], fmt) == want
    for seed, qp in ((0, 0), (1, 16)):
        y, uv = nv_frame(fmt, seed, h, w, "ramp")
        conv = restate(oracle, y, uv, fmt)
        try:
            want = oracle.encode(conv, FMT444[depth], qp=qp)
        except RuntimeError:                                       # the reference would abort on this frame
            with pytest.raises(Exception):
                enc.encode2_nv(y, uv, fmt, qp=qp)
            continue
        assert enc.encode2_nv(y, uv, fmt, qp=qp) == want, (fmt, qp)
    enc.close()


@pytest.mark.gpu
def test_nv_names_must_match_the_encoder(lib):
    from ffmpeg_ffv2_amd import FFV2Encoder
    from ffmpeg_ffv2_amd._lib import FFV2Error
    e8, e10, e12 = FFV2Encoder(64, 48, "yuv444p"), FFV2Encoder(64, 48, "yuv444p10le"), FFV2Encoder(64, 48, "yuv444p12le")
    for enc, bad in ((e8, ["p010le"]), (e10, ["nv12", "nv21", "nv16", "nv24", "nv42"]), (e12, list(FMTS))):
        for fmt in bad:
            with pytest.raises(FFV2Error) as ei:
                enc.nv_flags(fmt)
            assert ei.value.code == -22
    # the C-ABI itself: the depth picks the layout; everything else is EINVAL
    z = np.zeros((48, 128), np.uint16)
    data = (C.c_void_p * 4)(z.ctypes.data, z.ctypes.data, None, None)
    ls = (C.c_ssize_t * 4)(256, 256, 0, 0)
    out = np.zeros(1 << 16, np.uint8)
    n = C.c_size_t(0)
    for enc, flags in ((e8, FRAME_NV | FRAME_NV_VU | FRAME_YUV422), (e10, FRAME_NV | FRAME_NV_VU | FRAME_YUV420),
                       (e10, FRAME_NV | FRAME_YUV422), (e10, FRAME_NV), (e12, FRAME_NV | FRAME_YUV420),
                       (e8, FRAME_NV_VU | FRAME_YUV420), (e8, FRAME_NV | FRAME_YUV420 | FRAME_YUV422)):
        assert lib.ffv2amd_frame_bytes_nv(enc._h, flags) == 0, flags
        assert lib.ffv2amd_encode_frame_nv(enc._h, data, ls, flags, 0, out.ctypes.data, out.size, C.byref(n)) == -22, flags
        assert lib.ffv2amd_convert_nv_device(enc._h, 1, 256, 256, 256, 256, 0, flags, 256, None) == -22, flags
    assert lib.ffv2amd_frame_bytes_nv(e8._h, FRAME_NV | FRAME_YUV420) == 64 * 48 + 64 * 24
    assert lib.ffv2amd_frame_bytes_nv(e10._h, FRAME_NV | FRAME_YUV420) == 2 * (64 * 48 + 64 * 24)
    assert lib.ffv2amd_frame_bytes_nv(e8._h, FRAME_NV) == 3 * 64 * 48
    e8.ring_open(1)
    with pytest.raises(FFV2Error):
        e8.ring_send_nv(np.zeros((48, 64), np.uint8), np.zeros((24, 64), np.uint8), "p010le")
    assert lib.ffv2amd_ring_send(e8._h, data, ls, None, 0, FRAME_NV_VU) == -22
    e8.ring_close()
    g = FFV2Encoder(64, 48, "gbrp")
    assert lib.ffv2amd_frame_bytes_nv(g._h, FRAME_NV | FRAME_YUV420) == 0
    for e in (e8, e10, e12, g):
        e.close()


@pytest.mark.gpu
def test_ring_mixes_444_420_nv12_and_p010(oracle):
    """A 10-bit ring gets 4:4:4, yuv420p10le and p010le frames, an 8-bit ring 4:4:4, yuv420p, nv12, nv21, nv16 and
    nv24 frames: pinned, pageable and FFV2AMD_FRAME_REGISTER memory, packets in send order, each the oracle's."""
    from ffmpeg_ffv2_amd import frames as synth
    W, H = 640, 480
    for depth, nvs in ((10, ["p010le"]), (8, ["nv12", "nv21", "nv16", "nv24", "nv42"])):
        fmt = FMT444[depth]
        enc = _enc(W, H, depth)
        enc.ring_open(3)
        rng = np.random.default_rng(8)
        dt = np.uint8 if depth == 8 else np.dtype("<u2")
        f444 = synth.make("S2", 1, 3, H, W, depth)
        f420 = [rng.integers(0, 1 << depth, s).astype(dt) for s in ((H, W), (H // 2, W // 2), (H // 2, W // 2))]
        sends = [("444", f444, {}), ("420", f420, {})]
        for k, nvf in enumerate(nvs):
            a, b = nv_frame(nvf, 40 + k, H, W, "ramp"), nv_frame(nvf, 50 + k, H, W)
            pin = enc.pinned_frames_nv(1, nvf)[0]
            pin[0][:] = b[0]; pin[1][:] = b[1]
            sends += [(nvf, a, {}), (nvf, pin, {"pinned": True}), (nvf, b, {"register": True}), ("444", f444, {}),
                      (nvf, a, {"register": True})]
        want = {"444": oracle.encode(f444, fmt), "420": oracle.encode(oracle.sws_420_to_444(*f420, depth), fmt)}
        got, wanted = [], []
        for t, (kind, fr, kw) in enumerate(sends):
            if kind == "444":
                send = lambda: enc.ring_send(fr, tag=t)                # noqa: E731
                wanted.append(want["444"])
            elif kind == "420":
                send = lambda: enc.ring_send_420(*fr, tag=t)           # noqa: E731
                wanted.append(want["420"])
            else:
                send = lambda: enc.ring_send_nv(*fr, kind, tag=t, **kw)   # noqa: E731
                wanted.append(oracle.encode(restate(oracle, *fr, kind), fmt))
            while not send():
                got.append(enc.ring_receive())
        while enc.ring_pending():
            got.append(enc.ring_receive())
        assert [g[0] for g in got] == list(range(len(sends)))
        for t, (tag, pk) in enumerate(got):
            assert pk == wanted[t], (depth, t, sends[t][0])
        enc.ring_close()
        enc.free_pinned()
        enc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 10])
def test_qpring_batch_mixes_all_chroma_kinds(oracle, depth):
    from ffmpeg_ffv2_amd import frames as synth
    from tests.sws422 import yuv422
    W, H, qp = 200, 136, 16
    fmt = FMT444[depth]
    enc = _enc(W, H, depth)
    enc.qpring_open(qp, 4)
    rng = np.random.default_rng(6)
    dt = np.uint8 if depth == 8 else np.dtype("<u2")
    ch, cw = (H + 1) // 2, (W + 1) // 2
    nvs = ["nv12", "nv21", "nv16", "nv24", "nv42"] if depth == 8 else ["p010le"]
    sends = [("444", synth.make("S1", 2, 3, H, W, depth)), (nvs[0], nv_frame(nvs[0], 1, H, W, "ramp")),
             ("420", [rng.integers(0, 1 << depth, s).astype(dt) for s in ((H, W), (ch, cw), (ch, cw))]),
             ("422", yuv422(3, H, W, depth, "ramp"))]
    sends += [(f, nv_frame(f, 10 + k, H, W, "ramp")) for k, f in enumerate(nvs)]
    sends += [(nvs[-1], nv_frame(nvs[-1], 30, H, W, "ramp")), ("444", synth.make("S2", 3, 3, H, W, depth))]
    for t, (kind, fr) in enumerate(sends):
        assert enc.qpring_send(fr, tag=t, yuv420=kind == "420", yuv422=kind == "422",
                               nv=kind if kind in FMTS else None)
    assert enc.qpring_flush()
    for t, (kind, fr) in enumerate(sends):
        conv = (fr if kind == "444" else sws_422_to_444(oracle, *fr, depth) if kind == "422"
                else oracle.sws_420_to_444(*fr, depth) if kind == "420" else restate(oracle, *fr, kind))
        try:
            want = oracle.encode(conv, fmt, qp=qp)
        except RuntimeError:
            want = None
        if want is None:
            with pytest.raises(Exception):
                enc.qpring_receive()
            continue
        assert enc.qpring_receive() == (t, want), (t, kind)
    enc.qpring_close()
    enc.close()


def _drive(lib, ctx, frames, flags):
    from tests.codec_ctypes import Packet, frame_of
    out, sent = [], 0
    while len(out) < len(frames):
        while sent < len(frames):
            r = lib.ffv2amd_codec_send_frame(C.byref(ctx), C.byref(frame_of(frames[sent], 500 + sent)), flags)
            if r == -11:
                break
            assert r == 0, r
            sent += 1
        if sent == len(frames):
            assert lib.ffv2amd_codec_send_frame(C.byref(ctx), None, 0) in (0, -11)
        pkt = Packet()
        r = lib.ffv2amd_codec_receive_packet(C.byref(ctx), C.byref(pkt), 1)
        if r == -11:
            continue
        if r < 0:
            out.append((None, r))
            continue
        out.append((pkt.pts, bytes(pkt.data[: pkt.size])))
        lib.ffv2amd_packet_unref(C.byref(pkt))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("devices", [None, [0, 0]])
@pytest.mark.parametrize("qp,per_call", [(0, 0), (16, 0), (16, 3)])
@pytest.mark.parametrize("fmt", ["nv12", "p010le", "nv42"])
def test_nv_frames_through_send_frame(oracle, lib, devices, qp, per_call, fmt):
    from tests.codec_ctypes import make_ctx
    W, H = 322, 130
    flags, depth = FMTS[fmt][0], FMTS[fmt][1]
    src = [nv_frame(fmt, 70 + n, H, W, "noise" if n % 2 else "ramp") for n in range(5)]
    ctx = make_ctx(W, H, PIX444[depth], qp=qp, ring_depth=2, devices=devices, qp_frames_per_call=per_call)
    assert lib.ffv2amd_codec_init(C.byref(ctx)) == 0
    got = _drive(lib, ctx, src, flags)
    for n, (pts, pk) in enumerate(got):
        try:
            want = (500 + n, oracle.encode(restate(oracle, *src[n], fmt), FMT444[depth], qp=qp))
        except RuntimeError:
            want = (None, -1)
        assert (pts, pk) == want, n
    assert lib.ffv2amd_codec_close(C.byref(ctx)) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("fmt,h,w", [("p010le", 2160, 3840), ("nv12", 1080, 1920)])
def test_ring_nv_full_size(oracle, fmt, h, w):
    """3840x2160 P010 and 1920x1080 NV12 through the ring; the converted picture is also held sample by sample to the
    restatement."""
    import torch
    depth = FMTS[fmt][1]
    enc = _enc(w, h, depth)
    y, uv = nv_frame(fmt, 3, h, w, "ramp")
    rng = np.random.default_rng(5)
    uv[: h // 8] = (rng.integers(0, 1 << 16, uv[: h // 8].shape)).astype(uv.dtype)
    want444 = restate(oracle, y, uv, fmt)
    tdt = torch.uint8 if depth == 8 else torch.int16
    dy = torch.from_numpy(y.view(np.uint8 if depth == 8 else np.int16)).to("cuda:0")
    duv = torch.from_numpy(uv.view(np.uint8 if depth == 8 else np.int16)).to("cuda:0")
    assert dy.dtype == tdt
    got444 = enc.unpack_frames(enc.convert_nv(dy, duv, fmt).cpu().numpy())[0]
    bad = np.argwhere(got444 != want444)
    assert len(bad) == 0, "first mismatch at (plane, y, x) = %s" % (bad[0],)
    enc.ring_open(2)
    assert enc.ring_send_nv(y, uv, fmt, tag=7)
    tag, pk = enc.ring_receive()
    assert tag == 7 and pk == oracle.encode(want444, FMT444[depth])
    enc.ring_close()
    enc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["nv12", "p010le", "nv24"])
def test_strided_torch_surfaces_through_encode_batch_device(oracle, fmt):
    """Decoder-style surfaces: Y and chroma rows padded, frames one allocation apart, as strided torch views ->
    convert_nv -> encode_batch_device -> the oracle's packets."""
    import torch
    h, w = 136, 200
    depth = FMTS[fmt][1]
    enc = _enc(w, h, depth, max_batch=4)
    src = [nv_frame(fmt, 20 + f, h, w, "ramp") for f in range(4)]
    yv, uvv, _ = _pitched(torch, src[0][0], src[0][1], src, 56, 24, 0x33)
    assert not yv.is_contiguous() and not uvv.is_contiguous()
    frames = enc.convert_nv(yv, uvv, fmt)
    pk = enc.collect(*enc.encode_batch_device(frames))
    for f in range(4):
        assert pk[f] == oracle.encode(restate(oracle, *src[f], fmt), FMT444[depth]), f
    enc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["nv12", "p010le", "nv16", "nv42"])
def test_cli_nv_sync_and_async_match_python(tmp_path, fmt):
    subprocess.run(["make", "-s", "-C", ROOT, "examples/ffv2enc_cli"], check=True)
    cli = os.path.join(ROOT, "examples", "ffv2enc_cli")
    W, H = 320, 240
    depth = FMTS[fmt][1]
    src = [nv_frame(fmt, n, H, W, "ramp") for n in range(4)]
    raw = tmp_path / ("in.%s" % fmt)
    raw.write_bytes(b"".join(p.tobytes() for f in src for p in f))
    enc = _enc(W, H, depth)
    for qp in (0, 16):
        want = []
        for f in src:
            try:
                want.append(enc.encode2_nv(*f, fmt, qp=qp))
            except Exception:
                want = None
                break
        if want is None:
            continue
        want = b"".join(want)
        for extra in ([], ["--async", "3"]):
            out = tmp_path / ("out%d_%d.ffv2" % (qp, len(extra)))
            r = subprocess.run(["timeout", "-k", "10", "300", cli, str(W), str(H), fmt, str(raw), str(out), str(qp), "0"] + extra,
                               capture_output=True, text=True)
            assert r.returncode == 0, r.stderr
            assert out.read_bytes() == want and len(want) > 0, (qp, extra)
    enc.close()
    r = subprocess.run([cli, str(W), str(H), fmt, str(raw), str(tmp_path / "x.ffv2"), "--no-convert"],
                       capture_output=True, text=True)
    assert r.returncode == 2

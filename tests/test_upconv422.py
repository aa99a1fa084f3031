"""4:2:2 -> 4:4:4 front end: what the reference tool chain does in front of encode2() for yuv422p / yuv422p10le /
yuv422p12le sources (libavutil/pixdesc.c:2838-2873 picks yuv444p* of the same depth; libswscale's generic scaler:
chroma 2x up along x with the 4:2:0 path's bicubic, unscaled along y -- utils.c:303-310,353-362, output.c:320-330,
395-403).  PARITY UNPINNED: no libswscale binary or vector exists in this environment; the HIP kernel is checked
against tests/sws422.py, a numpy restatement that is itself tied to oracle.sws_420_to_444."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.sws422 import chroma_422_to_444, dtype_of, sws_422_to_444, yuv422

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMT444 = {8: "yuv444p", 10: "yuv444p10le", 12: "yuv444p12le"}
PIX444 = {8: 5, 10: 70, 12: 133}
FRAME_PINNED, FRAME_YUV420, FRAME_REGISTER, FRAME_YUV422 = 1, 2, 4, 8


@pytest.fixture(scope="module")
def lib():
    from ffmpeg_ffv2_amd import _lib, build
    build.build()
    lib = _lib.load()
    lib.ffv2amd_codec_encode_yuv422.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


# ---- the restatement against the 4:2:0 oracle (CPU) ----
@pytest.mark.parametrize("depth", [8, 10, 12])
@pytest.mark.parametrize("kind", ["noise", "ramp", "full16"])
def test_restatement_is_every_row_of_the_420_oracle_on_chroma_constant_along_y(oracle, depth, kind):
    """initFilter normalises every vertical row to 4096: fed chroma that is the same in every row, the 4:2:0
    path's output rows are all the 4:2:2 result of that row."""
    dt = dtype_of(depth)
    for w in list(range(8, 18)) + [51, 129, 1920, 3840]:
        _, u, v = yuv422(w * 7 + depth, 3, w, depth, kind)
        want_u, want_v = chroma_422_to_444(oracle, u, w, depth), chroma_422_to_444(oracle, v, w, depth)
        h420 = 6
        for r in range(u.shape[0]):
            uu = np.repeat(u[r: r + 1], (h420 + 1) // 2, 0)
            vv = np.repeat(v[r: r + 1], (h420 + 1) // 2, 0)
            out = oracle.sws_420_to_444(np.zeros((h420, w), dt), uu, vv, depth)
            assert (out[1] == want_u[r]).all() and (out[2] == want_v[r]).all(), (w, r)


@pytest.mark.parametrize("depth", [8, 10, 12])
def test_restatement_luma_identity_and_flat_chroma(oracle, depth):
    y, u, v = yuv422(3, 37, 50, depth)
    u[:] = 77 % (1 << depth)
    v[:] = (1 << depth) - 1
    out = sws_422_to_444(oracle, y, u, v, depth)
    assert out.shape == (3, 37, 50) and out.dtype == dtype_of(depth)
    assert (out[0] == y).all()
    assert (out[1] == u[0, 0]).all() and (out[2] == (1 << depth) - 1).all()      # flat stays flat, no overshoot


def test_library_exports_and_argument_checks(lib):
    """The 4:2:2 entry points exist and refuse NULL or bad arguments before touching a device."""
    for name in ("ffv2amd_frame_bytes_422", "ffv2amd_upconvert_422_device", "ffv2amd_encode_frame_422",
                 "ffv2amd_ring_send_422", "ffv2amd_qp_send_frame_422", "ffv2amd_codec_encode_yuv422"):
        assert hasattr(lib, name), name
    assert lib.ffv2amd_frame_bytes_422(None) == 0
    buf = (C.c_uint8 * 64)()
    data = (C.c_void_p * 3)(C.addressof(buf), C.addressof(buf), C.addressof(buf))
    ls = (C.c_ssize_t * 3)(8, 4, 4)
    n = C.c_size_t(0)
    assert lib.ffv2amd_upconvert_422_device(None, 1, C.addressof(buf), C.addressof(buf), None) == -22
    assert lib.ffv2amd_encode_frame_422(None, data, ls, 0, C.addressof(buf), 64, C.byref(n)) == -22
    assert lib.ffv2amd_ring_send_422(None, data, ls, None, 0, 0) == -22
    assert lib.ffv2amd_qp_send_frame_422(None, data, ls, 16, 0) == -22
    assert lib.ffv2amd_codec_encode_yuv422(None, None, None, None) == -22


# ---- HIP vs the restatement (GPU) ----
def _enc(w, h, depth, **kw):
    from ffmpeg_ffv2_amd import FFV2Encoder
    return FFV2Encoder(w, h, FMT444[depth], device=0, **kw)


CASES = [(8, 240, 320), (10, 128, 192), (12, 130, 200), (8, 65, 129), (10, 37, 51), (8, 16, 16), (12, 1080, 1920)]
# widths 8-16 (the 4:2:0 filter has fewer than 4 taps below 12) and heights below 8, every depth
NARROW = [((8, 10, 12)[w % 3], 1 + w % 7, w) for w in range(8, 17)] + [(10, 1, 40), (12, 7, 3), (8, 2, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("naive", [False, True], ids=["strips", "per-sample"])
@pytest.mark.parametrize("kind", ["noise", "ramp"])
def test_upconvert_422_matches_restatement(oracle, monkeypatch, naive, kind):
    if naive:
        monkeypatch.setenv("FFV2AMD_UPCONV422_NAIVE", "1")         # read per launch
    for depth, h, w in CASES + NARROW:
        enc = _enc(w, h, depth)
        y, u, v = yuv422(h * w + depth, h, w, depth, kind)
        got = enc.upconvert_422(y, u, v)
        want = sws_422_to_444(oracle, y, u, v, depth)
        bad = np.argwhere(got != want)
        assert len(bad) == 0, "%s: first mismatch at (plane, y, x) = %s: %d vs %d" % (
            (depth, h, w), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])
        enc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("depth,h,w", [(8, 240, 320), (10, 270, 480), (12, 135, 240)])
def test_encode_frame_422_equals_convert_then_encode(oracle, depth, h, w):
    """The literal yuv422p / 10le / 12le formats end to end at qp 0 and 16: host frame -> packet ==
    restated conversion followed by the oracle encoder."""
    fmt = FMT444[depth]
    enc = _enc(w, h, depth)
    for seed, qp in ((0, 0), (1, 16)):
        y, u, v = yuv422(seed, h, w, depth, "noise" if seed else "ramp")
        conv = sws_422_to_444(oracle, y, u, v, depth)
        try:
            want = oracle.encode(conv, fmt, qp=qp)
        except RuntimeError:                                       # the reference would abort on this frame
            with pytest.raises(Exception):
                enc.encode2_422(y, u, v, qp=qp)
            continue
        assert enc.encode2_422(y, u, v, qp=qp) == want, (seed, qp)
    if depth == 10:                                                # over-depth luma: the wide T-stage rerun
        y, u, v = yuv422(5, h, w, depth, "full16")
        assert enc.encode2_422(y, u, v) == oracle.encode(sws_422_to_444(oracle, y, u, v, depth), fmt)
    enc.close()


@pytest.mark.gpu
def test_422_front_end_needs_a_yuv444_encoder_and_one_chroma_flag(lib):
    from ffmpeg_ffv2_amd import FFV2Encoder
    from ffmpeg_ffv2_amd._lib import FFV2Error
    z = np.zeros((64, 64), np.uint8)
    c = np.zeros((64, 32), np.uint8)
    for fmt in ("gbrp", "gray"):
        enc = FFV2Encoder(64, 64, fmt, device=0)
        with pytest.raises(FFV2Error) as ei:
            enc.encode2_422(z, c, c)
        assert ei.value.code == -22
        with pytest.raises(FFV2Error) as ei:
            enc.upconvert_422(z, c, c)
        assert ei.value.code == -22
        enc.ring_open(1)
        with pytest.raises(FFV2Error) as ei:
            enc.ring_send_422(z, c, c)
        assert ei.value.code == -22
        enc.ring_close()
        enc.close()
    enc = FFV2Encoder(64, 64, "yuv444p", device=0)
    enc.qpring_open(16, 2)
    with pytest.raises(FFV2Error) as ei:
        enc.qpring_send((z, c, c), yuv420=True, yuv422=True)
    assert ei.value.code == -22
    enc.qpring_close()
    enc.close()
    from tests.codec_ctypes import frame_of, make_ctx
    ctx = make_ctx(64, 64, 5, ring_depth=2)
    assert lib.ffv2amd_codec_init(C.byref(ctx)) == 0
    assert lib.ffv2amd_codec_send_frame(C.byref(ctx), C.byref(frame_of((z, c, c), 0)), FRAME_YUV420 | FRAME_YUV422) == -22
    assert lib.ffv2amd_codec_close(C.byref(ctx)) == 0


@pytest.mark.gpu
def test_ring_mixes_422_420_and_444_frames(oracle):
    """ring_send_422 from pinned, pageable and pooled (FFV2AMD_FRAME_REGISTER) memory between ring_send and
    ring_send_420 frames on one ring: packets in send order, each the oracle's."""
    from ffmpeg_ffv2_amd import frames as synth
    W, H, depth = 640, 480, 10
    fmt = FMT444[depth]
    enc = _enc(W, H, depth)
    enc.ring_open(3)
    rng = np.random.default_rng(8)
    f444 = synth.make("S2", 1, 3, H, W, depth)
    f420 = [rng.integers(0, 1 << depth, s).astype("<u2") for s in ((H, W), (H // 2, W // 2), (H // 2, W // 2))]
    f422 = [yuv422(40 + n, H, W, depth, "noise" if n % 2 else "ramp") for n in range(4)]
    pin = enc.pinned_frames_422(1)
    for a, b in zip(pin[0], f422[1]):
        a[:] = b
    sends = [("422", f422[0], {}), ("444", f444, {}), ("422p", pin[0], {"pinned": True}),
             ("420", f420, {}), ("422", f422[2], {"register": True}), ("422", f422[3], {}), ("422", f422[2], {"register": True})]
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
            send = lambda: enc.ring_send_422(*fr, tag=t, **kw)     # noqa: E731
            wanted.append(oracle.encode(sws_422_to_444(oracle, *fr, depth), fmt))
        while not send():                                          # the ring is full: take a packet first
            got.append(enc.ring_receive())
    while enc.ring_pending():
        got.append(enc.ring_receive())
    assert [g[0] for g in got] == list(range(len(sends)))
    for t, (tag, pk) in enumerate(got):
        assert pk == wanted[t], (t, sends[t][0])
    enc.ring_close()
    enc.free_pinned()
    enc.close()


@pytest.mark.gpu
def test_qpring_batch_mixes_three_chroma_kinds(oracle):
    from ffmpeg_ffv2_amd import frames as synth
    W, H, depth, qp = 200, 136, 8, 16
    fmt = FMT444[depth]
    enc = _enc(W, H, depth)
    enc.qpring_open(qp, 4)
    rng = np.random.default_rng(6)
    ch, cw = (H + 1) // 2, (W + 1) // 2
    sends = [("422", yuv422(1, H, W, depth)), ("444", synth.make("S1", 2, 3, H, W, depth)),
             ("422", yuv422(3, H, W, depth, "ramp")), ("420", [rng.integers(0, 256, s).astype(np.uint8) for s in ((H, W), (ch, cw), (ch, cw))]),
             ("422", yuv422(4, H, W, depth)), ("422", yuv422(5, H, W, depth)), ("444", synth.make("S2", 3, 3, H, W, depth))]
    for t, (kind, fr) in enumerate(sends):
        assert enc.qpring_send(fr, tag=t, yuv420=kind == "420", yuv422=kind == "422")
    assert enc.qpring_flush()
    for t, (kind, fr) in enumerate(sends):
        conv = fr if kind == "444" else sws_422_to_444(oracle, *fr, depth) if kind == "422" else oracle.sws_420_to_444(*fr, depth)
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
def test_yuv422_frames_through_send_frame(oracle, lib, devices, qp, per_call):
    from tests.codec_ctypes import make_ctx
    W, H, depth = 322, 130, 10
    fmt = FMT444[depth]
    src = [yuv422(70 + n, H, W, depth, "noise" if n % 2 else "ramp") for n in range(5)]
    ctx = make_ctx(W, H, PIX444[depth], qp=qp, ring_depth=2, devices=devices, qp_frames_per_call=per_call)
    assert lib.ffv2amd_codec_init(C.byref(ctx)) == 0
    got = _drive(lib, ctx, src, FRAME_YUV422)
    for n, (pts, pk) in enumerate(got):
        try:
            want = (500 + n, oracle.encode(sws_422_to_444(oracle, *src[n], depth), fmt, qp=qp))
        except RuntimeError:
            want = (None, -1)
        assert (pts, pk) == want, n
    assert lib.ffv2amd_codec_close(C.byref(ctx)) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("depth,h,w", [(10, 2160, 3840), (12, 4320, 7680)])
def test_ring_422_literal_formats_full_size(oracle, depth, h, w):
    """3840x2160 yuv422p10le and 7680x4320 yuv422p12le as they are written: host frame in, packet out; the
    up-converted picture is also held sample by sample to the restatement."""
    fmt = FMT444[depth]
    enc = _enc(w, h, depth)
    y, u, v = yuv422(3, h, w, depth, "ramp")
    rng = np.random.default_rng(5)
    u[: h // 4] = rng.integers(0, 1 << depth, u[: h // 4].shape)       # noise and structure in one frame
    want444 = sws_422_to_444(oracle, y, u, v, depth)
    got444 = enc.upconvert_422(y, u, v)
    bad = np.argwhere(got444 != want444)
    assert len(bad) == 0, "first mismatch at (plane, y, x) = %s" % (bad[0],)
    enc.ring_open(2)
    assert enc.ring_send_422(y, u, v, tag=7)
    tag, pk = enc.ring_receive()
    assert tag == 7 and pk == oracle.encode(want444, fmt)
    enc.ring_close()
    enc.close()


@pytest.mark.gpu
def test_cli_yuv422p10le_sync_and_async_match_python(tmp_path):
    subprocess.run(["make", "-s", "-C", ROOT, "examples/ffv2enc_cli"], check=True)
    cli = os.path.join(ROOT, "examples", "ffv2enc_cli")
    W, H, depth = 320, 240, 10
    from ffmpeg_ffv2_amd import frames as synth
    # structured pictures (10-bit noise at qp 16 is a frame the reference aborts on), chroma taken every other column
    src = [(f[0], np.ascontiguousarray(f[1][:, ::2]), np.ascontiguousarray(f[2][:, ::2]))
           for f in (synth.make("S2" if n % 2 else "S1", n, 3, H, W, depth) for n in range(5))]
    raw = tmp_path / "in422.yuv"
    raw.write_bytes(b"".join(p.tobytes() for f in src for p in f))
    enc = _enc(W, H, depth)
    for qp in (0, 16):
        want = b"".join(enc.encode2_422(*f, qp=qp) for f in src)
        for extra in ([], ["--async", "3"]):
            out = tmp_path / ("out%d_%d.ffv2" % (qp, len(extra)))
            r = subprocess.run([cli, str(W), str(H), "yuv422p10le", str(raw), str(out), str(qp), "0"] + extra,
                               capture_output=True, text=True)
            assert r.returncode == 0, r.stderr
            assert out.read_bytes() == want and len(want) > 0, (qp, extra)
    enc.close()
    r = subprocess.run([cli, str(W), str(H), "yuv422p10le", str(raw), str(tmp_path / "x.ffv2"), "--no-convert"],
                       capture_output=True, text=True)
    assert r.returncode == 2                                       # 4:2:2 is not an encoder input either

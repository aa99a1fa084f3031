#!/usr/bin/env python3
"""4:2:2 front end on the MI355X: one JSON line for the literal 3840x2160 yuv422p10le.

  kernel : ffv2_upconv422_kernel alone (ffv2amd_debug_upconv422_time: device events, one warm-up launch) over an
           8-frame batch -- us per frame, and achieved bytes/s from the bytes the step needs, 2*ceil(w/2)*h*bps read
           + 2*w*h*bps written per frame, against the 8 TB/s HBM peak;
  ring   : host frames in, host packets out through the asynchronous ring (ring_send / _420 / _422, depth 4), each
           form for at least --seconds: Gpix/s and the bytes/s its source frames carry over PCIe.  4:4:4, 4:2:0 and
           4:2:2 from page-locked frames, 4:2:2 also from a pool of pageable buffers the ring registers
           (FFV2AMD_FRAME_REGISTER).
Needs the GPU; there is no fallback."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ffmpeg_ffv2_amd import FFV2Encoder, frames as synth  # noqa: E402
from ffmpeg_ffv2_amd import _lib  # noqa: E402

HBM_PEAK = 8e12


def kernel_rate(W, H, fmt, nframes, reps):
    enc = FFV2Encoder(W, H, fmt, device=0, max_batch=1)
    lib = enc._lib
    per = lib.ffv2amd_frame_bytes_422(enc._h)
    g = torch.Generator(device="cuda:0").manual_seed(1)
    src = (torch.randint(0, 1 << 10, (nframes * per // 2,), dtype=torch.int32, device="cuda:0", generator=g)
           .to(torch.int16).view(torch.uint8))
    dst = torch.empty(nframes * enc.info.frame_stride, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ms = C.c_float(0)
    _lib.check(lib.ffv2amd_debug_upconv422_time(enc._h, nframes, src.data_ptr(), dst.data_ptr(), reps, C.byref(ms)),
               "ffv2amd_debug_upconv422_time")
    enc.close()
    bps = 2
    moved = (2 * ((W + 1) // 2) * H * bps + 2 * W * H * bps) * nframes
    return {"us_per_frame": round(ms.value * 1e3 / nframes, 2), "frames_per_launch": nframes, "reps": reps,
            "bytes_per_frame": moved // nframes, "TB_per_s": round(moved / (ms.value * 1e-3) / 1e12, 3),
            "fraction_of_8TBps": round(moved / (ms.value * 1e-3) / HBM_PEAK, 3)}


def ring_rate(W, H, fmt, host444, form, seconds, depth=4):
    enc = FFV2Encoder(W, H, fmt, device=0, max_batch=1)
    enc.ring_open(depth)
    nsrc = len(host444)
    if form == "444":
        src = enc.pinned_frames(nsrc)
        src[:] = host444
        send = lambda n: enc.ring_send(src[n % nsrc], tag=n, pinned=True)                 # noqa: E731
        frame_bytes = 3 * W * H * 2
    elif form == "420":
        src = enc.pinned_frames_420(nsrc)
        for d, f in zip(src, host444):
            d[0][:], d[1][:], d[2][:] = f[0], f[1][::2, ::2], f[2][::2, ::2]
        send = lambda n: enc.ring_send_420(*src[n % nsrc], tag=n, pinned=True)            # noqa: E731
        frame_bytes = (W * H + 2 * ((W + 1) // 2) * ((H + 1) // 2)) * 2
    else:
        if form == "422_pinned":
            src = enc.pinned_frames_422(nsrc)
            for d, f in zip(src, host444):
                d[0][:], d[1][:], d[2][:] = f[0], f[1][:, ::2], f[2][:, ::2]
        else:                                                      # ordinary memory from a pool of long-lived buffers
            src = [(f[0].copy(), np.ascontiguousarray(f[1][:, ::2]), np.ascontiguousarray(f[2][:, ::2])) for f in host444]
        pinned, register = form == "422_pinned", form == "422_registered"
        send = lambda n: enc.ring_send_422(*src[n % nsrc], tag=n, pinned=pinned, register=register)   # noqa: E731
        frame_bytes = (W * H + 2 * ((W + 1) // 2) * H) * 2

    def run(until=None, count=None):
        first, sent, got = None, 0, 0
        t0 = time.perf_counter()
        while True:
            stop = (count is not None and sent >= count) or (until is not None and time.perf_counter() - t0 >= until)
            if not stop and send(sent):
                sent += 1
                continue
            if got == sent:
                break
            tag, pk = enc.ring_receive(wait=True)
            assert tag == got, "ring delivered out of order"
            first = pk if first is None else first
            got += 1
        return time.perf_counter() - t0, got, first

    run(count=2 * depth)                                           # warm-up (registrations happen here)
    dt, n, first = run(until=seconds)
    enc.ring_close()
    enc.free_pinned()
    enc.close()
    return {"gpix_per_s": round(W * H * n / dt / 1e9, 2), "GB_per_s": round(frame_bytes * n / dt / 1e9, 1),
            "frames": n, "seconds": round(dt, 3)}, first


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--seconds", type=float, default=0.6)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--skip-ring", action="store_true", help="the kernel only (for a profiler run)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_422 needs the MI355X"
    W, H, fmt = a.width, a.height, "yuv444p10le"
    out = {"metric": "yuv422p10le front end", "geometry": "%dx%d" % (W, H), "kernel": kernel_rate(W, H, fmt, 8, a.reps)}
    if not a.skip_ring:
        host = [synth.make("S1" if n % 2 == 0 else "S2", n, 3, H, W, 10) for n in range(4)]
        ring, firsts = {}, {}
        for form in ("444", "420", "422_pinned", "422_registered"):
            ring[form], firsts[form] = ring_rate(W, H, fmt, host, form, a.seconds)
        ring["422_pinned_bytes_vs_444"] = round(ring["422_pinned"]["GB_per_s"] / ring["444"]["GB_per_s"], 3)
        ring["422_pinned_gpix_vs_444"] = round(ring["422_pinned"]["gpix_per_s"] / ring["444"]["gpix_per_s"], 3)
        ring["422_registered_equals_pinned_packet0"] = firsts["422_pinned"] == firsts["422_registered"]
        out["ring_depth4_host_boundary"] = ring
    print(json.dumps(out))


if __name__ == "__main__":
    main()

/*
 * ffv2enc_cli.c -- raw planar 4:4:4 frames in, concatenated FFV2 packets out, through the
 * AVCodec-shaped host shim (include/ffv2_amd_codec.h).  The equivalent of
 *   ffmpeg -f rawvideo -s WxH -pix_fmt FMT -i in.yuv -c:v ffv2 -strict -2 -f rawvideo out.ffv2
 * on a machine that has an MI355X but no FFmpeg: the rawvideo
 * muxer writes packets back to back, which is what the reference's known-answer md5s are taken over.
 *
 *   ffv2enc_cli WIDTH HEIGHT PIX_FMT IN.yuv OUT.ffv2 [QP] [HIP_DEVICE] [--async N]
 *   --async N: avcodec_send_frame / avcodec_receive_packet instead of encode2 (same bytes out): N frames in flight
 *            at QP 0 (the asynchronous ring), batches of N frames coded side by side on the device at QP > 0
 *            (FFV2AMDCodecContext.qp_frames_per_call; drained with send_frame(NULL) at the end of the input).
 *   PIX_FMT: gray | yuv444p | yuv444p10le | yuv444p12le | gbrp | gbrp10le | gbrp12le
 *            yuv420p | yuv420p10le | yuv420p12le and yuv422p | yuv422p10le | yuv422p12le are converted
 *            first, as the ffmpeg tool does (choose_pixel_fmt -> yuv444p* + auto-inserted bicubic scale
 *            filter); --no-convert as a last argument hands them to encode2 unconverted, which refuses
 *            them (exit 2).  So are the semi-planar nv12 | nv21 | p010le | nv16 | nv24 | nv42 (Y, then one
 *            plane of interleaved chroma pairs: libswscale de-interleaves, P010 >> 6, then the same step),
 *            and the packed RGB rgb24 | bgr24 | argb | rgba | abgr | bgra | 0rgb | rgb0 | 0bgr | bgr0 (into gbrp)
 *            and rgb48le | rgb48be | bgr48le | bgr48be | rgba64le | rgba64be | bgra64le | bgra64be (into
 *            gbrp12le), converted by libswscale's exact unscaled converters (alpha and padding bytes dropped).
 * An output name ending in ".mkv" selects the Matroska writer (include/ffv2_amd_mkv.h,
 * "V_FFV2", 25 frames per second) instead of the back-to-back packet stream.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ffv2_amd.h"
#include "ffv2_amd_codec.h"
#include "ffv2_amd_mkv.h"

/* *sub: 0 for an encoder format, 420 / 422 for a subsampled source converted to the yuv444p* format returned;
   *nv: the FFV2AMD_FRAME_NV* flags of a semi-planar source (*sub 420 / 422 / 444), else 0;
   *pk: the FFV2AMD_PIX_* value of a packed RGB source converted to the gbrp* format returned (*planes: its
   components per pixel), else 0 */
static int parse_fmt(const char *s, int *planes, int *bps, int *sub, unsigned *nv, int *pk)
{
    static const struct { const char *n; int src, id, bps, nc; } packed[] = {
        { "rgb24", FFV2AMD_PIX_RGB24, FFV2AMD_PIX_GBRP, 1, 3 },     { "bgr24", FFV2AMD_PIX_BGR24, FFV2AMD_PIX_GBRP, 1, 3 },
        { "argb", FFV2AMD_PIX_ARGB, FFV2AMD_PIX_GBRP, 1, 4 },       { "rgba", FFV2AMD_PIX_RGBA, FFV2AMD_PIX_GBRP, 1, 4 },
        { "abgr", FFV2AMD_PIX_ABGR, FFV2AMD_PIX_GBRP, 1, 4 },       { "bgra", FFV2AMD_PIX_BGRA, FFV2AMD_PIX_GBRP, 1, 4 },
        { "0rgb", FFV2AMD_PIX_0RGB, FFV2AMD_PIX_GBRP, 1, 4 },       { "rgb0", FFV2AMD_PIX_RGB0, FFV2AMD_PIX_GBRP, 1, 4 },
        { "0bgr", FFV2AMD_PIX_0BGR, FFV2AMD_PIX_GBRP, 1, 4 },       { "bgr0", FFV2AMD_PIX_BGR0, FFV2AMD_PIX_GBRP, 1, 4 },
        { "rgb48be", FFV2AMD_PIX_RGB48BE, FFV2AMD_PIX_GBRP12LE, 2, 3 }, { "rgb48le", FFV2AMD_PIX_RGB48LE, FFV2AMD_PIX_GBRP12LE, 2, 3 },
        { "bgr48be", FFV2AMD_PIX_BGR48BE, FFV2AMD_PIX_GBRP12LE, 2, 3 }, { "bgr48le", FFV2AMD_PIX_BGR48LE, FFV2AMD_PIX_GBRP12LE, 2, 3 },
        { "rgba64be", FFV2AMD_PIX_RGBA64BE, FFV2AMD_PIX_GBRP12LE, 2, 4 }, { "rgba64le", FFV2AMD_PIX_RGBA64LE, FFV2AMD_PIX_GBRP12LE, 2, 4 },
        { "bgra64be", FFV2AMD_PIX_BGRA64BE, FFV2AMD_PIX_GBRP12LE, 2, 4 }, { "bgra64le", FFV2AMD_PIX_BGRA64LE, FFV2AMD_PIX_GBRP12LE, 2, 4 },
    };
    *pk = 0;
    for (size_t i = 0; i < sizeof(packed) / sizeof(packed[0]); i++)
        if (!strcmp(s, packed[i].n)) { *planes = packed[i].nc; *bps = packed[i].bps; *sub = 0; *nv = 0; *pk = packed[i].src; return packed[i].id; }
    static const struct { const char *n; int id, bps, sub; unsigned flags; } semi[] = {
        { "nv12", FFV2AMD_PIX_YUV444P, 1, 420, FFV2AMD_FRAME_NV | FFV2AMD_FRAME_YUV420 },
        { "nv21", FFV2AMD_PIX_YUV444P, 1, 420, FFV2AMD_FRAME_NV | FFV2AMD_FRAME_NV_VU | FFV2AMD_FRAME_YUV420 },
        { "p010le", FFV2AMD_PIX_YUV444P10LE, 2, 420, FFV2AMD_FRAME_NV | FFV2AMD_FRAME_YUV420 },
        { "nv16", FFV2AMD_PIX_YUV444P, 1, 422, FFV2AMD_FRAME_NV | FFV2AMD_FRAME_YUV422 },
        { "nv24", FFV2AMD_PIX_YUV444P, 1, 444, FFV2AMD_FRAME_NV },
        { "nv42", FFV2AMD_PIX_YUV444P, 1, 444, FFV2AMD_FRAME_NV | FFV2AMD_FRAME_NV_VU },
    };
    *nv = 0;
    for (size_t i = 0; i < sizeof(semi) / sizeof(semi[0]); i++)
        if (!strcmp(s, semi[i].n)) { *planes = 2; *bps = semi[i].bps; *sub = semi[i].sub; *nv = semi[i].flags; return semi[i].id; }
    static const struct { const char *n; int id, bps, sub; } conv[] = {
        { "yuv420p", FFV2AMD_PIX_YUV444P, 1, 420 }, { "yuv420p10le", FFV2AMD_PIX_YUV444P10LE, 2, 420 },
        { "yuv420p12le", FFV2AMD_PIX_YUV444P12LE, 2, 420 },
        { "yuv422p", FFV2AMD_PIX_YUV444P, 1, 422 }, { "yuv422p10le", FFV2AMD_PIX_YUV444P10LE, 2, 422 },
        { "yuv422p12le", FFV2AMD_PIX_YUV444P12LE, 2, 422 },
    };
    *sub = 0;
    for (size_t i = 0; i < sizeof(conv) / sizeof(conv[0]); i++)
        if (!strcmp(s, conv[i].n)) { *planes = 3; *bps = conv[i].bps; *sub = conv[i].sub; return conv[i].id; }
    static const struct { const char *n; int id, planes, bps; } tab[] = {
        { "gray", FFV2AMD_PIX_GRAY8, 1, 1 },           { "yuv444p", FFV2AMD_PIX_YUV444P, 3, 1 },
        { "gbrp", FFV2AMD_PIX_GBRP, 3, 1 },            { "yuv444p10le", FFV2AMD_PIX_YUV444P10LE, 3, 2 },
        { "gbrp10le", FFV2AMD_PIX_GBRP10LE, 3, 2 },    { "yuv444p12le", FFV2AMD_PIX_YUV444P12LE, 3, 2 },
        { "gbrp12le", FFV2AMD_PIX_GBRP12LE, 3, 2 },
    };
    for (size_t i = 0; i < sizeof(tab) / sizeof(tab[0]); i++)
        if (!strcmp(s, tab[i].n)) { *planes = tab[i].planes; *bps = tab[i].bps; return tab[i].id; }
    return -1;
}

int main(int argc, char **argv)
{
    if (argc < 6) {
        fprintf(stderr, "usage: %s WIDTH HEIGHT PIX_FMT IN.yuv OUT.ffv2 [QP] [HIP_DEVICE] [--async N]\n", argv[0]);
        return 2;
    }
    int planes = 0, bps = 0, sub = 0, pk = 0;
    unsigned nv = 0;
    FFV2AMDCodecContext ctx = { 0 };
    ctx.width = atoi(argv[1]);
    ctx.height = atoi(argv[2]);
    ctx.pix_fmt = parse_fmt(argv[3], &planes, &bps, &sub, &nv, &pk);
    if ((sub || pk) && !strcmp(argv[argc - 1], "--no-convert")) {
        fprintf(stderr, "%s is not an encoder input (ffv2enc.c:596-601)\n", argv[3]);
        return 2;
    }
    int async_n = 0;
    for (int i = 6; i + 1 < argc; i++)
        if (!strcmp(argv[i], "--async")) { async_n = atoi(argv[i + 1]); argc = i; break; }
    ctx.global_quality = argc > 6 ? atoi(argv[6]) : 0;
    ctx.hip_device = argc > 7 ? atoi(argv[7]) : 0;
    if (async_n > 0) { ctx.ring_depth = async_n; ctx.qp_frames_per_call = async_n; }
    if (ctx.pix_fmt < 0) { fprintf(stderr, "unsupported pix_fmt %s\n", argv[3]); return 2; }
    FILE *in = strcmp(argv[4], "-") ? fopen(argv[4], "rb") : stdin;
    const size_t olen = strlen(argv[5]);
    const int as_mkv = olen > 4 && !strcmp(argv[5] + olen - 4, ".mkv");
    FILE *out = as_mkv ? NULL : (strcmp(argv[5], "-") ? fopen(argv[5], "wb") : stdout);
    ffv2amd_mkv *mkv = NULL;
    if (as_mkv && ffv2amd_mkv_open(&mkv, argv[5], ctx.width, ctx.height, 25, 1) < 0) { perror("open"); return 1; }
    if (!in || (!out && !mkv)) { perror("open"); return 1; }
    int ret = ffv2amd_codec_init(&ctx);
    if (ret < 0) { fprintf(stderr, "init failed: %d\n", ret); return 1; }

    const size_t plane_bytes = (size_t)ctx.width * ctx.height * bps;
    const int cw = sub == 444 ? ctx.width : (ctx.width + 1) / 2, ch = sub == 420 ? (ctx.height + 1) / 2 : ctx.height;
    const size_t cplane_bytes = (size_t)cw * ch * bps;
    /* a semi-planar frame: Y, then ch rows of cw interleaved pairs (data[1], 2 * cw samples a row) */
    const size_t frame_bytes = sub ? plane_bytes + 2 * cplane_bytes : plane_bytes * planes;
    /* a packed RGB frame: h rows of w pixels of `planes` components (data[0]) */
    const unsigned sub_flag = pk ? FFV2AMD_FRAME_PACKED | FFV2AMD_FRAME_SRC_FMT(pk) : nv ? nv : sub == 420 ? FFV2AMD_FRAME_YUV420 : sub == 422 ? FFV2AMD_FRAME_YUV422 : 0;
    uint8_t *buf = malloc(frame_bytes);
    if (!buf) return 1;
    long nframes = 0;
    size_t nbytes = 0;
    if (async_n > 0) {
        /* one thread sends and receives, as with avcodec_send_frame / avcodec_receive_packet (encode.c:420,449): a frame
           is sent until the encoder takes it (EAGAIN: take a packet first), packets come back in send order; at the end
           of the input send_frame(NULL) lets batches that are not full go, then everything in flight is received.
           The frame buffer is reused at once: without FFV2AMD_FRAME_PINNED / _REGISTER the rows are copied by send. */
        long sent = 0;
        int eof = 0, drained = 0, done = 0;
        ret = 0;
        while (!done) {
            int have = !eof && fread(buf, 1, frame_bytes, in) == frame_bytes;
            FFV2AMDFrame fr = { 0 };
            if (!have) eof = 1;
            for (int p = 0; p < (pk ? 1 : planes) && have; p++) {
                fr.data[p] = sub ? (p ? buf + plane_bytes + (p - 1) * cplane_bytes : buf) : buf + p * plane_bytes;
                fr.linesize[p] = (ptrdiff_t)(sub && p ? (nv ? 2 * cw : cw) : pk ? ctx.width * planes : ctx.width) * bps;
            }
            fr.pts = sent;
            for (;;) {
                if (have) {
                    ret = ffv2amd_codec_send_frame(&ctx, &fr, sub_flag);
                    if (ret == 0) { sent++; break; }                    /* next frame */
                    if (ret != FFV2AMD_ERR_AGAIN) { done = 1; break; }
                } else if (!drained) {
                    ret = ffv2amd_codec_send_frame(&ctx, NULL, 0);
                    if (ret == 0) drained = 1;
                    else if (ret != FFV2AMD_ERR_AGAIN) { done = 1; break; }
                }
                FFV2AMDPacket pkt = { 0 };
                ret = ffv2amd_codec_receive_packet(&ctx, &pkt, 1);
                if (ret == FFV2AMD_ERR_AGAIN) {
                    if (drained && nframes == sent) { ret = 0; done = 1; break; }
                    continue;
                }
                if (ret < 0) { fprintf(stderr, "receive_packet failed on frame %ld: %d\n", nframes, ret); done = 1; break; }
                if (mkv) ret = ffv2amd_mkv_write_packet(mkv, pkt.data, (size_t)pkt.size, pkt.pts);
                else     fwrite(pkt.data, 1, (size_t)pkt.size, out);
                nbytes += (size_t)pkt.size;
                ffv2amd_packet_unref(&pkt);
                nframes++;
            }
        }
    } else
    while (fread(buf, 1, frame_bytes, in) == frame_bytes) {
        FFV2AMDFrame fr = { 0 };
        FFV2AMDPacket pkt = { 0 };
        int got = 0;
        for (int p = 0; p < (pk ? 1 : planes); p++) {
            fr.data[p] = sub ? (p ? buf + plane_bytes + (p - 1) * cplane_bytes : buf) : buf + p * plane_bytes;
            fr.linesize[p] = (ptrdiff_t)(sub && p ? (nv ? 2 * cw : cw) : pk ? ctx.width * planes : ctx.width) * bps;
        }
        fr.pts = nframes;
        ret = pk ? ffv2amd_codec_encode_packed(&ctx, &pkt, &fr, pk, &got)
            : nv ? ffv2amd_codec_encode_nv(&ctx, &pkt, &fr, nv, &got)
            : sub == 420 ? ffv2amd_codec_encode_yuv420(&ctx, &pkt, &fr, &got)
            : sub == 422 ? ffv2amd_codec_encode_yuv422(&ctx, &pkt, &fr, &got)
            : ffv2amd_codec_encode2(&ctx, &pkt, &fr, &got);
        if (ret < 0 || !got) { fprintf(stderr, "encode2 failed on frame %ld: %d\n", nframes, ret); break; }
        if (mkv) ret = ffv2amd_mkv_write_packet(mkv, pkt.data, (size_t)pkt.size, pkt.pts);
        else     fwrite(pkt.data, 1, (size_t)pkt.size, out);
        nbytes += (size_t)pkt.size;
        ffv2amd_packet_unref(&pkt);
        nframes++;
    }
    ffv2amd_codec_close(&ctx);
    free(buf);
    if (mkv) { const int r2 = ffv2amd_mkv_close(mkv); if (ret >= 0) ret = r2; }
    else if (out != stdout) fclose(out);
    fprintf(stderr, "%ld frames, %zu bytes\n", nframes, nbytes);
    return ret < 0 ? 1 : 0;
}
